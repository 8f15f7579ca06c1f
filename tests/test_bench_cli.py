"""bench.py's command line: a plain run prints the headline line only, --full
adds the per-kernel, census, roofline and baseline figures, and --dump-outputs
writes the last timed tick's outputs, identical from run to run.  The GPU
cases run the 10k-peer c2 network in-process, two timed ticks each."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("kernel_ms_per_tick", "census", "roofline", "roofline_kernels", "gossip_per_tick", "box", "cpu_baseline")


def _run(monkeypatch, capsys, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "c2", "--steps", "2", "--warmup", "1",
                                      *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "one JSON result line"
    return json.loads(lines[0])


def test_dump_sample_is_seeded_and_bounded():
    import bench
    small = np.arange(10.0).reshape(2, 5)
    assert np.array_equal(bench._dump_sample(small, 1), np.arange(10.0))
    big = np.arange(bench.DUMP_SAMPLE * 3, dtype=np.float64)
    a, b = bench._dump_sample(big, 7), bench._dump_sample(big, 7)
    assert a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert not np.array_equal(a, bench._dump_sample(big, 8))
    assert a.min() < bench.DUMP_SAMPLE and a.max() > 2 * bench.DUMP_SAMPLE, "positions over the whole array"


def test_c3_ring_outlasts_the_reuse_guard_on_long_runs():
    """--steps in the hundreds: the engine refuses a publication into a slot whose
    message had a new delivery less than (max(HistoryLength 5, HistoryGossip 3) +
    promise ticks 5 + 2) * ROUNDS = 120 rounds ago (deliver.hip reuse_guard).  A
    message gains deliveries while it is gossiped (HistoryGossip = 3 ticks) and one
    tick of IWANT answers after: 40 rounds.  Over 1000 ticks of C3's own schedule
    no slot of the ring comes round again sooner than the two together."""
    import bench
    n, T = bench.CONFIGS["c3"][0], bench.CONFIGS["c3"][2]
    sched = bench.message_schedule(n, T, range(1, 1001), seed=2)
    rounds = np.concatenate([np.full(len(sched[g]), g) for g in sorted(sched)])
    gap = rounds[bench.MSG_RING:] - rounds[:-bench.MSG_RING]
    assert gap.min() >= (12 + 4) * bench.ROUNDS, gap.min()


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dump_repeats(require_gpu, monkeypatch, capsys, tmp_path):
    outs = []
    for d in ("a", "b"):
        line = _run(monkeypatch, capsys, "--dump-outputs", str(tmp_path / d))
        for key in HEADLINE:
            assert key in line, key
        for key in FULL_ONLY:
            assert key not in line, f"{key} belongs to --full"
        assert line["steps"] == 2 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert line["value"] == pytest.approx(10_000 / (line["ms_per_step"] * 1e-3))
        assert line["deliveries_per_tick"]["accepted"] > 0, "the timed ticks delivered messages"
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert set(a) == set(b) >= {"scores.npy", "msg_stats.npy", "gossip_stats.npy", "census.npy", "tflags.npy",
                                "behaviour_penalty.npy"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), f"{name} differs between runs"
    assert a["scores.npy"].size == 10_000 * 32 and np.count_nonzero(a["scores.npy"]) > 0
    assert a["msg_stats.npy"][0] > 0 and a["census.npy"][0] > 0


@pytest.mark.gpu
def test_full_line_keeps_the_headline_and_adds_the_rest(require_gpu, monkeypatch, capsys):
    line = _run(monkeypatch, capsys, "--full", "--no-cpu-baseline")
    for key in HEADLINE + tuple(k for k in FULL_ONLY if k != "cpu_baseline"):
        assert key in line, key
    assert "cpu_baseline" not in line
    assert line["steps"] == 2 and line["kernel_ms_per_tick"]["heartbeat"] > 0
    assert line["census"]["records"] > 0

#!/usr/bin/env python3
"""The propagation report against the only other route to its numbers, on the
state the benchmark leaves:

    python tools/msg_report_times.py [--config c3] [--steps 20] [--warmup 3]

Builds bench.py's network, runs its warm-up and timed ticks, then on that state
  a) gsim_msg_report over the whole ring, device time between two
     gsim_event_record marks around the sized call (and the wall time of
     Engine.msg_report: the count-only call, the sized call, the host sort);
  b) gsim_read_field(GSIM_F_SEEN) plus the numpy reduction to the same rows,
     wall clock (--no-seen skips it: at c5 the [ring][N] view cannot exist);
  c) the cell bytes the report read and the rate they were read at.
The two results are compared row for row before anything is printed.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))


def seen_route(eng, ring_n):
    """F_SEEN to the host, then per published slot the numpy histogram."""
    from gsim import _abi
    t0 = time.perf_counter()
    seen = eng.read(_abi.F_SEEN)
    t1 = time.perf_counter()
    bins = _abi.REPORT_BINS
    rows = {}
    for m in range(seen.shape[0]):
        s = seen[m]
        got = s[s != _abi.UNSEEN]
        if not len(got):
            continue
        pub = int(got.min())                       # the origin's own cell: the publication round
        lat = got.astype(np.int64) - pub
        rows[m] = (pub, len(lat), int(lat.max()), np.bincount(np.minimum(lat, bins - 1), minlength=bins))
    t2 = time.perf_counter()
    return rows, t1 - t0, t2 - t1, seen.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-seen", action="store_true")
    args = ap.parse_args()
    import bench
    from gsim.engine import Engine
    cfg, scen = bench.CONFIGS[args.config], bench.SCENARIOS.get(args.config, {})
    eng, net = bench.build_engine(cfg, 1, 0, scen)
    T = cfg[2]
    nticks = args.warmup + args.steps
    sched = bench.message_schedule(net.n, T, range(1, nticks + 1), sub=net.sub if scen.get("zipf_per_peer") else None,
                                   rate=scen.get("msg_rate", bench.MSG_RATE))
    churn = bench.churn_schedule(net, scen["churn_frac"], range(1, nticks + 1)) if "churn_frac" in scen else None
    bench.run_ticks(eng, 0, nticks, sched, churn, px=bool(scen.get("px")))
    eng.synchronize()
    ring = eng._msg_cfg.ring
    out = {"config": args.config, "peers": net.n, "ring": ring, "ticks": nticks, "box": bench.box_info()}
    # a) the report
    n = ctypes.c_int64(0)
    eng._check(eng.lib.gsim_msg_report(eng.h, 0, (1 << 63) - 1, None, 0, ctypes.byref(n)))
    rep = np.zeros(n.value, dtype=Engine.MSG_REPORT_DTYPE)
    dev_ms, wall_ms = [], []
    for _ in range(args.reps):
        eng.event_record(0)
        eng._check(eng.lib.gsim_msg_report(eng.h, 0, (1 << 63) - 1, rep.ctypes.data, n.value, ctypes.byref(n)))
        eng.event_record(1)
        dev_ms.append(eng.event_elapsed_ms(0, 1))
        t0 = time.perf_counter()
        rep2 = eng.msg_report()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    assert rep2.tobytes() == rep.tobytes()
    cells = int(rep["subscribers"].astype(np.int64).sum()) if scen.get("topic_slots") else len(rep) * net.n
    out["report"] = {"messages": len(rep), "device_ms": dev_ms, "wall_ms_two_calls": wall_ms,
                     "cell_bytes": cells * 8, "gb_per_s": cells * 8 / (min(dev_ms) * 1e-3) / 1e9,
                     "reached_total": int(rep["reached"].astype(np.int64).sum()),
                     "max_latency": int(rep["max_latency"].max()) if len(rep) else 0}
    # b) F_SEEN + numpy
    if not args.no_seen:
        rows, copy_s, reduce_s, nbytes = seen_route(eng, ring)
        assert sorted(rows) == sorted(rep["slot"].tolist()), "the two routes select different slots"
        for r in rep:
            pub, reached, mx, hist = rows[int(r["slot"])]
            assert (pub, reached, mx) == (int(r["pub_round"]), int(r["reached"]), int(r["max_latency"])), r["slot"]
            assert (hist == r["hist"]).all(), r["slot"]
        out["seen_route"] = {"view_bytes": nbytes, "read_field_s": copy_s, "numpy_s": reduce_s,
                             "wall_ms": (copy_s + reduce_s) * 1e3, "rows_equal": True}
        out["speedup_wall"] = out["seen_route"]["wall_ms"] / min(wall_ms)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Events per second of gsim_score_tracer_events against the oracle's replay
of the same stream on the host's threads:

    python tools/tracer_events_times.py [--peers 1000000] [--degree 32] [--topics 16] [--messages 6]
                                        [--reps 5] [--threads 16] [--no-check]

Builds a random regular network with the engine's synthetic state (C3's
shape at the defaults), and turns the copies of `--messages` messages (round
robin over the topics) into a stream: every observer gets one copy per peer of
its mesh of the message's topic, the first a DeliverMessage, the others
DuplicateMessage, shuffled across observers (an observer's own order kept).
  gpu       gsim_score_tracer_events, wall time of the call (the stream's
            upload, sort, resolve, apply and the counters' read-back), median
            of --reps after one warm-up, each on fresh delivery records; with
            the library's own stage times (gsim_profile: tracer_sort,
            tracer_resolve, tracer_apply)
  baseline  tools/tracer_replay_baseline.c: the oracle's functions, one
            observer per OpenMP task on --threads threads, over the stream
            grouped by observer on the host first (timed apart)
The planes the two leave are compared bit for bit before anything is printed
(--no-check skips it).  The oracle's state is the engine's read back: at C3's
shape that is about 30 GB of host memory.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def build_stream(net, tflags, T, messages, t0, rng):
    """The copies of `messages` messages as score events, shuffled across observers."""
    from gsim import _abi, tracer
    owner = net.owner()
    parts = []
    for k in range(messages):
        # (gsim_read_field's view is in edge order: entry e is the record of owner[e] about col[e])
        e = np.flatnonzero(tflags[k % T] & _abi.TF_IN_MESH)
        part = np.zeros(len(e), dtype=tracer.EVENT_DTYPE)
        part["mid"], part["now_ns"], part["topic"] = k, t0 + k * 1_000_000, k % T
        part["observer"], part["peer"] = owner[e], net.col[e]
        parts.append(part)
    ev = np.concatenate(parts)
    order = np.lexsort((rng.random(len(ev)), ev["mid"], ev["observer"]))      # per observer: by message, copies shuffled
    ev = ev[order]
    first = np.r_[True, (ev["observer"][1:] != ev["observer"][:-1]) | (ev["mid"][1:] != ev["mid"][:-1])]
    ev["kind"] = np.where(first, tracer.EV_DELIVER, tracer.EV_DUPLICATE)
    r = rng.random(len(ev))
    r = r[np.lexsort((r, ev["observer"]))]                                     # ascending within each observer
    return np.ascontiguousarray(ev[np.argsort(r, kind="stable")])


def group(net, ev):
    """The stream grouped by observer (stable), its edges and segment bounds."""
    order = np.argsort(ev["observer"], kind="stable")
    g = np.ascontiguousarray(ev[order])
    rp = net.row_ptr.astype(np.int64)
    key = net.owner().astype(np.int64) * net.n + net.col
    edge = np.searchsorted(key, g["observer"].astype(np.int64) * net.n + g["peer"]).astype(np.int64)
    assert (key[edge] == g["observer"].astype(np.int64) * net.n + g["peer"]).all() and (edge < rp[-1]).all()
    heads = np.flatnonzero(np.r_[True, g["observer"][1:] != g["observer"][:-1]])
    return g, edge, np.r_[heads, len(g)].astype(np.int64)


def baseline_lib(tmp):
    so = os.path.join(tmp, "libtracer_replay.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "oracle"),
                           os.path.join(REPO, "tools", "tracer_replay_baseline.c"), "-o", so,
                           "-L", os.path.join(REPO, "oracle"), "-loracle", "-Wl,-rpath," + os.path.join(REPO, "oracle")])
    lib = ctypes.CDLL(so)
    lib.tracer_replay.restype = None
    lib.tracer_replay.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=1_000_000)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--topics", type=int, default=16)
    ap.add_argument("--messages", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()
    import oracle_binding as ob
    from fixtures import beacon_params, beacon_thresholds
    from gsim import Second, _abi
    from gsim.engine import Engine, random_regular
    T, now = args.topics, 1000 * Second
    net = random_regular(args.peers, args.degree, seed=5, n_topics=T)
    params, th = beacon_params(T), beacon_thresholds()
    eng = Engine(params, th)
    eng.load_graph(net)
    eng.fill_synthetic(seed=7, now=now, p_mesh=8 / args.degree)
    tflags = eng.read(_abi.F_TFLAGS)
    ev = build_stream(net, tflags, T, args.messages, now + Second, np.random.default_rng(11))
    n_obs = len(np.unique(ev["observer"]))
    st = ob.NetState(net, params, thresholds=th)
    st.pull_from_engine(eng)                                   # the state both sides start from
    out = {"peers": net.n, "edges": net.e, "topics": T, "messages": args.messages, "events": len(ev),
           "observers": n_obs, "threads": args.threads}

    # the capacity check counts the worst case: a record per Deliver / Duplicate event
    rec_cap, peers_cap = len(ev) + 1024, len(ev)
    wall, stages = [], []
    for rep in range(args.reps + 1):
        if rep == 1:
            for f in st.TOPIC_FIELDS + st.EDGE_FIELDS:         # the same start for the timed reps
                eng.write(st.FIELD_IDS[f], getattr(st, f))
        eng.tracer_config(rec_cap, peers_cap)
        eng.profile(True)
        eng.synchronize()
        t = time.perf_counter()
        eng.tracer_events(ev)
        wall.append((time.perf_counter() - t) * 1e3)
        prof = eng.profile_read()
        stages.append({k: prof[k][0] for k in ("tracer_sort", "tracer_resolve", "tracer_apply")})
        eng.profile(False)
        if rep == 0 and not args.no_check:
            gpu = ob.NetState(net, params, thresholds=th)
            gpu.pull_from_engine(eng)
    wall, stages = wall[1:], stages[1:]
    out["gpu_ms"] = wall
    out["gpu_median_ms"] = statistics.median(wall)
    out["gpu_stage_median_ms"] = {k: statistics.median(s[k] for s in stages) for k in stages[0]}
    out["gpu_events_per_s"] = len(ev) / (out["gpu_median_ms"] * 1e-3)
    out["tracer_stats"] = eng.tracer_stats()
    eng.close()

    lib = ob.load()
    lib.orc_set_threads(args.threads)
    t = time.perf_counter()
    g, edge, seg = group(net, ev)
    out["baseline_group_ms"] = (time.perf_counter() - t) * 1e3
    with tempfile.TemporaryDirectory() as tmp:
        rl = baseline_lib(tmp)
        t = time.perf_counter()
        st.view()
        rl.tracer_replay(ctypes.addressof(st._view), g.ctypes.data, edge.ctypes.data, seg.ctypes.data, len(seg) - 1)
        out["baseline_ms"] = (time.perf_counter() - t) * 1e3
    out["baseline_events_per_s"] = len(ev) / (out["baseline_ms"] * 1e-3)
    out["ratio"] = out["gpu_events_per_s"] / out["baseline_events_per_s"]
    if not args.no_check:
        for f in ("first", "meshd", "fail", "invalid", "graft_time", "tflags", "bp"):
            a, b = getattr(st, f), getattr(gpu, f)
            assert np.array_equal(a.view(np.uint64) if a.dtype.itemsize == 8 else a,
                                  b.view(np.uint64) if b.dtype.itemsize == 8 else b), f"{f} differs from the oracle"
        out["checked"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()

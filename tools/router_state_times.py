#!/usr/bin/env python3
"""Times of the router state calls (gsim_router_state_*) beside the score
tracer's on the same stream, box and session:

    python tools/router_state_times.py [--peers 200000] [--degree 32] [--topics 16] [--messages 6] [--reps 5]

Builds tools/tracer_events_times.py's network and stream (C3's shape at
200 000 peers by default): the copies of `--messages` messages, one per mesh
peer of every observer, shuffled across observers.
  seen      the copies as SEEN_ADD events through gsim_router_state_events:
            wall time of the call (upload, sort, resolve, apply, the answers'
            and counters' read-back), median of --reps after one warm-up, each
            on a fresh configuration, with the library's stage times
            (gsim_profile: router_sort, router_resolve, router_apply).  The
            answers are compared with a host dict first (the first copy of an
            (observer, id) in array order is new).
  sweep     one gsim_router_state_sweep that drops the first half of the ids
  promises  the same copies as PROMISE events (every (id, peer) is new), then
            one gsim_router_state_broken past every expiry
  tracer    gsim_score_tracer_events on the same stream as Deliver / Duplicate
            events, timed the same way: the comparison
Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def timed(eng, call, classes):
    """Wall milliseconds of call() (it synchronizes) and the stage times of `classes`."""
    eng.profile(True)
    eng.synchronize()
    t = time.perf_counter()
    ret = call()
    ms = (time.perf_counter() - t) * 1e3
    prof = eng.profile_read()
    eng.profile(False)
    return ms, {k: prof[k][0] for k in classes}, ret


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peers", type=int, default=200_000)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--topics", type=int, default=16)
    ap.add_argument("--messages", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from fixtures import beacon_params, beacon_thresholds
    from gsim import Second, _abi, routerstate as rs
    from gsim.engine import Engine, random_regular
    from tracer_events_times import build_stream
    T, now = args.topics, 1000 * Second
    net = random_regular(args.peers, args.degree, seed=5, n_topics=T)
    eng = Engine(beacon_params(T), beacon_thresholds())
    eng.load_graph(net)
    eng.fill_synthetic(seed=7, now=now, p_mesh=8 / args.degree)
    tev = build_stream(net, eng.read(_abi.F_TFLAGS), T, args.messages, now + Second, np.random.default_rng(11))
    n = len(tev)
    ev = np.zeros(n, dtype=rs.EVENT_DTYPE)
    for f in ("mid", "now_ns", "observer", "peer"):
        ev[f] = tev[f]
    ev["kind"] = rs.RS_SEEN_ADD
    # the host dict: the first copy of an (observer, id) in array order is new
    key = ev["observer"].astype(np.int64) * args.messages + ev["mid"].astype(np.int64)
    want = np.zeros(n, dtype=np.uint8)
    want[np.unique(key, return_index=True)[1]] = 1
    out = {"peers": net.n, "edges": net.e, "topics": T, "messages": args.messages, "events": n,
           "observers": int(len(np.unique(ev["observer"]))), "new": int(want.sum())}

    stages = ("router_sort", "router_resolve", "router_apply")
    wall, prof = [], []
    for rep in range(args.reps + 1):
        eng.router_state_config(n + 1024, 16, 0)
        ms, st, got = timed(eng, lambda: eng.router_state_events(ev), stages)
        if rep == 0:
            assert np.array_equal(got, want), "the seen answers differ from the host dict"
            out["checked"] = True
        else:
            wall.append(ms)
            prof.append(st)
    out["seen_ms"] = wall
    out["seen_median_ms"] = statistics.median(wall)
    out["seen_stage_median_ms"] = {k: statistics.median(s[k] for s in prof) for k in stages}
    out["seen_events_per_s"] = n / (out["seen_median_ms"] * 1e-3)

    ttl = 120 * Second
    half = int(ev["now_ns"][ev["mid"] == args.messages // 2].min())
    ms, st, _ = timed(eng, lambda: eng.router_state_sweep(half + ttl), ("router_sweep",))
    out["sweep_ms"], out["sweep_kernel_ms"] = ms, st["router_sweep"]
    out["swept"] = eng.router_state_stats()["swept"]

    ev["kind"] = rs.RS_PROMISE
    eng.router_state_config(16, n, 0)                      # (the observers' clocks start over)
    ms, st, got = timed(eng, lambda: eng.router_state_events(ev), stages)
    assert got.all(), "every (id, peer) promise is new"
    out["promise_ms"], out["promise_stage_ms"] = ms, st
    rows = np.zeros(n, dtype=rs.BROKEN_DTYPE)
    nrows = ctypes.c_int64(0)
    late = int(ev["now_ns"].max()) + 3600 * Second

    def broken():
        eng._check(eng.lib.gsim_router_state_broken(eng.h, late, 0, rows.ctypes.data, n, ctypes.byref(nrows)))
    ms, st, _ = timed(eng, broken, ("router_broken",))
    out["broken_ms"], out["broken_device_ms"], out["broken_rows"] = ms, st["router_broken"], nrows.value
    assert int(rows["count"][:nrows.value].sum()) == n == eng.router_state_stats()["broken"]

    tstages = ("tracer_sort", "tracer_resolve", "tracer_apply")
    wall, prof = [], []
    for rep in range(args.reps + 1):
        eng.tracer_config(n + 1024, n)
        ms, st, _ = timed(eng, lambda: eng.tracer_events(tev), tstages)
        if rep:
            wall.append(ms)
            prof.append(st)
    out["tracer_ms"] = wall
    out["tracer_median_ms"] = statistics.median(wall)
    out["tracer_stage_median_ms"] = {k: statistics.median(s[k] for s in prof) for k in tstages}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The peer delivery report against the propagation report, which streams the
same cells, and against the only other route to its numbers, on the state the
benchmark leaves:

    python tools/peer_report_times.py [--config c3] [--steps 20] [--warmup 3] [--classes 1,2]

Builds bench.py's network, runs its warm-up and timed ticks, then on that state
  a) gsim_peer_report over the whole ring, device time between two
     gsim_event_record marks around the sized call: both halves, the per-peer
     rows alone and the class rows alone, alternating with gsim_msg_report
     (the yardstick: the same bytes, reduced per message) in the same process;
  b) gsim_read_field(GSIM_F_SEEN) plus the numpy reduction to the per-peer
     rows, wall clock (--no-seen skips it: at c5 the [ring][N] view cannot
     exist).  First senders are not in that view: first_from has no other route.
  c) the cell bytes a call read and the rate they were read at.
--classes takes a list of class counts, measured one after the other on the same
state: K > 1 puts peer p in class p % K (the first senders' class gather).
The per-peer rows of the two routes are compared before anything is printed.
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

BIG = (1 << 63) - 1


def seen_route(eng, rep, sub):
    """F_SEEN to the host, then per selected slot the per-peer sums in numpy."""
    from gsim import _abi
    t0 = time.perf_counter()
    seen = eng.read(_abi.F_SEEN)
    t1 = time.perf_counter()
    n = seen.shape[1]
    acc = {f: np.zeros(n, dtype=np.int64) for f in ("expected", "received", "own", "missed", "lat_sum", "lat_max")}
    for r in rep:
        s = seen[int(r["slot"])]
        got = s != _abi.UNSEEN
        lat = np.where(got, s.astype(np.int64) - int(r["pub_round"]), 0)
        sb = ((sub >> np.uint64(int(r["topic"]))) & np.uint64(1)).astype(bool)
        acc["expected"] += sb
        acc["received"] += got
        acc["missed"] += sb & ~got
        acc["lat_sum"] += lat
        np.maximum(acc["lat_max"], lat, out=acc["lat_max"])
        if got[int(r["origin"])]:
            acc["own"][int(r["origin"])] += 1
    t2 = time.perf_counter()
    return acc, t1 - t0, t2 - t1, seen.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", default="1")
    ap.add_argument("--no-seen", action="store_true")
    args = ap.parse_args()
    import bench
    cfg, scen = bench.CONFIGS[args.config], bench.SCENARIOS.get(args.config, {})
    eng, net = bench.build_engine(cfg, 1, 0, scen)
    T = cfg[2]
    nticks = args.warmup + args.steps
    sched = bench.message_schedule(net.n, T, range(1, nticks + 1), sub=net.sub if scen.get("zipf_per_peer") else None,
                                   rate=scen.get("msg_rate", bench.MSG_RATE))
    churn = bench.churn_schedule(net, scen["churn_frac"], range(1, nticks + 1)) if "churn_frac" in scen else None
    bench.run_ticks(eng, 0, nticks, sched, churn, px=bool(scen.get("px")))
    eng.synchronize()
    n = net.n
    out = {"config": args.config, "peers": n, "ring": eng._msg_cfg.ring, "ticks": nticks, "topics": T,
           "box": bench.box_info(), "peer_report": {}}
    for K in [int(x) for x in args.classes.split(",")]:
        eng.set_peer_classes((np.arange(n) % K).astype(np.uint8) if K > 1 else None)
        rows, rep, wall_ms = measure(eng, n, args.reps, bool(scen.get("topic_slots")), out["peer_report"], K)
    if not args.no_seen:
        acc, copy_s, reduce_s, nbytes = seen_route(eng, rep, net.sub)
        for f, v in acc.items():
            assert (v == rows[f].astype(np.int64)).all(), f"the two routes differ in {f}"
        out["seen_route"] = {"view_bytes": nbytes, "read_field_s": copy_s, "numpy_s": reduce_s,
                             "wall_ms": (copy_s + reduce_s) * 1e3, "rows_equal": True}
        out["speedup_wall"] = out["seen_route"]["wall_ms"] / wall_ms
    eng.close()
    print(json.dumps(out))


def measure(eng, n, reps, compact, res, K):
    """One class count: the calls timed on the device, alternating; res[K] is filled."""
    from gsim.engine import Engine
    nc, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    eng._check(eng.lib.gsim_peer_report(eng.h, 0, BIG, 0, 0, None, None, 0, ctypes.byref(nc), ctypes.byref(nm)))
    rows = np.zeros(n, dtype=Engine.PEER_ROW_DTYPE)
    crow = np.zeros(nc.value, dtype=Engine.PEER_CLASS_ROW_DTYPE)
    rep = np.zeros(nm.value, dtype=Engine.MSG_REPORT_DTYPE)
    k = ctypes.c_int64(0)

    def timed(call):
        eng.event_record(0)
        eng._check(call())
        eng.event_record(1)
        return eng.event_elapsed_ms(0, 1)

    calls = {
        "both": lambda: eng.lib.gsim_peer_report(eng.h, 0, BIG, 0, n, rows.ctypes.data, crow.ctypes.data, nc.value,
                                                 ctypes.byref(nc), ctypes.byref(nm)),
        "peers_only": lambda: eng.lib.gsim_peer_report(eng.h, 0, BIG, 0, n, rows.ctypes.data, None, 0, ctypes.byref(nc),
                                                       ctypes.byref(nm)),
        "classes_only": lambda: eng.lib.gsim_peer_report(eng.h, 0, BIG, 0, 0, None, crow.ctypes.data, nc.value,
                                                         ctypes.byref(nc), ctypes.byref(nm)),
        "msg_report": lambda: eng.lib.gsim_msg_report(eng.h, 0, BIG, rep.ctypes.data, len(rep), ctypes.byref(k)),
    }
    for call in calls.values():                                  # warm-up: code objects, scratch
        timed(call)
    ms = {name: [] for name in calls}
    for _ in range(reps):                                        # alternating, the same process and state
        for name, call in calls.items():
            ms[name].append(timed(call))
    launch = eng.peer_report_launch()
    t0 = time.perf_counter()
    rows2, crow2 = eng.peer_report()
    wall_ms = (time.perf_counter() - t0) * 1e3
    calls["both"]()
    assert rows2.tobytes() == rows.tobytes() and crow2.tobytes() == crow.tobytes()
    cells = int(rep["subscribers"].astype(np.int64).sum()) if compact else len(rep) * n
    assert int(crow["received"].sum()) == int(rep["reached"].astype(np.int64).sum()), "the two reports disagree"
    best = {name: min(v) for name, v in ms.items()}
    res[str(K)] = {"messages": nm.value, "class_rows": nc.value, "launch": launch, "device_ms": ms,
                   "wall_ms_two_calls": wall_ms, "cell_bytes": cells * 8,
                   "gb_per_s": {name: cells * 8 / (v * 1e-3) / 1e9 for name, v in best.items()},
                   "ratio_to_msg_report": {name: v / best["msg_report"] for name, v in best.items()},
                   "received_total": int(rows["received"].astype(np.int64).sum()),
                   "missed_total": int(rows["missed"].astype(np.int64).sum())}
    return rows, rep, wall_ms


if __name__ == "__main__":
    main()

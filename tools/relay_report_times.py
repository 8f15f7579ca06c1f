#!/usr/bin/env python3
"""The relay report against the peer delivery report, which streams the same
cells, on the state the benchmark leaves:

    python tools/relay_report_times.py [--config c3] [--steps 20] [--warmup 3] [--classes 1] [--budget 0]

Builds bench.py's network, runs its warm-up and timed ticks, then on that state
times, on the device between two gsim_event_record marks around the sized call,
alternating in one process, each as the median of --reps (>= 5) after one
warm-up:
  peers      gsim_relay_report, the per-peer rows alone
  classes    ... with the class rows added
  messages   ... with the message rows added (the depth passes)
  push       gsim_relay_report for the rows of one peer: the selection, the
             batches' memsets and the whole push pass, with a fold over one wave;
             the push pass's scattered atomics divided by it is a lower bound of
             their rate
  peer_report  gsim_peer_report, both halves, the yardstick: there is no host
             path to first senders to compare against.
--budget: the per-batch scratch budget in bytes (0: the default).  The rows of
the calls are compared with each other and with the peer report before anything
is printed: first deliveries given == first deliveries received.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))

BIG = (1 << 63) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", default="1")
    ap.add_argument("--budget", default="0")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (a median)")
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
           "box": bench.box_info(), "relay_report": {}}
    for K in [int(x) for x in args.classes.split(",")]:
        eng.set_peer_classes((np.arange(n) % K).astype(np.uint8) if K > 1 else None)
        for budget in [int(x) for x in args.budget.split(",")]:
            eng.relay_report_budget(budget)
            out["relay_report"][f"classes={K},budget={budget}"] = measure(eng, n, args.reps, K)
    eng.relay_report_budget(0)
    eng.close()
    print(json.dumps(out))


def measure(eng, n, reps, K):
    """One class count and budget: the calls timed on the device, alternating."""
    from gsim.engine import Engine
    nc, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    fn = eng.lib.gsim_relay_report
    eng._check(fn(eng.h, 0, BIG, 0, 0, None, None, 0, ctypes.byref(nc), None, 0, ctypes.byref(nm)))
    rows = np.zeros(n, dtype=Engine.RELAY_ROW_DTYPE)
    one = np.zeros(1, dtype=Engine.RELAY_ROW_DTYPE)
    crow = np.zeros(nc.value, dtype=Engine.RELAY_CLASS_ROW_DTYPE)
    mrow = np.zeros(nm.value, dtype=Engine.RELAY_MSG_ROW_DTYPE)
    prow = np.zeros(n, dtype=Engine.PEER_ROW_DTYPE)
    pcrow = np.zeros(nc.value, dtype=Engine.PEER_CLASS_ROW_DTYPE)
    k1, k2 = ctypes.c_int64(0), ctypes.c_int64(0)

    def timed(call):
        eng.event_record(0)
        eng._check(call())
        eng.event_record(1)
        return eng.event_elapsed_ms(0, 1)

    def relay(lo, hi, p, c, m):
        return lambda: fn(eng.h, 0, BIG, lo, hi, p.ctypes.data if p is not None else None,
                          c.ctypes.data if c is not None else None, len(c) if c is not None else 0, ctypes.byref(nc),
                          m.ctypes.data if m is not None else None, len(m) if m is not None else 0, ctypes.byref(nm))

    calls = {
        "peers": relay(0, n, rows, None, None),
        "classes": relay(0, n, rows, crow, None),
        "messages": relay(0, n, rows, crow, mrow),
        "push": relay(0, 1, one, None, None),
        "peer_report": lambda: eng.lib.gsim_peer_report(eng.h, 0, BIG, 0, n, prow.ctypes.data, pcrow.ctypes.data, nc.value,
                                                        ctypes.byref(k1), ctypes.byref(k2)),
    }
    launch = {}
    for name, call in calls.items():                             # warm-up: code objects, scratch
        timed(call)
        if name != "peer_report":
            launch[name] = eng.relay_report_launch()
    ms = {name: [] for name in calls}
    for _ in range(reps):                                        # alternating, the same process and state
        for name, call in calls.items():
            ms[name].append(timed(call))
    calls["messages"]()
    given = int(rows["children"].sum())
    assert given == int(prow["received"].astype(np.int64).sum() - prow["own"].astype(np.int64).sum()), \
        "first deliveries given != first deliveries received"
    assert given == int(crow["children"].sum()) == int((mrow["reached"].astype(np.int64) - 1 - mrow["orphans"]).sum())
    assert one.tobytes() == rows[:1].tobytes() and not mrow["orphans"].any()
    med = {name: statistics.median(v) for name, v in ms.items()}
    atomics = given * (2 if K > 1 else 1)
    return {"messages": nm.value, "class_rows": nc.value, "launch": launch, "device_ms": ms, "median_ms": med,
            "ratio_to_peer_report": {name: v / med["peer_report"] for name, v in med.items()},
            "first_deliveries": given, "push_atomics": atomics,
            "push_atomics_per_s_lower_bound": atomics / (med["push"] * 1e-3),
            "depth_passes": launch["messages"]["depth_passes"], "depth_max": int(mrow["depth_max"].max()) if len(mrow) else 0,
            "leaf_share": float(crow["fanout"][:, 0].sum() / max(int(crow["held"].sum()), 1))}


if __name__ == "__main__":
    main()

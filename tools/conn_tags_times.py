#!/usr/bin/env python3
"""What the connection tags cost on the benchmark's network:

    python tools/conn_tags_times.py [--config c3] [--steps 10] [--warmup 3]

Builds bench.py's network, runs its warm-up ticks, configures the tags
(gsim_conn_tags_config, the reference's cap and bump) and runs the timed ticks
one gsim_step call each.  Device times between two gsim_event_record marks:
  a) the tick itself (gsim_step of one tick; the tags' fold is not in it: the
     explicit fold of b) left it nothing to do);
  b) the fold of that tick's first deliveries (gsim_conn_values with no output);
  c) a refresh that crosses one decay instant against the same refresh again
     (which crosses none): the difference is one decay pass;
  d) one forced trim, count only (low 24, high 0), and then the same trim for
     real (wall clock: it ends in gsim_set_connections).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--low", type=int, default=24)
    args = ap.parse_args()
    import bench
    from gsim import connmgr
    cfg, scen = bench.CONFIGS[args.config], bench.SCENARIOS.get(args.config, {})
    eng, net = bench.build_engine(cfg, 1, 0, scen)
    T = cfg[2]
    nticks = args.warmup + args.steps
    sched = bench.message_schedule(net.n, T, range(1, nticks + 1), sub=net.sub if scen.get("zipf_per_peer") else None,
                                   rate=scen.get("msg_rate", bench.MSG_RATE))
    bench.run_ticks(eng, 0, args.warmup, sched)
    eng.synchronize()
    interval = 1000 * bench.SECOND                       # no instant inside the timed ticks
    eng.conn_tags_config(decay_interval=interval, t0=bench.tick_time(0))
    tick_ms, fold_ms = [], []
    first0 = eng.msg_stats()[1]
    for kk in range(args.warmup + 1, nticks + 1):
        part = {g: sched[g] for g in range(kk * bench.ROUNDS, (kk + 1) * bench.ROUNDS) if g in sched}
        eng.event_record(0)
        eng.step(kk, 1, part)
        eng.event_record(1)
        eng._check(eng.lib.gsim_conn_values(eng.h, bench.tick_time(kk), 0, None, None))
        eng.event_record(2)
        tick_ms.append(eng.event_elapsed_ms(0, 1))
        fold_ms.append(eng.event_elapsed_ms(1, 2))
    firsts = eng.msg_stats()[1] - first0
    value, flags = eng.conn_values(bench.tick_time(nticks))
    out = {"config": args.config, "peers": net.n, "edges": net.e, "ticks": args.steps, "box": bench.box_info(),
           "tick_ms": tick_ms, "fold_ms": fold_ms, "fold_share_of_tick": float(np.mean(fold_ms) / np.mean(tick_ms)),
           "first_deliveries_per_tick": firsts / args.steps,
           "tagged_connections": int((value > 0).sum()), "value_sum": int(value.astype(np.int64).sum()),
           "value_max": int(value.max())}
    # c) one decay pass: a refresh crossing an instant minus the same refresh again
    cross, plain = [], []
    for m in range(1, 4):
        now = bench.tick_time(0) + m * interval
        eng.event_record(0)
        eng.refresh_scores(now)
        eng.event_record(1)
        eng.refresh_scores(now)
        eng.event_record(2)
        cross.append(eng.event_elapsed_ms(0, 1))
        plain.append(eng.event_elapsed_ms(1, 2))
    out["refresh_crossing_ms"], out["refresh_plain_ms"] = cross, plain
    out["decay_ms"] = float(min(cross) - min(plain))
    v2, _ = eng.conn_values(bench.tick_time(0) + 3 * interval)
    out["value_sum_after_3_decays"] = int(v2.astype(np.int64).sum())
    # d) the forced trim
    now = bench.tick_time(0) + 3 * interval + bench.SECOND // 2
    trim_ms = []
    for _ in range(3):
        eng.event_record(0)
        n = eng.conn_trim(nticks, now, args.low, 0, count_only=True)
        eng.event_record(1)
        trim_ms.append(eng.event_elapsed_ms(0, 1))
    t0 = time.perf_counter()
    pairs = eng.conn_trim(nticks, now, args.low, 0)
    out["trim"] = {"low": args.low, "high": 0, "count_only_ms": trim_ms, "pairs": int(n),
                   "real_wall_ms": (time.perf_counter() - t0) * 1e3, "closed": int(len(pairs)),
                   "protected_share_mean": float(np.nanmean(connmgr.protected_share(net, flags)))}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

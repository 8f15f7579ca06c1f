#!/usr/bin/env python3
"""Engine-only ticks on a network with planted hub rows, for kernel timing:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wide_row_times.py --net wide --ticks 2

--net wide   the network of tests/test_wide_rows.py (24 000 peers, 4 topics,
             hub rows of 8193 / 12 001 / 20 000 connections: the wide class)
--net giant  8000 peers, 6 topics, hub rows of 6000 and 5000 connections (the
             rows of tests/test_configs.py::test_rows_over_4096_bit_exact:
             k_heartbeat_hub_g)

Every tick: refresh, heartbeat, the rounds with publications, the PX
connector.  No oracle runs; the wall time per phase is printed, and the sum
of the hub rows' lengths, to turn a kernel's time into time per row position.
Tick 1 prunes the synthetic hub meshes (thousands over Dhi), later ticks are
the steady state.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("wide", "giant"), default="wide")
    ap.add_argument("--ticks", type=int, default=2)
    args = ap.parse_args()
    import test_wide_rows as w
    from gsim.engine import Engine
    from gsim.params import Second
    from gsim import graphs
    from test_delivery import R, T0
    from test_heartbeat import SEED, tick_time
    from tickrun import subscribed_schedule
    if args.net == "wide":
        net, T, hubs = w.wide_net(), w.T, [h for h, _ in w.HUBS]
    else:
        n, T, hubs = 8000, 6, [0, 1]
        net = w.planted(n, T, 81, ((0, 6000), (1, 5000)), np.random.default_rng(8192), 1024)
        sub = graphs.zipf_subscriptions(n, T, 3, seed=82)
        sub[:2] = (1 << T) - 1
        net = graphs.with_subscriptions(net, sub)
    deg = np.diff(net.row_ptr.astype(np.int64))
    print(f"net {args.net}: {net.n} peers, {net.e} edges, hub rows {[int(deg[h]) for h in hubs]} "
          f"(sum {int(sum(deg[h] for h in hubs))}), longest other row {int(np.delete(deg, hubs).max())}")
    rng, params, th, gp, st = w.setup(net, T, 1)
    ticks = list(range(1, args.ticks + 1))
    sched = subscribed_schedule(rng, ticks, net, T, 1.5, 0.0, member_only=False,
                                verdicts=[0.85, 0.05, 0.04, 0.03, 0.03])
    eng = Engine(params, th, gossip=gp)
    try:
        eng.load_graph(net)
        eng.set_seed(SEED)
        st.push_to_engine(eng)
        eng.msgs_init(1024, R, T0, Second)
        for kk in ticks:
            now = tick_time(kk)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.refresh_scores(now)
            eng.synchronize()
            t1 = time.perf_counter()
            eng.heartbeat(kk, now)
            eng.synchronize()
            t2 = time.perf_counter()
            for g in range(kk * R, kk * R + R):
                if g in sched:
                    eng.publish(sched[g], g)
                eng.round(g)
            eng.synchronize()
            t3 = time.perf_counter()
            made = eng.px_connect(now + Second // 2)
            t4 = time.perf_counter()
            print(f"tick {kk}: refresh {1e3 * (t1 - t0):.2f} ms, heartbeat {1e3 * (t2 - t1):.2f} ms, "
                  f"rounds {1e3 * (t3 - t2):.2f} ms, px_connect {1e3 * (t4 - t3):.2f} ms ({len(made)} connections)")
    finally:
        eng.close()


if __name__ == "__main__":
    main()

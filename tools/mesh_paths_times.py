#!/usr/bin/env python3
"""The mesh path report against the only other route to its numbers, on the
state the benchmark leaves:

    python tools/mesh_paths_times.py [--config c3] [--steps 20] [--warmup 3] [--classes 2]

Builds bench.py's network, runs its warm-up and timed ticks, then on that
state, for 64 random sources of topic 0 (peer p is class p % classes),
  a) gsim_mesh_paths without and with the last class blocked, without and
     with the per-peer arrays: device time between two gsim_event_record marks
     around the call (its per-level host reads included), the wall time of
     Engine.mesh_paths, the number of levels and the host synchronisations the
     call made (gsim_host_sync_count);
  b) gsim_read_field(GSIM_F_TFLAGS) and a numpy BFS on the host, one boolean
     frontier per source, for a few of the sources (--host-sources), wall
     clock, scaled per source to the 64.
The two results are compared field for field before anything is printed.
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


def host_route(eng, net, cls, topic, sources, blocked):
    """The ABI's view to the host, then the rows with a numpy BFS per source."""
    from gsim import _abi
    from gsim.engine import Engine
    t0 = time.perf_counter()
    tflags = eng.read(_abi.F_TFLAGS)
    t1 = time.perf_counter()
    n = net.n
    owner, col = net.owner().astype(np.int64), net.col.astype(np.int64)
    ann = ((net.sub >> np.uint64(topic)) & np.uint64(1)) != 0
    mesh = ((tflags[topic] & _abi.TF_MESH) != 0) & ann[owner] & ann[col]
    fan = ((tflags[topic] & _abi.TF_FANOUT) != 0) & ~ann[owner] & ann[col]
    mo, mc = owner[mesh], col[mesh]
    isblk = np.isin(cls, list(blocked))
    rows = np.zeros(len(sources), dtype=Engine.MESH_PATH_ROW_DTYPE)
    NC, BINS = _abi.NET_CLASSES, _abi.REPORT_BINS
    for k, s in enumerate(int(x) for x in sources):
        dist = np.full(n, -1, dtype=np.int64)
        front = np.zeros(n, dtype=bool)
        front[s] = True
        if ann[s]:
            dist[s] = 0
        level = 0
        while front.any():
            tgt = col[fan & (owner == s)] if level == 0 and not ann[s] else mc[front[mo]]
            new = np.zeros(n, dtype=bool)
            new[tgt] = True
            new &= dist < 0
            level += 1
            dist[new] = level
            front = new & ~isblk
        ok = dist >= 0
        r = rows[k]
        r["source"], r["topic"], r["reached"], r["subscribers"] = s, topic, ok.sum(), ann.sum()
        r["max_hops"] = dist.max() if ok.any() else 0
        r["reached_cls"][:] = np.bincount(cls[ok], minlength=NC)
        r["members_cls"][:] = np.bincount(cls[ann], minlength=NC)
        r["hist"][:] = np.bincount(np.minimum(dist[ok], BINS - 1), minlength=BINS)
    t2 = time.perf_counter()
    return rows, t1 - t0, t2 - t1, tflags.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--host-sources", type=int, default=4)
    args = ap.parse_args()
    import bench
    from gsim import _abi
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
    cls = (np.arange(net.n) % args.classes).astype(np.uint8)
    eng.set_peer_classes(cls)
    topic = 0
    src = np.random.default_rng(1).choice(net.n, size=_abi.PATH_SOURCES, replace=False).astype(np.uint32)
    blocked = (args.classes - 1,)
    mask = 1 << blocked[0]
    out = {"config": args.config, "peers": net.n, "edges": net.e, "topics": T, "classes": args.classes, "topic": topic,
           "sources": len(src), "blocked_classes": list(blocked), "ticks": nticks, "box": bench.box_info()}
    rows = np.zeros(len(src), dtype=Engine.MESH_PATH_ROW_DTYPE)
    rc, hs = np.zeros(net.n, dtype=np.uint32), np.zeros(net.n, dtype=np.uint32)
    syncs = ctypes.c_uint64(0)

    def timed(m, per_peer):
        ms, wall, ns = [], [], 0
        for _ in range(args.reps):
            eng.lib.gsim_host_sync_count(ctypes.byref(syncs))
            s0 = syncs.value
            eng.event_record(0)
            eng._check(eng.lib.gsim_mesh_paths(eng.h, topic, src.ctypes.data, len(src), m, 0, rows.ctypes.data,
                                               rc.ctypes.data if per_peer else None, hs.ctypes.data if per_peer else None))
            eng.event_record(1)
            ms.append(eng.event_elapsed_ms(0, 1))
            eng.lib.gsim_host_sync_count(ctypes.byref(syncs))
            ns = syncs.value - s0
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.mesh_paths(topic, src, blocked=blocked if m else (), per_peer=per_peer)
            wall.append((time.perf_counter() - t0) * 1e3)
        return {"device_ms": ms, "wall_ms": wall, "host_syncs": int(ns), "levels": int(rows["max_hops"].max()),
                "reached_mean": float(rows["reached"].mean()), "subscribers": int(rows["subscribers"][0])}

    out["plain"] = timed(0, False)
    plain = rows.copy()
    out["plain_per_peer"] = timed(0, True)
    out["blocked"] = timed(mask, False)
    cut = rows.copy()
    out["blocked_per_peer"] = timed(mask, True)
    from gsim import report
    out["censored_share_mean"] = float(np.nanmean(report.censored_share(plain, cut, blocked=blocked)))
    k = max(1, min(args.host_sources, len(src)))
    want, read_s, bfs_s, nbytes = host_route(eng, net, cls.astype(np.int64), topic, src[:k], ())
    wantb, _, bfsb_s, _ = host_route(eng, net, cls.astype(np.int64), topic, src[:k], blocked)
    for f in Engine.MESH_PATH_ROW_DTYPE.names:
        assert (want[f] == plain[f][:k]).all() and (wantb[f] == cut[f][:k]).all(), f
    scale = len(src) / k
    out["host_route"] = {"view_bytes": nbytes, "read_s": read_s, "bfs_sources": k, "bfs_s": bfs_s, "bfs_blocked_s": bfsb_s,
                         "wall_ms_scaled_to_all_sources": (read_s + bfs_s * scale) * 1e3, "rows_equal": True}
    out["speedup_wall"] = out["host_route"]["wall_ms_scaled_to_all_sources"] / min(out["plain"]["wall_ms"])
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

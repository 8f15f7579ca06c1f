#!/usr/bin/env python3
"""The network report against the only other route to its numbers, on the
state the benchmark leaves:

    python tools/net_report_times.py [--config c3] [--steps 20] [--warmup 3] [--classes 2]

Builds bench.py's network, runs its warm-up and timed ticks, then on that state
  a) gsim_net_report (both halves, then each alone), device time between two
     gsim_event_record marks around the sized call, and the wall time of
     Engine.net_report (the count-only call and the sized call);
  b) gsim_read_field(GSIM_F_TFLAGS / GSIM_F_ESTATE / GSIM_F_FANOUT_TOPICS) and
     gsim_read_scores plus the numpy reduction to the same rows, wall clock
     (--no-readback skips it: at c5 the [T][E] view cannot exist);
  c) the bytes the report must read -- the mflags planes (every topic's on
     dense planes; at least the announced topics' of each row on slot planes),
     score, estate, owner, col and sub -- and the rate that makes of the call.
The two results are compared field for field before anything is printed.
Classes: peer p is class p % classes.
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


def readback_route(eng, net, T, cls, edges):
    """The ABI's views to the host, then the report's rows with numpy."""
    from gsim import _abi
    from gsim.engine import Engine
    t0 = time.perf_counter()
    tflags = eng.read(_abi.F_TFLAGS)
    score = eng.scores()
    estate = eng.read(_abi.F_ESTATE)
    fan_topics = eng.read(_abi.F_FANOUT_TOPICS)
    t1 = time.perf_counter()
    n, C = net.n, int(cls.max()) + 1
    owner, col = net.owner().astype(np.int64), net.col.astype(np.int64)
    outb = net.outbound != 0
    ci, cj = cls[owner], cls[col]
    pair = ci * C + cj
    DB, OB, SB = _abi.NET_DEG_BINS, _abi.NET_OUT_BINS, _abi.NET_SCORE_BINS
    mesh = np.zeros(T * C, dtype=Engine.MESH_ROW_DTYPE)
    for t in range(T):
        ann = ((net.sub >> np.uint64(t)) & np.uint64(1)) != 0
        mbit = ((tflags[t] & _abi.TF_MESH) != 0) & ann[owner]
        fbit = ((tflags[t] & _abi.TF_FANOUT) != 0) & ~ann[owner]
        deg = np.bincount(owner[mbit], minlength=n)
        out = np.bincount(owner[mbit & outb], minlength=n)
        fan = ((fan_topics >> np.uint64(t)) & np.uint64(1)) != 0
        links = np.bincount(pair[mbit], minlength=C * C).reshape(C, C)
        outl = np.bincount(ci[mbit & outb], minlength=C)
        fanl = np.bincount(ci[fbit], minlength=C)
        for c in range(C):
            r = mesh[t * C + c]
            sel = ann & (cls == c)
            r["topic"], r["cls"], r["members"] = t, c, sel.sum()
            r["max_degree"] = deg[sel].max() if sel.any() else 0
            r["fanout_peers"] = (~ann & (cls == c) & fan).sum()
            r["mesh_links"][:C] = links[c]
            r["outbound_links"], r["fanout_links"] = outl[c], fanl[c]
            r["deg_hist"][:] = np.bincount(np.minimum(deg[sel], DB - 1), minlength=DB)
            r["out_hist"][:] = np.bincount(np.minimum(out[sel], OB - 1), minlength=OB)
    conn = (estate & _abi.ES_CONNECTED) != 0
    ret = ((estate & _abi.ES_TRACKED) != 0) & ~conn
    isnan = np.isnan(score)
    scores = np.zeros(C * C, dtype=Engine.SCORE_ROW_DTYPE)
    for q in range(C * C):
        r = scores[q]
        sel = pair == q
        ok = sel & conn & ~isnan
        r["obs_cls"], r["subj_cls"] = q // C, q % C
        r["connected"], r["retained"], r["nan"] = (sel & conn).sum(), (sel & ret).sum(), (sel & conn & isnan).sum()
        s = score[ok]
        r["min"], r["max"] = (s.min(), s.max()) if len(s) else (np.inf, -np.inf)
        r["hist"][:] = np.bincount(np.searchsorted(edges, s, side="right"), minlength=SB)
    t2 = time.perf_counter()
    return (mesh, scores), t1 - t0, t2 - t1, tflags.nbytes + score.nbytes + estate.nbytes + fan_topics.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--no-readback", action="store_true")
    args = ap.parse_args()
    import bench
    from gsim import report
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
    edges = report.threshold_edges(eng.thresholds)
    E = net.e
    out = {"config": args.config, "peers": net.n, "edges": E, "topics": T, "classes": args.classes,
           "score_edges": edges.tolist(), "ticks": nticks, "box": bench.box_info()}
    mesh, scores = eng.net_report(edges)
    ed = np.ascontiguousarray(edges)
    nm, ns = ctypes.c_int64(0), ctypes.c_int64(0)

    def timed(m, s):
        ms = []
        for _ in range(args.reps):
            eng.event_record(0)
            eng._check(eng.lib.gsim_net_report(eng.h, ed.ctypes.data, len(ed), m.ctypes.data if m is not None else None,
                                               len(m) if m is not None else 0, ctypes.byref(nm),
                                               s.ctypes.data if s is not None else None,
                                               len(s) if s is not None else 0, ctypes.byref(ns)))
            eng.event_record(1)
            ms.append(eng.event_elapsed_ms(0, 1))
        return ms

    m2, s2 = np.zeros_like(mesh), np.zeros_like(scores)
    both_ms, mesh_ms, score_ms = timed(m2, s2), timed(m2, None), timed(None, s2)
    assert m2.tobytes() == mesh.tobytes() and s2.tobytes() == scores.tobytes()
    wall_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.net_report(edges)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    uniq, inv = np.unique(net.sub, return_inverse=True)
    joined = np.array([bin(int(x) & ((1 << T) - 1)).count("1") for x in uniq], dtype=np.int64)[inv]
    all_joined = bool((joined == T).all())
    planes = int((joined * np.diff(net.row_ptr.astype(np.int64))).sum())     # = T * E when every peer joined every topic
    mesh_bytes = planes + 8 * net.n
    score_bytes = (8 + 1 + 4 + 4) * E
    out["report"] = {"device_ms": both_ms, "mesh_only_device_ms": mesh_ms, "scores_only_device_ms": score_ms,
                     "wall_ms_two_calls": wall_ms, "mflags_plane_bytes": planes,
                     "plane_bytes_are_a_lower_bound": not all_joined, "must_read_bytes": mesh_bytes + score_bytes,
                     "gb_per_s": (mesh_bytes + score_bytes) / (min(both_ms) * 1e-3) / 1e9,
                     "mesh_gb_per_s": mesh_bytes / (min(mesh_ms) * 1e-3) / 1e9,
                     "scores_gb_per_s": score_bytes / (min(score_ms) * 1e-3) / 1e9,
                     "members": int(mesh["members"].astype(np.int64).sum()),
                     "mesh_links": int(mesh["mesh_links"].sum()), "max_degree": int(mesh["max_degree"].max()),
                     "connected": int(scores["connected"].sum()), "retained": int(scores["retained"].sum())}
    if not args.no_readback:
        (wm, ws), copy_s, reduce_s, nbytes = readback_route(eng, net, T, cls.astype(np.int64), edges)
        for f in Engine.MESH_ROW_DTYPE.names:
            assert (wm[f] == mesh[f]).all(), f
        for f in Engine.SCORE_ROW_DTYPE.names:
            assert (ws[f] == scores[f]).all(), f
        out["readback_route"] = {"view_bytes": nbytes, "read_s": copy_s, "numpy_s": reduce_s,
                                 "wall_ms": (copy_s + reduce_s) * 1e3, "rows_equal": True}
        out["speedup_wall"] = out["readback_route"]["wall_ms"] / min(wall_ms)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

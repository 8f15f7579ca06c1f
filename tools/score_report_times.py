#!/usr/bin/env python3
"""The score report against the only other route to its numbers, on the state
the benchmark leaves:

    python tools/score_report_times.py [--config c3] [--steps 20] [--warmup 3] [--classes 2]

Builds bench.py's network, runs its warm-up and timed ticks (the last tick's
meshMessageDeliveries increments stay pending and meshTime lazy: the state a
report meets between ticks), then on that state
  a) gsim_score_report (all three thirds), device time between two
     gsim_event_record marks around the sized call, under the engine's own
     parameters and under a what-if set (MeshMessageDeliveriesWeight doubled,
     another TopicScoreCap), and the wall time of Engine.score_report (the
     count-only call and the sized call);
  b) the yardstick: k_refresh_score's per-launch device time on the same
     state from gsim_profile over --yard-ticks more ticks (that kernel reads the
     same planes and also writes them), after which a) is repeated;
  c) gsim_read_field of the seven [T][E] planes and of bp, p6 and estate plus
     the numpy restatement of the header's definition, wall clock
     (--no-readback skips it: at c5 the [T][E] views cannot exist);
  d) the bytes the pass must read and the rate that makes of the call.
The two results are compared field for field before anything is printed.
Classes: peer p is class p % classes.
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "go-libp2p-pubsub_amd"))

FLAGS = ("in_mesh", "p1_capped", "first_at_cap", "active", "p3_deficit", "p3b_nonzero", "p4_nonzero", "negative")


def stated_bin(x):
    """The part histogram's bin from the header's stated bounds (comparisons
    against the even powers of two); the callers pass no NaN."""
    pows = 2.0 ** np.arange(-6, 23, 2)
    m = np.searchsorted(pows, np.abs(x), side="right")
    return np.where(x == 0, 16, np.where(x < 0, 15 - m, 17 + m))


def readback_route(eng, net, T, cls, edges, p5):
    """The ABI's views to the host, then the report's rows with numpy."""
    from gsim import _abi
    from gsim.engine import Engine
    t0 = time.perf_counter()
    first, meshd, fail, invalid = (eng.read(f) for f in (_abi.F_FIRST, _abi.F_MESHD, _abi.F_FAIL, _abi.F_INVALID))
    mesh_time, tflags = eng.read(_abi.F_MESH_TIME), eng.read(_abi.F_TFLAGS)
    bp, p6, estate = eng.read(_abi.F_BP), eng.read(_abi.F_P6), eng.read(_abi.F_ESTATE)
    t1 = time.perf_counter()
    nbytes = sum(a.nbytes for a in (first, meshd, fail, invalid, mesh_time, tflags, bp, p6, estate))
    E, C = net.e, int(cls.max()) + 1
    NP, NB, NC, SB = _abi.SR_PARTS, _abi.SR_BINS, _abi.SR_CAUSES, _abi.NET_SCORE_BINS
    obs, subj = net.owner().astype(np.int64), net.col.astype(np.int64)
    pair = cls[obs] * C + cls[subj]
    conn = (estate & _abi.ES_CONNECTED) != 0
    tracked = (estate & _abi.ES_TRACKED) != 0
    sc = conn & tracked
    pp, tps = eng.params.to_c(), eng.params.topic_array(eng.topics)
    part = np.zeros((NP, E))
    topics = np.zeros(T * C * C, dtype=Engine.SCORE_TOPIC_ROW_DTYPE)
    with np.errstate(all="ignore"):
        for t in range(T):
            tp = tps[t]
            for q in range(C * C):
                r = topics[t * C * C + q]
                r["topic"], r["obs_cls"], r["subj_cls"] = t, q // C, q % C
            if not tp.scored:
                continue
            inm, act = (tflags[t] & _abi.TF_IN_MESH) != 0, (tflags[t] & _abi.TF_ACTIVE) != 0
            qn = int(tp.time_in_mesh_quantum_ns)
            if qn != 0:
                mt = mesh_time[t]
                quot = np.where((mt < 0) != (qn < 0), -1, 1) * (np.abs(mt) // abs(qn))     # truncation toward zero
                p1raw = np.where(inm, quot.astype(np.float64), 0.0)
            else:
                p1raw = np.zeros(E)
            p1cap = p1raw > tp.time_in_mesh_cap
            p1 = np.where(inm, np.where(p1cap, tp.time_in_mesh_cap, p1raw) * tp.time_in_mesh_weight, 0.0)
            p2 = first[t] * tp.first_message_deliveries_weight
            deficit = act & (meshd[t] < tp.mesh_message_deliveries_threshold)
            d = tp.mesh_message_deliveries_threshold - meshd[t]
            p3 = np.where(deficit, (d * d) * tp.mesh_message_deliveries_weight, 0.0)
            p3b = fail[t] * tp.mesh_failure_penalty_weight
            p4 = (invalid[t] * invalid[t]) * tp.invalid_message_deliveries_weight
            ts = ((((0.0 + p1) + p2) + p3) + p3b) + p4
            tw = tp.topic_weight
            for k, p in enumerate((p1, p2, p3, p3b, p4, ts)):
                part[k] += p * tw
            fl = (inm, inm & p1cap, first[t] >= tp.first_message_deliveries_cap, act, deficit, fail[t] != 0,
                  invalid[t] != 0, ts * tw < 0)
            for k, f in enumerate(FLAGS):
                topics[f][t * C * C:(t + 1) * C * C] = np.bincount(pair[fl[k] & sc], minlength=C * C)
        capped = (part[_abi.SR_TOPICS] > pp.topic_score_cap) if pp.topic_score_cap > 0 else np.zeros(E, dtype=bool)
        part[_abi.SR_TOPICS] = np.where(capped, pp.topic_score_cap, part[_abi.SR_TOPICS])
        part[_abi.SR_P5] = p5[subj] * pp.app_specific_weight
        part[_abi.SR_P6] = p6 * pp.ip_colocation_factor_weight
        ex = bp - pp.behaviour_penalty_threshold
        part[_abi.SR_P7] = np.where(bp > pp.behaviour_penalty_threshold, (ex * ex) * pp.behaviour_penalty_weight, 0.0)
        part[:, ~tracked] = 0.0
        part[_abi.SR_TOTAL] = ((part[_abi.SR_TOPICS] + part[_abi.SR_P5]) + part[_abi.SR_P6]) + part[_abi.SR_P7]
        cand = part[[_abi.SR_P3, _abi.SR_P3B, _abi.SR_P4, _abi.SR_P5, _abi.SR_P6, _abi.SR_P7]]
        neg = cand < 0
        cause = np.where(neg.any(axis=0), np.argmin(np.where(neg, cand, np.inf), axis=0), NC - 1)
    total = part[_abi.SR_TOTAL]
    tnan = np.isnan(total)
    tbin = np.searchsorted(edges, np.where(tnan, 0.0, total), side="right")
    parts = np.zeros(C * C * NP, dtype=Engine.SCORE_PART_ROW_DTYPE)
    causes = np.zeros(C * C, dtype=Engine.SCORE_CAUSE_ROW_DTYPE)
    for q in range(C * C):
        sel = conn & (pair == q)
        for k in range(NP):
            r = parts[q * NP + k]
            r["obs_cls"], r["subj_cls"], r["part"] = q // C, q % C, k
            v = part[k][sel]
            ok = ~np.isnan(v)
            r["nan"] = (~ok).sum()
            r["min"], r["max"] = (v[ok].min(), v[ok].max()) if ok.any() else (np.inf, -np.inf)
            r["hist"][:] = np.bincount(stated_bin(v[ok]), minlength=NB)
        r = causes[q]
        r["obs_cls"], r["subj_cls"] = q // C, q % C
        r["connected"], r["retained"] = sel.sum(), (tracked & ~conn & (pair == q)).sum()
        r["nan"], r["capped"] = (sel & tnan).sum(), (sel & capped & sc).sum()
        ok = sel & ~tnan
        r["cause"][:] = np.bincount(tbin[ok] * NC + cause[ok], minlength=SB * NC).reshape(SB, NC)
    t2 = time.perf_counter()
    return (parts, causes, topics), t1 - t0, t2 - t1, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--yard-ticks", type=int, default=3)
    ap.add_argument("--no-readback", action="store_true")
    args = ap.parse_args()
    import bench
    from gsim import report
    from gsim.engine import _score_what_if, app_scores
    cfg, scen = bench.CONFIGS[args.config], bench.SCENARIOS.get(args.config, {})
    eng, net = bench.build_engine(cfg, 1, 0, scen)
    T = cfg[2]
    nticks = args.warmup + args.steps + args.yard_ticks
    sched = bench.message_schedule(net.n, T, range(1, nticks + 1), sub=net.sub if scen.get("zipf_per_peer") else None,
                                   rate=scen.get("msg_rate", bench.MSG_RATE))
    churn = bench.churn_schedule(net, scen["churn_frac"], range(1, nticks + 1)) if "churn_frac" in scen else None
    px = bool(scen.get("px"))
    bench.run_ticks(eng, 0, args.warmup + args.steps, sched, churn, px=px)
    eng.synchronize()
    cls = (np.arange(net.n) % args.classes).astype(np.uint8)
    eng.set_peer_classes(cls)
    edges = np.ascontiguousarray(report.threshold_edges(eng.thresholds))
    E = net.e
    out = {"config": args.config, "peers": net.n, "edges": E, "topics": T, "classes": args.classes,
           "score_edges": edges.tolist(), "box": bench.box_info()}
    rows = eng.score_report(edges)
    wp = copy.deepcopy(eng.params)
    wp.TopicScoreCap = 100.0
    for tp in wp.Topics.values():
        tp.MeshMessageDeliveriesWeight = 2.0 * tp.MeshMessageDeliveriesWeight
    wif, keep = _score_what_if(eng, wp, None)
    cnt = [ctypes.c_int64(0) for _ in range(3)]

    def timed(what_if, bufs):
        ms = []
        for _ in range(args.reps):
            a = []
            for b, c in zip(bufs, cnt):
                a += [b.ctypes.data, len(b), ctypes.byref(c)]
            eng.event_record(0)
            eng._check(eng.lib.gsim_score_report(eng.h, ctypes.byref(what_if) if what_if is not None else None,
                                                 edges.ctypes.data, len(edges), *a))
            eng.event_record(1)
            ms.append(eng.event_elapsed_ms(0, 1))
        return ms

    bufs = tuple(np.zeros_like(r) for r in rows)
    own_ms = timed(None, bufs)
    assert all(b.tobytes() == r.tobytes() for b, r in zip(bufs, rows))
    wbufs = tuple(np.zeros_like(r) for r in rows)
    wif_ms = timed(wif, wbufs)
    wall_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng.score_report(edges)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    census = eng.census()
    conn = int(rows[1]["connected"].sum())
    uniq, inv = np.unique(net.sub, return_inverse=True)
    joined = np.array([bin(int(x) & ((1 << T) - 1)).count("1") for x in uniq], dtype=np.int64)[inv]
    planes = int((joined * np.diff(net.row_ptr.astype(np.int64))).sum())     # (topic, record) pairs with a slot: T * E when dense
    per_rec = 1 + 4 + 4 + 8 + 8                                    # estate, owner, col, bp, p6
    per_plane = 1 + 1 + 8 + 8 + 8 + 8                              # tflags, mcnt, first, meshd, fail, graft or meshTime
    must = per_rec * E + per_plane * planes
    must_inv = must + 8 * planes                                   # + the invalid planes while any counter is non-zero
    out["report"] = {"device_ms": own_ms, "what_if_device_ms": wif_ms, "wall_ms_two_calls": wall_ms,
                     "plane_records": planes, "must_read_bytes": must, "must_read_bytes_with_invalid": must_inv,
                     "nz_invalid_records": census["nz_invalid"],
                     "gb_per_s": must / (min(own_ms) * 1e-3) / 1e9, "bytes_per_record": must / E,
                     "connected": conn, "retained": int(rows[1]["retained"].sum()),
                     "capped": int(rows[1]["capped"].sum()),
                     "cause_totals": rows[1]["cause"].sum(axis=(0, 1)).tolist()}
    if not args.no_readback:
        p5 = app_scores(eng.params.AppSpecificScore, net.n) if eng.params.AppSpecificScore is not None else np.zeros(net.n)
        want, copy_s, reduce_s, nbytes = readback_route(eng, net, T, cls.astype(np.int64), edges, np.asarray(p5, dtype=np.float64))
        for got_rows, want_rows in zip(rows, want):
            for f in got_rows.dtype.names:
                assert (got_rows[f] == want_rows[f]).all(), f
        out["readback_route"] = {"view_bytes": nbytes, "read_s": copy_s, "numpy_s": reduce_s,
                                 "wall_ms": (copy_s + reduce_s) * 1e3, "rows_equal": True}
        out["speedup_wall"] = out["readback_route"]["wall_ms"] / min(wall_ms)
    # the yardstick: the refresh pass on the same state
    eng.profile(True)
    eng.profile_read()
    bench.run_ticks(eng, args.warmup + args.steps, args.yard_ticks, sched, churn, px=px)
    prof = eng.profile_read()
    eng.profile(False)
    ms, launches = prof["refresh_score"]
    out["refresh_score"] = {"ms": ms, "launches": launches, "ms_per_launch": ms / max(launches, 1)}
    again = timed(None, bufs)
    out["report"]["device_ms_after_yardstick_ticks"] = again
    out["report_over_refresh"] = min(min(own_ms), min(again)) / max(out["refresh_score"]["ms_per_launch"], 1e-9)
    del keep
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Score tracer events (gsim_score_tracer_*, include/gsim.h): peerScore's
RawTracer surface driven from outside.  The expectation is the CPU oracle's
restatement of the same methods (oracle/oracle.c), one `orc_drecs` per
observer, replayed event by event (`Replay` below); every comparison is bit
for bit."""
import collections
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import REPO
from gsim import _abi, tracer
from gsim.engine import Engine, GsimError, Network
from gsim.params import Millisecond, PeerScoreParams, PeerScoreThresholds, Second, TopicScoreParams
from peerscore_harness import T0 as PS_T0
from peerscore_harness import PeerScore, star_network

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")
CASES = json.load(open(GOLDEN))["cases"]
MY = "mytopic"
STATE_FIELDS = ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags", "bp", "estate", "expire")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


# ---- the oracle replay -----------------------------------------------------------

class Replay:
    """The expectation: the oracle's function of the same name for each event
    in turn, one `orc_drecs` per observer, on a NetState of any network.  A
    Python shadow of the delivery records (status, peers, times) only counts
    which branches a stream took and what `tracer_stats` must report; the
    numbers come from the oracle."""

    def __init__(self, st, ttl=0):
        self.st, self.lib, self.v = st, ob.load(), st.view()
        self.ttl = int(ttl) if ttl else 120 * Second
        self.drecs = {}
        self.shadow = {}              # (observer, mid) -> [status, peers (edges), validated, expire], in creation order
        self.branches = collections.Counter()
        self.applied = self.collected = 0
        self.refreshed = False        # a refresh ran since the replay began
        self.pending = set()          # (topic, edge) records with pending mcnt increments on the engine
        self.touched = set()          # observers whose records an event may have settled
        net = st.net
        self.rp, self.col = net.row_ptr.astype(np.int64), net.col
        self.tp = [st.params.Topics.get(name) for name in st.topics]

    def close(self):
        for d in self.drecs.values():
            self.lib.orc_drecs_free(d)
        self.drecs = {}

    def edge(self, o, p):
        lo, hi = self.rp[o], self.rp[o + 1]
        k = lo + int(np.searchsorted(self.col[lo:hi], p))
        assert k < hi and self.col[k] == p, f"{p} is no connection of {o}"
        return int(k)

    def _drec(self, o):
        if o not in self.drecs:
            self.drecs[o] = self.lib.orc_drecs_new(self.ttl)
        return self.drecs[o]

    def _rec(self, o, mid, now):
        r = self.shadow.get((o, mid))
        if r is None:
            r = self.shadow[(o, mid)] = [0, set(), 0, now + self.ttl]
        return r

    def apply(self, events):
        for (mid, now, o, p, arg, t, kind, _pad) in np.asarray(events).tolist():
            self.one(mid, now, o, p, arg, t, kind)

    def one(self, mid, now, o, p, arg, t, kind):
        lib, v, st, B = self.lib, self.v, self.st, self.branches
        e = self.edge(o, p)
        self.applied += 1
        if kind == tracer.EV_ADD_PENALTY:
            lib.orc_add_penalty(v, e, arg)
            return
        tp = self.tp[t]
        tracked = bool(st.estate[e] & _abi.ES_TRACKED)
        live = tracked and tp is not None
        if kind != tracer.EV_VALIDATE:
            B["untracked"] += not tracked
            B["unscored"] += tp is None
        if kind == tracer.EV_GRAFT:
            B["graft_after_refresh"] += live and self.refreshed
            lib.orc_graft(v, e, t, now)
            return
        if kind == tracer.EV_PRUNE:
            if (live and (st.tflags[t, e] & _abi.TF_ACTIVE) and st.meshd[t, e] < tp.MeshMessageDeliveriesThreshold
                    and (t, e) in self.pending and o not in self.touched):
                B["prune_deficit_pending"] += 1
            self.touched.add(o)
            lib.orc_prune(v, e, t)
            return
        d = self._drec(o)
        in_mesh = live and bool(st.tflags[t, e] & _abi.TF_IN_MESH)
        if kind == tracer.EV_VALIDATE:
            self._rec(o, mid, now)
            lib.orc_validate_message(v, d, mid, now)
            return
        self.touched.add(o)
        if kind == tracer.EV_DELIVER:
            r = self._rec(o, mid, now)
            if r[0] == 0:
                B["valid_with_pending"] += bool(r[1] - {e})
                r[0], r[2] = 1, now
            lib.orc_deliver_message(v, d, e, mid, t, now)
            B["first_cap"] += live and st.first[t, e] == tp.FirstMessageDeliveriesCap
            B["mesh_cap"] += in_mesh and st.meshd[t, e] == tp.MeshMessageDeliveriesCap
        elif kind == tracer.EV_REJECT:
            if arg in (tracer.REJECT_VALIDATION_THROTTLED, tracer.REJECT_VALIDATION_FAILED,
                       tracer.REJECT_VALIDATION_IGNORED):
                r = self._rec(o, mid, now)
                if r[0] == 0:
                    B["reject_with_pending"] += arg == tracer.REJECT_VALIDATION_FAILED and bool(r[1])
                    r[0] = {tracer.REJECT_VALIDATION_FAILED: 2, tracer.REJECT_VALIDATION_IGNORED: 3,
                            tracer.REJECT_VALIDATION_THROTTLED: 4}[arg]
                    r[1] = set()
            lib.orc_reject_message(v, d, e, mid, t, arg, now)
        else:
            assert kind == tracer.EV_DUPLICATE
            r = self._rec(o, mid, now)
            if e in r[1]:
                B["dedupe"] += 1
            elif r[0] == 0:
                r[1].add(e)
            elif r[0] == 1:
                r[1].add(e)
                if in_mesh:
                    dt = now - r[2]
                    B["window_miss"] += dt > tp.MeshMessageDeliveriesWindow
                    B["window_edge"] += dt == tp.MeshMessageDeliveriesWindow
            lib.orc_duplicate_message(v, d, e, mid, t, now)
            B["mesh_cap"] += in_mesh and st.meshd[t, e] == tp.MeshMessageDeliveriesCap

    def gc(self, now):
        for d in self.drecs.values():
            self.lib.orc_drecs_gc(d, now)
        dead = [k for k, r in self.shadow.items() if now > r[3]]
        for k in dead:
            del self.shadow[k]
        self.collected += len(dead)

    def stats(self):
        return {"records": len(self.shadow), "peer_entries": sum(len(r[1]) for r in self.shadow.values()),
                "events": self.applied, "collected": self.collected}


# ---- CPU: layout and the replay helper itself ---------------------------------------

def test_event_layout_matches_c(tmp_path):
    """EVENT_DTYPE and the ctypes struct against sizeof / offsetof of gsim_score_event (a compiled probe)."""
    fields = [f for f, _ in _abi.CScoreEvent._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsim.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsim_score_event));']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof(gsim_score_event, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == 32 == ctypes.sizeof(_abi.CScoreEvent) == tracer.EVENT_DTYPE.itemsize
    for f in fields:
        assert int(got[f]) == getattr(_abi.CScoreEvent, f).offset == tracer.EVENT_DTYPE.fields[f][1], f
    # the header's constants and the builders
    hdr = open(os.path.join(REPO, "include", "gsim.h")).read()
    import re
    for name in ("VALIDATE", "DELIVER", "REJECT", "DUPLICATE", "GRAFT", "PRUNE", "ADD_PENALTY"):
        assert re.search(rf"#define GSIM_EV_{name}\s+{getattr(tracer, 'EV_' + name)}\b", hdr), name
    for name, val in ob_reject_reasons().items():
        assert re.search(rf"#define GSIM_REJECT_{name}\s+{val}\b", hdr) and getattr(tracer, "REJECT_" + name) == val
    row = tracer.batch([tracer.reject(3, 4, 2, 77, tracer.REJECT_SELF_ORIGIN, 99)])[0]
    assert (row["observer"], row["peer"], row["topic"], row["mid"], row["arg"], row["now_ns"], row["kind"]) == \
        (3, 4, 2, 77, 10, 99, tracer.EV_REJECT)


def ob_reject_reasons():
    """oracle.h ORC_REJECT_*: the order of tracer.go:28-38."""
    names = ["BLACKLISTED_PEER", "BLACKLISTED_SOURCE", "MISSING_SIGNATURE", "UNEXPECTED_SIGNATURE",
             "UNEXPECTED_AUTH_INFO", "INVALID_SIGNATURE", "VALIDATION_QUEUE_FULL", "VALIDATION_THROTTLED",
             "VALIDATION_FAILED", "VALIDATION_IGNORED", "SELF_ORIGIN"]
    return {n: i for i, n in enumerate(names)}


def golden_params(case):
    pp = dict(case["peer_params"])
    app = pp.pop("AppSpecificScore", 0.0)
    params = PeerScoreParams(AppSpecificScore=lambda p, v=app: v, **pp)
    if case["topic_params"]:
        params.Topics[MY] = TopicScoreParams(**case["topic_params"])
    return params


class GoldenRun:
    """One golden case on the one-peer star: the oracle through `Replay`, and
    (eng given) the engine through one-event batches."""

    def __init__(self, case, gpu):
        self.case = case
        self.ps = PeerScore(golden_params(case), peers=["A"], extra_topics=[MY])
        self.rp = Replay(self.ps.st)
        self.eng = None
        if gpu:
            self.eng = Engine(self.ps.params, PeerScoreThresholds(), topics=[MY], validate=False)
            self.eng.load_graph(self.ps.net)
            self.eng.tracer_config(256, 256)
            if case["events"][0][0] != "add_peer":
                est = self.eng.read(_abi.F_ESTATE)      # newPeerScore: nobody added yet
                est[0] = 0
                self.eng.write(_abi.F_ESTATE, est)
            self.connected = case["events"][0][0] == "add_peer"
        self.fresh = True
        self.mid = 0

    def event(self, row):
        ev = tracer.batch([row])
        self.rp.apply(ev)
        if self.eng:
            self.eng.tracer_events(ev)

    def score(self):
        want = self.ps.Score("A")
        if self.eng:
            self.eng.compute_scores()
            got = self.eng.scores()[0]
            assert bits(np.float64(got)) == bits(np.float64(want)), (got, want)
        return want

    def run(self):
        ps, now = self.ps, lambda: self.ps.now
        expected = None
        for ev in self.case["events"]:
            op = ev[0]
            if op == "add_peer":
                ps.AddPeer("A")
                if self.eng and not self.connected:     # (else: the state load_graph leaves)
                    self.eng.set_connections([(0, 1)], True, now())
                self.connected = True
            elif op == "remove_peer":
                ps.RemovePeer("A")
                if self.eng:
                    self.eng.set_connections([(0, 1)], False, now())
                self.connected = False
            elif op == "add_penalty":
                self.event(tracer.add_penalty(0, 1, ev[1], now()))
            elif op == "graft":
                self.event(tracer.graft(0, 1, 0, now()))
            elif op == "sleep":
                ps.sleep(ev[1])
            elif op in ("refresh", "refresh_n"):
                for _ in range(ev[1] if op == "refresh_n" else 1):
                    ps.refreshScores()
                    if self.eng:
                        self.eng.refresh_scores(now())
            elif op == "deliver_first":
                for _ in range(ev[1]):
                    self.event(tracer.validate(0, 1, 0, self.mid, now()))
                    self.event(tracer.deliver(0, 1, 0, self.mid, now()))
                    self.mid += 1
            elif op == "expect":
                expected = float(ev[1])
                assert self.score() == expected, f"{self.case['source']}: after {ev}"
            elif op == "expect_mul":
                expected = 1.0
                for f in ev[1]:
                    expected *= f
                assert self.score() == expected, f"{self.case['source']}: after {ev}"
            elif op == "expect_scale":
                for _ in range(ev[2]):
                    expected *= ev[1]
                assert self.score() == expected, f"{self.case['source']}: after {ev}"
            else:
                raise AssertionError(f"unknown event {op}")
        self.rp.close()
        if self.eng:
            self.eng.close()


@pytest.mark.parametrize("name", ["first_message_deliveries", "first_message_deliveries_cap",
                                  "first_message_deliveries_decay"])
def test_replay_helper_reproduces_golden_literals(name):
    """The replay helper alone (events through `Replay`, no device) gives the
    reference's literals: the expectation is pinned before it judges the GPU."""
    GoldenRun(next(c for c in CASES if c["name"] == name), gpu=False).run()


def test_from_trace_orders_and_maps():
    """from_trace on records in gsim_trace_read's order (REJECT and DUPLICATE
    before DELIVER within a timestamp): per (timestamp, router, message) the
    first reception precedes its duplicates, a first reception is Validate +
    Deliver / Reject with the verdict's reason, a bad signature gets no
    Validate, GRAFT / PRUNE follow the messages of their timestamp, the other
    trace types carry nothing."""
    rows = [
        # ts, msg_id, router, other, topic, type, reason -- sorted as gsim_trace_read sorts
        (100, 0, 1, 9, -1, _abi.TRACE_ADD_PEER, 0),
        (100, 0, 1, 4, 2, _abi.TRACE_GRAFT, 0),
        (200, 7, 1, 3, 2, _abi.TRACE_REJECT_MESSAGE, 1),        # a rejected first reception
        (200, 5, 1, 2, 2, _abi.TRACE_DUPLICATE_MESSAGE, 0),     # message 5's duplicates sort before its DELIVER
        (200, 5, 1, 3, 2, _abi.TRACE_DUPLICATE_MESSAGE, 0),
        (200, 7, 1, 4, 2, _abi.TRACE_DUPLICATE_MESSAGE, 0),
        (200, 5, 1, 4, 2, _abi.TRACE_DELIVER_MESSAGE, 0),
        (200, 5, 1, 4, 2, _abi.TRACE_RECV_RPC, 0),
        (200, 0, 1, 2, 2, _abi.TRACE_PRUNE, 0),
        (200, 5, 2, 1, 2, _abi.TRACE_PUBLISH_MESSAGE, 0),
        (200, 6, 2, 1, 0, _abi.TRACE_REJECT_MESSAGE, 2),
        (200, 8, 2, 1, 0, _abi.TRACE_REJECT_MESSAGE, 3),
        (200, 9, 2, 1, 0, _abi.TRACE_REJECT_MESSAGE, 4),        # bad signature: never validated
        (200, 6, 2, 3, 0, _abi.TRACE_DUPLICATE_MESSAGE, 0),
        (300, 5, 1, 2, 2, _abi.TRACE_DUPLICATE_MESSAGE, 0),
        (300, 0, 1, 0, 2, _abi.TRACE_JOIN, 0),
    ]
    tr = np.zeros(len(rows), dtype=Engine.TRACE_DTYPE)
    for q, (ts, mid, a, b, t, ty, rs) in enumerate(rows):
        tr[q] = (ts, mid, a, b, t, ty, rs, 0)
    assert np.array_equal(np.lexsort((tr["msg_id"], tr["topic"], tr["reason"], tr["other"], tr["type"], tr["peer"],
                                      tr["timestamp"])), np.arange(len(tr)))        # (the order a read gives)
    ev = tracer.from_trace(tr)
    assert ev.dtype == tracer.EVENT_DTYPE
    got = [(int(x["now_ns"]), int(x["observer"]), int(x["kind"]), int(x["peer"]), int(x["topic"]), int(x["mid"]),
            int(x["arg"])) for x in ev]
    V, D, R, U, G, P = (tracer.EV_VALIDATE, tracer.EV_DELIVER, tracer.EV_REJECT, tracer.EV_DUPLICATE, tracer.EV_GRAFT,
                        tracer.EV_PRUNE)
    assert got == [
        (100, 1, G, 4, 2, 0, 0),
        (200, 1, V, 3, 2, 7, 0), (200, 1, R, 3, 2, 7, tracer.REJECT_VALIDATION_FAILED),
        (200, 1, V, 4, 2, 5, 0), (200, 1, D, 4, 2, 5, 0),
        (200, 1, U, 2, 2, 5, 0), (200, 1, U, 3, 2, 5, 0), (200, 1, U, 4, 2, 7, 0),
        (200, 1, P, 2, 2, 0, 0),
        (200, 2, V, 1, 0, 6, 0), (200, 2, R, 1, 0, 6, tracer.REJECT_VALIDATION_IGNORED),
        (200, 2, V, 1, 0, 8, 0), (200, 2, R, 1, 0, 8, tracer.REJECT_VALIDATION_THROTTLED),
        (200, 2, R, 1, 0, 9, tracer.REJECT_INVALID_SIGNATURE),
        (200, 2, U, 3, 0, 6, 0),
        (300, 1, U, 2, 2, 5, 0),
    ]
    # the contract, stated on the output: per (timestamp, router, message) no duplicate before the first reception
    seen = set()
    for (ts, o, k, p, t, mid, arg) in got:
        if k in (D, R):
            seen.add((ts, o, mid))
        if k == U and any(g[:2] == (ts, o) and g[5] == mid and g[2] in (D, R) for g in got):
            assert (ts, o, mid) in seen
    # per-observer times never go back (what gsim_score_tracer_events requires)
    for o in (1, 2):
        ts = [g[0] for g in got if g[1] == o]
        assert ts == sorted(ts)
    assert len(tracer.from_trace(tr[:0])) == 0
    bad = tr[2:3].copy()
    bad["reason"] = 9
    with pytest.raises(ValueError, match="unknown verdict 9"):
        tracer.from_trace(bad)


# ---- GPU 1: the reference literals, event by event ------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gpu_reference_kat_through_events(require_gpu, case):
    GoldenRun(case, gpu=True).run()


# ---- GPU 2: record states and reject reasons on the four-peer star ---------------------

class StarPair:
    """peerScore on the star (observer 0; A, B, C, D = peers 1..4), oracle and engine side by side."""

    def __init__(self, params, topics, ttl=0, sub0=None, cfg=(256, 256)):
        self.ps = PeerScore(params, peers=["A", "B", "C", "D"], extra_topics=topics, seen_ttl=0)
        ps = self.ps
        if sub0 is not None:
            ps.net.sub[0] = sub0
        for p in ps.peers:
            ps.AddPeer(p)                       # the state load_graph leaves
        self.rp = Replay(ps.st, ttl)
        self.eng = Engine(params, PeerScoreThresholds(), topics=ps.topics, validate=False)
        self.eng.load_graph(ps.net)
        if cfg:
            self.eng.tracer_config(cfg[0], cfg[1], ttl)
        self.m = len(ps.peers)

    def peer(self, name):
        return 1 + self.ps.peers.index(name)

    def send(self, rows):
        ev = tracer.batch(rows)
        self.rp.apply(ev)
        self.eng.tracer_events(ev)

    def refresh(self, now):
        self.ps.lib.orc_refresh_scores(self.ps.v, now)
        self.eng.refresh_scores(now)
        self.rp.refreshed = True

    def gc(self, now):
        self.rp.gc(now)
        self.eng.tracer_gc(now)

    def planes(self):
        fid = ob.NetState.FIELD_IDS
        return {f: self.eng.read(fid[f]) for f in STATE_FIELDS}

    def check(self, what=""):
        m, st = self.m, self.ps.st
        for f, got in self.planes().items():
            want = getattr(st, f)
            assert np.array_equal(bits(got[..., :m]), bits(want[..., :m])), (what, f, got[..., :m], want[..., :m])
            if f != "estate":                   # (the peers' own rows hold no events)
                assert not got[..., m:].any(), (what, f)
        self.eng.compute_scores()
        live = self.eng.scores()
        for q, p in enumerate(self.ps.peers):
            assert bits(np.float64(live[q])) == bits(np.float64(self.ps.Score(p))), (what, p)
        assert self.eng.tracer_stats() == self.rp.stats(), what

    def close(self):
        self.rp.close()
        self.eng.close()


def star_topic(**over):
    kw = dict(TopicWeight=1, TimeInMeshQuantum=Second, TimeInMeshWeight=0.01, TimeInMeshCap=10,
              FirstMessageDeliveriesWeight=1, FirstMessageDeliveriesDecay=0.9, FirstMessageDeliveriesCap=3,
              MeshMessageDeliveriesWeight=-1, MeshMessageDeliveriesDecay=0.9, MeshMessageDeliveriesCap=5,
              MeshMessageDeliveriesThreshold=4, MeshMessageDeliveriesActivation=Second,
              MeshMessageDeliveriesWindow=10 * Millisecond, MeshFailurePenaltyWeight=-1,
              MeshFailurePenaltyDecay=0.9, InvalidMessageDeliveriesWeight=-1, InvalidMessageDeliveriesDecay=0.9)
    kw.update(over)
    return TopicScoreParams(**kw)


@pytest.mark.gpu
def test_gpu_record_states_and_reject_reasons(require_gpu):
    """TestScoreRejectMessageDeliveries restated (the records are collected by
    a gc past their TTL where the Go test rewinds the head's expiry), every
    reject reason, a duplicate in each of the five record states, the same
    duplicate twice, Deliver and Reject with pending peers, a Graft timed
    before the last refresh: after every event every plane, the live score
    and the record counts equal the oracle's."""
    ttl = 50 * Millisecond
    params = PeerScoreParams(AppSpecificScore=lambda p: 0.0, DecayInterval=Second, DecayToZero=0.01,
                             BehaviourPenaltyWeight=-1, BehaviourPenaltyDecay=0.9, Topics={MY: star_topic()})
    sp = StarPair(params, [], ttl)
    A, B, C, D = (sp.peer(x) for x in "ABCD")
    t = [PS_T0]

    def now(dt=0):
        t[0] += dt
        sp.ps.now = t[0]
        return t[0]

    def step(what, row):
        sp.send([row])
        sp.check(what)

    try:
        for p in (A, B, C):
            step("graft", tracer.graft(0, p, 0, now()))
        sp.refresh(now(2 * Second))                          # meshTime 2 s > activation: the deficit is active
        sp.check("refresh")
        # score_test.go's reject sequence on message 0 (A first, B the duplicate)
        for r in (tracer.REJECT_BLACKLISTED_PEER, tracer.REJECT_BLACKLISTED_SOURCE,
                  tracer.REJECT_VALIDATION_QUEUE_FULL):
            step("silent reasons", tracer.reject(0, A, 0, 0, r, now()))
        for reason in (tracer.REJECT_VALIDATION_THROTTLED, tracer.REJECT_VALIDATION_IGNORED,
                       tracer.REJECT_VALIDATION_FAILED):
            step("validate", tracer.validate(0, A, 0, 0, now()))
            step("reject", tracer.reject(0, A, 0, 0, reason, now()))
            step("duplicate after reject", tracer.duplicate(0, B, 0, 0, now()))     # throttled / ignored / invalid
            step("the same duplicate again", tracer.duplicate(0, B, 0, 0, now()))
            sp.gc(now(ttl + 1))
            sp.check("gc")
            assert sp.rp.stats()["records"] == 0
        step("validate", tracer.validate(0, A, 0, 0, now()))
        step("pending duplicate", tracer.duplicate(0, B, 0, 0, now()))              # unknown
        step("reject with a pending peer", tracer.reject(0, A, 0, 0, tracer.REJECT_VALIDATION_FAILED, now()))
        assert sp.ps.topic_stat("A", MY, "invalid") == 2 and sp.ps.topic_stat("B", MY, "invalid") == 3
        # the signature / origin reasons penalise at once, whatever the record
        for mid, r in enumerate((tracer.REJECT_MISSING_SIGNATURE, tracer.REJECT_UNEXPECTED_SIGNATURE,
                                 tracer.REJECT_UNEXPECTED_AUTH_INFO, tracer.REJECT_INVALID_SIGNATURE,
                                 tracer.REJECT_SELF_ORIGIN), start=10):
            step("signature reasons", tracer.reject(0, C, 0, mid, r, now(1)))
        assert sp.ps.topic_stat("C", MY, "invalid") == 5
        # Deliver with two near-first peers pending (and the first sender's own
        # duplicate): P3 for B and C with no window, A counted once
        step("validate", tracer.validate(0, A, 0, 20, now()))
        for p in (A, B, C, D, B):
            step("pending duplicates", tracer.duplicate(0, p, 0, 20, now(1)))
        before = {p: sp.ps.topic_stat(p, MY, "meshd") for p in "ABCD"}
        step("deliver", tracer.deliver(0, A, 0, 20, now(Second)))                  # far past the window
        after = {p: sp.ps.topic_stat(p, MY, "meshd") for p in "ABCD"}
        assert [after[p] - before[p] for p in "ABCD"] == [1, 1, 1, 0]               # D is not in the mesh
        assert sp.ps.topic_stat("A", MY, "first") == 1
        # duplicates of a valid record: within the window, on it, past it, twice
        step("validate", tracer.validate(0, A, 0, 21, now()))
        step("deliver", tracer.deliver(0, A, 0, 21, now()))
        W = 10 * Millisecond
        step("duplicate on the window", tracer.duplicate(0, B, 0, 21, now(W)))
        assert sp.ps.topic_stat("B", MY, "meshd") == after["B"] + 1
        step("duplicate past the window", tracer.duplicate(0, C, 0, 21, now(1)))
        assert sp.ps.topic_stat("C", MY, "meshd") == after["C"]
        step("the same duplicate again", tracer.duplicate(0, B, 0, 21, now()))
        assert sp.rp.branches["dedupe"] == 2 and sp.rp.branches["window_miss"] == 1 == sp.rp.branches["window_edge"]
        # Reject with three pending peers: all of them and the sender are penalised
        step("validate", tracer.validate(0, D, 0, 22, now()))
        for p in (A, B, C):
            step("pending duplicates", tracer.duplicate(0, p, 0, 22, now()))
        inv = {p: sp.ps.topic_stat(p, MY, "invalid") for p in "ABCD"}
        step("reject", tracer.reject(0, D, 0, 22, tracer.REJECT_VALIDATION_FAILED, now()))
        assert all(sp.ps.topic_stat(p, MY, "invalid") == inv[p] + 1 for p in "ABCD")
        # Prune with an active deficit, AddPenalty, a refresh stamped later
        # than the events that follow it: the Graft's time precedes it
        step("prune", tracer.prune(0, C, 0, now()))
        assert sp.ps.topic_stat("C", MY, "fail") > 0
        step("penalty", tracer.add_penalty(0, D, 3, now()))
        sp.refresh(t[0] + 10 * Second)
        sp.check("refresh ahead of the events")
        step("graft before the last refresh", tracer.graft(0, D, 0, now(1)))
        step("graft", tracer.graft(0, C, 0, now(1)))
        sp.refresh(t[0] + 11 * Second)
        sp.check("refresh")
    finally:
        sp.close()


# ---- GPU 3 / 4: a real network ------------------------------------------------------------

N_PEERS, HUB, T_NET, W_NET = 300, 300, 3, 5 * Millisecond
TOPICS = ["topic00", "topic01", "topic02"]              # topic02 has no score parameters


def hub_network():
    """300 peers on a random 8-regular graph, a hub (peer 300) connected to 200
    of them (its row runs on the hub class), Zipf subscriptions of 2 of 3 topics."""
    from gsim import graphs
    from gsim.engine import random_regular
    rng = np.random.default_rng(4242)
    base = random_regular(N_PEERS, 8, seed=41, n_topics=T_NET)
    src = base.owner().astype(np.int64)
    keep = src < base.col
    others = rng.choice(N_PEERS, size=200, replace=False)
    u = np.concatenate([src[keep], np.full(200, HUB, np.int64)])
    v = np.concatenate([base.col[keep].astype(np.int64), others])
    n = N_PEERS + 1
    row_ptr, col, outbound = graphs._csr_from_pairs(n, u, v)
    sub = graphs.zipf_subscriptions(n, T_NET, 2, seed=43)
    sub[HUB] = 0b111
    assert int(np.diff(row_ptr.astype(np.int64)).max()) == 200
    return Network(n, row_ptr, col, outbound, sub, np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), n)


def hub_params():
    from fixtures import beacon_params, beacon_topic
    params = beacon_params(0, RetainScore=3 * Second)
    for q, name in enumerate(TOPICS[:2]):
        params.Topics[name] = beacon_topic(TopicWeight=0.25 + 0.05 * q, FirstMessageDeliveriesCap=3,
                                           MeshMessageDeliveriesCap=5, MeshMessageDeliveriesThreshold=4,
                                           MeshMessageDeliveriesWindow=W_NET, MeshMessageDeliveriesActivation=Second)
    return params


def hub_state(net, params, th, gp, rng):
    from fixtures import synthetic_state
    from test_heartbeat import tick_time
    from tickrun import restrict_to_subscriptions
    st = ob.NetState(net, params, thresholds=th, gossip=gp, topics=TOPICS)
    synthetic_state(st, rng, tick_time(0), 0.3)
    in_mesh = (st.tflags & _abi.TF_IN_MESH) != 0
    st.first[...] = rng.integers(0, 13, st.first.shape) * 0.25          # within the caps 3 and 5
    st.meshd[...] = np.where(in_mesh, rng.integers(0, 21, st.meshd.shape) * 0.25, 0.0)
    for f in ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags"):
        getattr(st, f)[2] = 0                                            # no topicStats without score parameters
    restrict_to_subscriptions(st, net)
    return st


def lockstep_tick(eng, st, msgs, net, kk, sched, down):
    """One simulated tick on both sides (the call order of tickrun.run_parity),
    nothing read back: the deliveries' mcnt increments stay pending.  Returns
    the records the rounds credited."""
    from test_delivery import R
    from test_heartbeat import SEED, tick_time
    lib, now = ob.load(), tick_time(kk)
    st.churn(down, up=False, now=now - Second // 2)
    eng.set_connections(down, up=False, now=now - Second // 2)
    eng.refresh_scores(now)
    eng.heartbeat(kk, now)
    v = st.view()
    lib.orc_refresh_scores(v, now)
    msgs.penalties(st, now)
    lib.orc_ip_colocation(v)
    lib.orc_compute_scores(v)
    msgs.heartbeat(st, kk, now, SEED)
    before = st.meshd.copy()
    for g in range(kk * R, kk * R + R):
        for (mid, t, o, inv) in sched.get(g, []):
            msgs.publish(st, mid, t, o, inv, g)
        if g in sched:
            eng.publish(sched[g], g)
        msgs.round(st, g)
        eng.round(g)
    return {(int(t), int(e)) for t, e in np.argwhere(st.meshd != before)}


def refresh_both(eng, st, msgs, now):
    lib, v = ob.load(), st.view()
    eng.refresh_scores(now)
    lib.orc_refresh_scores(v, now)
    msgs.penalties(st, now)
    lib.orc_ip_colocation(v)
    lib.orc_compute_scores(v)


def interleave(per_obs, rng):
    """Shuffle across observers, keep each observer's order."""
    rows, keys = [], []
    for evs in per_obs:
        rows.extend(evs)
        keys.append(np.sort(rng.random(len(evs))))
    order = np.argsort(np.concatenate(keys), kind="stable")
    return tracer.batch(rows)[order]


def needs_slot(have, p, t, kind):
    """The event touches a record of a scored topic whose peer holds no slot for
    it: the engine grows the slot masks (ensure_slots) before it applies the batch."""
    return tracer.EV_DELIVER <= kind <= tracer.EV_PRUNE and t < 2 and not (int(have[p]) >> t) & 1


def random_batch(net, st, rng, t_lo, per_observer, skip=(), only=None, have=None):
    """per_observer events of all kinds for every observer, times non-decreasing
    from t_lo, message ids from a pool of 40 per observer (the id fixes the topic).
    have: the slot masks; the events that would grow them are left out."""
    rp = net.row_ptr.astype(np.int64)
    kinds = np.array([tracer.EV_VALIDATE, tracer.EV_DELIVER, tracer.EV_REJECT, tracer.EV_DUPLICATE, tracer.EV_GRAFT,
                      tracer.EV_PRUNE, tracer.EV_ADD_PENALTY])
    out = []
    for o in range(net.n):
        evs = []
        out.append(evs)
        if o in skip or (only is not None and o != only):
            continue
        mine = [t for t in range(T_NET) if (int(net.sub[o]) >> t) & 1]
        n_ev = per_observer if o != HUB else 2 * per_observer
        kk = rng.choice(kinds, size=n_ev, p=[0.08, 0.2, 0.1, 0.42, 0.07, 0.07, 0.06])
        # gaps: mostly within the 5 ms window, some far past it
        gaps = np.where(rng.random(n_ev) < 0.7, rng.integers(0, 2 * Millisecond, n_ev),
                        rng.integers(0, 30 * Millisecond, n_ev))
        times = t_lo + np.cumsum(gaps)
        es = rng.integers(rp[o], rp[o + 1], n_ev)
        ms = rng.integers(0, 40, n_ev)
        rs = rng.integers(0, 11, n_ev)
        for k, now, e, m, r in zip(kk.tolist(), times.tolist(), es.tolist(), ms.tolist(), rs.tolist()):
            p, t, mid = int(net.col[e]), mine[m % len(mine)], o * 1000 + m
            if have is not None and needs_slot(have, p, t, k):
                continue
            if k == tracer.EV_REJECT:
                evs.append(tracer.reject(o, p, t, mid, r, now))
            elif k == tracer.EV_ADD_PENALTY:
                evs.append(tracer.add_penalty(o, p, 1 + r % 3, now))
            elif k in (tracer.EV_GRAFT, tracer.EV_PRUNE):
                evs.append((tracer.graft if k == tracer.EV_GRAFT else tracer.prune)(o, p, t, now))
            else:
                evs.append({tracer.EV_VALIDATE: tracer.validate, tracer.EV_DELIVER: tracer.deliver,
                            tracer.EV_DUPLICATE: tracer.duplicate}[k](o, p, t, mid, now))
    return out


def window_plant(net, st, o, t_lo):
    """On observer o: three mesh peers, a delivery, a duplicate exactly on the
    window (credited) and one a nanosecond past it (not)."""
    t = next(t for t in range(2) if (int(net.sub[o]) >> t) & 1)
    es = [e for e in range(int(net.row_ptr[o]), int(net.row_ptr[o + 1]))
          if st.estate[e] == (_abi.ES_TRACKED | _abi.ES_CONNECTED)][:3]
    p1, p2, p3 = (int(net.col[e]) for e in es)
    mid = o * 1000 + 999
    return [tracer.graft(o, p1, t, t_lo), tracer.graft(o, p2, t, t_lo), tracer.graft(o, p3, t, t_lo),
            tracer.validate(o, p1, t, mid, t_lo), tracer.deliver(o, p1, t, mid, t_lo + 1),
            tracer.duplicate(o, p2, t, mid, t_lo + 1 + W_NET), tracer.duplicate(o, p3, t, mid, t_lo + 2 + W_NET)], es, t


def pending_plants(net, st, pending, t_lo):
    """On records whose meshd the simulated rounds credited (mcnt pending on
    the engine), each first among its observer's events: Prunes on records with
    an active deficit, and first deliveries from mesh peers on others (markFirst
    raises meshd).  One plant per observer: {observer: row}, {observer: row}."""
    owner = net.owner()
    prunes, firsts = {}, {}
    for (t, e) in sorted(pending):
        o = int(owner[e])
        if o in prunes or o in firsts or o == HUB or not (st.estate[e] & _abi.ES_TRACKED):
            continue
        if (st.tflags[t, e] & _abi.TF_ACTIVE) and st.meshd[t, e] < 4 and len(prunes) < 40:
            prunes[o] = tracer.prune(o, int(net.col[e]), t, t_lo)
        elif (st.tflags[t, e] & _abi.TF_IN_MESH) and st.meshd[t, e] < 5:
            firsts[o] = tracer.deliver(o, int(net.col[e]), t, o * 1000 + 997, t_lo)
    return prunes, firsts


@pytest.fixture(scope="module")
def hubnet():
    return hub_network()


def hub_engine(net, params, th, gp, st, cfg):
    from test_heartbeat import SEED
    eng = Engine(params, th, gossip=gp, topics=TOPICS)
    eng.load_graph(net)
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    eng.tracer_config(*cfg)
    return eng


def assert_net_equal(eng, st, net, params, th, gp, what):
    from test_heartbeat import assert_same
    gpu = ob.NetState(net, params, thresholds=th, gossip=gp, topics=TOPICS)
    gpu.pull_from_engine(eng)
    try:
        assert_same(st, gpu)
    except AssertionError as ex:
        raise AssertionError(f"{what}: {ex}") from None


@pytest.mark.gpu
def test_gpu_random_batches_on_a_network(require_gpu, hubnet):
    """One simulated tick in lockstep (a down batch first: retained and
    untracked records; pending mcnt increments left in place), then six
    shuffled batches of about 20 000 events of every kind, a refresh between
    them: every plane and the record counts equal the replay after each."""
    from gsim.params import GossipSubParams
    from test_delivery import R, T0
    from test_heartbeat import tick_time
    from tickrun import subscribed_schedule
    net, params = hubnet, hub_params()
    th = PeerScoreThresholds(GossipThreshold=-20, PublishThreshold=-40, GraylistThreshold=-300)
    gp = GossipSubParams(D=6, Dlo=4, Dhi=10, Dscore=3, Dout=2)
    rng = np.random.default_rng(20240)
    st = hub_state(net, params, th, gp, rng)
    assert net.sub.min() > 0 and (net.sub != 0b111).any()                  # slot planes in use
    eng = hub_engine(net, params, th, gp, st, (1 << 16, 1 << 17, 0))
    rp = Replay(st)
    try:
        eng.msgs_init(256, R, T0, Second)
        msgs = ob.Msgs(net.n, st.T, 256, R, T0, Second)
        sched = subscribed_schedule(rng, [1], net, T_NET, 6.0, 0.0)
        src = net.owner()
        und = np.stack([src, net.col], axis=1)
        und = und[und[:, 0] < und[:, 1]]
        down = und[rng.choice(len(und), size=len(und) // 15, replace=False)]
        rp.pending = lockstep_tick(eng, st, msgs, net, 1, sched, down)
        assert ((st.estate & _abi.ES_CONNECTED) == 0).sum() == 2 * len(down)
        assert (st.estate == _abi.ES_TRACKED).any() and (st.estate == 0).any()      # retained and untracked
        have = net.sub.copy()                       # the slot masks: the announced topics (members publish)
        wo = 7
        for b in range(6):
            t_lo = tick_time(2 + b) + 100 * Millisecond
            if b == 0:
                # the batch that meets the pending mcnt increments grows no slot
                # mask (growing them settles every pending increment first)
                per_obs = random_batch(net, st, rng, t_lo, 76, have=have)
                prunes, firsts = pending_plants(net, st, rp.pending, t_lo)
                assert len(prunes) >= 3 and len(firsts) >= 3
                for o, row in list(prunes.items()) + list(firsts.items()):
                    per_obs[o].insert(0, row)
            else:
                per_obs = random_batch(net, st, rng, t_lo, 65, skip={wo} if b == 1 else ())
            if b == 1:
                per_obs[wo], wes, wt = window_plant(net, st, wo, t_lo)
                w_before = [st.meshd[wt, x] for x in wes]
            ev = interleave(per_obs, rng)
            assert 19000 < len(ev) < 22000, len(ev)
            grow = [(int(p), int(t)) for p, t, k in zip(ev["peer"], ev["topic"], ev["kind"]) if needs_slot(have, p, t, k)]
            for p, t in grow:
                have[p] |= np.uint64(1 << t)
            if b == 0:
                assert not grow
                assert eng.tracer_settled() == (0, True)                  # the engine holds pending increments
            if b == 1:
                assert len(grow) > 100                                       # events from peers without the slot
            rp.apply(ev)
            eng.tracer_events(ev)
            if b == 0:
                # on the device: the planted records' pending counts were non-zero when the events met them
                settled, left = eng.tracer_settled()
                assert settled >= len(prunes) + len(firsts) and left, (settled, len(prunes), len(firsts))
                assert rp.branches["prune_deficit_pending"] == len(prunes)
            assert_net_equal(eng, st, net, params, th, gp, f"batch {b}")
            assert eng.tracer_stats() == rp.stats(), f"batch {b}"
            if b == 1:
                # on the window: credited; a nanosecond past it: not
                assert st.meshd[wt, wes[1]] == min(w_before[1] + 1, 5) and st.meshd[wt, wes[2]] == w_before[2]
            refresh_both(eng, st, msgs, tick_time(3 + b))
            rp.refreshed = True
            assert_net_equal(eng, st, net, params, th, gp, f"refresh {b}")
        B = rp.branches
        for need in ("dedupe", "window_miss", "window_edge", "first_cap", "mesh_cap", "valid_with_pending",
                     "reject_with_pending", "untracked", "unscored", "prune_deficit_pending",
                     "graft_after_refresh"):
            assert B[need] > 0, (need, dict(B))
    finally:
        rp.close()
        eng.close()


@pytest.mark.gpu
def test_gpu_one_heavy_observer(require_gpu, hubnet):
    """The hub receives 5 000 events in one batch, among them one message with
    200 pending duplicates (one per connection) before its Deliver."""
    from gsim.params import GossipSubParams
    from test_heartbeat import tick_time
    net, params = hubnet, hub_params()
    th, gp = PeerScoreThresholds(), GossipSubParams()
    rng = np.random.default_rng(555)
    st = hub_state(net, params, th, gp, rng)
    eng = hub_engine(net, params, th, gp, st, (1 << 13, 1 << 13, 0))
    rp = Replay(st)
    try:
        t_lo = tick_time(1)
        lo, hi = int(net.row_ptr[HUB]), int(net.row_ptr[HUB + 1])
        rows = [tracer.validate(HUB, int(net.col[lo]), 0, 7777, t_lo)]
        rows += [tracer.duplicate(HUB, int(net.col[e]), 0, 7777, t_lo + 1 + (e - lo)) for e in range(lo, hi)]
        rows.append(tracer.deliver(HUB, int(net.col[lo + 5]), 0, 7777, t_lo + Second))
        rest = random_batch(net, st, rng, t_lo + Second, (5000 - len(rows)) // 2 + 1, only=HUB)[HUB]
        rows += rest[:5000 - len(rows)]
        mesh_before = st.meshd[0, lo:hi].copy()
        ev = tracer.batch(rows)
        assert len(ev) == 5000 and (ev["observer"] == HUB).all()
        rp.apply(ev[:202])
        in_mesh = (st.tflags[0, lo:hi] & _abi.TF_IN_MESH) != 0
        assert in_mesh.sum() > 20 and (st.meshd[0, lo:hi] != mesh_before).sum() > 10     # the list was walked
        rp.apply(ev[202:])
        eng.tracer_events(ev)
        assert_net_equal(eng, st, net, params, th, gp, "hub batch")
        assert eng.tracer_stats() == rp.stats() and rp.stats()["peer_entries"] >= 200
    finally:
        rp.close()
        eng.close()


# ---- GPU 5: capacity and gc ------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_capacity_and_gc(require_gpu):
    ttl = 3 * Second
    params = PeerScoreParams(AppSpecificScore=lambda p: 0.0, DecayInterval=Second, DecayToZero=0.01,
                             Topics={MY: star_topic()})
    sp = StarPair(params, [], ttl, cfg=(64, 4))
    A, B = sp.peer("A"), sp.peer("B")
    t0 = PS_T0
    try:
        sp.send([tracer.graft(0, A, 0, t0), tracer.graft(0, B, 0, t0)])
        rows = [tracer.deliver(0, A, 0, 0, t0)] + [tracer.validate(0, A, 0, mid, t0) for mid in range(1, 64)]
        sp.send(rows)
        sp.check("64 records")
        assert sp.eng.tracer_stats()["records"] == 64
        before = sp.planes()
        more = [tracer.validate(0, A, 0, 100 + k, t0 + 1) for k in range(8)] + [tracer.duplicate(0, B, 0, 0, t0 + 1)]
        for batch in (more[:1], more):                      # a 65th record, in the smallest batch too
            with pytest.raises(GsimError) as ex:
                sp.eng.tracer_events(tracer.batch(batch))
            assert ex.value.rc == _abi.GSIM_ERANGE
            after = sp.planes()
            assert all(np.array_equal(bits(before[f]), bits(after[f])) for f in before)
            assert sp.eng.tracer_stats() == sp.rp.stats()
        sp.gc(t0 + ttl)                                     # now == expire: strict, nothing goes
        assert sp.eng.tracer_stats()["collected"] == 0 == sp.rp.stats()["collected"]
        assert sp.eng.tracer_stats()["records"] == 64
        with pytest.raises(GsimError):
            sp.eng.tracer_events(tracer.batch(more))
        sp.gc(t0 + ttl + 1)
        assert sp.eng.tracer_stats() == sp.rp.stats() and sp.rp.stats()["collected"] == 64
        meshd = sp.ps.topic_stat("B", MY, "meshd")
        sp.send(more)                                       # fits now; id 0 is a fresh record, status unknown
        sp.check("after gc")
        assert sp.ps.topic_stat("B", MY, "meshd") == meshd and sp.rp.stats()["records"] == 9
        # a duplicate of a live valid record does earn the credit (the contrast)
        sp.send([tracer.deliver(0, A, 0, 200, t0 + ttl), tracer.duplicate(0, B, 0, 200, t0 + ttl)])
        sp.check("credit")
        assert sp.ps.topic_stat("B", MY, "meshd") == meshd + 1
        # the peers-list pool (4 entries, 2 in use): a released list's entries come back at the next gc
        t1 = t0 + ttl
        three = [tracer.duplicate(0, p, 0, 300, t1) for p in (A, B, sp.peer("C"))]
        with pytest.raises(GsimError) as ex:
            sp.eng.tracer_events(tracer.batch(three))
        assert ex.value.rc == _abi.GSIM_ERANGE and sp.eng.tracer_stats() == sp.rp.stats()
        sp.send(three[:2])
        sp.send([tracer.reject(0, A, 0, 300, tracer.REJECT_VALIDATION_FAILED, t1)])     # releases the two
        sp.check("released")
        assert sp.rp.stats()["peer_entries"] == 2
        with pytest.raises(GsimError):
            sp.eng.tracer_events(tracer.batch(three[2:]))
        sp.gc(t1)                                          # collects nothing, compacts the pool
        assert sp.rp.stats()["collected"] == 64
        sp.send([tracer.duplicate(0, A, 0, 301, t1), tracer.duplicate(0, B, 0, 301, t1)])
        sp.check("pool after gc")
    finally:
        sp.close()


# ---- GPU 6: refusals ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_refusals(require_gpu):
    params = PeerScoreParams(AppSpecificScore=lambda p: 0.0, DecayInterval=Second, DecayToZero=0.01,
                             Topics={MY: star_topic(), "other": star_topic()})
    sp = StarPair(params, [], 0, sub0=0b01, cfg=None)          # the observer announced only topic 0 ("mytopic")
    A, B = sp.peer("A"), sp.peer("B")
    t0 = PS_T0
    eng = sp.eng
    try:
        assert sp.ps.topics == [MY, "other"]
        with pytest.raises(GsimError) as ex:
            eng.tracer_events(tracer.batch([tracer.graft(0, A, 0, t0)]))
        assert ex.value.rc == _abi.GSIM_ESTATE
        for call in (lambda: eng.tracer_gc(t0), eng.tracer_stats):
            with pytest.raises(GsimError) as ex:
                call()
            assert ex.value.rc == _abi.GSIM_ESTATE
        eng.tracer_config(64, 64)
        good = [tracer.graft(0, A, 0, t0), tracer.validate(0, A, 0, 1, t0 + 5), tracer.deliver(0, A, 0, 1, t0 + 5),
                tracer.duplicate(0, B, 0, 1, t0 + 6)]
        sp.send(good)
        sp.check("good")
        before, stats = sp.planes(), eng.tracer_stats()
        ok = tracer.duplicate(0, B, 0, 2, t0 + 7)
        bad_kind = list(tracer.validate(0, A, 0, 3, t0 + 7))
        bad_kind[6] = 7
        bad = {
            "unknown kind": tuple(bad_kind),
            "reject reason": tracer.reject(0, A, 0, 3, 11, t0 + 7),
            "observer out of range": tracer.validate(5, A, 0, 3, t0 + 7),
            "peer out of range": tracer.validate(0, 5, 0, 3, t0 + 7),
            "not a connection": tracer.validate(A, B, 0, 3, t0 + 7),
            "topic out of range": tracer.graft(0, A, 2, t0 + 7),
            "not announced": tracer.deliver(0, A, 1, 3, t0 + 7),
            "time goes backwards": tracer.prune(0, A, 0, t0 + 6),           # within the batch: after `ok` at t0 + 7
        }
        for what, row in bad.items():
            with pytest.raises(ValueError, match=r"^event 2: ") as ex:
                eng.tracer_events(tracer.batch([ok, ok, row, tracer.validate(9, 9, 9, 9, 0)]))
            after = sp.planes()
            assert all(np.array_equal(bits(before[f]), bits(after[f])) for f in before), what
            assert eng.tracer_stats() == stats, what
        # against the observer's last event of an earlier batch (t0 + 6); another observer is free
        with pytest.raises(ValueError, match=r"^event 1: time goes backwards"):
            eng.tracer_events(tracer.batch([tracer.validate(A, 0, 0, 1, t0), tracer.validate(0, A, 0, 3, t0 + 5)]))
        assert eng.tracer_stats() == stats
        # an ADD_PENALTY carries no topic: its topic byte is not checked
        row = list(tracer.add_penalty(0, A, 2, t0 + 6))
        row[5] = 200
        sp.send([tuple(row)])
        sp.check("penalty")
    finally:
        sp.close()


@pytest.mark.gpu
def test_gpu_refused_on_a_shard(require_gpu):
    from fixtures import beacon_params, beacon_thresholds
    from gsim.engine import random_regular
    from gsim.shard import ShardedEngine
    net = random_regular(400, 8, seed=3, n_topics=2)
    grp = ShardedEngine(beacon_params(2), beacon_thresholds(), shards=2)
    try:
        grp.load_graph(net)
        lib, h = grp.lib, grp._shard_handle(0)
        ev = tracer.batch([tracer.graft(0, int(net.col[0]), 0, 1)])
        out = np.zeros(4, dtype=np.int64)
        assert lib.gsim_score_tracer_config(h, 64, 64, 0) == _abi.GSIM_ESTATE
        assert b"shard" in lib.gsim_last_error(h)
        assert lib.gsim_score_tracer_events(h, ev.ctypes.data, 1) == _abi.GSIM_ESTATE
        assert lib.gsim_score_tracer_gc(h, 5) == _abi.GSIM_ESTATE
        assert lib.gsim_score_tracer_stats(h, out.ctypes.data) == _abi.GSIM_ESTATE
    finally:
        grp.close()


# ---- GPU 7: the engine's own trace, replayed ---------------------------------------------------

@pytest.mark.gpu
def test_gpu_replay_of_the_engines_own_trace(require_gpu):
    """A simulated tick traced over all routers (accept and reject verdicts, no
    validation latency), its trace turned into score events by from_trace and
    applied to a fresh engine of the same graph: the counters, the score bits
    and the graft times equal the simulated engine's."""
    from fixtures import beacon_params, beacon_thresholds
    from gsim.engine import random_regular
    from gsim.params import GossipSubParams
    from test_delivery import R, T0
    from test_heartbeat import SEED, tick_time
    from tickrun import subscribed_schedule
    n, T = 400, 2
    net = random_regular(n, 8, seed=77, n_topics=T)
    params, th, gp = beacon_params(T), beacon_thresholds(), GossipSubParams(D=4, Dlo=3, Dhi=6, Dscore=2, Dout=1)
    rng = np.random.default_rng(707)
    # (a rejected message stops at its first receivers: half the messages, to have some dozens of REJECTs)
    sched = subscribed_schedule(rng, [1], net, T, 10.0, 0.0, verdicts=[0.5, 0.5, 0.0, 0.0, 0.0])
    sim = Engine(params, th, gossip=gp)
    rep = Engine(params, th, gossip=gp)
    try:
        sim.load_graph(net)
        sim.set_seed(SEED)
        sim.msgs_init(128, R, T0, Second)
        sim.trace_config(0, n, 1 << 20)
        now = tick_time(1)
        sim.refresh_scores(now)
        sim.heartbeat(1, now)
        for g in range(R, 2 * R):
            if g in sched:
                sim.publish(sched[g], g)
            sim.round(g)
        tr = sim.trace_read()
        ev = tracer.from_trace(tr)
        kinds = np.bincount(ev["kind"], minlength=7)
        assert kinds[tracer.EV_DELIVER] > 1000 and kinds[tracer.EV_REJECT] > 20 and kinds[tracer.EV_DUPLICATE] > 1000, kinds
        assert kinds[tracer.EV_GRAFT] > 500
        rep.load_graph(net)
        rep.tracer_config(1 << 16, 1 << 17)
        rep.tracer_events(ev)
        diff = {}
        for name, fid, mask in (("first", _abi.F_FIRST, None), ("meshd", _abi.F_MESHD, None),
                                ("invalid", _abi.F_INVALID, None), ("fail", _abi.F_FAIL, None),
                                ("tflags", _abi.F_TFLAGS, _abi.TF_IN_MESH | _abi.TF_ACTIVE),
                                ("graft", _abi.F_GRAFT_TIME, None)):
            a, b = sim.read(fid), rep.read(fid)
            if mask is not None:
                a, b = a & mask, b & mask
            bad = np.argwhere(bits(a) != bits(b))
            if len(bad):
                i = tuple(bad[0])
                diff[name] = (len(bad), i, a[i], b[i])
        assert not diff, diff
        assert (sim.read(_abi.F_FIRST) != 0).sum() > 1000 and (sim.read(_abi.F_INVALID) != 0).sum() > 20
    finally:
        sim.close()
        rep.close()

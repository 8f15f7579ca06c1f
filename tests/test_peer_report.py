"""Peer delivery report (gsim_peer_report / gsim_group_peer_report, gsim.report):
per peer and per (topic, class of the receiving peer) the messages expected,
received and missed, the latencies, and the first deliveries by the class of
the first sender, reduced on the device from the seen-set cells.

CPU part: the struct layouts against a C probe, the numpy helpers on
hand-written rows, the host-side merge of the shards' class rows under the
host sanitizers.  GPU part: every expectation comes from the ORACLE alone
(never from the engine's F_SEEN): received, missed, latencies and histograms
from Msgs.seen / .topic / .origin and the oracle network's subscription masks,
first senders from the oracle's event log (every EV_SEEN event with x == 1 is
(peer a, sender b, message mid); b == 0xFFFFFFFF marks an own publication).

With a validation latency the oracle logs a first delivery in the round the
validation completes, while the engine's cell holds the sender from the round
the copy arrived.  A committed cell without an event yet is PENDING: a peer
with a pending cell among the selected messages has its first_from checked by
the invariant sum(first_from) == received - own and by expected <= reported
element-wise; every other peer, and every other field of every peer, is
compared exactly.  Class rows follow the same rule per check point."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

import oracle_binding as ob
from conftest import REPO
from gsim import _abi, report
from gsim.engine import Engine, GsimError, random_regular
from gsim.params import Second
from gsim.presets import beacon_params
from test_delivery import R, T0
from test_heartbeat import SEED, tick_time
from test_msg_report import (GP, TH, VERDICTS, WIDE_RING, WIDE_WINDOWS, compact_case, cycle_network, dense_case,
                             fixed_schedule, lockstep, wide_ring_case)

BINS = _abi.REPORT_BINS
NC = _abi.NET_CLASSES
UNSEEN = _abi.UNSEEN
OWN = 0xFFFFFFFF                      # EV_SEEN's sender of an own publication
PEER_FIELDS = ["expected", "received", "own", "missed", "lat_max", "lat_sum"]
CLASS_FIELDS = ["topic", "cls", "peers", "messages", "expected", "received", "own", "missed", "lat_sum", "lat_max", "hist"]


# ---- CPU ---------------------------------------------------------------------

def test_peer_report_struct_layout_matches_c(tmp_path):
    """sizeof and every offsetof of struct gsim_peer_row (48 bytes) and struct
    gsim_peer_class_row (352) equal the ctypes structs' and the numpy dtypes'."""
    structs = [("gsim_peer_row", _abi.CPeerRow, Engine.PEER_ROW_DTYPE),
               ("gsim_peer_class_row", _abi.CPeerClassRow, Engine.PEER_CLASS_ROW_DTYPE)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsim.h"', "int main(void){",
             'printf("classes %d\\n", GSIM_NET_CLASSES);', 'printf("bins %d\\n", GSIM_REPORT_BINS);']
    for name, py, _ in structs:
        lines.append(f'printf("{name} %zu\\n", sizeof(struct {name}));')
        for fname, _t in py._fields_:
            lines.append(f'printf("{name}.{fname} %zu\\n", offsetof(struct {name}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["classes"]) == NC == 4 and int(got["bins"]) == BINS == 32
    for name, py, dt in structs:
        assert int(got[name]) == ctypes.sizeof(py) == dt.itemsize, name
        for fname, _t in py._fields_:
            assert int(got[f"{name}.{fname}"]) == getattr(py, fname).offset == dt.fields[fname][1], (name, fname)
    assert int(got["gsim_peer_row"]) == 48 and int(got["gsim_peer_class_row"]) == 352
    assert int(got["gsim_peer_row.first_from"]) == 32 and int(got["gsim_peer_row.lat_sum"]) == 24
    assert int(got["gsim_peer_class_row.first_from"]) == 64 and int(got["gsim_peer_class_row.hist"]) == 96


def test_peer_report_helpers_on_hand_written_rows():
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # zero denominators raise no warning
        rows = np.zeros(5, dtype=Engine.PEER_ROW_DTYPE)
        rows["expected"] = [10, 8, 0, 4, 6]
        rows["missed"] = [0, 6, 0, 4, 3]
        rows["received"] = [10, 2, 3, 0, 3]                     # row 2: cells of a topic it does not announce
        rows["own"] = [1, 0, 3, 0, 0]
        rows["first_from"] = [[6, 3, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]
        ratio = report.delivery_ratio(rows)
        assert ratio[0] == 1.0 and ratio[1] == 0.25 and np.isnan(ratio[2]) and ratio[3] == 0.0 and ratio[4] == 0.5
        assert report.starved(rows, 0.5).tolist() == [1, 3]      # nothing expected: never starved
        assert report.starved(rows, 0.0).tolist() == [] and report.starved(rows, 1.01).tolist() == [0, 1, 3, 4]
        share = report.source_share(rows)
        assert share.shape == (5, NC)
        assert share[0].tolist() == [6 / 9, 3 / 9, 0.0, 0.0] and share[1].tolist() == [0.0, 1.0, 0.0, 0.0]
        assert np.isnan(share[2]).all() and np.isnan(share[3]).all()
        assert np.allclose(share[4], [1 / 3, 1 / 3, 1 / 3, 0.0])
        assert len(report.delivery_ratio(rows[:0])) == 0 and len(report.starved(rows[:0], 0.5)) == 0
        assert report.source_share(rows[:0]).shape == (0, NC)

        cls = np.zeros(4, dtype=Engine.PEER_CLASS_ROW_DTYPE)
        cls["expected"] = [100, 100, 0, 50]
        cls["missed"] = [0, 98, 0, 50]
        for k, hist in enumerate([{0: 1, 1: 9, 2: 30, 3: 40, 4: 20}, {5: 1, 31: 1}, {}, {}]):
            for b, c in hist.items():
                cls[k]["hist"][b] = c
        cls["first_from"][0] = [0, 99, 0, 0]
        cls["first_from"][1] = [1, 0, 0, 1]
        lat, over = report.class_latency_quantile(cls, 0.5)
        assert lat.tolist() == [3, 5, 0, 0] and not over.any()
        lat, over = report.class_latency_quantile(cls, 0.99)
        assert lat.tolist() == [4, BINS - 1, 0, 0] and over.tolist() == [False, True, False, False]
        with pytest.raises(ValueError):
            report.class_latency_quantile(cls, -0.1)
        r2 = report.delivery_ratio(cls)                          # class rows share the fields
        assert r2[0] == 1.0 and r2[1] == 0.02 and np.isnan(r2[2]) and r2[3] == 0.0
        s2 = report.source_share(cls)
        assert s2[0].tolist() == [0.0, 1.0, 0.0, 0.0] and s2[1].tolist() == [0.5, 0.0, 0.0, 0.5] and np.isnan(s2[2]).all()
        lat, over = report.class_latency_quantile(cls[:0], 0.5)
        assert len(lat) == 0 and len(over) == 0


def test_peer_report_merge_under_host_sanitizers(tmp_path):
    """The host-side merge of the shards' class rows (csrc/report_merge.cpp)
    built into a stand-alone program with AddressSanitizer and UBSan and run:
    sums, maxima, disagreeing keys, messages and selected counts refused."""
    exe = tmp_path / "report_merge_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "go-libp2p-pubsub_amd", "csrc"),
                           os.path.join(REPO, "tools", "report_merge_check.cpp"),
                           os.path.join(REPO, "go-libp2p-pubsub_amd", "csrc", "report_merge.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), "peer"], capture_output=True, text=True)
    assert out.returncode == 0 and "peer report merge ok" in out.stdout, out.stdout + out.stderr


# ---- the expectation, from the oracle alone -------------------------------------

class FirstSenders:
    """The oracle's first deliveries, [ring][n]: the sender of every committed
    cell the event log has shown so far (NONE: no event yet, MINE: the peer's
    own publication), kept per slot for the slot's current message."""
    NONE, MINE = -2, -1

    def __init__(self, ring, n):
        self.snd = np.full((ring, n), self.NONE, dtype=np.int64)
        self.row_mid = np.full(ring, -1, dtype=np.int64)
        self.events = 0

    def update(self, msgs):
        ev = msgs.events()
        ev = ev[(ev["kind"] == ob.EV_SEEN) & (ev["x"] == 1)]
        published = msgs.seen[np.arange(len(msgs.origin)), msgs.origin] != UNSEEN
        slot_of = {}
        for m in np.nonzero(published)[0]:
            slot_of.setdefault(int(msgs.mid[m]), int(m))
        for a, b, mid in zip(ev["a"].tolist(), ev["b"].tolist(), ev["mid"].tolist()):
            m = slot_of.get(mid)
            if m is None:
                continue                                         # its slot holds a newer message by now
            if self.row_mid[m] != mid:                           # a reused slot: the new message only
                self.snd[m] = self.NONE
                self.row_mid[m] = mid
            assert self.snd[m, a] == self.NONE, "one first delivery per (message, peer)"
            self.snd[m, a] = self.MINE if b == OWN else b
            self.events += 1
        for m in np.nonzero(published)[0]:                       # a republished slot without an event yet
            if self.row_mid[m] != int(msgs.mid[m]):
                self.snd[m] = self.NONE
                self.row_mid[m] = int(msgs.mid[m])


def expected_peer_report(msgs, st, first, cls, C, lo=0, hi=None):
    """(peer_rows, class_rows, pending[n], selection): the report from the
    oracle's arrays and its first senders; pending marks the peers holding a
    committed cell without an event among the selected messages."""
    seen = msgs.seen.astype(np.int64)
    ring, n = seen.shape
    T = st.T
    cls = np.zeros(n, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    org = msgs.origin.astype(np.int64)
    pub = seen[np.arange(ring), org]
    pick = (pub != UNSEEN) & (pub >= lo)
    if hi is not None:
        pick &= pub < hi
    idx = np.nonzero(pick)[0]
    S = seen[idx]
    committed = S != UNSEEN
    lat = np.where(committed, S - pub[idx, None], 0)
    assert (lat >= 0).all()
    top = msgs.topic[idx].astype(np.int64)
    sub = st.net.sub.astype(np.uint64)
    subbit = ((sub[None, :] >> top[:, None].astype(np.uint64)) & np.uint64(1)).astype(bool)
    mine = committed & (np.arange(n)[None, :] == org[idx][:, None])
    snd = first.snd[idx]
    pending = committed & (snd == FirstSenders.NONE)
    assert ((snd == FirstSenders.MINE) == (mine & ~pending)).all(), "the log's own publications are the origins' cells"
    other = committed & (snd >= 0)
    sc = cls[np.where(snd >= 0, snd, 0)]

    rows = np.zeros(n, dtype=Engine.PEER_ROW_DTYPE)
    rows["expected"] = subbit.sum(axis=0)
    rows["received"] = committed.sum(axis=0)
    rows["own"] = mine.sum(axis=0)
    rows["missed"] = (subbit & ~committed).sum(axis=0)
    rows["lat_sum"] = lat.sum(axis=0)
    rows["lat_max"] = lat.max(axis=0) if len(idx) else 0
    for c in range(NC):
        rows["first_from"][:, c] = (other & (sc == c)).sum(axis=0)

    crow = np.zeros(T * C, dtype=Engine.PEER_CLASS_ROW_DTYPE)
    binned = np.minimum(lat, BINS - 1)
    for t in range(T):
        mt = top == t
        for c in range(C):
            pc = cls == c
            x = crow[t * C + c]
            x["topic"], x["cls"] = t, c
            x["peers"] = int((((sub >> np.uint64(t)) & np.uint64(1)).astype(bool) & pc).sum())
            x["messages"] = int(mt.sum())
            x["expected"] = int(x["peers"]) * int(x["messages"])
            blk = committed[mt][:, pc]
            x["received"] = int(blk.sum())
            x["own"] = int(mine[mt][:, pc].sum())
            x["missed"] = int((subbit & ~committed)[mt][:, pc].sum())
            x["lat_sum"] = int(lat[mt][:, pc].sum())
            x["lat_max"] = int(lat[mt][:, pc].max()) if blk.size else 0
            x["hist"][:] = np.bincount(binned[mt][:, pc][blk], minlength=BINS)
            o = other[mt][:, pc]
            for k in range(NC):
                x["first_from"][k] = int((o & (sc[mt][:, pc] == k)).sum())
    return rows, crow, pending.any(axis=0), dict(idx=idx, committed=committed, pending=pending, snd=snd)


def assert_peer_rows(got, want, pending, where=""):
    assert len(got) == len(want), f"{where}: {len(got)} peer rows, expected {len(want)}"
    for f in PEER_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{where}: peer field {f} differs, first at peer {bad[0]}: {got[f][bad[0]]} vs {want[f][bad[0]]}"
    ff, wf = got["first_from"].astype(np.int64), want["first_from"].astype(np.int64)
    assert (ff.sum(axis=1) == got["received"].astype(np.int64) - got["own"]).all(), f"{where}: sum(first_from) == received - own"
    assert (got["received"].astype(np.int64) + got["missed"] >= got["expected"]).all()
    exact = ~pending
    bad = np.nonzero((ff[exact] != wf[exact]).any(axis=1))[0]
    assert len(bad) == 0, (f"{where}: first_from differs at peer {np.nonzero(exact)[0][bad[0]]}: "
                           f"{ff[exact][bad[0]]} vs {wf[exact][bad[0]]}")
    assert (wf[pending] <= ff[pending]).all(), f"{where}: a pending peer's logged first deliveries exceed the reported ones"


def assert_class_rows(got, want, any_pending, where=""):
    assert len(got) == len(want), f"{where}: {len(got)} class rows, expected {len(want)}"
    for f in CLASS_FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, f"{where}: class field {f} differs, first at {bad[0].tolist()}: {got[f][bad[0][0]]} vs {want[f][bad[0][0]]}"
    ff, wf = got["first_from"].astype(np.int64), want["first_from"].astype(np.int64)
    assert (ff.sum(axis=1) == got["received"].astype(np.int64) - got["own"].astype(np.int64)).all()
    assert (got["hist"].sum(axis=1) == got["received"]).all()
    assert (got["expected"] == got["peers"].astype(np.uint64) * got["messages"].astype(np.uint64)).all()
    if any_pending:
        assert (wf <= ff).all(), f"{where}: logged first deliveries exceed the reported ones"
    else:
        assert (ff == wf).all(), f"{where}: class first_from differs: {ff.tolist()} vs {wf.tolist()}"


def run_with_peer_report(make_engine, net, params, st, ticks, sched, cls=None, after=None, windows=(), **kw):
    """run_parity on an engine of the test's; the oracle's event log runs from
    before the first round and the report is checked after every tick (the
    whole ring, then every round window of `windows`).
    after(kk, eng, got, want, pending, sel): the test's own checks per tick."""
    from tickrun import run_parity
    eng = make_engine()
    eng.load_graph(net)
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    C = 1
    if cls is not None:
        eng.set_peer_classes(cls)
        C = int(np.max(cls)) + 1
    state = {"first": None, "ticks": 0, "pending": []}

    def after_heartbeat(kk, eng_, st_, msgs):
        if state["first"] is None:                               # before the first round
            msgs.log()
            state["first"] = FirstSenders(*msgs.seen.shape)

    def after_tick(kk, st_, msgs):
        first = state["first"]
        first.update(msgs)
        want_p, want_c, pending, sel = expected_peer_report(msgs, st_, first, cls, C)
        got_p, got_c = eng.peer_report()
        assert_peer_rows(got_p, want_p, pending, f"tick {kk}")
        assert_class_rows(got_c, want_c, bool(pending.any()), f"tick {kk}")
        for lo, hi in windows:
            w_p, w_c, w_pending, _ = expected_peer_report(msgs, st_, first, cls, C, lo, hi)
            g_p, g_c = eng.peer_report(lo, hi)
            assert_peer_rows(g_p, w_p, w_pending, f"tick {kk} [{lo}, {hi})")
            assert_class_rows(g_c, w_c, bool(w_pending.any()), f"tick {kk} [{lo}, {hi})")
        state["ticks"] += 1
        state["pending"].append(int(sel["pending"].sum()))
        if after:
            after(kk, eng, (got_p, got_c), (want_p, want_c), pending, sel, msgs)

    msgs, _ = run_parity(net, params, TH, GP, st, ticks, sched, eng=eng, after_heartbeat=after_heartbeat,
                         after_tick=after_tick, **kw)
    assert state["ticks"] == len(ticks) and state["first"].events > 0
    return msgs, state


def three_classes(n):
    """Class 1: a third of the peers; class 2: a small set of about 30."""
    p = np.arange(n)
    cls = np.where(p % 3 == 1, 1, 0).astype(np.uint8)
    cls[p % 33 == 5] = 2
    return cls


# ---- GPU -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1003, 20011])
def test_peer_report_dense_ring(require_gpu, n):
    """Dense ring, odd N (every other slot off the 16-byte grid).  1003 peers in
    three classes, class 2 a small set (sparse (topic, class) rows, more than
    one first_from bin); 20011 peers without classes: the C = 1 path with no
    class gather, and enough peer waves that the slots are not split.  The
    class rows agree with msg_report on the same state."""
    net, params, st, ticks, sched = dense_case(n, 301)
    cls = three_classes(n) if n == 1003 else None
    last = {}

    def after(kk, eng, got, want, pending, sel, msgs):
        assert not pending.any(), "no validation latency: every committed cell has its event"
        launch = eng.peer_report_launch()
        assert launch["messages"] == len(sel["idx"]) and launch["waves"] == (n + 63) // 64
        if n == 20011:
            assert launch["parts"] == 1, "enough peer waves: every lane walks all the slots"
        # consistency with the propagation report on the same state
        rep = eng.msg_report()
        got_c = got[1]
        for t in range(st.T):
            rows = got_c[got_c["topic"] == t]
            mr = rep[rep["topic"] == t]
            assert int(rows["received"].sum()) == int(mr["reached"].astype(np.int64).sum())
            assert (rows["hist"].sum(axis=0) == mr["hist"].astype(np.uint64).sum(axis=0)).all()
            assert int(rows["messages"][0]) == len(mr)
        last["got"], last["want"] = got, want

    run_with_peer_report(lambda: Engine(params, TH, gossip=GP), net, params, st, ticks, sched, cls=cls, after=after, ring=64)
    got_p, got_c = last["got"]
    if n == 1003:
        assert len(got_c) == 2 * 3 and int(got_c["peers"][got_c["cls"] == 2][0]) == int((cls == 2).sum()) < 40
        assert int(last["want"][0]["expected"].sum()) == 24072 and int(last["want"][0]["missed"].sum()) == 13834
        assert ((got_c["first_from"] > 0).sum(axis=1) > 1).any(), "first deliveries from more than one class"
        assert ((got_p["first_from"] > 0).sum(axis=1) > 1).any()
        ratio = report.delivery_ratio(got_p)
        assert len(report.starved(got_p, 0.5)) == int((ratio < 0.5).sum()) > 0
    else:
        assert len(got_c) == 2 and (got_p["first_from"][:, 1:] == 0).all()
    assert (got_p["missed"] > 0).sum() > n // 2


@pytest.mark.gpu
def test_peer_report_member_compacted(require_gpu):
    """Member-compacted sub-rings: topic 3 has 41 members, fewer than a wave,
    every peer sits in 2 of 4 topics; validation latencies 0 and 2, so some
    cells are pending at every tick end (the module docstring's rule)."""
    net, params, st, ticks, sched = compact_case()
    cls = (np.arange(net.n) % 2).astype(np.uint8)
    vd = {m[0]: m[4] for batch in sched.values() for m in batch}
    exact = []

    def after(kk, eng, got, want, pending, sel, msgs):
        mids = msgs.mid[sel["idx"]]
        for k in range(len(sel["idx"])):
            if vd[int(mids[k])] == 2:
                recv = sel["committed"][k]
                exact.append((int((recv & ~pending).sum()), int(recv.sum())))

    msgs, state = run_with_peer_report(lambda: Engine(params, TH, gossip=GP), net, params, st, ticks, sched, cls=cls,
                                       after=after, topic_slots=8)
    assert max(state["pending"]) > 0, "the oracle itself must leave cells pending with vdelay 2"
    # the oracle alone: no cell is pending after tick 1 (its vdelay-2 messages, of 5 and 6
    # receivers, are compared exactly everywhere); after ticks 2 and 3, 233 and 333 peers hold a
    # pending cell and the widest vdelay-2 message is exact for 177 of 403 and 320 of 653 receivers
    assert any(tot >= 5 and 2 * ex > tot for ex, tot in exact), \
        "a vdelay-2 message compared exactly for most of its receivers"
    assert any(tot > 300 and ex > 100 for ex, tot in exact), "and a widely spread one for many of them"
    members3 = int(((net.sub >> np.uint64(3)) & np.uint64(1)).sum())
    assert members3 < 64


@pytest.mark.gpu
def test_peer_report_overflow_bin(require_gpu):
    """The 80-peer cycle: one message walks 40 hops each way, a round per hop:
    latencies past 31, exact lat_max and lat_sum per peer."""
    n = 80
    net = cycle_network(n)
    params = beacon_params(1)
    st = ob.NetState(net, params, thresholds=TH, gossip=GP)
    ticks = [1, 2, 3, 4, 5]
    sched = {R + 2: [(7, 0, 11, 0)]}
    last = {}

    def after(kk, eng, got, want, pending, sel, msgs):
        last["got"] = got

    msgs, _ = run_with_peer_report(lambda: Engine(params, TH, gossip=GP), net, params, st, ticks, sched, after=after, ring=64)
    lat = msgs.seen[7 % 64].astype(np.int64)
    ok = lat != UNSEEN
    lat = np.where(ok, lat - (R + 2), 0)
    assert lat.max() > 31 and (lat >= 31).sum() >= 2, "the oracle's own latencies must reach the overflow bin"
    got_p, got_c = last["got"]
    assert (got_p["lat_max"] == lat).all() and (got_p["lat_sum"] == lat).all() and (got_p["received"] == ok).all()
    assert len(got_c) == 1 and got_c[0]["hist"][31] == (lat >= 31).sum() and got_c[0]["lat_max"] == lat.max()
    assert got_c[0]["lat_sum"] == lat.sum() and got_c[0]["own"] == 1


@pytest.mark.gpu
def test_peer_report_slot_split(require_gpu):
    """Few peers, a large ring: 301 peers are 5 waves, so the launch rule
    splits the selected slots over the grid's second dimension and the parts'
    per-peer sums meet in atomics on the rows."""
    from fixtures import synthetic_state
    rng = np.random.default_rng(11)
    n, T = 301, 2
    net = random_regular(n, 8, seed=12, n_topics=T)
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=TH, gossip=GP)
    synthetic_state(st, rng, tick_time(0), 0.7)
    ticks = [1, 2, 3, 4]
    sched = fixed_schedule(rng, ticks, net, T, 5, verdicts=VERDICTS)
    cls = (np.arange(n) % 3).astype(np.uint8)
    parts = []

    def after(kk, eng, got, want, pending, sel, msgs):
        launch = eng.peer_report_launch()
        assert launch["waves"] == 5 and launch["messages"] == len(sel["idx"])
        parts.append(launch["parts"])
        # the per-peer half alone, and a sub-range, take the same path
        sub_p, none_c = eng.peer_report(peers=(70, 200), classes=False)
        assert len(none_c) == 0 and sub_p.tobytes() == got[0][70:200].tobytes()

    run_with_peer_report(lambda: Engine(params, TH, gossip=GP), net, params, st, ticks, sched, cls=cls, after=after, ring=512)
    assert sum(len(b) for b in sched.values()) == 40
    assert parts[-1] > 1 and parts[0] == 1, f"the slots of the last ticks must be split: {parts}"


@pytest.mark.gpu
def test_peer_report_ring_past_one_selection_pass(require_gpu):
    """A ring of 2048 slots (test_msg_report.wide_ring_case): the whole ring and
    each tick's window select slots below and from 1024 on, so the second
    selection pass appends behind the first's rows and adds to its per-topic
    message counts."""
    net, params, st, ticks, sched = wide_ring_case()
    cls = (np.arange(net.n) % 3).astype(np.uint8)
    seen = []

    def after(kk, eng, got, want, pending, sel, msgs):
        seen.append((sel["idx"].tolist(), got[1]["messages"].tolist()))

    run_with_peer_report(lambda: Engine(params, TH, gossip=GP), net, params, st, ticks, sched, cls=cls, after=after,
                         windows=WIDE_WINDOWS, ring=WIDE_RING)
    idx, messages = seen[-1]
    assert idx == [3, 1023, 1024, 1500, 2047]
    assert messages == [3, 3, 3, 2, 2, 2], "topic 0: ids 3, 2047, 1500; topic 1: ids 1024, 1023"


@pytest.mark.gpu
def test_peer_report_calling_convention(require_gpu):
    from fixtures import synthetic_state
    rng = np.random.default_rng(5)
    n, T, ring = 301, 2, 8
    net = random_regular(n, 6, seed=9, n_topics=T)
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=TH, gossip=GP)
    synthetic_state(st, rng, tick_time(0), 0.7)
    cls = (np.arange(n) % 2).astype(np.uint8)
    eng = Engine(params, TH, gossip=GP)
    try:
        eng.load_graph(net)
        eng.set_seed(SEED)
        st.push_to_engine(eng)
        eng.set_peer_classes(cls)
        lib, big = eng.lib, 1 << 40
        nc, nm = ctypes.c_int64(-1), ctypes.c_int64(-1)
        rc = lib.gsim_peer_report(eng.h, 0, big, 0, n, None, None, 0, ctypes.byref(nc), ctypes.byref(nm))
        assert rc == _abi.GSIM_ESTATE and nc.value == T * 2 and nm.value == 0, "before gsim_msgs_init"
        with pytest.raises(GsimError):
            eng.peer_report()
        eng.msgs_init(ring, R, T0, Second)
        msgs = ob.Msgs(n, T, ring, R, T0, Second)
        msgs.log()
        first = FirstSenders(ring, n)
        got_p, got_c = eng.peer_report()                         # nothing published yet
        assert len(got_p) == n and not got_p["received"].any() and not got_p["expected"].any()
        assert len(got_c) == T * 2 and not got_c["messages"].any() and got_c["peers"].sum() == 2 * n
        # ids 0..7 fill the ring in ticks 1-2; ids 8..11 reuse slots 0..3 in tick 20
        sched = {R + 1: [(0, 0, 5, 0), (1, 1, 17, 1)], R + 4: [(2, 0, 250, 0)], R + 9: [(3, 1, 300, 0), (4, 0, 0, 2)],
                 2 * R: [(5, 1, 99, 0)], 2 * R + 5: [(6, 0, 42, 0), (7, 1, 7, 0)],
                 20 * R + 3: [(8, 1, 200, 0), (9, 0, 150, 0)], 20 * R + 8: [(10, 0, 64, 3), (11, 1, 63, 0)]}

        def check(where, lo=0, hi=None):
            first.update(msgs)
            want_p, want_c, pending, sel = expected_peer_report(msgs, st, first, cls, 2, lo, hi)
            assert not pending.any()
            got_p, got_c = eng.peer_report(lo, hi)
            assert_peer_rows(got_p, want_p, pending, where)
            assert_class_rows(got_c, want_c, False, where)
            return got_p, got_c, sel

        def after_round(g):
            # directly after a round: its claims are committed by the call
            if g % R in (1, 5, 9) or g in sched:
                check(f"round {g}")

        lockstep(eng, st, msgs, list(range(1, 21)), sched, after_round)
        stats = eng.msg_stats()
        full_p, full_c, sel = check("whole ring")
        assert sorted(msgs.mid[sel["idx"]].tolist()) == list(range(4, 12)), "reused slots: the new message only"
        assert int(full_c["messages"][full_c["cls"] == 0].sum()) == ring
        # count-only calls
        for pp, cc, cap in ((None, None, 0), (None, None, 5)):
            nc.value = nm.value = -1
            assert lib.gsim_peer_report(eng.h, 0, big, 0, 0, pp, cc, cap, ctypes.byref(nc), ctypes.byref(nm)) == 0
            assert nc.value == T * 2 and nm.value == ring
        cbuf = np.full(T * 2 * 352, 0xAB, dtype=np.uint8).view(Engine.PEER_CLASS_ROW_DTYPE)
        keep = cbuf.copy()
        nc.value = nm.value = -1
        assert lib.gsim_peer_report(eng.h, 0, big, 0, 0, None, cbuf.ctypes.data, 0, ctypes.byref(nc), ctypes.byref(nm)) == 0
        assert nm.value == ring and cbuf.tobytes() == keep.tobytes(), "class_cap 0 counts"
        pbuf = np.full(n * 48, 0xCD, dtype=np.uint8).view(Engine.PEER_ROW_DTYPE)
        pkeep = pbuf.copy()
        nc.value = nm.value = -1
        rc = lib.gsim_peer_report(eng.h, 0, big, 0, n, pbuf.ctypes.data, cbuf.ctypes.data, T * 2 - 1, ctypes.byref(nc),
                                  ctypes.byref(nm))
        assert rc == _abi.GSIM_ERANGE and nc.value == T * 2 and nm.value == ring, "class cap one short"
        assert cbuf.tobytes() == keep.tobytes() and pbuf.tobytes() == pkeep.tobytes(), "nothing written"
        # peers == NULL: the class rows alone; classes == NULL: the peer rows alone
        only_c = eng.lib.gsim_peer_report(eng.h, 0, big, 0, n, None, cbuf.ctypes.data, T * 2, ctypes.byref(nc), ctypes.byref(nm))
        assert only_c == 0 and cbuf.tobytes() == full_c.tobytes()
        p2, c2 = eng.peer_report(classes=False)
        assert len(c2) == 0 and p2.tobytes() == full_p.tobytes()
        # a sub-range that starts and ends off the wave grid equals the same rows of the full call
        for lo_p, hi_p in ((70, 201), (1, 64), (130, 131), (300, 301), (0, 0), (301, 301)):
            sp, sc_ = eng.peer_report(peers=(lo_p, hi_p))
            assert len(sp) == hi_p - lo_p and sp.tobytes() == full_p[lo_p:hi_p].tobytes(), (lo_p, hi_p)
            assert sc_.tobytes() == full_c.tobytes(), "the class rows cover every peer whatever the range"
            sp2, _ = eng.peer_report(peers=(lo_p, hi_p), classes=False)
            assert sp2.tobytes() == sp.tobytes()
        # invalid ranges
        for lo_p, hi_p in ((-1, 5), (5, 4), (0, n + 1), (n + 1, n + 1)):
            nc.value = nm.value = -1
            rc = lib.gsim_peer_report(eng.h, 0, big, lo_p, hi_p, pbuf.ctypes.data, None, 0, ctypes.byref(nc), ctypes.byref(nm))
            assert rc == _abi.GSIM_EINVAL and pbuf.tobytes() == pkeep.tobytes(), (lo_p, hi_p)
        # the host synchronisations are counted
        syncs = ctypes.c_uint64(0)
        lib.gsim_host_sync_count(ctypes.byref(syncs))
        before = syncs.value
        eng.peer_report()
        lib.gsim_host_sync_count(ctypes.byref(syncs))
        assert syncs.value > before
        # a window of one tick's rounds: exactly that tick's messages; empty windows
        _, c_t2, sel2 = check("tick 2", 2 * R, 3 * R)
        assert sorted(msgs.mid[sel2["idx"]].tolist()) == [5, 6, 7] and int(c_t2["messages"][c_t2["cls"] == 0].sum()) == 3
        _, c_new, sel3 = check("tick 20", 20 * R)
        assert sorted(msgs.mid[sel3["idx"]].tolist()) == [8, 9, 10, 11]
        for lo_r, hi_r in ((3 * R, 20 * R), (5, 5)):
            pe, ce = eng.peer_report(lo_r, hi_r)
            assert not pe["expected"].any() and not pe["received"].any() and not ce["messages"].any()
            assert (ce["peers"] == full_c["peers"]).all()
        assert eng.msg_stats() == stats == msgs.stats, "the report changes no state"
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("case", ["dense", "compact"])
def test_peer_report_sharded(require_gpu, case, shards):
    """gsim_group_peer_report over in-process shards equals the single-engine
    expectation: every shard reports the peers it owns, per-peer rows come back
    in global ids, classes are set through gsim_group_set_peer_classes, and a
    first sender owned by another shard counts under its class."""
    from gsim.shard import ShardedEngine
    if case == "dense":
        net, params, st, ticks, sched = dense_case(1003, 301)
        kw = dict(ring=64)
        cls = three_classes(net.n)
    else:
        net, params, st, ticks, sched = compact_case()
        kw = dict(topic_slots=8)
        cls = (np.arange(net.n) % 2).astype(np.uint8)
    made = []
    crossed = []

    def make():
        made.append(ShardedEngine(params, TH, gossip=GP, shards=shards))
        return made[0]

    def after(kk, eng, got, want, pending, sel, msgs):
        bounds = np.asarray(eng.bounds)
        snd = sel["snd"]
        k, p = np.nonzero(snd >= 0)
        sp = np.searchsorted(bounds, p, side="right")
        ss = np.searchsorted(bounds, snd[k, p], side="right")
        cross = (sp != ss) & (cls[p] != cls[snd[k, p]])
        crossed.append(int(cross.sum()))
        if cross.any():                                          # a victim whose first sender another shard owns
            v = int(p[np.nonzero(cross)[0][0]])
            if not pending[v]:
                assert (got[0][v]["first_from"] == want[0][v]["first_from"]).all()
        lo_p, hi_p = int(bounds[1]) - 37, int(bounds[1]) + 29     # a range across a shard boundary
        sub_p, _ = eng.peer_report(peers=(lo_p, hi_p), classes=False)
        assert sub_p.tobytes() == got[0][lo_p:hi_p].tobytes(), "per-peer rows in global ids"

    run_with_peer_report(make, net, params, st, ticks, sched, cls=cls, after=after, **kw)
    assert len(made[0].bounds) == shards + 1 and max(crossed) > 0

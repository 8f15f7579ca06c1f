"""k_send_tm's batched walk: the layer layout issues both peers'
loads together, and an iteration of the copy walk runs in phases over all of a
thread's copies (row state, committed bit, cell, stores).  Every case runs the
bit-exact harness (tickrun.run_parity: engine against oracle per tick, totals,
seen-set, lastput and every state plane) and states, as an assertion on the
oracle's own numbers per round, that the run reached the code it is about."""
import numpy as np
import pytest

import oracle_binding as ob
from gsim import _abi
from gsim.params import GossipSubParams, PeerScoreThresholds, Second

from test_delivery import R
from test_heartbeat import tick_time

K_TM_WIN = 8192          # deliver.hip kTmWin: flattened edges tabled in LDS at once
CHUNK = 1024             # peers per chunk of a dense 512-thread block
PER_IT = 512 * 2         # copies per iteration (threads x GSIM_TM_P)

TH = PeerScoreThresholds(GossipThreshold=-100, PublishThreshold=-200, GraylistThreshold=-300)
GP = GossipSubParams(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2)


def watch_rounds(monkeypatch, fn):
    """Call fn(msgs, st, g, forwarders, stats_before, seen_before) around every oracle
    round g of the harness: forwarders[m, p] = peer p forwards slot m in round g (it
    first saw the slot's valid message in round g - 1)."""
    orig = ob.Msgs.round

    def round_(self, st, g):
        fw = (self.seen == np.uint32(g - 1)) & (self.invalid == 0)[:, None] if g > 0 else np.zeros_like(self.seen, bool)
        before, seen0 = list(self.stats), self.seen.copy()
        orig(self, st, g)
        fn(self, st, g, fw, before, seen0)

    monkeypatch.setattr(ob.Msgs, "round", round_)


def regular_case(n, k, T, seed, gp=GP, th=TH, params=None):
    from fixtures import beacon_params, synthetic_state
    from gsim.engine import random_regular
    rng = np.random.default_rng(seed)
    params = params or beacon_params(T)
    net = random_regular(n, k, seed=seed + 1, n_topics=T)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    synthetic_state(st, rng, tick_time(0), 8 / k)
    return rng, net, params, st


def has_penalised(sched):
    return any(m[3] == _abi.VERDICT_REJECT for b in sched.values() for m in b)


@pytest.mark.gpu
def test_many_iterations_and_shared_cells(require_gpu, monkeypatch):
    """One chunk, one block: 1024 peers of 32 connections, one topic, D = 8, a few
    messages every round.  A round with more than 2048 copies ran at least two full
    iterations with both of a thread's copies valid, and with at most 1024 receivers
    some cell took three copies or more in that round."""
    from tickrun import run_parity, subscribed_schedule
    rng, net, params, st = regular_case(1024, 32, 1, 7)
    ticks = [1, 2]
    sched = subscribed_schedule(rng, ticks, net, 1, 30, 0.1)
    assert has_penalised(sched)
    copies = []
    watch_rounds(monkeypatch, lambda msgs, st_, g, fw, s0, seen0:
                 copies.append(msgs.stats[1] + msgs.stats[2] - s0[1] - s0[2]))
    run_parity(net, params, TH, GP, st, ticks, sched, ring=256)
    print("copies per round:", copies)
    assert max(copies) > 2 * PER_IT, "a round of at least two full iterations"


@pytest.mark.gpu
def test_ragged_ends(require_gpu, monkeypatch):
    """1027 peers: the second chunk holds three, its last thread one valid peer; rounds
    whose copies are no multiple of an iteration's 1024 leave a ragged last iteration
    (the walked edges are the copies and the few edges no copy goes out on)."""
    from tickrun import run_parity, subscribed_schedule
    rng, net, params, st = regular_case(1027, 16, 1, 11)
    ticks = [1, 2]
    sched = subscribed_schedule(rng, ticks, net, 1, 12, 0.1)
    assert has_penalised(sched)
    tail_first, ragged = [], []

    def see(msgs, st_, g, fw, s0, seen0):
        new = (seen0 == ob.UNSEEN) & (msgs.seen != ob.UNSEEN)
        tail_first.append(int(new[:, CHUNK:].sum()))
        c = msgs.stats[1] + msgs.stats[2] - s0[1] - s0[2]
        ragged.append(c > 0 and c % PER_IT != 0)

    watch_rounds(monkeypatch, see)
    run_parity(net, params, TH, GP, st, ticks, sched, ring=256)
    print("first deliveries among peers 1024-1026 per round:", tail_first)
    assert max(tail_first) > 0, "first deliveries among the last chunk's three peers"
    assert any(ragged), "a round whose copies are no multiple of an iteration"


@pytest.mark.gpu
@pytest.mark.parametrize("zipf,topic_slots", [(False, 0), (True, 0), (True, 64)])
def test_hubs_next_to_masked_rows(require_gpu, monkeypatch, zipf, topic_slots):
    """A small power law: rows over 64 connections (hub list or whole row: the second
    trip of the layout) and rows of at most 64 (mesh masks) forward in one chunk of
    one topic in the same round -- every peer subscribed (dense instance), Zipf
    subscriptions (sparse instance: slot masks), and those on sub-rings with
    member-compacted cells (the member tables' trip)."""
    from fixtures import beacon_params, synthetic_state
    from gsim import graphs
    from tickrun import restrict_to_subscriptions, run_parity, subscribed_schedule
    rng = np.random.default_rng(77)
    n, T = 2000, 4
    net = graphs.power_law(n, 16, 2.5, 1024, seed=41, n_topics=T)
    if zipf:
        net = graphs.with_subscriptions(net, graphs.zipf_subscriptions(n, T, 2, seed=42))
    deg = np.diff(net.row_ptr.astype(np.int64))
    assert (deg > 64).sum() > 3 and (deg <= 64).sum() > n // 2, "hubs and short rows present"
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=TH, gossip=GP)
    synthetic_state(st, rng, tick_time(0), 0.3)
    if zipf:
        restrict_to_subscriptions(st, net)
    ticks = [1, 2, 3]
    sched = subscribed_schedule(rng, ticks, net, T, 6.0, 0.1, member_only=True)
    assert has_penalised(sched)
    both = []

    def see(msgs, st_, g, fw, s0, seen0):
        hit = 0
        for m in np.nonzero(fw.any(axis=1))[0]:
            for c0 in range(0, n, CHUNK):
                f = fw[m, c0:c0 + CHUNK]
                d = deg[c0:c0 + CHUNK]
                hit += int((f & (d > 64)).any() and (f & (d <= 64)).any())
        both.append(hit)

    watch_rounds(monkeypatch, see)
    run_parity(net, params, TH, GP, st, ticks, sched, ring=256, topic_slots=topic_slots)
    print("(slot, chunk) pairs per round with a hub and a short row forwarding:", both)
    assert max(both) > 0, "a hub and a short row forward in one chunk in some round"


@pytest.mark.gpu
def test_layer_wider_than_the_sender_window(require_gpu, monkeypatch):
    """The origin of a message is a row of more than 8192 connections: it walks its
    whole row, so its chunk's layer is wider than one sender-table window."""
    from fixtures import beacon_params, synthetic_state
    from test_wide_rows import planted
    from tickrun import run_parity
    rng = np.random.default_rng(8200)
    n, T = 9000, 1
    net = planted(n, T, 5, ((0, 8250),), rng, 64)
    deg = np.diff(net.row_ptr.astype(np.int64))
    assert deg[0] > K_TM_WIN
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=TH, gossip=GP)
    synthetic_state(st, rng, tick_time(0), 0.01)
    ticks = [1]
    g0 = R + 1
    sched = {g0: [(0, 0, 0, 0), (1, 0, 17, 1)], g0 + 2: [(2, 0, 0, 1), (3, 0, 0, 0)]}
    widths = []

    def see(msgs, st_, g, fw, s0, seen0):
        # walk lengths of chunk 0's forwarders: a mesh mask is no longer than its row,
        # the origin's walk is its row
        w = 0
        for m in np.nonzero(fw[:, :CHUNK].any(axis=1))[0]:
            if fw[m, 0] and msgs.origin[m] == 0:
                w = max(w, int(deg[0]))
        widths.append((w, msgs.stats[1] - s0[1]))

    watch_rounds(monkeypatch, see)
    run_parity(net, params, TH, GP, st, ticks, sched, ring=64)
    print("(origin walk length, first deliveries) per round:", widths)
    assert any(w > K_TM_WIN and first > 0 for w, first in widths), "the wide origin forwarded and delivered"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["flood", "direct", "trace", "latency"])
def test_rare_paths_hoisted(require_gpu, monkeypatch, case):
    """The rare paths' loads run as batched steps of their own: flood publish, a
    direct peer outside the mesh, trace on for a few peers, a validation latency of
    two rounds -- each with penalised messages."""
    from tickrun import run_parity, subscribed_schedule
    gp, params, trace, vdelays = GP, None, None, None
    n, k, T = 1500, 16, 2
    if case == "flood":
        gp = GossipSubParams(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2, FloodPublish=True)
    if case == "latency":
        from test_validation_latency import _params
        params = _params(T, 5 * 60 * Second)
        vdelays = (2,)
    rng, net, params, st = regular_case(n, k, T, 23, gp=gp, params=params)
    owner = net.owner()
    if case == "direct":
        und = np.nonzero(owner < net.col)[0]
        pick = und[rng.random(len(und)) < 0.05]
        st.direct[pick] = 1
        st.direct[st.rev[pick]] = 1
    if case == "trace":
        trace = (100, 140)
    ticks = [1, 2, 3]
    sched = subscribed_schedule(rng, ticks, net, T, 8, 0.1, vdelays=vdelays)
    assert has_penalised(sched)
    reached = []

    def see(msgs, st_, g, fw, s0, seen0):
        if case == "direct":
            # a forwarder's direct edge whose mesh bit is off for the slot's topic
            hit = 0
            for m in np.nonzero(fw.any(axis=1))[0]:
                t = int(msgs.topic[m])
                e = (st_.direct != 0) & ((st_.tflags[t] & _abi.TF_MESH) == 0) & fw[m][owner]
                hit += int(e.sum())
            reached.append(hit)
        elif case == "flood":
            # an origin forwards its own message: the flood walk of its row
            reached.append(int(sum(fw[m, int(msgs.origin[m])] for m in np.nonzero(fw.any(axis=1))[0])))
        elif case == "trace":
            reached.append(int(fw[:, trace[0]:trace[1]].sum()))
        else:
            reached.append(msgs.stats[1] - s0[1])

    watch_rounds(monkeypatch, see)
    log = []
    run_parity(net, params, TH, gp, st, ticks, sched, ring=256, trace=trace, trace_log=log if trace else None)
    print(case, "per round:", reached)
    assert sum(reached) > 0, f"{case}: the path ran"
    if case == "trace":
        rpcs = sum(int(c[_abi.TRACE_SEND_RPC] + c[_abi.TRACE_RECV_RPC]) for c, _ in log)
        assert rpcs > 0, "message RPCs of the traced peers were recorded"

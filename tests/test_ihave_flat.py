"""The IHAVE walk's flat push side: in the slot loop of the
instances that are not member-major, the holders of a push slot with rows of
at most 64 connections read their emitGossip choices as bit masks, and the
wave's (holder, target) pairs run one per lane, through a per-wave table of
FLAT_TAB pairs; holders with longer rows keep the lane-group walk.

Every case runs the engine against the oracle tick by tick (tickrun.run_parity:
every state array, the seen-set, the mcache puts and the delivery totals), at
the smallest shapes at which that walk can go wrong.  Where the trace is on,
every IWANT request (receiver, advertiser, message) is compared with the
oracle's log as well, and gossip_stats' ids against their number."""
import numpy as np
import pytest

import oracle_binding as ob
from gsim import _abi
from gsim.params import GossipSubParams, PeerScoreThresholds, Second
from test_delivery import R
from test_heartbeat import tick_time

FLAT_ROW = 64      # kIhFlatRow (deliver.hip): the longest row a mask covers
FLAT_TAB = 256     # kIhFlatTab: pairs in a wave's table
TH = PeerScoreThresholds(GossipThreshold=-20, PublishThreshold=-50, GraylistThreshold=-300)
TICKS = list(range(1, 8))


def _gp(**kw):
    return GossipSubParams(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2, **kw)


def _state(net, T, gp, rng, retained, low_scores=0.0):
    from fixtures import beacon_params, synthetic_state
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=TH, gossip=gp)
    synthetic_state(st, rng, tick_time(0), retained)
    if low_scores:
        st.bp[rng.random(net.e) < low_scores] = 12.0      # the gossip and IWANT gates close on these edges
    return params, st


def _push_pairs(net, st, msgs, kk, gp):
    """From the oracle's state once heartbeat kk ran: per push slot, the
    (holder, target) pairs of each 64-peer word [(slot, word, pairs, holders)],
    with k_gossip_count's holders / wanting receivers and k_ihave's direction
    rule.  (No slot is reused in these runs: a cell is its message's.)"""
    lo = max((kk - gp.HistoryGossip) * R, 0)
    marks = msgs.ihave_marks(net.e)                       # [T][E] at the receivers' edges
    owner, rev = net.owner(), net.rev()
    nwords = (net.n + 63) // 64
    out = []
    for m in np.nonzero((msgs.seen != ob.UNSEEN).any(axis=1))[0]:
        t, seen = int(msgs.topic[m]), msgs.seen[m]
        hold = (seen != ob.UNSEEN) & (seen >= lo) & (seen < kk * R)
        if msgs.invalid[m]:
            hold &= np.arange(net.n) == msgs.origin[m]
        want = (seen == ob.UNSEEN) & (((net.sub >> np.uint64(t)) & np.uint64(1)) != 0)
        nh, nw = int(hold.sum()), int(want.sum())
        if not nh or not nw or not nh * 4 < nw * 32:
            continue
        per_peer = np.bincount(owner, weights=marks[t][rev], minlength=net.n) * hold
        pairs = np.bincount(np.arange(net.n) // 64, weights=per_peer, minlength=nwords)
        holders = np.bincount(np.arange(net.n) // 64, weights=hold, minlength=nwords)
        out += [(int(m), w, int(pairs[w]), int(holders[w])) for w in range(nwords) if holders[w]]
    return out


def _run(net, T, gp, st, params, sched, ring=512, trace=True, eng=None, **kw):
    """run_parity with the trace of every router; returns (gossip_stats,
    IWANT records in the oracle's log, the push words seen per tick)."""
    from tickrun import run_parity
    log, words = [], []

    def after_heartbeat(kk, eng_, st_, msgs):
        words.extend(_push_pairs(net, st_, msgs, kk, gp))

    _, gs = run_parity(net, params, TH, gp, st, TICKS, sched, ring=ring, trace=(0, net.n) if trace else None,
                       trace_log=log, after_heartbeat=after_heartbeat, eng=eng, **kw)
    iwant = int(sum(x[1][2] for x in log))                 # SEND_RPC + RECV_RPC of reason 2, one pair per id
    if trace:
        assert gs["iwant_ids"] * 2 == iwant, "gossip_stats' IWANT ids against the oracle's log"
    print(gs, "IWANT records of the oracle:", iwant, "most pairs in a push word:", max([x[2] for x in words] + [0]))
    return gs, iwant, words


def _assert_gossiped(gs, words):
    assert gs["iwant_ids"] > 0 and gs["iwant_responses"] > 0
    assert any(pairs > 0 for (_, _, pairs, _) in words), "no push slot with a pair: the flat walk did not run"


@pytest.mark.gpu
def test_ragged_ends(require_gpu):
    """n = 1100 (no multiple of 64 or 256), k = 32, T = 3: two holders walk per
    wave group in the parent, the last wave has idle lanes and the last block
    fewer than four waves."""
    from gsim.engine import random_regular
    from test_delivery import _schedule
    n, k, T = 1100, 32, 3
    rng = np.random.default_rng(1100)
    net = random_regular(n, k, seed=n, n_topics=T)
    assert n % 64 and ((n + 63) // 64) % 4
    gp = _gp()
    params, st = _state(net, T, gp, rng, 8 / k, low_scores=0.03)
    sched = _schedule(rng, TICKS, T, R, 4, 0.05, net.n)
    gs, _, words = _run(net, T, gp, st, params, sched)
    _assert_gossiped(gs, words)


@pytest.mark.gpu
def test_mixed_rows_in_one_wave(require_gpu):
    """A power law with rows of up to 300 connections, longest first: masked
    holders (rows of <= 32 and of 33 - 64), group-walk holders (65 - 256 and
    beyond 4 W, whole-wave walks) and peers without a connection share waves,
    and agree with the oracle in the same slots."""
    from gsim import graphs
    from test_delivery import _schedule
    n, T = 3000, 2
    rng = np.random.default_rng(3000)
    net = graphs.power_law(n, 14, 2.5, 300, seed=41, n_topics=T)
    deg = np.diff(net.row_ptr.astype(np.int64))
    # the walk's lane group (ihave_walk's rule): long rows, short mean -> 16
    assert deg.max() > 32 and net.e <= 24 * net.n
    W = 16
    cls = np.where(deg == 0, 0, np.where(deg <= 32, 1, np.where(deg <= FLAT_ROW, 2, np.where(deg <= 256, 3, 4))))
    for c in range(5):
        assert (cls == c).any(), f"row class {c} missing"
    assert (deg > 4 * W).any() and FLAT_ROW >= 4 * W
    # masked and fallback holders in one wave (64 peers)
    word = np.arange(n) // 64
    assert any(((cls[word == w] == 2) | (cls[word == w] == 1)).any() and (cls[word == w] >= 3).any()
               for w in range((n + 63) // 64))
    gp = _gp()
    params, st = _state(net, T, gp, rng, 0.35, low_scores=0.03)
    sched = _schedule(rng, TICKS, T, R, 4, 0.05, n)
    gs, _, words = _run(net, T, gp, st, params, sched)
    _assert_gossiped(gs, words)


@pytest.mark.gpu
def test_many_pairs_per_wave(require_gpu):
    """GossipFactor = 1: every candidate is a target (about 24 a holder), so a
    wave's push slot has hundreds of pairs: several batches, more than one
    window of the table, more responses than the staging holds."""
    from gsim.engine import random_regular
    from test_delivery import _schedule
    n, k, T = 1000, 32, 2
    rng = np.random.default_rng(77)
    net = random_regular(n, k, seed=78, n_topics=T)
    gp = _gp(GossipFactor=1.0)
    params, st = _state(net, T, gp, rng, 8 / k)
    sched = _schedule(rng, TICKS, T, R, 5, 0.0, n)
    gs, _, words = _run(net, T, gp, st, params, sched)
    _assert_gossiped(gs, words)
    most = max(pairs for (_, _, pairs, _) in words)
    assert most > FLAT_TAB, f"no 64-peer word of a push slot with more than {FLAT_TAB} pairs (most: {most})"


@pytest.mark.gpu
def test_no_targets(require_gpu):
    """Dlazy = 0 and GossipFactor = 0: emitGossip chooses nobody, every mask is
    empty and no IWANT is sent; the holders of push slots still count as walks."""
    from gsim.engine import random_regular
    from test_delivery import _schedule
    n, k, T = 1000, 32, 2
    rng = np.random.default_rng(5)
    net = random_regular(n, k, seed=6, n_topics=T)
    gp = _gp(Dlazy=0, GossipFactor=0.0)
    params, st = _state(net, T, gp, rng, 8 / k)
    sched = _schedule(rng, TICKS, T, R, 4, 0.0, n)
    gs, iwant, words = _run(net, T, gp, st, params, sched)
    assert iwant == 0 and gs["iwant_ids"] == 0 and gs["iwant_responses"] == 0
    assert all(pairs == 0 for (_, _, pairs, _) in words)
    assert sum(h for (_, _, _, h) in words) > 0, "no push slot in the run"
    # a holder of a push slot counts as a walk with or without targets (the oracle keeps no such
    # count: the benchmark's output dumps compare it with the lane-group walk's)
    assert gs["ihave_walks"] > 0


@pytest.mark.gpu
def test_gates(require_gpu):
    """IGNORE_IWANT on a third of the peers (no response), bp = 12 on 3 % of the
    edges (gossip and IWANT gates closed in either direction), and a message
    with a bad signature, which only its origin serves (GetForPeer's count)."""
    from gsim.engine import random_regular
    from test_delivery import _schedule
    n, k, T = 1000, 32, 2
    rng = np.random.default_rng(31)
    net = random_regular(n, k, seed=32, n_topics=T)
    gp = _gp()
    params, st = _state(net, T, gp, rng, 8 / k, low_scores=0.03)
    beh = (rng.random(n) < 1 / 3).astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT
    sched = _schedule(rng, TICKS, T, R, 4, 0.0, n)
    g_sig = 2 * R + 7                                      # late in tick 2: few holders at heartbeat 3
    mid = 1 + max(m[0] for b in sched.values() for m in b)
    sched.setdefault(g_sig, []).append((mid, 0, int(np.nonzero(beh == 0)[0][0]), _abi.VERDICT_SIGNATURE))
    gs, _, words = _run(net, T, gp, st, params, sched, behaviour=beh)
    _assert_gossiped(gs, words)
    assert gs["iwant_responses"] < gs["iwant_ids"]


@pytest.mark.gpu
def test_sparse_layout(require_gpu):
    """Zipf subscriptions (3 of 6 topics a peer): a holder's mask comes from its
    own slot plane, and a holder without a plane of the topic has none."""
    from gsim import graphs
    from gsim.engine import random_regular
    from tickrun import restrict_to_subscriptions, subscribed_schedule
    n, k, T = 1000, 32, 6
    rng = np.random.default_rng(61)
    net = random_regular(n, k, seed=62, n_topics=T)
    net = graphs.with_subscriptions(net, graphs.zipf_subscriptions(n, T, 3, seed=63))
    gp = _gp()
    params, st = _state(net, T, gp, rng, 8 / k, low_scores=0.03)
    restrict_to_subscriptions(st, net)
    sched = subscribed_schedule(rng, TICKS, net, T, 4.0, 0.03, member_only=False)
    gs, _, words = _run(net, T, gp, st, params, sched)
    _assert_gossiped(gs, words)


@pytest.mark.gpu
def test_validation_latency(require_gpu):
    """vdelay = 1 on every message: the instance with validation latencies."""
    from gsim.engine import random_regular
    from tickrun import subscribed_schedule
    n, k, T = 1000, 32, 2
    rng = np.random.default_rng(41)
    net = random_regular(n, k, seed=42, n_topics=T)
    gp = _gp()
    params, st = _state(net, T, gp, rng, 8 / k, low_scores=0.03)
    sched = subscribed_schedule(rng, TICKS, net, T, 4.0, 0.03, vdelays=[1])
    gs, _, words = _run(net, T, gp, st, params, sched, trace=False)
    _assert_gossiped(gs, words)


@pytest.mark.gpu
def test_two_shards_agree_with_one_engine(require_gpu):
    """Two in-process shards: receivers are the shard's own peers, holders
    include its ghosts, keys use global ids.  Both the single engine and the
    shards agree with the oracle, and their gossip totals with each other."""
    from gsim.engine import random_regular
    from gsim.shard import ShardedEngine
    from test_delivery import _schedule
    from tickrun import SEED
    n, k, T = 1000, 32, 2
    out = []
    for shards in (0, 2):
        rng = np.random.default_rng(51)
        net = random_regular(n, k, seed=52, n_topics=T)
        gp = _gp()
        params, st = _state(net, T, gp, rng, 8 / k, low_scores=0.03)
        sched = _schedule(rng, TICKS, T, R, 4, 0.05, n)
        eng = None
        if shards:
            eng = ShardedEngine(params, TH, gossip=gp, shards=shards)
            eng.load_graph(net)
            eng.set_seed(SEED)
            st.push_to_engine(eng)
        gs, _, words = _run(net, T, gp, st, params, sched, trace=False, eng=eng)
        _assert_gossiped(gs, words)
        out.append(gs)
    for f in ("iwant_ids", "iwant_responses", "broken_promises"):
        assert out[0][f] == out[1][f], f

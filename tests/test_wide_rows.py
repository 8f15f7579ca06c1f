"""Rows of more than 8192 connections (the reference's heartbeat, fanout
maintenance and makePrune have no degree bound, gossipsub.go:1386-1557,
1558-1596, 1118): the streamed "wide" row class (k_heartbeat_wide,
k_fanout_heartbeat_wide, k_fanout_publish_wide, k_px_emit_wide), one block
walking the row in 1024-position tiles with its state in global scratch.
Bit-exact against the oracle every tick, every plane (tickrun.run_parity).

The network: a power law (rows <= 256) with three planted hubs --
  peer 0      8193 connections: the first row of the wide class
  peer 1      12 001: neither a multiple of 64 nor of the tile, a partial last tile
  peer n - 1  20 000: beyond any doubling of the 8192 class; another shard than 0 and 1
-- dense hub meshes (Dhi prunes over thousands of positions), opportunistic
grafting, PX, sybil IPs on hub neighbours, direct peers of hub 1, Zipf
subscriptions (hub 1 outside topic T - 1: its publications there are fanout).
"""
import numpy as np
import pytest

import oracle_binding as ob
from gsim import _abi
from gsim.params import GossipSubParams, PeerScoreThresholds, Second

from fixtures import planted
from test_heartbeat import tick_time

N, T = 24000, 4
HUBS = ((0, 8193), (1, 12001), (N - 1, 20000))
DHI = 12
_cache = {}


def wide_net():
    """The shared network (built once per session, never modified)."""
    if "net" not in _cache:
        from gsim import graphs
        rng = np.random.default_rng(20000)
        net = planted(N, T, 91, HUBS, rng, 256)
        sub = graphs.zipf_subscriptions(N, T, 2, seed=92)
        sub[0] = sub[N - 1] = (1 << T) - 1                # hubs 0 and n - 1 hold every topic
        sub[1] = (1 << (T - 1)) - 1                       # hub 1 all but the last: a fanout publisher there
        _cache["net"] = graphs.with_subscriptions(net, sub)
    net = _cache["net"]
    deg = np.diff(net.row_ptr.astype(np.int64))
    for hub, d in HUBS:
        assert deg[hub] >= d, f"hub {hub}: {deg[hub]} connections"
    assert deg[0] <= 8192 + 256, "the first wide row sits at the class boundary"
    return net


def setup(net, T_, seed):
    from fixtures import beacon_params, synthetic_state
    from tickrun import restrict_to_subscriptions
    rng = np.random.default_rng(seed)
    params = beacon_params(T_, RetainScore=3 * Second)
    th = PeerScoreThresholds(GossipThreshold=-20, PublishThreshold=-40, GraylistThreshold=-300,
                             AcceptPXThreshold=0.0, OpportunisticGraftThreshold=5)
    gp = GossipSubParams(D=8, Dlo=6, Dhi=DHI, Dscore=4, Dout=2, FanoutTTL=3 * Second, OpportunisticGraftTicks=2,
                         PeerExchange=True)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    synthetic_state(st, rng, tick_time(0), 0.3)           # hub meshes in the thousands: Dhi prunes over them
    restrict_to_subscriptions(st, net)
    return rng, params, th, gp, st


def direct_on_hub1(net, st, rng):
    e = int(net.row_ptr[1]) + rng.choice(int(net.row_ptr[2] - net.row_ptr[1]), size=5, replace=False)
    st.direct[e] = 1
    st.direct[st.rev[e]] = 1                              # WithDirectPeers is mutual here


def schedule(rng, net, ticks, fanout_ticks=()):
    from tickrun import subscribed_schedule
    from test_delivery import R
    sched = subscribed_schedule(rng, ticks, net, T, 1.5, 0.0, member_only=False,
                                verdicts=[0.85, 0.05, 0.04, 0.03, 0.03])
    mid = 1 + max((m[0] for b in sched.values() for m in b), default=0)
    for k in fanout_ticks:                                # hub 1 publishes outside its topics: its fanout
        sched.setdefault(k * R + 2, []).append((mid, T - 1, 1, 0))
        mid += 1
    return sched


def churn_pairs(rng, net, frac):
    src = net.owner()
    und = np.stack([src, net.col], axis=1)
    und = und[und[:, 0] < und[:, 1]]
    down = und[rng.choice(len(und), size=int(len(und) * frac), replace=False)]
    hub_edges = sum(int(((down[:, 0] == h) | (down[:, 1] == h)).sum()) for h, _ in HUBS)
    assert hub_edges > 0, "the churn takes hub connections down"
    return down


def hub_mesh(st, net, hub):
    """Mesh size of the hub's row per topic (router mesh bit, edge order)."""
    lo, hi = int(net.row_ptr[hub]), int(net.row_ptr[hub + 1])
    return ((st.tflags[:, lo:hi] & _abi.TF_MESH) != 0).sum(axis=1)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_wide_rows_bit_exact(require_gpu):
    """Ticks 1-4 with publications of every verdict, hub 1's fanout (created
    at tick 1, maintained and gossiped, published to again at tick 3), 1 % of
    the connections (hub connections among them) down at tick 2 and up at
    tick 4, PX, and the hubs' GRAFT / PRUNE trace events.

    About 25 s, nearly all of it the oracle's tick 1 (the PX lists of the
    ~10 000 PRUNEs that bring the three synthetic hub meshes down to D, each a
    pass over the hub's row): a run of ticks 1-3 measured 23 s, so taking
    ticks out does not shorten it, and the engine's tick is under 0.2 s."""
    from tickrun import run_parity
    net = wide_net()
    rng, params, th, gp, st = setup(net, T, 1)
    direct_on_hub1(net, st, rng)
    ticks = [1, 2, 3, 4]
    sched = schedule(rng, net, ticks, fanout_ticks=(1, 3))
    down = churn_pairs(rng, net, 0.01)
    churn = {2: [(down, False)], 4: [(down, True)]}
    before = {h: hub_mesh(st, net, h) for h, _ in HUBS}
    for h, _ in HUBS:
        assert before[h].max() > DHI, f"hub {h} starts over Dhi"
    seen = {}

    def after_heartbeat(kk, eng, st_, msgs):
        if kk == 1:
            for h, _ in HUBS:
                seen[h] = hub_mesh(st_, net, h)

    def after_tick(kk, st_, msgs):
        if kk == 1:
            seen["fan"] = int(st_.fan_topics[1])

    log = []
    run_parity(net, params, th, gp, st, ticks, sched, ring=1024, churn=churn, px_log=log, trace=(0, 2),
               after_heartbeat=after_heartbeat, after_tick=after_tick)
    print("PX connections per tick:", log, "hub meshes", before, "->", seen)
    for h, _ in HUBS:                                     # the Dhi path ran on every wide row
        over = before[h] > DHI
        assert (seen[h][over] <= DHI).all(), f"hub {h}: {before[h]} -> {seen[h]}"
    assert sum(log) >= 1, "PX made at least one connection"
    assert (seen["fan"] >> (T - 1)) & 1, "hub 1 holds a fanout for the topic it published to"


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_wide_rows_step_and_leave(require_gpu):
    """The one-call tick (gsim_step) on the same network; hub 0 Leaves topic
    1 before tick 3 (PRUNE with PX to its whole mesh, px_leave_list over the
    wide row) and Joins again before tick 4.  About 22 s, most of it the
    oracle's tick 1 (see test_wide_rows_bit_exact).  The Leave is not moved
    earlier: after tick 1 the hub's mesh still holds the 852 outbound GRAFTs it
    accepted, and Leave's PX lists for them, made by one thread like the rest
    of gsim_set_subscriptions, took the test to 60 s."""
    from tickrun import run_parity
    net = wide_net()
    rng, params, th, gp, st = setup(net, T, 2)
    ticks = [1, 2, 3, 4]
    sched = schedule(rng, net, ticks, fanout_ticks=(2,))
    pair = np.array([(0, 1)], dtype=np.uint32)
    subs = {3: [(pair, False)], 4: [(pair, True)]}
    left = []

    def after_tick(kk, st_, msgs):
        if kk in (1, 2):
            left.append(int(hub_mesh(st_, net, 0)[1]))

    run_parity(net, params, th, gp, st, ticks, sched, ring=1024, subs=subs, step=True, after_tick=after_tick)
    print("hub 0's mesh in topic 1 after ticks 1 and 2:", left)
    assert left[1] > 0, "hub 0 had a mesh in the topic it left"


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_wide_rows_two_shards(require_gpu):
    """Two shards: wide rows on both (peers 0 and 1 on the first, n - 1 on the
    second), ghost neighbours, PX lists to the other shard, connections down
    before tick 2 (the PX connector then finds peers to dial) and up before
    tick 3.  About 21 s, as above (ticks 1-2 alone measured 20 s)."""
    from gsim.shard import ShardedEngine
    from tickrun import SEED, run_parity
    net = wide_net()
    rng, params, th, gp, st = setup(net, T, 3)
    direct_on_hub1(net, st, rng)
    eng = ShardedEngine(params, th, gossip=gp, shards=2)
    eng.load_graph(net)
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    ticks = [1, 2, 3]
    sched = schedule(rng, net, ticks, fanout_ticks=(1,))
    down = churn_pairs(rng, net, 0.01)
    churn = {2: [(down, False)], 3: [(down, True)]}
    log = []
    run_parity(net, params, th, gp, st, ticks, sched, ring=1024, churn=churn, px_log=log, eng=eng)
    print("PX connections per tick:", log)
    assert sum(log) >= 1, "PX made at least one connection"


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rows_at_8192_unchanged(require_gpu):
    """The class boundary from both sides: a row of exactly 8192 connections
    (k_heartbeat_hub_g, as before) and one of 8193 (the wide class) in one
    network, two ticks."""
    from gsim import graphs
    from tickrun import run_parity, subscribed_schedule
    n = 10000
    rng = np.random.default_rng(8193)
    net = planted(n, T, 93, ((0, 8192), (1, 8193)), rng, 64, exact=True)
    deg = np.diff(net.row_ptr.astype(np.int64))
    assert deg[0] == 8192 and deg[1] == 8193 and deg[2:].max() <= 8192
    sub = graphs.zipf_subscriptions(n, T, 2, seed=94)
    sub[:2] = (1 << T) - 1
    net = graphs.with_subscriptions(net, sub)
    rng, params, th, gp, st = setup(net, T, 4)
    ticks = [1, 2]
    sched = subscribed_schedule(rng, ticks, net, T, 1.5, 0.0, member_only=False,
                                verdicts=[0.85, 0.05, 0.04, 0.03, 0.03])
    log = []
    run_parity(net, params, th, gp, st, ticks, sched, ring=1024, px_log=log)

"""The heartbeat's steady-state fast path (heartbeat.hip, hb_observer): lane
groups skip a topic's mesh maintenance in one wave-uniform branch when no
group of the wave needs it -- no negative-score mesh peer, Dlo <= mesh <= Dhi,
Dout outbound mesh peers, no opportunistic tick.  Every case runs the engine
against the oracle bit-exact (tickrun.run_parity) and asserts on the oracle's
own state that the clause it is about fired: waves with one group on either
side of the test, waves where every group maintains, each lane width in the
dense and the slot-mask layout, the opportunistic tick, and negative scores
alone."""
import numpy as np
import pytest

import oracle_binding as ob
from gsim import _abi
from gsim.params import GossipSubParams, PeerScoreThresholds, Second

from test_heartbeat import tick_time

MESH = np.uint8(_abi.TF_MESH)


class HeartbeatWatch:
    """run_parity hooks that keep, per tick, the oracle's mesh just before the
    heartbeat, the scores the heartbeat read and the edges it grafted and
    pruned (control is handled in the rounds after it, so the mesh at the
    end of a tick is not the heartbeat's)."""

    def __init__(self, st):
        self.before = (st.tflags & MESH) != 0
        self.mesh, self.score, self.grafted, self.pruned = {}, {}, {}, {}

    def after_heartbeat(self, kk, eng, st, msgs):
        now = (st.tflags & MESH) != 0
        self.mesh[kk] = self.before
        self.score[kk] = st.score.copy()
        self.grafted[kk] = now & ~self.before
        self.pruned[kk] = self.before & ~now

    def after_tick(self, kk, st, msgs):
        self.before = (st.tflags & MESH) != 0


def per_observer(net, x):
    """[T, E] edge values summed over each observer's row: [T, N]."""
    owner = net.owner()
    return np.stack([np.bincount(owner, weights=row, minlength=net.n) for row in x.astype(np.float64)]).astype(np.int64)


def dense_network(n_topics, seed=5):
    from gsim.engine import random_regular
    net = random_regular(512, 32, seed=seed, n_topics=n_topics)
    assert (net.sub == np.uint64((1 << n_topics) - 1)).all(), "every peer joined every topic: the dense layout"
    return net


def beacon_case(net, T, p_mesh, seed, gp=None):
    from fixtures import beacon_params, beacon_thresholds, synthetic_state
    params, th = beacon_params(T), beacon_thresholds()
    gp = gp or GossipSubParams(D=8, Dlo=6, Dhi=12)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    synthetic_state(st, np.random.default_rng(seed), tick_time(0), p_mesh)
    return params, th, gp, st


def run(net, params, th, gp, st, ticks, rate=2.0, seed=1, **kw):
    from tickrun import run_parity, subscribed_schedule
    sched = subscribed_schedule(np.random.default_rng(seed), ticks, net, st.T, rate, 0.02)
    assert {m[1] for b in sched.values() for m in b} == set(range(st.T)), "publications in every topic"
    w = HeartbeatWatch(st)
    run_parity(net, params, th, gp, st, ticks, sched, ring=512, after_heartbeat=w.after_heartbeat,
               after_tick=w.after_tick, **kw)
    return w


@pytest.mark.gpu
def test_mixed_waves_dense(require_gpu):
    """Meshes around D: some (observer, topic) pairs change and most do not,
    and two observers that share a wavefront (rows of 32 connections in
    order: observers 2i and 2i+1) differ in that -- one group of the wave
    maintains its mesh, the other is carried through the same branch
    untouched.  Gossip is on with publications in every topic, so the code
    behind the branch (mesh masks, emitGossip) runs on both paths."""
    T = 16
    net = dense_network(T)
    params, th, gp, st = beacon_case(net, T, 8 / 32, seed=21)
    w = run(net, params, th, gp, st, [1, 2, 3], seed=22)
    split = 0
    for kk in (1, 2, 3):
        changed = per_observer(net, w.grafted[kk] | w.pruned[kk]) > 0       # [T, N]
        assert changed.any() and not changed.all(), f"tick {kk}: pairs that change and pairs that do not"
        split += int((changed[:, 0::2] != changed[:, 1::2]).sum())
    assert not changed.all(axis=0).any() and changed.mean() < 0.5, "the last tick is mostly steady"
    assert split > 0, "a wave with one observer changed and its neighbour not"


@pytest.mark.gpu
@pytest.mark.parametrize("p_mesh,what", [(0.5, "pruned"), (0.05, "grafted")])
def test_every_group_maintains(require_gpu, p_mesh, what):
    """Meshes far over Dhi (p_mesh 0.5: 16 of 32) or under Dlo (0.05): in the
    first tick nearly every group of every wave maintains its mesh (of
    Binomial(32, 0.5) mesh sizes 89 % exceed Dhi = 12, of Binomial(32, 0.05)
    ones 99 % are under Dlo = 6; "most" below is more than half)."""
    T = 16
    net = dense_network(T)
    params, th, gp, st = beacon_case(net, T, p_mesh, seed=31)
    w = run(net, params, th, gp, st, [1, 2], seed=32)
    size = per_observer(net, w.mesh[1])
    out_of_bounds = (size > gp.Dhi) if what == "pruned" else (size < gp.Dlo)
    assert out_of_bounds.mean() > 0.5
    done = per_observer(net, getattr(w, what)[1]) > 0
    assert done[out_of_bounds].all() and done.mean() > 0.5, f"most (observer, topic) pairs {what} in the first tick"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["dense", "slot_masks"])
def test_every_lane_width(require_gpu, layout):
    """A power-law graph with rows of <= 8, 9-16, 17-32 and 33-64 connections
    (8-, 16-, 32- and 64-lane groups: 8, 4, 2 and 1 observers per wavefront),
    once with every peer joined to all 9 topics (the dense kernels) and once
    with Zipf subscriptions of 3 topics each (slot masks; 9 topics cross the
    8-topic flag chunk)."""
    from gsim import graphs
    from tickrun import restrict_to_subscriptions
    T = 9
    net = graphs.power_law(600, 14, 2.5, 64, seed=41, n_topics=T)
    deg = np.diff(net.row_ptr.astype(np.int64))
    for lo, hi in ((1, 8), (9, 16), (17, 32), (33, 64)):
        assert ((deg >= lo) & (deg <= hi)).any(), f"rows of {lo}-{hi} connections"
    assert deg.max() <= 64
    if layout == "slot_masks":
        net = graphs.with_subscriptions(net, graphs.zipf_subscriptions(net.n, T, 3, seed=42))
        assert (net.sub >> np.uint64(8)).any() and not (net.sub == np.uint64((1 << T) - 1)).any()
    else:
        assert (net.sub == np.uint64((1 << T) - 1)).all()
    gp = GossipSubParams(D=6, Dlo=4, Dhi=10, Dscore=3, Dout=2)
    params, th, gp, st = beacon_case(net, T, 0.3, seed=43, gp=gp)
    if layout == "slot_masks":
        restrict_to_subscriptions(st, net)
    w = run(net, params, th, gp, st, [1, 2, 3], rate=3.0, seed=44)
    joined = ((net.sub[None, :] >> np.arange(T, dtype=np.uint64)[:, None]) & np.uint64(1)) != 0     # [T, N]
    for kk in (1, 3):
        changed = per_observer(net, w.grafted[kk] | w.pruned[kk]) > 0
        for lo, hi in ((1, 8), (9, 16), (17, 32), (33, 64)):
            rows = (deg >= lo) & (deg <= hi)
            c = changed[:, rows][joined[:, rows]]
            if kk == 1:     # (later ticks may leave a small class untouched)
                assert c.any(), f"tick {kk}: rows of {lo}-{hi} connections with a changed mesh"
            assert not c.all(), f"tick {kk}: rows of {lo}-{hi} connections with an unchanged mesh"


@pytest.mark.gpu
def test_opportunistic_tick(require_gpu):
    """C4's shape at 1000 peers (sybils behind few addresses, one topic) with
    OpportunisticGraftTicks = 2 over ticks 1-3: at tick 2 every wave takes
    the maintenance branch for the opportunistic clause alone -- a graft
    into a mesh that was inside every bound with no negative score can only
    be an opportunistic one."""
    from fixtures import beacon_params, synthetic_state
    from gsim import graphs
    from gsim.engine import random_regular
    rng = np.random.default_rng(51)
    n = 1000
    net = random_regular(n, 32, seed=9, n_topics=1)
    ip_ptr, ip_ids, n_ips, syb = graphs.sybil_ips(n, 0.2, 40, seed=3)
    net = graphs.with_ips(net, ip_ptr, ip_ids, n_ips)
    params = beacon_params(1)
    th = PeerScoreThresholds(GossipThreshold=-100, PublishThreshold=-500, GraylistThreshold=-1000,
                             AcceptPXThreshold=100, OpportunisticGraftThreshold=25)
    gp = GossipSubParams(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2, OpportunisticGraftTicks=2)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    synthetic_state(st, rng, tick_time(0), 8 / 32)
    beh = syb.astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT
    w = run(net, params, th, gp, st, [1, 2, 3], rate=10.0, seed=52, behaviour=beh)
    mesh, score = w.mesh[2], w.score[2]
    size = per_observer(net, mesh)[0]
    outb = per_observer(net, mesh & (net.outbound[None, :] != 0))[0]
    neg = per_observer(net, mesh & (score[None, :] < 0))[0]
    quiet = (size >= gp.Dlo) & (size <= gp.Dhi) & (outb >= gp.Dout) & (neg == 0)
    opp = per_observer(net, w.grafted[2])[0]
    assert (opp[quiet] > 0).any(), "an opportunistic graft at tick 2"
    assert not w.pruned[2][0][quiet[net.owner()]].any()
    for kk in (1, 3):       # no other tick grafts into such a mesh
        size = per_observer(net, w.mesh[kk])[0]
        outb = per_observer(net, w.mesh[kk] & (net.outbound[None, :] != 0))[0]
        neg = per_observer(net, w.mesh[kk] & (w.score[kk][None, :] < 0))[0]
        quiet = (size >= gp.Dlo) & (size <= gp.Dhi) & (outb >= gp.Dout) & (neg == 0)
        assert quiet.any() and not per_observer(net, w.grafted[kk])[0][quiet].any()


@pytest.mark.gpu
def test_negative_scores_only(require_gpu):
    """Every mesh holds exactly D = 8 peers, at least Dout + 1 of them
    outbound, nothing scores below zero -- but for a handful of mesh
    neighbours with a large behaviour penalty (P7).  The heartbeat prunes
    exactly those positions, and grafts nothing: the negative-score clause
    is the only one that sends a wave into the maintenance."""
    from fixtures import beacon_params, beacon_thresholds
    T = 4
    net = dense_network(T, seed=6)
    rng = np.random.default_rng(61)
    params, th = beacon_params(T), beacon_thresholds()
    gp = GossipSubParams(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    E, k, now = net.e, 32, tick_time(0)
    outbound = net.outbound.reshape(net.n, k) != 0
    assert (outbound.sum(axis=1) >= 3).all() and ((~outbound).sum(axis=1) >= 5).all()
    in_mesh = np.zeros((T, net.n, k), dtype=bool)
    for t in range(T):
        for i in range(net.n):
            o, r = np.nonzero(outbound[i])[0], np.nonzero(~outbound[i])[0]
            in_mesh[t, i, rng.choice(o, 3, replace=False)] = True
            in_mesh[t, i, rng.choice(r, 5, replace=False)] = True
    in_mesh = in_mesh.reshape(T, E)
    # a healthy state: first deliveries only (P2 > 0), no deficit, failure or invalid penalties
    st.tflags[...] = np.where(in_mesh, _abi.TF_IN_MESH | _abi.TF_MESH, 0).astype(np.uint8)
    st.graft_time[...] = np.where(in_mesh, now - rng.integers(0, 3600, (T, E)) * Second, 0)
    st.mesh_time[...] = np.where(in_mesh, now - st.graft_time, 0)
    st.first[...] = rng.integers(1, 2000, (T, E)) * 0.25
    st.meshd[...] = np.where(in_mesh, 400.0, 0.0)           # at the cap: no P3 deficit once active
    st.estate[...] = _abi.ES_TRACKED | _abi.ES_CONNECTED
    # the offenders: 12 non-outbound edges that are in some topic's mesh
    pool = np.nonzero(in_mesh.any(axis=0) & (net.outbound == 0))[0]
    bad = rng.choice(pool, 12, replace=False)
    st.bp[bad] = 100.0
    w = run(net, params, th, gp, st, [1, 2], rate=4.0, seed=62)
    negative = w.score[1] < 0
    assert np.array_equal(np.nonzero(negative)[0], np.sort(bad)), "the offenders alone score below zero"
    want = w.mesh[1] & negative[None, :]
    assert want.sum() >= len(bad) and np.array_equal(w.pruned[1], want), "exactly their mesh positions are pruned"
    assert not w.grafted[1].any()
    owner = net.owner()
    hit = np.zeros(net.n, dtype=bool)
    hit[owner[bad]] = True
    assert (hit[0::2] != hit[1::2]).any(), "a wave with one observer pruning and its neighbour steady"

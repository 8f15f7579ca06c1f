"""Parity over the score-parameter space, on every kernel that scores.

P1-P7 are restated by hand in many places on the device: the refresh / score
kernel (its own decay, DecayToZero, activation, lazy meshTime, the invalid
plane's skip, the relaunch after a purge), the live re-score of emitGossip,
the sticky P3b credit of every prune site, the capped delivery credits of the
delivery walk (the pending-increment counts and their spill path, three window
tests, the late credits) and the five threshold comparisons.  With the beacon
numbers most of those branches are never taken at their edge: no cap is
reached, the quantum is one second, every comparison sees random doubles.

Each case below is one PeerScoreParams / TopicScoreParams / PeerScoreThresholds
setting run through tickrun.run_parity (every plane, the seen-set, the totals,
lastput and the PX connections, bit for bit after every tick).  Each case
names, with a minimum count, the events of the oracle's score-branch census
(oracle.h ORC_SB_*) that it aims at; the condition is on the inputs, so the
oracle alone decides it (test_case_reaches_its_branches, no GPU).

Networks (built once per module, never modified):
  regular  random_regular(1500, 16), T = 3, every peer in every topic
  short    test_param_space.network("short"): rows of 8 ... 1024 connections,
           Zipf subscriptions (2 of 3 topics a peer), sparse slot masks
Run shape: ticks 1-3 (dyadic, fast_decay, slow_decay and retain: 1-4), publications in
every round with rejected ones among them, 1 % of the connections down before
tick 2 and up before tick 3 (retain: down before tick 1; dyadic: down before
tick 1, retained until tick 2's clock exactly, purged at tick 3, up before
tick 4), an opportunistic tick at 2.

Where a case names a fraction ("the cap was reached on 10 % of the records"),
it is of the census events of that kind: credits that reached or met the cap
among all credits, P1 evaluations at or over TimeInMeshCap among all, capped
topic sums among the records scored.

Every parameter set passes the library's validation but `quantum`, which sets
MeshMessageDeliveriesActivation 0 on a topic with a P3 weight (the reference
asks for at least a second): the activation edge at meshTime > 0 is the case.
IPColocationFactorThreshold is an int in the reference and here; the 3.5 arm of
p6_p7 truncates to 3 on both sides.
"""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

import oracle_binding as ob
from fixtures import beacon_params, beacon_topic, synthetic_state
from gsim import _abi, graphs
from gsim.engine import random_regular
from gsim.params import GossipSubParams, Minute, PeerScoreThresholds, Second, TopicScoreParams
from test_delivery import HB, R, T0
from test_gpu_score import multi_ips
from test_heartbeat import SEED, tick_time

T = 3
NAMES = [f"topic{t:02d}" for t in range(T)]
_nets = {}


def round_time(g):
    """oracle.h T(g) (asserted against orc_round_time by test_round_time_formula)."""
    return T0 + (g // R) * HB + ((g % R + 1) * HB) // (R + 1)


# within a tick every round comes 90 909 091 ns after the one before: with this window a
# duplicate one round after the first copy is exactly at the edge (one ns less: just outside)
ONE_ROUND = round_time(R + 1) - round_time(R)


def network(kind):
    if kind not in _nets:
        if kind == "regular":
            _nets[kind] = random_regular(1500, 16, seed=77, n_topics=T)
        else:
            import test_param_space
            _nets[kind] = test_param_space.network("short")[0]
    return _nets[kind]


def mixed_ips(net, rng, solo=()):
    """multi_ips (0-3 IPs a peer from a shared pool) but for the peers in
    `solo`, which get one IP of their own each (their P6 is 0)."""
    pool = max(8, net.n // 40)
    ip_ptr, ip_ids, _ = multi_ips(net.n, rng, pool)
    lists = [ip_ids[ip_ptr[i]:ip_ptr[i + 1]] for i in range(net.n)]
    for q, p in enumerate(solo):
        lists[int(p)] = np.array([pool + q], dtype=np.uint32)
    ptr = np.zeros(net.n + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return graphs.with_ips(net, ptr, np.concatenate(lists).astype(np.uint32), pool + len(solo))


# ---- the cases ------------------------------------------------------------------

GP = dict(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2, FanoutTTL=3 * Second, OpportunisticGraftTicks=2)
TH = dict(GossipThreshold=-100, PublishThreshold=-200, GraylistThreshold=-300, AcceptPXThreshold=0.0,
          OpportunisticGraftThreshold=1000.0)
EQUAL = ("p1_at_cap", "act_edge", "p3_at_threshold", "decay_first_edge", "decay_meshd_edge", "decay_fail_edge",
         "decay_invalid_edge", "decay_bp_edge", "tsc_at_cap", "p6_at_threshold", "p7_at_threshold", "retain_edge",
         "win_edge", "th_gossip_equal", "th_publish_equal", "th_graylist_equal", "th_accept_px_equal",
         "th_opp_graft_equal")


class Case:
    """One run.  topics(case) -> {name: TopicScoreParams} (a missing name is an
    unscored topic); peer: PeerScoreParams fields over beacon_params';
    reach: {census event: minimum count}; check(table): further conditions on
    the census; plant(case, ctx): changes the start state."""

    def __init__(self, cid, kind="regular", topics=None, peer=None, th=None, gp=None, reach=None, check=None,
                 plant=None, ticks=(1, 2, 3), rate=6.0, inv_frac=0.1, inv_ticks=None, topic_slots=0, shards=0,
                 validate=True, ips=None, behaviour=0.0, vdelays=None, down=0.01, down_at=2, retain_plant=False,
                 recap=False, seed=0, up_at=3, ring=1024):
        self.id, self.kind, self.topics, self.peer, self.th, self.gp = cid, kind, topics, peer or {}, th or TH, gp or {}
        self.reach, self.check, self.plant, self.ticks = reach or {}, check, plant, list(ticks)
        self.rate, self.inv_frac, self.inv_ticks = rate, inv_frac, inv_ticks
        self.topic_slots, self.shards, self.validate, self.ips = topic_slots, shards, validate, ips
        self.behaviour, self.vdelays, self.down, self.down_at = behaviour, vdelays, down, down_at
        self.retain_plant, self.recap, self.seed, self.up_at, self.ring = retain_plant, recap, seed, up_at, ring

    @property
    def run_id(self):
        return f"{self.id}/{self.kind}"


def beacon_topics(**over):
    return lambda case: {n: beacon_topic(TopicWeight=0.25 + 0.05 * t, MeshMessageDeliveriesThreshold=100 - 3 * t, **over)
                         for t, n in enumerate(NAMES)}


# -- dyadic: the equality case ----------------------------------------------------
# every number a power of two or a small integer: the arithmetic is exact and the planted
# records sit on every boundary after tick 1's decay
DY_CAP = 8.0                                   # TopicScoreCap
DY_GROUPS = {"gossip": -4.0, "publish": -8.0, "graylist": -16.0, "accept_px": 2.0, "opp": 1.0, "half": 0.5}
DY_SHARE = {"gossip": 0.05, "publish": 0.05, "graylist": 0.05, "accept_px": 0.05, "opp": 0.25, "half": 0.2}


def dyadic_topics(case):
    tp = TopicScoreParams(TopicWeight=1, TimeInMeshWeight=0.25, TimeInMeshQuantum=Second, TimeInMeshCap=8,
                          FirstMessageDeliveriesWeight=4, FirstMessageDeliveriesDecay=0.5, FirstMessageDeliveriesCap=16,
                          MeshMessageDeliveriesWeight=-0.25, MeshMessageDeliveriesDecay=0.5,
                          MeshMessageDeliveriesCap=32, MeshMessageDeliveriesThreshold=4,
                          MeshMessageDeliveriesWindow=ONE_ROUND, MeshMessageDeliveriesActivation=2 * Second,
                          MeshFailurePenaltyWeight=-0.5, MeshFailurePenaltyDecay=0.5,
                          InvalidMessageDeliveriesWeight=-1, InvalidMessageDeliveriesDecay=0.5)
    # the window: a copy one round late is at the edge in topic 0, 1 ns outside in 1, 1 ns inside in 2
    return {n: replace(tp, MeshMessageDeliveriesWindow=ONE_ROUND + (0, -1, 1)[t]) for t, n in enumerate(NAMES)}


DY_PEER = dict(TopicScoreCap=DY_CAP, AppSpecificWeight=1.0, IPColocationFactorWeight=-2.0, IPColocationFactorThreshold=2,
               BehaviourPenaltyWeight=-1.0, BehaviourPenaltyThreshold=2.0, BehaviourPenaltyDecay=0.5, DecayToZero=0.25,
               # a connection that goes down half a second before tick 1 expires at tick 2's clock exactly
               RetainScore=3 * Second // 2)
DY_TH = dict(GossipThreshold=-4, PublishThreshold=-8, GraylistThreshold=-16, AcceptPXThreshold=2, OpportunisticGraftThreshold=1)
DY_GP = dict(PeerExchange=True, FloodPublish=True)


def dyadic_groups(net, rng):
    """The pinned peers: every observer scores a peer of group g at DY_GROUPS[g]
    exactly while its topic sum stays over TopicScoreCap (first deliveries
    planted at their cap: 4 x 8 a shared topic after tick 1's decay), through
    an app score of DY_GROUPS[g] - DY_CAP, an IP of its own and no penalty."""
    perm = rng.permutation(net.n)
    groups, lo = {}, 0
    for g, share in DY_SHARE.items():
        groups[g] = perm[lo:lo + int(share * net.n)]
        lo += int(share * net.n)
    return groups, perm[lo:]


def dyadic_plant(case, c):
    st, rng, net = c["st"], c["rng"], c["net"]
    E = net.e
    now1 = tick_time(1)
    q4 = lambda hi, shape: rng.integers(0, hi, shape) * 0.25          # noqa: E731  quarter-integers
    in_mesh = (st.tflags & _abi.TF_IN_MESH) != 0
    st.first[...] = q4(64, (T, E))
    st.meshd[...] = np.where(in_mesh, q4(64, (T, E)), 0.0)
    st.fail[...] = np.where(rng.integers(0, 8, (T, E)) == 0, q4(40, (T, E)), 0.0)
    st.invalid[...] = np.where(rng.integers(0, 32, (T, E)) == 0, q4(12, (T, E)), 0.0)
    st.bp[...] = np.where(rng.integers(0, 16, E) == 0, q4(24, E), 0.0)
    for f in ("first", "meshd", "fail", "invalid"):
        r = rng.random((T, E))
        live = in_mesh if f == "meshd" else np.ones((T, E), bool)
        getattr(st, f)[(r < 0.04) & live] = 0.5                       # x 0.5 = DecayToZero exactly: kept
        getattr(st, f)[(r >= 0.04) & (r < 0.08) & live] = 0.25        # snaps to zero
    r = rng.random(E)
    st.bp[r < 0.05] = 4.0                                             # 2 x BehaviourPenaltyThreshold
    st.bp[(r >= 0.05) & (r < 0.08)] = 0.5
    st.bp[(r >= 0.08) & (r < 0.11)] = 0.25
    r = rng.random((T, E))
    at_thr = in_mesh & (r < 0.06)                                     # active, meshd 8: the threshold after the decay
    st.meshd[at_thr] = 8.0
    st.tflags[at_thr] |= _abi.TF_ACTIVE
    at_act = in_mesh & (r >= 0.06) & (r < 0.11)                       # meshTime == Activation at tick 1: not active
    st.graft_time[at_act] = now1 - 2 * Second
    st.tflags[at_act] &= np.uint8(~_abi.TF_ACTIVE & 0xFF)
    at_cap = in_mesh & (r >= 0.11) & (r < 0.16)                       # meshTime == Cap x Quantum at tick 1
    st.graft_time[at_cap] = now1 - 8 * Second
    st.mesh_time[...] = np.where(in_mesh, tick_time(0) - st.graft_time, 0)
    # the pinned peers
    p5 = rng.integers(-8, 9, net.n) * 0.25 - rng.integers(0, 3, net.n) * 4.0
    for g, peers in c["groups"].items():
        p5[peers] = DY_GROUPS[g] - DY_CAP
    pinned = np.isin(net.col, np.concatenate(list(c["groups"].values())))
    st.first[:, pinned] = 16.0
    st.fail[:, pinned] = 0.0
    st.invalid[:, pinned] = 0.0
    st.bp[pinned] = 0.0
    # a topic sum of TopicScoreCap exactly: outside every mesh, first deliveries 4 in topic 0 alone
    r = rng.random(E)
    flat = (r < 0.05) & ~pinned
    for f in ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags"):
        getattr(st, f)[:, flat] = 0
    st.first[0, flat] = 4.0
    c["p5"] = p5


def dyadic_extra_publishers(case, c, sched, mid):
    """Flood publications from the graylist and publish groups: their
    neighbours compare them with the graylist threshold, they compare their
    neighbours with the publish threshold."""
    rng = c["rng"]
    for k in case.ticks:
        for g in ("graylist", "publish", "gossip"):
            for o in rng.choice(c["groups"][g], size=4, replace=False):
                member = [t for t in range(T) if (int(c["net"].sub[o]) >> t) & 1]
                sched.setdefault(k * R + int(rng.integers(0, R)), []).append((mid, int(rng.choice(member)), int(o), 0))
                mid += 1
        # a PRUNE handled while its sender's mesh credits of the same tick are pending: the sender
        # pruned at the heartbeat, so only its own flood publication of the round before still
        # reaches the pruned peer in round 0 (a rare event: sixty publications in the last round of
        # every tick give a handful).
        for o in rng.choice(c["net"].n, size=60, replace=False):
            member = [t for t in range(T) if (int(c["net"].sub[o]) >> t) & 1]
            sched.setdefault(k * R + R - 1, []).append((mid, int(rng.choice(member)), int(o), 0))
            mid += 1
    return mid


def dyadic_case(cid, kind, **kw):
    reach = {e: 20 for e in EQUAL}
    reach.update({f"th_{t}_{side}": 20 for t in ("gossip", "publish", "graylist", "accept_px", "opp_graft")
                  for side in ("below", "above")})
    reach.update(p1_capped=20, p1_uncapped=20, act_set=20, p3_deficit=20, p3_inactive=20, prune_deficit=20,
                 prune_no_deficit=20, tsc_applied=20, tsc_negative=20, p6_surplus=20, p6_whitelisted=20, p6_multi_ip=20,
                 p7_excess=20, retain_purged=20, prune_pending=3, win_inside=20, win_outside=20, first_reach=20, first_at=20,
                 decay_first_zero=20, decay_meshd_zero=20, decay_fail_zero=20, decay_invalid_zero=20, decay_bp_zero=20)
    return Case(cid, kind, topics=dyadic_topics, peer=DY_PEER, th=DY_TH, gp=DY_GP, reach=reach, plant=dyadic_plant,
                ips="dyadic", down_at=1, up_at=4, ticks=(1, 2, 3, 4), rate=12.0, **kw)


# -- small_caps ------------------------------------------------------------------

SMALL = dict(FirstMessageDeliveriesCap=2.5, MeshMessageDeliveriesCap=3, TimeInMeshCap=1.5, MeshMessageDeliveriesThreshold=2)


def small_caps_plant(case, c):
    st = c["st"]                                   # a reachable start: no counter over its cap
    np.minimum(st.first, 2.5, out=st.first)
    np.minimum(st.meshd, 3.0, out=st.meshd)


def small_caps_check(lo, hi):
    def check(tb):
        assert lo <= tb["mesh_pending_max"] <= hi, f"most pending mesh increments on a record: {tb['mesh_pending_max']}"
        for kind in ("first", "mesh"):
            hit, n = tb[f"{kind}_reach"] + tb[f"{kind}_at"], tb[f"{kind}_below"] + tb[f"{kind}_reach"] + tb[f"{kind}_at"]
            assert hit >= 0.1 * n, f"{kind} credits at their cap: {hit} of {n}"
        hit = tb["p1_capped"] + tb["p1_at_cap"]
        assert hit >= 0.1 * (hit + tb["p1_uncapped"] + tb["p1_negative"]), f"P1 at TimeInMeshCap: {hit}"
        assert tb["tsc_applied"] >= 0.1 * c_records(tb), f"TopicScoreCap applied: {tb['tsc_applied']}"
    return check


def c_records(tb):
    return tb["_scored"]                           # records scored (connections x ticks), set by the runner


def small_caps_case(cid, kind, rate, lo, hi, **kw):
    return Case(cid, kind, topics=lambda case: {n: beacon_topic(TopicWeight=0.25 + 0.05 * t, **SMALL)
                                                for t, n in enumerate(NAMES)},
                peer=dict(TopicScoreCap=0.75), plant=small_caps_plant, rate=rate, check=small_caps_check(lo, hi),
                reach=dict(first_reach=100, first_at=100, mesh_reach=100, mesh_at=100, p1_capped=100, tsc_applied=100),
                **kw)


# -- quantum -----------------------------------------------------------------------

def quantum_topics(case):
    return {NAMES[0]: beacon_topic(TimeInMeshQuantum=7 * 10**6, TimeInMeshCap=10**6, MeshMessageDeliveriesActivation=0),
            NAMES[1]: beacon_topic(TimeInMeshQuantum=333_333_333, MeshMessageDeliveriesActivation=2 * 3600 * Second),
            NAMES[2]: beacon_topic(TimeInMeshQuantum=10_000 * Second)}


def quantum_plant(case, c):
    st, rng = c["st"], c["rng"]
    in_mesh = (st.tflags & _abi.TF_IN_MESH) != 0
    st.tflags[1] &= np.uint8(~_abi.TF_ACTIVE & 0xFF)                  # activation longer than any mesh time
    # graft times after tick 1's clock (and some after tick 2's): negative meshTime, Go's
    # truncating division (-0.5 s / 333 333 333 ns = -1, not -2), the refresh's mt < 0 store
    r = rng.random(st.tflags.shape)
    late = in_mesh & (r < 0.03)
    st.graft_time[late] = tick_time(1) + rng.integers(1, 1500, int(late.sum())) * 10**6
    st.tflags[late] &= np.uint8(~_abi.TF_ACTIVE & 0xFF)
    fresh = in_mesh & (r >= 0.03) & (r < 0.06) & (np.arange(T)[:, None] == 0)   # topic 0: active at meshTime > 0
    st.graft_time[fresh] = tick_time(0)
    st.tflags[fresh] &= np.uint8(~_abi.TF_ACTIVE & 0xFF)
    st.mesh_time[...] = np.where(in_mesh, tick_time(0) - st.graft_time, 0)


# -- weights_off ---------------------------------------------------------------------

def weights_off_topics(case):
    return {NAMES[0]: beacon_topic(MeshMessageDeliveriesWeight=0.0, MeshMessageDeliveriesThreshold=100),
            # topic 1 has no score parameters
            NAMES[2]: beacon_topic(TopicWeight=0.0)}


def weights_off_plant(case, c):
    st = c["st"]                                   # an unscored topic has no topicStats
    for f in ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time"):
        getattr(st, f)[1] = 0
    st.tflags[1] &= np.uint8(_abi.TF_MESH | _abi.TF_FANOUT)


# -- fast / slow decay -----------------------------------------------------------------

def fast_decay_topics(case):
    # (a mesh-delivery threshold of 1: with these decays every counter is near zero at each
    # refresh, and the usual threshold would put every peer below the graylist)
    return {n: beacon_topic(FirstMessageDeliveriesDecay=0.1, MeshMessageDeliveriesDecay=0.07 - 0.02 * t,
                            MeshMessageDeliveriesThreshold=1,
                            MeshFailurePenaltyDecay=0.01 + 0.03 * t, InvalidMessageDeliveriesDecay=0.05,
                            TopicWeight=0.25 + 0.05 * t)
            for t, n in enumerate(NAMES)}


def fast_decay_plant(case, c):
    c["st"].invalid[...] = 0.0                      # the invalid plane starts all-zero


def slow_decay_topics(case):
    d = 0.9999999
    return {n: beacon_topic(TopicWeight=0.123456789012345 + 0.0987654321 * t, TimeInMeshWeight=0.00271828182845904,
                            TimeInMeshCap=1e6, FirstMessageDeliveriesWeight=0.664377123456789,
                            FirstMessageDeliveriesDecay=d, FirstMessageDeliveriesCap=1e6,
                            MeshMessageDeliveriesWeight=-0.257731958762887, MeshMessageDeliveriesDecay=d,
                            MeshMessageDeliveriesCap=1e6, MeshMessageDeliveriesThreshold=100.3333333333333,
                            MeshFailurePenaltyWeight=-0.251327412287183, MeshFailurePenaltyDecay=d,
                            InvalidMessageDeliveriesWeight=-99.1415926535898, InvalidMessageDeliveriesDecay=d)
            for t, n in enumerate(NAMES)}


# -- window ------------------------------------------------------------------------------

def window_topics(case):
    return {NAMES[0]: beacon_topic(MeshMessageDeliveriesWindow=0),
            NAMES[1]: beacon_topic(MeshMessageDeliveriesWindow=ONE_ROUND),
            NAMES[2]: beacon_topic(MeshMessageDeliveriesWindow=5 * Minute)}


# -- retain --------------------------------------------------------------------------------

def negative_app_scores(case, c):
    """RemovePeer keeps only non-positive scores: a third of the peers score below zero."""
    rng, n = c["rng"], c["net"].n
    c["p5"] = np.where(rng.random(n) < 0.35, -20.0 - rng.integers(0, 40, n), 0.0)


RETAIN_REACH = dict(retain_purged=50, retain_edge=20, retain_skipped=20)

# -- recap ------------------------------------------------------------------------------------

def recap_topics(case):
    # (topic 0's threshold is under the cap it will get: the recap does not open a deficit on every record)
    return {n: beacon_topic(TopicWeight=0.25 + 0.05 * t, MeshMessageDeliveriesThreshold=20 if t == 0 else 100 - 3 * t)
            for t, n in enumerate(NAMES)}


def recap_params(case, params):
    """After tick 2: topic 0's caps drop below most current values; topic 2
    changes weights and its threshold alone."""
    a = replace(params.Topics[NAMES[0]], FirstMessageDeliveriesCap=7.5, MeshMessageDeliveriesCap=33.0)
    b = replace(params.Topics[NAMES[2]], TopicWeight=0.7, FirstMessageDeliveriesWeight=0.3, MeshMessageDeliveriesWeight=-0.6,
                MeshFailurePenaltyWeight=-0.1, MeshMessageDeliveriesThreshold=37.5)
    return [(0, a), (2, b)]


RECAP_REACH = dict(first_reach=1000, first_at=100, mesh_reach=100, mesh_at=100)
CASES = [
    dyadic_case("dyadic", "regular"),
    dyadic_case("dyadic", "short", seed=1),
    dyadic_case("dyadic_shards", "regular", shards=2),
    # (the ring holds every message of the run: a slot may not be reused while its message can be gossiped)
    small_caps_case("small_caps", "regular", 160.0, 128, 10**9, ring=2048),
    small_caps_case("small_caps_few", "regular", 12.0, 1, 200),
    small_caps_case("small_caps", "short", 300.0, 128, 10**9, ring=4096),
    small_caps_case("small_caps_rings", "regular", 160.0, 128, 10**9, topic_slots=640),
    Case("quantum", topics=quantum_topics, plant=quantum_plant, validate=False,
         reach=dict(p1_negative=200, p1_capped=1000, p1_uncapped=1000, act_set=100, p3_inactive=1000)),
    Case("weights_off_p6", topics=weights_off_topics, plant=weights_off_plant, peer=dict(IPColocationFactorWeight=0.0),
         ips="multi", reach=dict(unscored_skipped=10000, prune_deficit=100, p6_surplus=100, p7_excess=20)),
    Case("weights_off_p7", topics=weights_off_topics, plant=weights_off_plant, peer=dict(BehaviourPenaltyWeight=0.0),
         ips="multi", reach=dict(unscored_skipped=10000, prune_deficit=100, p6_surplus=100, p7_excess=20)),
    Case("fast_decay", topics=fast_decay_topics, plant=fast_decay_plant, ticks=(1, 2, 3, 4), rate=20.0, inv_frac=0.3, inv_ticks=(1,),
         # (the origin of a rejected message advertises it while its mcache's gossip windows hold it, and
         # whoever asks rejects it in turn: one window, so the rejections end with tick 2)
         gp=dict(HistoryLength=2, HistoryGossip=1),
         peer=dict(DecayToZero=0.5, BehaviourPenaltyDecay=0.05),
         reach=dict(decay_first_zero=1000, decay_meshd_zero=1000, decay_fail_zero=1000, decay_invalid_zero=100,
                    decay_bp_zero=100)),
    Case("slow_decay", topics=slow_decay_topics, ticks=(1, 2, 3, 4), peer=dict(DecayToZero=1e-9),
         reach=dict(p3_deficit=1000, p1_uncapped=1000, first_below=1000, mesh_below=1000)),
    Case("window", topics=window_topics, reach=dict(win_edge=1, win_inside=100, win_outside=100)),
    Case("window_vdelay", topics=window_topics, vdelays=(0, 2), reach=dict(win_edge=1, win_inside=100, win_outside=100)),
    Case("p6_1_p7_0", peer=dict(IPColocationFactorThreshold=1, BehaviourPenaltyThreshold=0.0), ips="multi", behaviour=0.3,
         reach=dict(p6_surplus=1000, p6_at_threshold=1000, p6_whitelisted=100, p6_multi_ip=1000, p7_excess=100)),
    Case("p6_3_p7_2", peer=dict(IPColocationFactorThreshold=3.5, BehaviourPenaltyThreshold=2.0), ips="multi", behaviour=0.3,
         reach=dict(p6_surplus=5, p6_at_threshold=20, p6_whitelisted=100, p6_multi_ip=1000, p7_excess=100)),
    Case("p6_10000_p7_2", peer=dict(IPColocationFactorThreshold=10000, BehaviourPenaltyThreshold=2.0), ips="multi",
         behaviour=0.3, reach=dict(p6_whitelisted=100, p6_multi_ip=1000, p7_excess=100)),
    Case("p6_3_p7_0", "short", peer=dict(IPColocationFactorThreshold=3.5, BehaviourPenaltyThreshold=0.0), ips="multi",
         behaviour=0.3, reach=dict(p6_surplus=100, p6_at_threshold=100, p6_whitelisted=100, p6_multi_ip=1000,
                                   p7_excess=100)),
    Case("retain_0", peer=dict(RetainScore=0), plant=negative_app_scores, ticks=(1, 2, 3, 4), down=0.05, down_at=1,
         retain_plant=True, reach=dict(retain_purged=50, retain_edge=20)),
    Case("retain_hb", peer=dict(RetainScore=HB), plant=negative_app_scores, ticks=(1, 2, 3, 4), down=0.05, down_at=1,
         retain_plant=True, reach=RETAIN_REACH),
    Case("recap", topics=recap_topics, recap=True, rate=30.0, reach=RECAP_REACH),
    # (64 slots a topic hold the whole run's messages at 12 a tick)
    Case("recap_slots", "short", topics=recap_topics, recap=True, rate=12.0, topic_slots=64, reach=RECAP_REACH),
]
BY_ID = {c.run_id: c for c in CASES}
RUNS = [c.run_id for c in CASES]


# ---- one run ----------------------------------------------------------------------

def setup(case):
    """Everything both sides start from: a dict (net, params, th, gp, st, p5,
    white, sched, churn, behaviour)."""
    from tickrun import restrict_to_subscriptions, subscribed_schedule
    net = network(case.kind)
    rng = np.random.default_rng(sum(map(ord, case.run_id)) + 1000 * case.seed)
    c = dict(rng=rng, p5=None, white=None, groups=None)
    if case.ips == "dyadic":
        c["groups"], _ = dyadic_groups(net, rng)
        net = mixed_ips(net, rng, solo=np.concatenate(list(c["groups"].values())))
    elif case.ips == "multi":
        net = mixed_ips(net, rng)
    if case.ips:
        c["white"] = (rng.random(net.n_ips) < 0.1).astype(np.uint8)
    c["net"] = net
    params = beacon_params(T, RetainScore=3 * Second)
    params.Topics = dict((case.topics or beacon_topics())(case))
    for k, v in case.peer.items():
        setattr(params, k, v)
    if case.validate:
        params.validate()
    th = PeerScoreThresholds(**case.th)
    th.validate()
    gp = GossipSubParams(**{**GP, **case.gp})
    c.update(params=params, th=th, gp=gp)
    st = c["st"] = ob.NetState(net, params, thresholds=th, gossip=gp, topics=NAMES, ip_white=c["white"])
    deg = np.diff(net.row_ptr.astype(np.int64))
    synthetic_state(st, rng, tick_time(0), 0.7 if case.kind == "regular" else np.where(deg[net.owner()] <= 65, 0.9, 0.3))
    if case.plant:
        case.plant(case, c)
    restrict_to_subscriptions(st, net)
    if c["p5"] is not None:
        st.p5[...] = c["p5"]
    sched = subscribed_schedule(rng, case.ticks, net, T, case.rate, case.inv_frac, member_only=True, vdelays=case.vdelays)
    if case.inv_ticks is not None:                       # rejected messages in these ticks alone
        sched = {g: [m if g // R in case.inv_ticks else (m[0], m[1], m[2], 0) + tuple(m[4:]) for m in b]
                 for g, b in sched.items()}
    mid = 1 + max((m[0] for b in sched.values() for m in b), default=0)
    if case.ips == "dyadic":
        dyadic_extra_publishers(case, c, sched, mid)
    c["sched"] = sched
    own = net.owner()
    und = np.stack([own, net.col], axis=1)
    und = und[und[:, 0] < und[:, 1]]
    pick = rng.permutation(len(und))
    n_down = int(len(und) * case.down)
    down = und[pick[:n_down]]
    c["churn"] = {1: [], 2: [], 3: [], 4: []}
    c["churn"][case.up_at].append((down, True))
    c["churn"][case.down_at].append((down, False))
    if case.retain_plant:
        # connections that went down before the run, their retention ending at a tick's clock
        # exactly (RemovePeer itself at now = the tick's clock - RetainScore); up again before tick 4
        gone = []
        for q, k in enumerate((1, 2, 3)):
            pairs = und[pick[n_down + 60 * q:n_down + 60 * (q + 1)]]
            st.churn(pairs, up=False, now=tick_time(k) - int(params.RetainScore))
            gone.append(pairs)
        c["churn"][4].append((np.concatenate(gone), True))
    c["behaviour"] = (rng.random(net.n) < case.behaviour).astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT \
        if case.behaviour else None
    return c


def recap_on(st, idx, newp):
    """orc_set_topic_params on the oracle's side (score.go:201-241)."""
    cp = newp.to_c(True)
    slot = ctypes.cast(ctypes.addressof(st.tp) + idx * ctypes.sizeof(_abi.CTopicScoreParams), ctypes.c_void_p)
    ob.load().orc_set_topic_params(st.view(), idx, slot, ctypes.cast(ctypes.byref(cp), ctypes.c_void_p))


def ring_of(case):
    return T * case.topic_slots if case.topic_slots else case.ring


def oracle_run(case, before_refresh=None, after_tick=None, after_refresh=None, after_scores=None):
    """The oracle's half of tickrun.run_parity alone, with the score census on.
    before_refresh / after_refresh / after_scores(kk, now, st), after_tick(kk, st, msgs): hooks."""
    c = setup(case)
    net, st, sched, gp = c["net"], c["st"], c["sched"], c["gp"]
    msgs = ob.Msgs(net.n, T, ring_of(case), R, T0, Second, behaviour=c["behaviour"], topic_slots=case.topic_slots)
    lib = ob.load()
    planes, dialled = {}, 0
    with ob.ScoreCensus() as census:
        for kk in case.ticks:
            now = tick_time(kk)
            for (pairs, up) in c["churn"].get(kk, []):
                st.churn(pairs, up=up, now=now - Second // 2)
            if before_refresh:
                before_refresh(kk, now, st)
            v = st.view()
            lib.orc_refresh_scores(v, now)
            if after_refresh:
                after_refresh(kk, now, st)
            msgs.penalties(st, now)
            lib.orc_ip_colocation(v)
            lib.orc_compute_scores(v)
            if after_scores:
                after_scores(kk, now, st)
            msgs.heartbeat(st, kk, now, SEED)
            for g in range(kk * R, kk * R + R):
                for m in sched.get(g, []):
                    msgs.publish(st, m[0], m[1], m[2], m[3], g, vdelay=m[4] if len(m) > 4 else 0)
                msgs.round(st, g)
            if gp.PeerExchange:
                dialled += len(st.px_connect(now + Second // 2))
            planes[kk] = bool(st.invalid.any())
            if case.recap and kk == 2:
                for idx, newp in recap_params(case, c["params"]):
                    recap_on(st, idx, newp)
                    c["params"].Topics[NAMES[idx]] = newp
            if after_tick:
                after_tick(kk, st, msgs)
    census.table["_scored"] = net.e * len(case.ticks)
    census.table["_dialled"] = dialled
    return census.table, planes, msgs


def check_census(case, table, planes):
    missed = {e: (table[e], lo) for e, lo in case.reach.items() if table[e] < lo}
    assert not missed, f"{case.run_id}: census events under their minimum (count, minimum): {missed}"
    if case.check:
        case.check(table)
    if case.id == "fast_decay":
        # the invalid plane: all-zero at the start, live after ticks 1 and 2 (the rejected messages
        # of tick 1, and tick 2's IWANT answers for them), all-zero again once tick 3 has decayed it
        # (1 x 0.05 < DecayToZero) and after tick 4: the refresh's skip flips twice
        assert planes[1] and planes[2] and not planes[3] and not planes[4], f"invalid plane live after ticks: {planes}"


def test_round_time_formula():
    msgs = ob.Msgs(4, 1, 4, R, T0, HB)
    assert all(msgs.round_time(g) == round_time(g) for g in range(0, 6 * R))
    assert {round_time(g + 1) - round_time(g) for g in range(R, 2 * R - 1)} == {ONE_ROUND}


def test_score_census_off_by_default():
    case = BY_ID["window/regular"]
    lib = ob.load()
    lib.orc_score_census_reset()
    c = setup(case)
    lib.orc_refresh_scores(c["st"].view(), tick_time(1))
    lib.orc_compute_scores(c["st"].view())
    out = np.zeros(len(ob.SCORE_CENSUS), dtype=np.uint64)
    lib.orc_score_census_read(out.ctypes.data_as(ctypes.c_void_p))
    assert not out.any()


@pytest.mark.parametrize("rid", RUNS)
def test_case_reaches_its_branches(rid):
    """The inputs of every case: the oracle alone takes the branches the case
    names, each at least as often as stated (no GPU)."""
    case = BY_ID[rid]
    table, planes, msgs = oracle_run(case)
    print(rid, {k: v for k, v in table.items() if v})
    check_census(case, table, planes)
    assert msgs.stats[1] > 0 and msgs.stats[2] > 0, "messages were delivered, with duplicates"
    if case.gp.get("PeerExchange") and case.kind == "short":
        # (a PX connection needs a triangle with one side down: the regular network has next to
        # none, there the accept-PX comparison is covered by the census and the PX marks' parity)
        assert table["_dialled"] > 0, "PX made connections"


@pytest.mark.gpu
@pytest.mark.parametrize("rid", RUNS)
def test_score_space_bit_exact(require_gpu, rid):
    from gsim.engine import Engine
    from tickrun import run_parity
    case = BY_ID[rid]
    c = setup(case)
    net, params, th, gp, st = c["net"], c["params"], c["th"], c["gp"], c["st"]
    if case.shards:
        from gsim.shard import ShardedEngine
        assert case.validate, "the sharded engine always validates"
        eng = ShardedEngine(params, th, gossip=gp, topics=NAMES, shards=case.shards)
    else:
        eng = Engine(params, th, gossip=gp, topics=NAMES, validate=case.validate)
    eng.load_graph(net)
    eng.set_app_score(st.p5)
    if c["white"] is not None:
        eng.set_ip_whitelist(c["white"])
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    planes, px = {}, []

    def after_tick(kk, st_, msgs):
        planes[kk] = bool(st_.invalid.any())
        if case.recap and kk == 2:
            for idx, newp in recap_params(case, params):
                eng.set_topic_score_params(NAMES[idx], newp)
                recap_on(st_, idx, newp)

    with ob.ScoreCensus() as census:
        msgs, gstats = run_parity(net, params, th, gp, st, case.ticks, c["sched"], ring=ring_of(case), behaviour=c["behaviour"],
                                  churn=c["churn"], eng=eng, after_tick=after_tick, px_log=px,
                                  topic_slots=case.topic_slots)
    census.table["_scored"] = net.e * len(case.ticks)
    print(f"{rid}: totals {msgs.stats}, engine gossip {gstats}, PX connections {px}")
    check_census(case, census.table, planes)
    assert gstats["iwant_ids"] > 0, "gossip ran on both sides and was asked for"
    if gp.PeerExchange and case.kind == "short":
        assert sum(px) > 0, "PX made connections"

"""Parity over the topic and subscription space, at every layout edge.

The engine chooses its memory layout (dense [T][E] planes, or slot masks with
S = the largest popcount), its kernel instances and its host-side shortcuts
(all_joined, unjoined_zero, sub_dynamic, the topic-major block table) from the
topic count and the subscription masks.  Each case below is one
tickrun.run_parity (every plane, the seen-set, the totals, lastput, the trace
where on and the PX connections, bit for bit after every tick) at one edge of
that axis; test_case_reaches_its_edges decides from the inputs and the oracle
alone (no GPU) that the case sits at the edge it is named for.

Networks (the topology is built once per module and never modified; every
case gets its own copy of the subscription masks and the outbound flags, which
the oracle's Join / Leave and PX connector update in place):
  regular   random_regular(1500, 16), the score sweep's network
  short     the parameter sweep's network (2000 peers, planted rows of exactly
            8 ... 1024 connections), in its Zipf form and with every peer in
            every topic (the dense kernels then meet rows over 64)
  small12   random_regular(1500, 12): no row over 16, none under 9
  tiny_n    random_regular(n, 8), n = 63, 64, 65
  tail      random_regular(1000, 16) followed by 37 peers with no connections
Run shape: synthetic_state + restrict_to_subscriptions, ticks 1-3 (1-4 where a
case changes subscriptions twice), an opportunistic tick at 2, publications in
every tick from members and from any peer (non-members publish through a
fanout), 5 % rejected, 30 % of the peers ignore IWANT, 1 % of the connections
down before tick 2 and up before tick 3.  From T = 31 on, one publication per
topic and tick on average.

Structural conditions (exact, Case.struct): `dense`, the layout the loader
chooses (dense iff every mask is full); S0 / S1, the slot planes at load and
at the end (the largest popcount of the masks ever held: sub, Joins, fanout
publications); `empty`, the peers with an empty mask; `members`, {topic:
member count}; `max_row` / `min_row`; `isolated`, peers with no connection.

Event conditions (Case.reach, minimum counts; from the oracle's log and
census, per run):
  fanout        peers holding a fanout after some tick (the most after any)
  join_fanouts  Joins of a topic the peer holds a fanout of (it becomes the mesh)
  join_grafts   GRAFTs sent by the Joins (EV_GRAFT inside set_subscriptions)
  unsub_prunes  PRUNEs with CTL_UNSUB pending right after the Leaves
  left_copies   copies arriving at a peer that has left their topic
  first_tN      first deliveries in topic N; first_top: in topic T - 1
  ans_top       IWANT answers (EV_RPC_MSG, x = 1) in topic T - 1
  dhi_hub       Dhi prunes on rows over 64 connections (census classes 4-7)
  direct_out    copies over a direct link that is in no mesh of the copy's topic
  iso_pubs      publications by peers with no connection
  empty_pubs    publications by peers whose mask was empty at load
  joins, leaves tracer.Join / tracer.Leave events

The oracle's counts per case (test_case_reaches_its_edges prints them):
  dense_t1                     dense S 1, first_top 31525, ans_top 416; 246039 copies
  dense_t31                    dense S 31, first_top 22512, ans_top 433; 1265387 copies
  dense_t32                    dense S 32, first_top 18033, ans_top 187; 1214620 copies
  dense_t33                    dense S 33, first_top 25663, ans_top 229; 1299857 copies
  dense_t63                    dense S 63, first_top 24023, ans_top 232; 2018809 copies
  dense_t64                    dense S 64, first_top 22507, ans_top 287; 1958670 copies
  dense_t64/32 slots           dense S 64, first_top 22507, ans_top 287; 1958670 copies
  dense_t64/2 shards           dense S 64, first_top 22507, ans_top 287; 1958670 copies
  masks_t31                    masks S 3 -> 4, first_top 12627, fanout 43; 99194 copies
  masks_t32                    masks S 3 -> 5, first_top 11508, fanout 40; 85850 copies
  masks_t33                    masks S 3 -> 4, first_top 13568, fanout 40; 112499 copies
  masks_t63                    masks S 3 -> 5, first_top 11055, fanout 35; 77914 copies
  masks_full_peer              masks S 64, first_top 17304, fanout 63; 204087 copies
  masks_full_peer/32 slots     masks S 64, first_top 17304, fanout 63; 204087 copies
  masks_edges                  masks S 8 -> 10, fanout 49, empty_pubs 9, pubs_t40 6, pubs_t63 6; 58211 copies
  masks_edges/32 slots         masks S 8 -> 10, fanout 49, empty_pubs 9, pubs_t40 6, pubs_t63 6; 58211 copies
  one_short_of_dense           masks S 16, first_top 21001, ans_top 225; 701672 copies
  dense_hubs_direct            dense S 3, dhi_hub 60, direct_out 2365; 179838 copies
  dense_hubs_direct_t64        dense S 64, dhi_hub 1070, direct_out 2871, first_top 13468; 454255 copies
  grow_join                    masks S 2 -> 8, join_grafts 146, unsub_prunes 17, fanout 37, joins 66, leaves 4, join_fanouts 6; 61058 copies
  grow_join_slots/64 slots     masks S 2 -> 8, join_grafts 151, unsub_prunes 13, fanout 34, joins 66, leaves 4, join_fanouts 6; 49019 copies
  grow_join_shards/2 shards    masks S 2 -> 8, join_grafts 162, unsub_prunes 16, fanout 32, joins 66, leaves 4, join_fanouts 6; 48696 copies
  grow_join_hub                masks S 3, joins 3, leaves 3, join_grafts 24, unsub_prunes 345; 92510 copies
  grow_fanout_empty            masks S 2 -> 3, empty_pubs 3, fanout 41; 56555 copies
  dense_leave_join             dense S 3, unsub_prunes 783, join_grafts 140, left_copies 3088, leaves 120, joins 60; 530366 copies
  dense_leave_join_step        dense S 3, unsub_prunes 760, join_grafts 140, left_copies 3259, leaves 120, joins 60; 637092 copies
  dense_leave_join_shards/2 shards dense S 3, unsub_prunes 768, join_grafts 151, left_copies 1794, leaves 120, joins 60; 486481 copies
  dense_leave_small_rows       dense S 3, unsub_prunes 661, join_grafts 57, left_copies 1757, leaves 120, joins 60; 367768 copies
  tiny_63                      dense S 2, first_top 2887, ans_top 11; 18167 copies
  tiny_64                      dense S 2, first_top 2481, ans_top 3; 18537 copies
  tiny_64_t64                  dense S 64, first_top 968; 62448 copies
  tiny_65                      dense S 2, first_top 2880, ans_top 5; 18763 copies
  tail_isolated                dense S 3, iso_pubs 9, first_top 18334, ans_top 49; 214516 copies
(tiny_63 / 64 / 65: a network of 64 peers gives no 20 IWANT answers in three ticks; the minimum is
the oracle's exact count.  masks_edges: topic 63 has one member, topic 40 none: the publications
there are counted, exactly.)
"""
import numpy as np
import pytest

import oracle_binding as ob
from fixtures import beacon_params, synthetic_state
from gsim import _abi, graphs
from gsim.engine import Network, random_regular
from gsim.params import GossipSubParams, PeerScoreThresholds, Second
from test_delivery import R, T0
from test_heartbeat import SEED, tick_time
from test_score_space import GP, TH

_topo = {}
ISOLATED = 37
STATE_PLANES = ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags")


def topology(kind):
    """The shared, never modified connection graph of a network kind."""
    if kind not in _topo:
        if kind == "regular":
            import test_score_space
            _topo[kind] = test_score_space.network("regular")
        elif kind == "short":
            import test_param_space
            _topo[kind] = test_param_space.network("short")[0]
        elif kind == "small12":
            _topo[kind] = random_regular(1500, 12, seed=78, n_topics=1)
        elif kind.startswith("tiny_"):
            n = int(kind[5:])
            _topo[kind] = random_regular(n, 8, seed=n, n_topics=1)
        elif kind == "tail":
            b = random_regular(1000, 16, seed=79, n_topics=1)
            n = b.n + ISOLATED
            row_ptr = np.concatenate([b.row_ptr, np.full(ISOLATED, b.row_ptr[-1], dtype=np.uint32)])
            _topo[kind] = Network(n, row_ptr, b.col, b.outbound, np.ones(n, dtype=np.uint64),
                                  np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32), n)
        else:
            raise KeyError(kind)
    return _topo[kind]


def hubs():
    import test_param_space
    return test_param_space.network("short")[1]


def full(T):
    return (1 << T) - 1 if T < 64 else (1 << 64) - 1


def popcount(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.array([bin(int(x)).count("1") for x in a], dtype=np.int64)


def has(sub, t):
    return ((np.asarray(sub, dtype=np.uint64) >> np.uint64(t)) & np.uint64(1)).astype(bool)


# ---- subscription masks ----------------------------------------------------------

def sub_dense(case, topo):
    return np.full(topo.n, full(case.T), dtype=np.uint64)


def sub_zipf(per, seed=5, top_heavy=False):
    """Zipf masks, `per` topics a peer; top_heavy: topic T - 1 is the most
    popular one and topic 0 the rarest (the order of the bits reversed)."""
    def make(case, topo):
        sub = graphs.zipf_subscriptions(topo.n, case.T, per, seed=seed + case.T)
        if top_heavy:
            rev = np.zeros_like(sub)
            for t in range(case.T):
                rev |= ((sub >> np.uint64(t)) & np.uint64(1)) << np.uint64(case.T - 1 - t)
            sub = rev
        return sub
    return make


FULL_PEER = 700


def sub_full_peer(case, topo):
    sub = sub_zipf(8, top_heavy=True)(case, topo)
    sub[FULL_PEER] = full(case.T)
    return sub


EMPTY = np.arange(100, 1100, 50)             # 20 peers that hold nothing
LONE = 901                                   # topic 63's only member


def sub_edges(case, topo):
    sub = sub_zipf(8)(case, topo)
    sub &= ~np.uint64((1 << 40) | (1 << 63))
    sub[LONE] = (sub[LONE] & (sub[LONE] - np.uint64(1))) | np.uint64(1 << 63)     # (one topic less: still 8 at most)
    sub[EMPTY] = 0
    return sub


def sub_one_short(case, topo):
    sub = sub_dense(case, topo)
    sub[333] &= ~np.uint64(1 << 15)
    return sub


def sub_short(case, topo):
    """The short network's own Zipf masks; the planted row of 1024, which holds
    every topic there, gives up topic 0: its Join of topic 0 puts the new slot
    before the two it holds, so the planes of topics 1 and 2 of a row of 1024
    move (the rows of 65 and 257 lack topic 2: their new slot comes last)."""
    sub = topo.sub.copy()
    for h, d in hubs():
        if d == 1024:
            sub[h] &= ~np.uint64(1)
    return sub


GROWER = 40                                  # grow_join: joins every topic it lacks
BARE = 55                                    # grow_fanout_empty: holds nothing, publishes to three topics


def sub_grow(case, topo):
    sub = sub_zipf(2)(case, topo)
    if case.id.startswith("grow_fanout_empty"):
        sub[BARE] = 0
    return sub


# ---- Joins and Leaves ---------------------------------------------------------------

def pairs_of(peers, topics):
    return np.array([(int(p), int(t)) for p in np.atleast_1d(peers) for t in np.atleast_1d(topics)], dtype=np.uint32)


def subs_grow_join(case, c):
    sub = c["net"].sub
    lack = [t for t in range(case.T) if not (int(sub[GROWER]) >> t) & 1]
    assert len(lack) == case.T - 2
    pool = np.setdiff1d(np.nonzero(~has(sub, 5))[0], [GROWER])
    fans = pool[:5]                              # (extra_grow: they publish to topic 5 in tick 1, through a fanout)
    crowd = np.concatenate([fans, c["rng"].choice(pool[5:], size=55, replace=False)])
    return {2: [(np.concatenate([pairs_of(GROWER, lack), pairs_of(crowd, 5)]), True)],
            3: [(pairs_of(GROWER, lack[:4]), False)]}


def extra_grow(case, c):
    """Tick 1: the peer that will Join six topics publishes to one of them, and
    five of the sixty that will Join topic 5 publish there: their Joins turn a
    fanout into the mesh and delete it."""
    sub = c["net"].sub
    lack = [t for t in range(case.T) if not (int(sub[GROWER]) >> t) & 1]
    pool = np.setdiff1d(np.nonzero(~has(sub, 5))[0], [GROWER])
    return [(1, 3, lack[0], GROWER)] + [(1, 2 + q, 5, int(p)) for q, p in enumerate(pool[:5])]


def subs_grow_hub(case, c):
    sub = c["net"].sub
    pairs = np.array([(h, 0 if d == 1024 else 2) for h, d in hubs() if d in (65, 257, 1024)], dtype=np.uint32)
    assert len(pairs) == 3 and not ((sub[pairs[:, 0]] >> pairs[:, 1].astype(np.uint64)) & np.uint64(1)).any()
    big = int(pairs[pairs[:, 1] == 0][0, 0])
    assert int(sub[big]) == 0b110, "the row of 1024 holds topics 1 and 2: its Join of topic 0 moves both planes"
    return {2: [(pairs, True)], 3: [(pairs, False)]}


def subs_dense_leave(case, c):
    lo, hi = case.trace or (0, c["net"].n)
    gone = c["rng"].choice(np.arange(lo, hi), size=120, replace=False)
    return {2: [(pairs_of(gone, 1), False)], 4: [(pairs_of(gone[:60], 1), True)]}


# ---- further publications: [(tick, round of the tick, topic, origin)] --------------------

def extra_edges(case, c):
    out = []
    for k in case.ticks:
        out += [(k, 1 + q, 3 * q, int(p)) for q, p in enumerate(EMPTY[:3])]          # empty masks publish
        out += [(k, 2, 40, 10), (k, 5, 40, 1200)]                                      # a topic nobody holds
        out += [(k, 3, 63, LONE)]                                                      # its only member
    return out


def extra_fanout_empty(case, c):
    return [(2, 1, 1, BARE), (2, 4, 6, BARE), (2, 8, 3, BARE)]


def extra_tail(case, c):
    n = c["net"].n
    return [(k, 2 * q, q % case.T, n - 1 - 5 * q) for k in case.ticks for q in range(3)]


def extra_hubs(case, c):
    """Every planted row over 64 publishes in the last round of each tick."""
    return [(k, R - 1, (q + k) % case.T, h) for k in case.ticks for q, (h, d) in enumerate(hubs()) if d > 64]


# ---- the cases ------------------------------------------------------------------

class Case:
    def __init__(self, cid, kind="regular", T=3, sub=sub_dense, ticks=(1, 2, 3), rate=None, topic_slots=0, shards=0,
                 trace=None, step=False, px=False, subs=None, extra=None, direct=False, struct=None, reach=None,
                 fan=0):
        # fan: further publishers a tick that do not hold their topic (each builds a fanout)
        self.fan = fan
        self.id, self.kind, self.T, self.sub, self.ticks = cid, kind, T, sub, list(ticks)
        self.rate = rate if rate is not None else (4.0 if T <= 3 else 1.0)
        self.topic_slots, self.shards, self.trace, self.step, self.px = topic_slots, shards, trace, step, px
        self.subs, self.extra, self.direct, self.struct, self.reach = subs, extra, direct, struct or {}, reach or {}

    @property
    def run_id(self):
        return self.id + (f"/{self.topic_slots} slots" if self.topic_slots else "") + \
            (f"/{self.shards} shards" if self.shards else "")


def variants(cid, slots=0, shards=0, **kw):
    out = [Case(cid, **kw)]
    if slots:
        out.append(Case(cid, topic_slots=slots, **kw))
    if shards:
        out.append(Case(cid, shards=shards, **kw))
    return out


def dense(T, **kw):
    reach = dict(first_top=20, ans_top=20)
    return variants(f"dense_t{T}", T=T, struct=dict(dense=True, S0=T, S1=T), reach=reach, **kw)


def masks(T):
    # (Zipf 3 of T: a fanout publication grows a peer's mask, to at most 3 + the ticks' publications)
    return Case(f"masks_t{T}", T=T, sub=sub_zipf(3, top_heavy=True), fan=8, struct=dict(dense=False, S0=3),
                reach=dict(first_top=20, fanout=20))


GJ = dict(T=8, sub=sub_grow, subs=subs_grow_join, extra=extra_grow, fan=10, struct=dict(dense=False, S0=2, S1=8),
          # (join_fanouts: the six Joins of extra_grow's publishers, exactly)
          reach=dict(join_grafts=20, unsub_prunes=4, fanout=20, joins=66, leaves=4, join_fanouts=6))
DL = dict(T=3, ticks=(1, 2, 3, 4), subs=subs_dense_leave, struct=dict(dense=True, S0=3, S1=3),
          reach=dict(unsub_prunes=20, join_grafts=20, left_copies=20, leaves=120, joins=60))
CASES = [
    *dense(1), *dense(31), *dense(32), *dense(33), *dense(63), *dense(64, slots=32, shards=2),
    masks(31), masks(32), masks(33), masks(63),
    *variants("masks_full_peer", slots=32, T=64, sub=sub_full_peer, struct=dict(dense=False, S0=64, S1=64),
              reach=dict(first_top=20, fanout=20)),
    *variants("masks_edges", slots=32, T=64, sub=sub_edges, extra=extra_edges,
              struct=dict(dense=False, S0=8, empty=20, members={40: 0, 63: 1}),
              # (exact counts.  Topic 63: its one member publishes once a tick, and the schedule draws
              # three more publications there from peers that do not hold it, through a fanout to
              # the one member where they are connected to it; topic 40: six publications by
              # non-members, nobody to receive them)
              reach=dict(fanout=20, empty_pubs=9, pubs_t40=6, pubs_t63=6)),
    Case("one_short_of_dense", T=16, sub=sub_one_short, struct=dict(dense=False, S0=16, S1=16),
         reach=dict(first_top=20, ans_top=20)),
    Case("dense_hubs_direct", "short", T=3, direct=True, extra=extra_hubs, struct=dict(dense=True, S0=3, max_row=1024),
         reach=dict(dhi_hub=20, direct_out=20)),
    Case("dense_hubs_direct_t64", "short", T=64, direct=True, extra=extra_hubs, ticks=(1, 2), rate=0.5,
         struct=dict(dense=True, S0=64, max_row=1024), reach=dict(dhi_hub=20, direct_out=20, first_top=20)),
    Case("grow_join", trace=(0, 1500), **GJ),
    Case("grow_join_slots", topic_slots=64, **GJ),
    Case("grow_join_shards", shards=2, **GJ),
    Case("grow_join_hub", "short", T=3, sub=sub_short, subs=subs_grow_hub, px=True,
         struct=dict(dense=False, S0=3, S1=3, max_row=1024),
         # (three Joins: D GRAFTs each; three Leaves: the meshes they built)
         reach=dict(joins=3, leaves=3, join_grafts=18, unsub_prunes=18)),
    Case("grow_fanout_empty", T=8, sub=sub_grow, extra=extra_fanout_empty, fan=10, struct=dict(dense=False, S0=2, empty=1),
         reach=dict(empty_pubs=3, fanout=20)),
    Case("dense_leave_join", trace=(0, 600), **DL),
    Case("dense_leave_join_step", step=True, **DL),
    Case("dense_leave_join_shards", shards=2, **DL),
    Case("dense_leave_small_rows", "small12", **{**DL, "struct": dict(dense=True, S0=3, S1=3, max_row=12, min_row=12)}),
    Case("tiny_63", "tiny_63", T=2, rate=12.0, struct=dict(dense=True, n=63), reach=dict(first_top=20, ans_top=11)),
    Case("tiny_64", "tiny_64", T=2, rate=12.0, struct=dict(dense=True, n=64), reach=dict(first_top=20, ans_top=3)),
    Case("tiny_64_t64", "tiny_64", T=64, struct=dict(dense=True, n=64, S0=64), reach=dict(first_top=20)),
    Case("tiny_65", "tiny_65", T=2, rate=12.0, struct=dict(dense=True, n=65), reach=dict(first_top=20, ans_top=5)),
    Case("tail_isolated", "tail", T=3, extra=extra_tail, struct=dict(dense=True, isolated=ISOLATED, n=1037),
         reach=dict(iso_pubs=9, first_top=20, ans_top=20)),
]
BY_ID = {c.run_id: c for c in CASES}
RUNS = list(BY_ID)
assert len(RUNS) == len(CASES)


# ---- one run ----------------------------------------------------------------------

def schedule(case, rng, net):
    """Poisson(rate) publications per topic and tick at uniform rounds, 5 %
    rejected; the origin is a member of the topic or, as often, any peer
    (a non-member publishes through a fanout)."""
    sched, mid = {}, 0
    members = [np.nonzero(has(net.sub, t))[0] for t in range(case.T)]
    connected = np.nonzero(np.diff(net.row_ptr.astype(np.int64)) > 0)[0]
    for k in case.ticks:
        for t in range(case.T):
            for _ in range(rng.poisson(case.rate)):
                pool = members[t] if rng.random() < 0.5 and len(members[t]) else connected
                o = int(pool[rng.integers(0, len(pool))])
                sched.setdefault(k * R + int(rng.integers(0, R)), []).append((mid, t, o, int(rng.random() < 0.05)))
                mid += 1
    return sched, mid


def setup(case):
    from tickrun import restrict_to_subscriptions
    topo = topology(case.kind)
    rng = np.random.default_rng(sum(map(ord, case.id)) + 31 * case.T)
    T = case.T
    net = Network(topo.n, topo.row_ptr, topo.col, topo.outbound.copy(), case.sub(case, topo).astype(np.uint64),
                  topo.ip_ptr, topo.ip_ids, topo.n_ips)
    sub0 = net.sub.copy()
    params = beacon_params(T, RetainScore=3 * Second)
    th = PeerScoreThresholds(**TH)
    gp = GossipSubParams(**{**GP, "PeerExchange": case.px})
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    deg = np.diff(net.row_ptr.astype(np.int64))
    synthetic_state(st, rng, tick_time(0), 0.7 if case.kind != "short" else np.where(deg[net.owner()] <= 65, 0.9, 0.3))
    if case.direct:
        # five mutual direct links on every planted row over 64; two of them in no mesh at all
        for h, d in hubs():
            if d <= 64:
                continue
            b = int(net.row_ptr[h])
            pick = b + rng.choice(d, size=5, replace=False)
            both = np.concatenate([pick, st.rev[pick]])
            st.direct[both] = 1
            bare = np.concatenate([pick[:2], st.rev[pick[:2]]])
            for f in STATE_PLANES:
                getattr(st, f)[:, bare] = 0
    restrict_to_subscriptions(st, net)
    sched, mid = schedule(case, rng, net)
    c = dict(net=net, params=params, th=th, gp=gp, st=st, rng=rng, sub0=sub0)
    more = case.extra(case, c) if case.extra else []
    top = np.nonzero(has(net.sub, T - 1) & (deg > 0))[0]
    for k in case.ticks:
        # the highest topic: three members publish in each of a tick's last two rounds (the next
        # heartbeat's gossip then advertises messages its receivers have not seen: IWANT answers)
        if len(top) > 1:
            more += [(k, R - 1 - q % 2, T - 1, int(o)) for q, o in enumerate(rng.choice(top, size=6))]
        for _ in range(case.fan):
            o = int(rng.integers(0, net.n))
            lack = [t for t in range(T) if not (int(net.sub[o]) >> t) & 1]
            if lack and deg[o]:
                more.append((k, int(rng.integers(0, R)), int(rng.choice(lack)), o))
    for (k, r, t, o) in more:
        sched.setdefault(k * R + r, []).append((mid, t, o, 0))
        mid += 1
    own = net.owner()
    und = np.stack([own, net.col], axis=1)
    und = und[und[:, 0] < und[:, 1]]
    down = und[rng.choice(len(und), size=max(1, len(und) // 100), replace=False)]
    c.update(sched=sched, churn={2: [(down, False)], 3: [(down, True)]},
             behaviour=(rng.random(net.n) < 0.3).astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT)
    c["subs"] = case.subs(case, c) if case.subs else {}
    return c


def structure(case, c):
    """What the loader will choose, from the inputs by gsim_load_graph's rule,
    and the slot planes once every Join and fanout publication has grown them."""
    net, sub0, T = c["net"], c["sub0"], case.T
    mask = np.uint64(full(T))
    assert not (sub0 & ~mask).any(), "a subscription bit at or beyond T"
    is_dense = bool(((sub0 & mask) == mask).all())
    ever = sub0.copy()
    for evs in c["subs"].values():
        for pairs, join in evs:
            if join:
                np.bitwise_or.at(ever, pairs[:, 0].astype(np.int64), np.uint64(1) << pairs[:, 1].astype(np.uint64))
    for batch in c["sched"].values():
        for m in batch:
            ever[m[2]] |= np.uint64(1) << np.uint64(m[1])            # a member's bit is there; a fanout's is added
    deg = np.diff(net.row_ptr.astype(np.int64))
    return dict(dense=is_dense, S0=T if is_dense else max(1, int(popcount(sub0).max())),
                S1=T if is_dense else max(1, int(popcount(ever).max())), empty=int((sub0 == 0).sum()),
                members={t: int(has(sub0, t).sum()) for t in range(T)}, max_row=int(deg.max()),
                min_row=int(deg[deg > 0].min()), isolated=int((deg == 0).sum()), n=net.n)


def check_structure(case, c):
    got = structure(case, c)
    for k, want in case.struct.items():
        if k == "members":
            assert {t: got[k][t] for t in want} == want, f"{case.run_id}: topic members {got[k]}"
        else:
            assert got[k] == want, f"{case.run_id}: {k} is {got[k]}, the case is named for {want}"
    if case.id.startswith("masks_t"):
        assert got["S1"] > got["S0"], "fanout publications grow a mask"
    return got


def check_reach(case, counts):
    missed = {e: (counts[e], lo) for e, lo in case.reach.items() if counts[e] < lo}
    assert not missed, f"{case.run_id}: events under their minimum (count, minimum): {missed}"


class Counter:
    def __init__(self, case, c):
        self.case, self.c = case, c
        self.n = dict(fanout=0, join_fanouts=0, join_grafts=0, unsub_prunes=0, left_copies=0, ans_top=0, dhi_hub=0, direct_out=0,
                      iso_pubs=0, empty_pubs=0, joins=0, leaves=0, first_top=0)
        self.n.update({f"first_t{t}": 0 for t in range(case.T)})
        self.n.update({f"pubs_t{t}": 0 for t in range(case.T)})
        net = c["net"]
        self.key = net.owner().astype(np.int64) * net.n + net.col.astype(np.int64)      # sorted: rows are
        self.deg = np.diff(net.row_ptr.astype(np.int64))

    def after_subs(self, ev, st):
        n = self.n
        n["join_grafts"] += int((ev["kind"] == ob.EV_GRAFT).sum())
        n["joins"] += int((ev["kind"] == ob.EV_JOIN).sum())
        n["leaves"] += int((ev["kind"] == ob.EV_LEAVE).sum())
        n["unsub_prunes"] += int(((st.ctl & _abi.CTL_UNSUB) != 0).sum())

    def after_tick(self, ev, st):
        n, case, net = self.n, self.case, self.c["net"]
        kind, x, a, b, topic = ev["kind"], ev["x"], ev["a"], ev["b"], ev["topic"]
        first = (kind == ob.EV_SEEN) & (x == 1) & (b != 0xFFFFFFFF)
        per = np.bincount(topic[first], minlength=case.T)
        pub = kind == ob.EV_PUBLISH
        ppt = np.bincount(topic[pub], minlength=case.T)
        for t in range(case.T):
            n[f"first_t{t}"] += int(per[t])
            n[f"pubs_t{t}"] += int(ppt[t])
        n["first_top"] = n[f"first_t{case.T - 1}"]
        n["ans_top"] += int(((kind == ob.EV_RPC_MSG) & (x == 1) & (topic == case.T - 1)).sum())
        n["fanout"] = max(n["fanout"], int((st.fan_topics != 0).sum()))
        n["iso_pubs"] += int((self.deg[a[pub]] == 0).sum())
        n["empty_pubs"] += int((self.c["sub0"][a[pub]] == 0).sum())
        copy = (kind == ob.EV_RPC_MSG) & (x != 3)
        n["left_copies"] += int((((net.sub[b[copy]] >> topic[copy].astype(np.uint64)) & np.uint64(1)) == 0).sum())
        if case.direct:
            fwd = (kind == ob.EV_RPC_MSG) & (x == 0)
            e = np.searchsorted(self.key, a[fwd].astype(np.int64) * net.n + b[fwd].astype(np.int64))
            out = (st.direct[e] != 0) & ((st.tflags[topic[fwd], e] & _abi.TF_MESH) == 0)
            n["direct_out"] += int(out.sum())


def oracle_run(case):
    """The oracle's half of run_parity alone, with the event log and the branch census on."""
    c = setup(case)
    net, st, sched, T = c["net"], c["st"], c["sched"], case.T
    ring = T * case.topic_slots if case.topic_slots else 1024
    msgs = ob.Msgs(net.n, T, ring, R, T0, Second, behaviour=c["behaviour"], topic_slots=case.topic_slots)
    msgs.log()
    lib = ob.load()
    cnt = Counter(case, c)
    with ob.Census() as census:
        for kk in case.ticks:
            now = tick_time(kk)
            for (pairs, up) in c["churn"].get(kk, []):
                st.churn(pairs, up=up, now=now - Second // 2)
            msgs.events()
            for (pairs, join) in c["subs"].get(kk, []):
                if join:
                    held = (st.fan_topics[pairs[:, 0].astype(np.int64)] >> pairs[:, 1].astype(np.uint64)) & np.uint64(1)
                    cnt.n["join_fanouts"] += int(held.sum())
                st.set_subscriptions(pairs, join, kk, now - Second // 2, SEED)
            if c["subs"].get(kk):
                cnt.after_subs(msgs.events(), st)
            v = st.view()
            lib.orc_refresh_scores(v, now)
            msgs.penalties(st, now)
            lib.orc_ip_colocation(v)
            lib.orc_compute_scores(v)
            msgs.heartbeat(st, kk, now, SEED)
            for g in range(kk * R, kk * R + R):
                for (mid, t, o, inv) in sched.get(g, []):
                    msgs.publish(st, mid, t, o, inv, g)
                msgs.round(st, g)
            cnt.after_tick(msgs.events(), st)
            if c["gp"].PeerExchange:
                st.px_connect(now + Second // 2)
    cnt.n["dhi_hub"] = int(census.table["dhi_prune"][4:8].sum())
    return c, cnt.n, msgs


@pytest.mark.parametrize("rid", RUNS)
def test_case_reaches_its_edges(rid):
    """The inputs of every case: the layout, the slot planes and the members
    are what the case is named for, and the oracle alone produces its events,
    each at least as often as stated (no GPU)."""
    case = BY_ID[rid]
    c, counts, msgs = oracle_run(case)
    got = check_structure(case, c)
    shown = {k: got[k] for k in ("dense", "S0", "S1")}
    shown.update({k: counts[k] for k in case.reach})
    print(rid, shown, "totals", msgs.stats)
    check_reach(case, counts)
    assert msgs.stats[1] > 0, "messages were delivered"


def make_engine(case, c):
    from gsim.engine import Engine
    if case.shards:
        from gsim.shard import ShardedEngine
        eng = ShardedEngine(c["params"], c["th"], gossip=c["gp"], shards=case.shards)
    else:
        eng = Engine(c["params"], c["th"], gossip=c["gp"])
    eng.load_graph(c["net"])
    eng.set_seed(SEED)
    c["st"].push_to_engine(eng)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("rid", RUNS)
def test_topic_space_bit_exact(require_gpu, rid):
    """One run_parity at the case's topic count, masks and subscription
    changes: every plane, the seen-set, lastput and the totals after every
    tick, the trace where the case has one, the PX connections where PX is on.
    What each case reaches: the module docstring."""
    from tickrun import run_parity
    case = BY_ID[rid]
    c = setup(case)
    check_structure(case, c)
    eng = make_engine(case, c)
    msgs, gstats = run_parity(c["net"], c["params"], c["th"], c["gp"], c["st"], case.ticks, c["sched"], ring=1024,
                              behaviour=c["behaviour"], churn=c["churn"], eng=eng, subs=c["subs"],
                              topic_slots=case.topic_slots, trace=case.trace, step=case.step)
    print(f"{rid}: totals {msgs.stats}, engine gossip {gstats}")
    assert msgs.stats[1] > 0, "messages were delivered"


# ---- refusals -----------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_change_nothing(require_gpu):
    """A subscription bit at or beyond T at load, a (peer, topic) pair out of
    range in gsim_set_subscriptions (a topic of 2^31 or more among them: it is
    no negative number) and T = 65 at create: each returns its error, and the
    loaded network, its state and the totals are as before."""
    from gsim.engine import Engine, GsimError
    from test_clock_space import assert_unchanged, engine_state, small_engine
    net, params, th, gp, st, eng = small_engine()
    try:
        eng.msgs_init(8, 2, T0, Second)
        before = engine_state(eng, st)
        bad = Network(net.n, net.row_ptr, net.col, net.outbound, net.sub.copy(), net.ip_ptr, net.ip_ids, net.n_ips)
        bad.sub[7] |= np.uint64(2)                       # T = 1: bit 1 is beyond it
        with pytest.raises(ValueError, match="beyond n_topics"):
            eng.load_graph(bad)
        assert_unchanged(before, eng, st)
        for pair in ((net.n, 0), (0, 1), (0, 64), (0, 1 << 31), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0)):
            for join in (True, False):
                with pytest.raises(ValueError, match="out of range"):
                    eng.set_subscriptions([(3, 0), pair], join, 1, T0 + Second // 2)     # (a good pair first)
                assert_unchanged(before, eng, st)
        with pytest.raises(GsimError) as err:
            Engine(beacon_params(65), th, gossip=gp)
        assert err.value.rc == _abi.GSIM_ERANGE
        assert_unchanged(before, eng, st)
    finally:
        eng.close()


# ---- the reports on these layouts ---------------------------------------------------

REPORT_CASES = ("dense_t64", "masks_edges", "grow_join")
PATH_TOPICS = {"dense_t64": (0, 63), "masks_edges": (0, 40, 63), "grow_join": (5, 7)}


def two_classes(n):
    return (np.arange(n) % 5 == 2).astype(np.uint8)


def report_expectations(case, c, msgs, st, first, cls):
    """The six reports' numpy references (each from its own module), on the
    oracle's state after the last tick."""
    from test_mesh_paths import expected_paths
    from test_msg_report import expected_report, vdelays_of
    from test_net_report import EDGES as NET_EDGES, expected_net_report
    from test_peer_report import expected_peer_report
    from test_relay_report import expected_relay_report
    from test_score_report import EDGES as SCORE_EDGES, expected_score_report
    net, vd = c["net"], vdelays_of(c["sched"])
    src = np.array([0, LONE, GROWER, net.n - 1], dtype=np.uint32)
    return dict(msg=expected_report(msgs, st, vd), net=expected_net_report(st, net, cls, NET_EDGES),
                peer=expected_peer_report(msgs, st, first, cls, 2), score=expected_score_report(st, net, cls, SCORE_EDGES),
                relay=expected_relay_report(msgs, net.sub, st.T, first, cls, 2, vd),
                paths={(t, b): expected_paths(st, net, cls, t, src, blocked=b) for t in PATH_TOPICS[case.id]
                       for b in ((), (1,))}, src=src)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", REPORT_CASES)
def test_reports_on_the_layout(require_gpu, cid):
    """After the last tick of the case (run once, bit-exact as above, without
    the trace: the first senders come from the same event log) each of the six
    read-only reports equals its module's numpy reference, with two peer
    classes: msg, net, peer, score, relay, and the mesh paths of the topics
    in PATH_TOPICS (masks_edges: a topic nobody holds and one with a single
    member among them), nothing blocked and class 1 blocked."""
    from test_mesh_paths import assert_paths_equal
    from test_msg_report import assert_report_equal
    from test_net_report import EDGES as NET_EDGES, assert_net_equal
    from test_peer_report import FirstSenders, assert_class_rows, assert_peer_rows
    from test_relay_report import assert_relay
    from test_score_report import EDGES as SCORE_EDGES, assert_score_equal
    from tickrun import run_parity
    case = BY_ID[cid]
    c = setup(case)
    eng = make_engine(case, c)
    cls = two_classes(c["net"].n)
    eng.set_peer_classes(cls)
    state, done = {}, []

    def after_heartbeat(kk, eng_, st_, msgs):
        if "first" not in state:                               # before the first round
            msgs.log()
            state["first"] = FirstSenders(*msgs.seen.shape)

    def after_tick(kk, st_, msgs):
        state["first"].update(msgs)
        if kk != case.ticks[-1]:
            return
        want = report_expectations(case, c, msgs, st_, state["first"], cls)
        assert_report_equal(eng.msg_report(), want["msg"], cid)
        assert_net_equal(eng.net_report(NET_EDGES), want["net"], cid)
        got_p, got_c = eng.peer_report()
        want_p, want_c, pending, _ = want["peer"]
        assert_peer_rows(got_p, want_p, pending, cid)
        assert_class_rows(got_c, want_c, bool(pending.any()), cid)
        assert_score_equal(eng.score_report(SCORE_EDGES), want["score"], cid)
        assert_relay(eng.relay_report(), want["relay"][:3], want["relay"][3], cid)
        for (t, b), w in want["paths"].items():
            got = eng.mesh_paths(t, want["src"], blocked=b, per_peer=True)
            assert_paths_equal(got, w, f"{cid} topic {t} blocked {b}")
        done.append(len(want["paths"]))

    run_parity(c["net"], c["params"], c["th"], c["gp"], c["st"], case.ticks, c["sched"], ring=1024,
               behaviour=c["behaviour"], churn=c["churn"], eng=eng, subs=c["subs"], after_heartbeat=after_heartbeat,
               after_tick=after_tick)
    assert done == [2 * len(PATH_TOPICS[cid])]


# ---- slot growth with connection tags configured ---------------------------------------

def conn_tags_case():
    """test_conn_tags' planted network (rows of 1 ... 4100 connections) at T = 4
    with every peer, the planted ones too, in 2 of the 4 topics: S starts at
    2.  Before tick 3 the hub, three more planted rows and 30 pool peers Join
    both topics they lack: S grows by two planes in one call."""
    import test_conn_tags as tc
    from test_msg_report import fixed_schedule
    from tickrun import restrict_to_subscriptions
    T = 4
    rng = np.random.default_rng(83)
    net = tc.planted_net(T, False)
    p = np.arange(net.n)
    net.sub[:] = (np.uint64(1) << (p % T).astype(np.uint64)) | (np.uint64(1) << ((p + 1) % T).astype(np.uint64))
    params = beacon_params(T)
    st = ob.NetState(net, params, thresholds=tc.TH, gossip=tc.GP)
    synthetic_state(st, rng, tick_time(0), 0.6)
    restrict_to_subscriptions(st, net)
    ticks = [1, 2, 3]
    sched = fixed_schedule(rng, ticks, net, T, 3, verdicts=tc.VERDICTS)
    sched = {g: [m[:4] for m in batch] for g, batch in sched.items()}
    who = np.concatenate([[tc.HUB, 2, 5, 8], rng.choice(np.arange(len(tc.ROWS), net.n), size=30, replace=False)])
    join = np.array([(int(q), t) for q in who for t in range(T) if not (int(net.sub[q]) >> t) & 1], dtype=np.uint32)
    return dict(T=T, net=net, params=params, st=st, ticks=ticks, sched=sched, join=join, who=who, topic_slots=0, ring=128)


def test_conn_tags_case_reaches_its_edges():
    c = conn_tags_case()
    assert int(popcount(c["net"].sub).max()) == 2 and len(c["join"]) == 2 * len(c["who"]) == 68
    sub = c["net"].sub.copy()
    np.bitwise_or.at(sub, c["join"][:, 0].astype(np.int64), np.uint64(1) << c["join"][:, 1].astype(np.uint64))
    assert int(popcount(sub).max()) == 4, "S 2 -> 4: two planes in one call"
    deg = np.diff(c["net"].row_ptr.astype(np.int64))
    assert deg[c["who"][0]] == 4100, "a row of 17 tiles is laid out again"


@pytest.mark.gpu
def test_grow_conn_tags(require_gpu):
    """grow_conn_tags: the tags equal the port's after ticks 1 and 2, right
    after the Join that grows S from 2 to 4 (non-zero tags moved with their
    planes, the joined topics' start at 0) and after tick 3; the state, the
    seen-set and the totals bit-exact after tick 3."""
    import test_conn_tags as tc
    c = conn_tags_case()
    run = tc.Lockstep(c)
    try:
        for kk in (1, 2):
            run.tick(kk)
            run.check(kk, state=False)
        before = run.log[2]
        assert (before != 0).sum() >= 20, "tags are configured and non-zero before the Join"
        run.subscriptions(c["join"], True, 3, tick_time(3) - Second // 2)
        run.check("joined", state=False)
        lo, hi = int(c["net"].row_ptr[tc.HUB]), int(c["net"].row_ptr[tc.HUB + 1])
        assert before[:, lo:hi].any() and run.log["joined"][:, lo:hi].any(), "the hub row holds tags across the new layout"
        run.tick(3)
        run.check(3, state=True)
        assert run.counts[ob.EV_JOIN] == len(c["join"])
    finally:
        run.close()


# ---- a Leave on a state no write has touched ----------------------------------------------

@pytest.mark.gpu
def test_leave_after_device_fill(require_gpu):
    """Every parity case above pushes its state, and a written field already
    tells the engine that no record may be skipped (unjoined_zero = false), so
    none of them depends on the Leave clearing that flag.  Here the state comes
    from gsim_fill_synthetic on a network loaded dense (the flag stays set,
    nothing is skipped while all are joined) and is pulled into the oracle;
    120 peers Leave topic 1 before tick 2.  Their neighbours keep the topic's
    records about them (first deliveries over 20 of them non-zero, from the
    oracle's state): the score pass must go on reading and decaying those."""
    from gsim.engine import Engine
    from tickrun import run_parity
    T = 3
    topo = topology("regular")
    rng = np.random.default_rng(97)
    net = Network(topo.n, topo.row_ptr, topo.col, topo.outbound.copy(), np.full(topo.n, full(T), dtype=np.uint64),
                  topo.ip_ptr, topo.ip_ids, topo.n_ips)
    params, th, gp = beacon_params(T, RetainScore=3 * Second), PeerScoreThresholds(**TH), GossipSubParams(**GP)
    eng = Engine(params, th, gossip=gp)
    eng.load_graph(net)
    eng.set_seed(SEED)
    eng.fill_synthetic(seed=31, now=tick_time(0), p_mesh=0.5)
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    st.pull_from_engine(eng)
    case = Case("leave_after_device_fill", T=T)
    sched, _ = schedule(case, rng, net)
    gone = rng.choice(net.n, size=120, replace=False)
    kept = []

    def after_tick(kk, st_, msgs):
        if kk == case.ticks[-1]:
            about = np.isin(net.col, gone)
            kept.append(int((st_.first[1, about] != 0).sum()))

    run_parity(net, params, th, gp, st, case.ticks, sched, ring=1024, eng=eng, subs={2: [(pairs_of(gone, 1), False)]},
               after_tick=after_tick)
    assert kept and kept[0] >= 20, f"records of topic 1 about the peers that left: {kept}"

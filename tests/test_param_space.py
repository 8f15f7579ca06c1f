"""Parity over the GossipSub parameter space, at every row-class boundary.

The heartbeat evaluates D / Dlo / Dhi / Dscore / Dout / Dlazy / GossipFactor /
OpportunisticGraftPeers / PrunePeers in data-parallel closed forms, written
once per row class (lane groups of 8 / 16 / 32 / 64, the block classes up to
4096, the 4097-8192 scratch class, the streamed class above); the oracle
evaluates them as the reference's sequential loops.  Each case below runs one
parameter setting through tickrun.run_parity (every plane, the seen-set, the
totals, lastput and the PX connections, bit for bit after every tick) on a
network that holds rows of exactly 8, 9, 16, 17, ... connections, and asserts
from the oracle's branch census (oracle.h ORC_CB_*) that the branches the
case aims at were taken in the row classes written beside it.

Networks (built once per module, never modified):
  short  2000 peers, T = 3, Zipf subscriptions (2 topics a peer), power-law
         base capped at 64, planted rows of exactly SHORT_ROWS connections
  tall   9000 peers, T = 2 (1 topic a peer), base capped at 64, planted rows
         of exactly TALL_ROWS connections; the cases with `tall=` run here too
Each also in a variant whose connections were dialled by their
higher-numbered end with probability 0.15 (the planted rows are the highest
numbered: they hold few outbound connections, so the Dout rotation's second
loop moves several peers).  Planted rows alternate between holding every
topic and holding all but the last (they publish there through a fanout).

Run shape: meshes start dense (probability 0.9 on rows of at most 65
connections, the planted 65 included, 0.3 on longer ones: Dhi prunes in every class that can pass
Dhi), ticks 1-3, an opportunistic tick at 2, publications from tick 1 (every
planted row publishes in the last round of each tick, so its next emitGossip
advertises a message its neighbours have not seen), 1 % of the connections
down before tick 2 and up before tick 3 (with PX: a tenth, down before tick
1, so that the PRUNEs of the dense start list peers their receivers can
dial).  Before tick 3 every planted row loses all but KEEP of its
connections: the kernels of the long rows then run the small counts too.
The sinkhole state (Case.sink) runs ticks 1-5 and thins the rows at tick 2.

Two cases start topic 1 of the planted rows differently (Case.topic1; every
planted row of the short network holds topic 1, and one per planted class of
the tall one): `dout_max` from a mesh of up to 10 peers that all dialled the
row, so the outbound quota's graft runs on every class, the block, scratch
and streamed ones included; `all_score` from an empty mesh, so the Dlo graft
takes D of hundreds there.

The census assertion is a condition on the inputs, not on the engine: the
oracle alone decides it (test_case_reaches_its_branches, no GPU).  Each case
names, per branch, the row classes of the short network in which the branch
must be reached.  ALL is every class.  A narrower range is of one of two
kinds:
  structural  the rows of the other classes cannot take the branch: a mesh
              cannot pass Dhi = 12 on a row of 9 (about two thirds of a row
              hold a topic), so dhi_prune, rot_* and px_* start at class 1 or
              2 (big_d, Dhi = 32: at class 5); more than 64 PX candidates
              need class 4; a list cannot be cut to 100 among 85 candidates,
              nor left whole at PrunePeers = 64 among 300 (the upper ends of
              px_full, the lower ends of px_trunc_big); gossip_select needs
              more than Dlazy candidates (class 1; factor_big, Dlazy = 64 and
              factor 0.5: class 4); gossip_zero of factor_only needs fewer
              than 4 (classes 0 and 1)
  empirical   the other classes could take it but did not at these seeds:
              dlo_trunc (0, 4) of tight, dlo_trunc (1, 7) of all_score,
              opp_all (1, 5) and opp_trunc (4, 7) of opp_7, gossip_both
              (0, 2) of lazy_lt_dlo (the sinkhole cases reach it in ALL),
              fanout_topup (5, 7) of usual
On the tall network every named branch must be reached in each of the four
planted classes (fanout_topup: in the three that hold a fanout publisher);
its classes 0-4 are not asserted, the short network covers them.  neg_prune
is asserted by `usual`, everywhere.
"""
import numpy as np
import pytest

import oracle_binding as ob
from fixtures import beacon_params, planted, synthetic_state
from gsim import _abi, graphs
from gsim.params import GossipSubParams, PeerScoreThresholds, Second
from test_delivery import R, T0
from test_heartbeat import SEED, tick_time

SHORT_ROWS = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
TALL_ROWS = (1025, 2048, 2049, 4096, 4097, 8192, 8193)
SHAPE = {"short": (2000, 3, 2, SHORT_ROWS, 41), "tall": (9000, 2, 1, TALL_ROWS, 43)}
KEEP = 8                     # connections a planted row keeps once the others go down
_nets = {}


def network(kind, rare_out=False):
    """(net, hubs): the shared network and its planted rows [(peer, length)]."""
    key = (kind, rare_out)
    if key not in _nets:
        n, T, per_peer, rows, seed = SHAPE[kind]
        base = graphs.power_law(n, 8, 2.5, 64, seed=seed, n_topics=T, i0=1)   # planted()'s base
        bdeg = np.diff(base.row_ptr.astype(np.int64))
        ids = np.nonzero(bdeg <= min(rows))[0][-len(rows):]                 # short enough to plant on, highest numbered
        hubs = [(int(h), d) for h, d in zip(ids, rows)]
        assert all(bdeg[h] <= d for h, d in hubs)
        rng = np.random.default_rng(seed + 1)
        net = planted(n, T, seed, hubs, rng, 64, exact=True, dial=0.15 if rare_out else 0.5)
        # (planted()'s sybil IPs cover a whole network of this size: every peer its own IP but a few)
        ip_ids = np.arange(n, dtype=np.uint32)
        ip_ids[100:160] = 100 + np.arange(60, dtype=np.uint32) // 3
        net = graphs.with_ips(net, np.arange(n + 1, dtype=np.uint32), ip_ids, n)
        sub = graphs.zipf_subscriptions(n, T, per_peer, seed=seed + 2)
        for q, (h, _) in enumerate(hubs):
            sub[h] = (1 << T) - 1 if q % 2 == 0 else (1 << (T - 1)) - 1
        _nets[key] = (graphs.with_subscriptions(net, sub), hubs)
    net, hubs = _nets[key]
    deg = np.diff(net.row_ptr.astype(np.int64))
    for h, d in hubs:                                                       # the degree census
        assert deg[h] == d, f"planted row {h}: {deg[h]} connections, not {d}"
    rest = np.delete(deg, [h for h, _ in hubs])
    assert (rest <= 8).sum() >= 50 and rest.max() <= 64 + len(hubs), "the base: rows of at most 8, capped near 64"
    classes = np.unique(ob.row_class(deg))
    want = np.arange(8) if kind == "short" else np.r_[np.arange(4), 8:12]
    assert set(want) <= set(classes.tolist()), f"row classes {classes}"
    return net, hubs


# ---- the cases ------------------------------------------------------------------

USUAL = dict(D=8, Dlo=6, Dhi=12, Dscore=4, Dout=2)
ALL = (0, 7)                 # every row class of the short network
HUBS = (8, 11)               # the planted classes of the tall network


class Case:
    """reach: {branch: (lo, hi)}, the row classes of the short network in which
    the oracle must take the branch; tall: the branches it must take in each of
    the tall network's planted classes (None: the case does not run there)."""

    def __init__(self, cid, gp, reach, tall=None, rare_out=False, sink=False, px=False, behaviour=False,
                 topic_slots=0, shards=0, verdicts=False, seeds=(0, 0), topic1=None):
        self.id, self.gp, self.reach, self.tall, self.rare_out, self.sink = cid, gp, reach, tall, rare_out, sink
        self.px, self.behaviour, self.topic_slots, self.shards, self.verdicts = px, behaviour, topic_slots, shards, verdicts
        # the sinkhole state stays two more ticks: its planted rows run the small lists from tick 2
        # topic1: how topic 1 starts on the planted rows that hold it (every one of the short
        # network, one per planted class of the tall one): "inbound", a mesh of up to 10 peers
        # that all dialled the row (between Dlo and Dhi, no outbound peer: the outbound quota graft
        # on the long rows); "empty" (the Dlo graft takes D of hundreds); None: dense like the rest
        self.topic1 = topic1
        self.seeds = dict(short=seeds[0], tall=seeds[1])      # of the state, the schedule and the churn
        self.ticks = [1, 2, 3, 4, 5] if sink else [1, 2, 3]
        self.sparse_at = 2 if sink else 3

    def params(self):
        kw = dict(FanoutTTL=3 * Second, OpportunisticGraftTicks=2)
        kw.update(USUAL)
        kw.update(self.gp)
        if self.px:
            kw["PeerExchange"] = True
        return GossipSubParams(**kw)


def px_case(pp, reach, **kw):
    return Case(f"px_{pp}", dict(PrunePeers=pp), reach, px=True, **kw)


LAZY = dict(D=8, Dlo=6, Dhi=12, Dlazy=2, GossipFactor=0.0)
OFF = dict(Dlazy=0, GossipFactor=0.0)
GOSSIP = {"gossip_select": (1, 7), "gossip_all": ALL}
CASES = [
    Case("tight", dict(D=4, Dlo=4, Dhi=4, Dscore=2, Dout=1, Dlazy=4), {"dhi_prune": ALL, "dlo_all": ALL, "dlo_trunc": (0, 4)}),
    Case("d1", dict(D=1, Dlo=1, Dhi=2, Dscore=1, Dout=0, Dlazy=1), {"dhi_prune": ALL, "dlo_trunc": ALL, "gossip_select": ALL}),
    Case("no_quota", dict(D=6, Dlo=4, Dhi=8, Dscore=0, Dout=0), {"dhi_prune": (1, 7)}),
    Case("all_score", dict(D=6, Dlo=5, Dhi=9, Dscore=9, Dout=2), {"dhi_prune": (1, 7), "dlo_trunc": (1, 7)},
         tall=("dhi_prune", "dlo_trunc"), topic1="empty"),
    Case("dout_max", dict(D=8, Dlo=5, Dhi=12, Dscore=2, Dout=4),
         {"dhi_prune": (2, 7), "rot_pass1": (2, 7), "rot_pass2": (2, 7), "dout_graft": ALL},
         tall=("dhi_prune", "rot_pass1", "rot_pass2", "dout_graft"), rare_out=True, topic1="inbound", seeds=(1, 0)),
    Case("big_d", dict(D=24, Dlo=20, Dhi=32, Dscore=16, Dout=8, Dlazy=24),
         {"dhi_prune": (5, 7), "rot_pass2": (5, 7), "dlo_all": ALL}, tall=("dhi_prune", "rot_pass2"), rare_out=True),
    Case("lazy_lt_dlo", LAZY, {"gossip_fill": ALL, "gossip_two": ALL, "gossip_both": (0, 2)}),
    Case("lazy_lt_dlo_sink", LAZY, {"gossip_fill": ALL, "gossip_two": ALL, "gossip_both": ALL},
         tall=("gossip_fill", "gossip_two", "gossip_both"), sink=True, seeds=(2, 19)),
    Case("lazy_lt_dlo_slots", LAZY, {"gossip_fill": ALL, "gossip_two": ALL, "gossip_both": ALL}, sink=True, topic_slots=96,
         seeds=(17, 0)),
    Case("gossip_off", OFF, {"gossip_zero": ALL}, tall=("gossip_zero",)),
    Case("gossip_off_sink", OFF, {"gossip_zero": ALL, "gossip_fill": ALL}, tall=("gossip_zero", "gossip_fill"), sink=True),
    Case("factor_only", dict(Dlazy=0, GossipFactor=0.25), {"gossip_zero": (0, 1), "gossip_select": (1, 7), "gossip_two": ALL}),
    Case("factor_one", dict(Dlazy=1, GossipFactor=1.0), {"gossip_all": ALL}),
    Case("factor_big", dict(Dlazy=64, GossipFactor=0.5), {"gossip_all": ALL, "gossip_select": (4, 7)},
         tall=("gossip_all", "gossip_select")),
    Case("opp_all", dict(OpportunisticGraftPeers=0, OpportunisticGraftTicks=1), {"opp_all": ALL}, tall=("opp_all",)),
    Case("opp_7", dict(OpportunisticGraftPeers=7), {"opp_trunc": (4, 7), "opp_all": (1, 5)}),
    px_case(1, {"px_trunc_small": (2, 4), "px_trunc_big": (4, 7)}),
    px_case(3, {"px_trunc_small": (2, 4), "px_trunc_big": (4, 7)}),
    px_case(64, {"px_full": (2, 4), "px_trunc_big": (4, 7)}, shards=2),
    px_case(65, {"px_full": (2, 4), "px_trunc_big": (4, 7)}, tall=("px_trunc_big",)),
    Case("px_65_slots", dict(PrunePeers=65), {"px_full": (2, 4), "px_trunc_big": (4, 7)}, px=True, topic_slots=96),
    px_case(100, {"px_full": (2, 5), "px_trunc_big": (5, 7)}, tall=("px_trunc_big",)),
    px_case(256, {"px_full": (2, 6), "px_trunc_big": (6, 7)}),
    px_case(300, {"px_full": (2, 7), "px_trunc_big": (6, 7)}, tall=("px_trunc_big",)),
    Case("hist_1_1", dict(HistoryLength=1, HistoryGossip=1), GOSSIP, behaviour=True),
    Case("hist_6_6", dict(HistoryLength=6, HistoryGossip=6), GOSSIP, behaviour=True),
    Case("hist_12_1", dict(HistoryLength=12, HistoryGossip=1), GOSSIP, behaviour=True),
    Case("ihave_min", dict(MaxIHaveMessages=1, MaxIHaveLength=1, IWantFollowupTime=1 * Second), GOSSIP, behaviour=True),
    Case("usual", dict(),
         {"dhi_prune": (2, 7), "px_full": (2, 3), "px_trunc_small": (2, 4), "px_trunc_big": (4, 7), "gossip_select": (1, 7),
          "gossip_all": ALL, "fanout_topup": (5, 7), "neg_prune": ALL},
         tall={"dhi_prune": HUBS, "px_trunc_big": HUBS, "gossip_select": HUBS, "gossip_all": HUBS, "neg_prune": HUBS,
               "fanout_topup": (8, 10)}, px=True, verdicts=True),
]
BY_ID = {c.id: c for c in CASES}
RUNS = [(c.id, "short") for c in CASES] + [(c.id, "tall") for c in CASES if c.tall is not None]


def check_census(case, kind, table):
    want = case.reach if kind == "short" else case.tall if isinstance(case.tall, dict) else {b: HUBS for b in case.tall}
    for b, (lo, hi) in want.items():
        missed = [c for c in range(lo, hi + 1) if table[b][c] == 0]
        assert not missed, f"{case.id}/{kind}: branch {b} not reached in row classes {missed} (counts {table[b]})"


# ---- one run ----------------------------------------------------------------------

def setup(case, kind):
    from tickrun import restrict_to_subscriptions, subscribed_schedule
    net, hubs = network(kind, case.rare_out)
    n, T = net.n, SHAPE[kind][1]
    rng = np.random.default_rng(sum(map(ord, case.id)) + (7 if kind == "tall" else 0) + 1000 * case.seeds[kind])
    params = beacon_params(T, RetainScore=3 * Second)
    thk = dict(GossipThreshold=-100, PublishThreshold=-200, GraylistThreshold=-300, AcceptPXThreshold=0.0,
               OpportunisticGraftThreshold=1000.0)
    th = PeerScoreThresholds(**thk)
    gp = case.params()
    p5 = None
    keep = {}                                           # the connections a planted row keeps at tick 3
    for h, _ in hubs:
        row = net.col[net.row_ptr[h]:net.row_ptr[h + 1]]
        keep[h] = rng.choice(row, size=min(KEEP, len(row)), replace=False)
    if case.sink:
        # every peer but the planted rows and four neighbours of each far below the gossip
        # threshold: a planted row has fewer than Dlo gossip candidates and hundreds of topic
        # peers.  Four more neighbours sit between the thresholds (never grafted: candidates
        # that stay candidates).
        p5 = np.full(n, -1000.0)
        for h, _ in hubs:
            p5[keep[h][:4]] = 0.0
            p5[keep[h][4:8]] = -50.0
        p5[[h for h, _ in hubs]] = 0.0
    st = ob.NetState(net, params, thresholds=th, gossip=gp, p5=p5)
    deg = np.diff(net.row_ptr.astype(np.int64))
    synthetic_state(st, rng, tick_time(0), np.where(deg[net.owner()] <= 65, 0.9, 0.3))
    restrict_to_subscriptions(st, net)
    if case.topic1:
        for h, _ in hubs:
            if not (int(net.sub[h]) >> 1) & 1:
                continue
            b, en = int(net.row_ptr[h]), int(net.row_ptr[h + 1])
            for f in ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags"):
                getattr(st, f)[1, b:en] = 0
            if case.topic1 == "inbound":
                e = b + np.nonzero((net.outbound[b:en] == 0) & (((net.sub[net.col[b:en]] >> np.uint64(1)) & np.uint64(1)) != 0))[0]
                e = rng.choice(e, size=min(10, len(e)), replace=False)
                st.tflags[1, e] = _abi.TF_IN_MESH | _abi.TF_MESH
                st.graft_time[1, e] = tick_time(0) - 100 * Second
                st.mesh_time[1, e] = 100 * Second
    verdicts = [0.85, 0.05, 0.04, 0.03, 0.03] if case.verdicts else None
    sched = subscribed_schedule(rng, case.ticks, net, T, 2.0, 0.0, member_only=False, verdicts=verdicts)
    mid = 1 + max((m[0] for b in sched.values() for m in b), default=0)
    for k in case.ticks:                                # the planted rows, in every topic (fanout in the last for half)
        for h, _ in hubs:
            for t in range(T):
                sched.setdefault(k * R + R - 1, []).append((mid, t, h, 0))
                mid += 1
    own = net.owner()
    und = np.stack([own, net.col], axis=1)
    und = und[und[:, 0] < und[:, 1]]
    down = und[rng.choice(len(und), size=len(und) // (10 if case.px else 100), replace=False)]
    # before tick 3 every planted row loses all but KEEP of its connections: the long rows'
    # kernels then run the small counts (took-all grafts, the gossip fill, target >= n, n < 4)
    lost = np.concatenate([np.stack([np.full(net.row_ptr[h + 1] - net.row_ptr[h], h),
                                     net.col[net.row_ptr[h]:net.row_ptr[h + 1]]], axis=1)[
        ~np.isin(net.col[net.row_ptr[h]:net.row_ptr[h + 1]], keep[h])] for h, _ in hubs]).astype(np.int64)
    lost = np.unique(np.sort(lost, axis=1), axis=0)
    # (with PX the connections go down before tick 1: the PRUNEs of the dense start then list
    # peers their receivers can dial)
    churn = {1: [], 2: [], 3: [(down, True)]}
    churn[1 if case.px else 2].append((down, False))
    churn[case.sparse_at].append((lost, False))
    behaviour = None
    if case.behaviour:
        behaviour = (rng.random(n) < 0.3).astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT
    return net, params, th, gp, st, p5, sched, churn, behaviour


def oracle_run(case, kind):
    """The oracle's half of tickrun.run_parity alone, with the census on."""
    net, params, th, gp, st, p5, sched, churn, behaviour = setup(case, kind)
    T = st.T
    ring = T * case.topic_slots if case.topic_slots else 1024
    msgs = ob.Msgs(net.n, T, ring, R, T0, Second, behaviour=behaviour, topic_slots=case.topic_slots)
    lib = ob.load()
    marks = dialled = 0
    with ob.Census() as census:
        for kk in case.ticks:
            now = tick_time(kk)
            for (pairs, up) in churn.get(kk, []):
                st.churn(pairs, up=up, now=now - Second // 2)
            v = st.view()
            lib.orc_refresh_scores(v, now)
            msgs.penalties(st, now)
            lib.orc_ip_colocation(v)
            lib.orc_compute_scores(v)
            msgs.heartbeat(st, kk, now, SEED)
            marks += int(msgs.ihave_marks(net.e).sum())
            for g in range(kk * R, kk * R + R):
                for (mid, t, o, inv) in sched.get(g, []):
                    msgs.publish(st, mid, t, o, inv, g)
                msgs.round(st, g)
            if gp.PeerExchange:
                dialled += len(st.px_connect(now + Second // 2))
    return census.table, marks, dialled


@pytest.mark.parametrize("cid,kind", RUNS)
def test_case_reaches_its_branches(cid, kind):
    """The inputs of every case: the oracle alone takes the branches the case
    names, in every row class that can (no GPU)."""
    case = BY_ID[cid]
    table, marks, dialled = oracle_run(case, kind)
    check_census(case, kind, table)
    assert dialled > 0 or not case.px, "PX made connections"
    if cid.startswith("gossip_off"):
        assert marks == 0, "gossip switched off: no IHAVE"
    else:
        assert marks > 0, "the heartbeats emitted gossip"


@pytest.mark.gpu
@pytest.mark.parametrize("cid,kind", RUNS)
def test_param_space_bit_exact(require_gpu, cid, kind):
    from gsim.engine import Engine
    from tickrun import run_parity
    case = BY_ID[cid]
    net, params, th, gp, st, p5, sched, churn, behaviour = setup(case, kind)
    if case.shards:
        from gsim.shard import ShardedEngine
        eng = ShardedEngine(params, th, gossip=gp, shards=case.shards)
    else:
        eng = Engine(params, th, gossip=gp)
    eng.load_graph(net)
    if p5 is not None:
        eng.set_app_score(p5)
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    marks, px, mesh1, px_sent = [], [], {}, {}
    _, hubs = network(kind, case.rare_out)

    def hub_mesh(st_, h):
        return ((st_.tflags[:, net.row_ptr[h]:net.row_ptr[h + 1]] & _abi.TF_MESH) != 0).sum(axis=1)

    mesh0 = {h: hub_mesh(st, h) for h, _ in hubs}

    def after_heartbeat(kk, eng_, st_, msgs):
        marks.append(int(msgs.ihave_marks(net.e).sum()))
        if kk == 1:
            mesh1.update({h: hub_mesh(st_, h) for h, _ in hubs})
            for h, _ in hubs:                           # PRUNEs with PX: only the Dhi prune sends them
                out = st_.ctl[0][:, st_.rev[net.row_ptr[h]:net.row_ptr[h + 1]]]
                px_sent[h] = bool((out & _abi.CTL_PX).any())

    with ob.Census() as census:
        msgs, gstats = run_parity(net, params, th, gp, st, case.ticks, sched, ring=1024, behaviour=behaviour, churn=churn,
                                  eng=eng, after_heartbeat=after_heartbeat, px_log=px, topic_slots=case.topic_slots)
    print(f"{cid}/{kind}: IHAVE marks per tick {marks}, engine gossip {gstats}, PX connections {px}")
    check_census(case, kind, census.table)
    if cid.startswith("gossip_off"):
        # (ihave_walks counts the unseen (receiver, message) pairs examined, advertised or not)
        assert sum(marks) == 0 and gstats["iwant_ids"] == 0 and gstats["iwant_responses"] == 0, \
            f"gossip switched off: no IHAVE on either side ({marks}, {gstats})"
    else:
        assert sum(marks) > 0 and gstats["iwant_ids"] > 0, "gossip ran on both sides and was asked for"
    if case.px:
        assert sum(px) > 0, "PX made connections"
    if cid in ("usual", "tight"):
        # the class boundaries themselves: every planted row started over Dhi in a topic and was
        # brought to Dhi at most (negative-score prunes alone) or cut to D (plus the outbound
        # quota's graft).  At the usual setting the rows of 8, 9, 16
        # and 17 connections are too short to pass Dhi = 12 in one topic (about two thirds of a
        # row hold it); at `tight` (Dhi = 4) they pass it too.
        for h, d in hubs:
            over = mesh0[h] > gp.Dhi
            assert (cid == "usual" and d < 32) or over.any(), f"planted row of {d}: meshes {mesh0[h]} start under Dhi"
            assert cid != "usual" or d < 32 or px_sent[h], f"planted row of {d}: no PRUNE with PX, so no Dhi prune"
            assert (mesh1[h][over] <= max(gp.Dhi, gp.D + gp.Dout)).all(), f"planted row of {d}: {mesh0[h]} -> {mesh1[h]}"

"""Parity over the message clock and ring: rounds, heartbeat, slot reuse.

Every other parity run uses one gsim_msg_config clock (10 rounds a tick, a
heartbeat of one second, ticks from 1, sequential ids, a ring that holds the
whole run).  Here each case is one tickrun.run_parity (every plane, the
seen-set, lastput, the totals, and the trace where named, bit for bit after
every tick) at another clock or ring; the events it aims at are counted from
the oracle's event log (test_case_reaches_its_events, no GPU), each with a
minimum.

Networks (test_score_space.network, never modified):
  regular  random_regular(1500, 16), T = 3, dense start
  short    2000 peers with planted rows to 1024 connections
Common to every case unless it says otherwise: 30 % of the peers ignore
IWANT (`hb_100ms` on 2 shards: 70 %, see the case), CUT peers a tick are taken out of every mesh after the heartbeat (on
both sides: they recover by IHAVE / IWANT; on shards between two ticks, so
they miss what is sent before their GRAFTs are handled), publications in every round, 5 %
rejected, an opportunistic tick every second tick.

The counted events (from the log, per run):
  ans_r0        IWANT answers (EV_RPC_MSG, x = 1) arriving in round 0 of a tick:
                with two rounds a tick that is the tick after their request
  ans_last      answers arriving in a tick's last round
  first_last    first deliveries in a tick's last round (committed by the next
                tick's flush)
  ans_down      IWANTs whose connection went down before their answer's round
  ans_lost      answers sent and lost with their connection (EV_RPC_MSG, x = 3)
  tr_ans, tr_iwant  traced answers / IWANTs (reasons 1 and 2) whose SEND and RECV
                lie on different sides of a heartbeat / in one tick
  lat_1..lat_4  first validations completing 1..4 ticks after the publication
  dup_cross     duplicates received while the first copy validates, credited
                after a later heartbeat
  broken, broken_late  broken promises, each matched to its AddPromise in the log;
                those made 30 or more heartbeats before the pass that broke them
  repub, repub_live    publications into a slot used before; those in a tick
                in which other messages were promised
  serves        IWANTs served (GetForPeer counts, keyed by id)
  high_rounds   seen-set cells above 2^31 - 64 at the end
  win_*         the score census's window events (ORC_SB_WIN_*)

The oracle's counts per case (test_case_reaches_its_events prints them; min_gap: the
fewest rounds between a slot's last first delivery and its republication, the guard
being 14):
  r2/regular                 ans_r0 1469
  r2/short                   ans_r0 11137
  r2_churn/regular           ans_r0 1740, ans_down 41, ans_lost 11
  r2_churn/regular/2 shards  ans_r0 1570, ans_down 32, ans_lost 12
  r2_step/regular            ans_r0 1200
  r2_trace/regular           tr_ans 282, tr_iwant 1621
  r3/regular                 ans_last 1781, first_last 22522
  r6_window/regular          win_inside 102627, win_edge 21038, win_outside 124532
  r2_lat/regular             lat_1 2751, lat_2 13107, lat_3 4150, lat_4 4965, dup_cross 8455
  r3_lat/regular             lat_1 17156, lat_2 12295, lat_3 8468, lat_4 6401, dup_cross 12836
  hb_100ms/regular           broken 35, broken_late 35, ans_r0 10362
  wrap/regular               repub 150, repub_live 150, ans_r0 10003, min_gap 14
  wrap_slots/regular         repub 30, repub_live 30, ans_r0 1622, min_gap 15
  wrap/regular/2 shards      repub 150, repub_live 150, ans_r0 8142, min_gap 16
  ring_1/regular             repub 2, min_gap 16
  ring_33/regular            repub 39, repub_live 39, ans_r0 2083, min_gap 14
  ring_63/regular            repub 74, repub_live 74, ans_r0 4574, min_gap 14
  ring_65/regular            repub 76, repub_live 76, ans_r0 4612, min_gap 14
  ring_301/regular           repub 352, repub_live 352, ans_r0 21223, min_gap 14
  slots_1/regular            repub 21, min_gap 16
  slots_33/regular           repub 117, repub_live 117, ans_r0 6884, min_gap 14
  ring_8192/regular          serves 1314
  ids/regular                serves 758, repub 1, min_gap 15
  ids_slots/regular          serves 694
  far/regular                high_rounds 161149, ans_r0 4157
  far_lat/regular            ans_r0 3230, lat_1 1207
  r2/regular/2 shards        ans_r0 1268
  hb_100ms/regular/2 shards  broken 28, broken_late 28
"""
from dataclasses import replace

import numpy as np
import pytest

import oracle_binding as ob
from fixtures import beacon_params, synthetic_state
from gsim import _abi
from gsim.params import GossipSubParams, PeerScoreThresholds, Second
from test_delivery import T0
from test_gossip import cut_mesh
from test_heartbeat import SEED
from test_score_space import GP, TH, T, network

CUT = 6
WRAP_GP = dict(HistoryLength=2, HistoryGossip=1, IWantFollowupTime=1 * Second)
SPACING = 12                 # ticks between two publications into one slot in the wrap cases
FAR = 1073741800             # `far`: ticks FAR .. FAR + 22, the last round is 2^31 - 3
MS = Second // 1000


def prom_ticks(rounds, hb, followup):
    """gsim.h: the promise ring's length in ticks."""
    return (hb // (rounds + 1) + followup) // hb + 2


def reuse_guard(gp, rounds, hb):
    return (max(gp.HistoryLength, gp.HistoryGossip) + prom_ticks(rounds, hb, gp.IWantFollowupTime) + 2) * rounds


class Case:
    def __init__(self, cid, kind="regular", rounds=2, hb=Second, ticks=6, first=1, ring=1024, topic_slots=0, shards=0,
                 gp=None, vdelays=None, churn=0.0, step=False, trace=None, rate=4.0, cut=CUT, wrap=False, ids=False,
                 window=False, seed=0, ignore=0.3, quiet=False, reach=None):
        self.id, self.kind, self.rounds, self.hb, self.first = cid, kind, rounds, hb, first
        self.ticks = list(range(first, first + ticks))
        self.ring, self.topic_slots, self.shards, self.gp = ring, topic_slots, shards, gp or {}
        self.vdelays, self.churn, self.step, self.trace, self.rate, self.cut = vdelays, churn, step, trace, rate, cut
        self.wrap, self.ids, self.window, self.seed, self.reach = wrap, ids, window, seed, reach or {}
        self.ignore, self.quiet = ignore, quiet

    @property
    def run_id(self):
        return f"{self.id}/{self.kind}" + (f"/{self.shards} shards" if self.shards else "")

    @property
    def n_ring(self):
        return T * self.topic_slots if self.topic_slots else self.ring


def wrap_case(cid, ring=0, topic_slots=0, wraps=2, **kw):
    reach = kw.pop("reach", dict(repub=20, repub_live=20, ans_r0=20))
    return Case(cid, ring=ring, topic_slots=topic_slots, gp=WRAP_GP, ticks=wraps * SPACING + 2, wrap=True, reach=reach,
                **kw)


R2 = dict(ans_r0=20)
LAT = dict(lat_1=20, lat_2=20, lat_3=20, lat_4=20, dup_cross=20)
CASES = [
    Case("r2", reach=R2),
    Case("r2", "short", reach=R2),
    Case("r2_churn", churn=0.01, trace=(0, 400), reach=dict(ans_r0=20, ans_down=5, ans_lost=5)),
    Case("r2_churn", churn=0.01, shards=2, reach=dict(ans_r0=20, ans_down=5, ans_lost=5)),
    Case("r2_step", step=3, cut=0, reach=R2),
    Case("r2_trace", ticks=4, trace=(0, 700), reach=dict(tr_ans=20, tr_iwant=20)),
    Case("r3", rounds=3, reach=dict(ans_last=20, first_last=20)),
    Case("r6_window", rounds=6, window=True, ticks=4, reach=dict(win_inside=20, win_edge=20, win_outside=20)),
    Case("r2_lat", vdelays=tuple(range(8)), ticks=8, reach=LAT),
    Case("r3_lat", rounds=3, vdelays=tuple(range(8)), ticks=8, reach=LAT),
    Case("hb_100ms", hb=100 * MS, ticks=45, rate=2.0, cut=16, reach=dict(broken=20, broken_late=20, ans_r0=20)),
    wrap_case("wrap", ring=128),
    wrap_case("wrap_slots", topic_slots=8),
    wrap_case("wrap", ring=128, shards=2),
    wrap_case("ring_1", ring=1, reach=dict(repub=2)),
    wrap_case("ring_33", ring=33),
    wrap_case("ring_63", ring=63),
    wrap_case("ring_65", ring=65),
    wrap_case("ring_301", ring=301, seed=1),
    # (one slot a topic: three republications a wrap, so seven wraps, 86 ticks; nothing else is
    # live when a slot is republished, so no repub_live; a quiet network: no P3 / P3b, see setup)
    wrap_case("slots_1", topic_slots=1, wraps=7, quiet=True, reach=dict(repub=20)),
    wrap_case("slots_33", topic_slots=33),
    Case("ring_8192", rounds=10, ring=8192, ticks=3, rate=8.0, reach=dict(serves=20)),
    Case("ids", ring=64, gp=WRAP_GP, ticks=11, ids=True, trace=(0, 700), reach=dict(serves=20, repub=1)),
    Case("ids_slots", topic_slots=8, gp=WRAP_GP, ticks=11, ids=True, trace=(0, 700), reach=dict(serves=20)),
    Case("far", first=FAR, ticks=23, rate=2.0, reach=dict(high_rounds=20, ans_r0=20)),
    # (20 ticks: the last round, 2^31 - 9, is the last one a latency may run in, see
    # test_completion_round_beyond_a_cell_is_refused)
    Case("far_lat", first=FAR, ticks=20, rate=2.0, vdelays=tuple(range(8)), reach=dict(ans_r0=20, lat_1=20)),
    Case("r2", shards=2, reach=R2),
    # (70 % of the peers ignore IWANT here, not 30 %: cut between ticks, a peer is grafted again at
    # the next heartbeat and at 30 % fewer than 20 promises break, 6 in the oracle)
    Case("hb_100ms", hb=100 * MS, ticks=45, rate=2.0, cut=16, shards=2, ignore=0.7, reach=dict(broken=20, broken_late=20)),
]
BY_ID = {c.run_id: c for c in CASES}
RUNS = list(BY_ID)
assert len(RUNS) == len(CASES)


def round_time(case, g):
    R, hb = case.rounds, case.hb
    return T0 + (g // R) * hb + ((g % R + 1) * hb) // (R + 1)


def wrap_schedule(case, rng, net):
    """Message i goes to slot i % ring (sub-rings: its topic's next slot) in
    tick first + (i * SPACING) // ring: a slot is republished every SPACING
    ticks exactly, 5 % rejected."""
    R, sched = case.rounds, {}
    per_topic = case.topic_slots or 0
    n_slots = per_topic if per_topic else case.ring
    i = 0
    while True:
        k = case.first + (i * SPACING) // n_slots
        if k > case.ticks[-1]:
            break
        g = k * R + int(rng.integers(0, R))
        for t in (range(T) if per_topic else [int(rng.integers(0, T))]):
            sched.setdefault(g, []).append((i * T + t if per_topic else i, t, int(rng.integers(0, net.n)),
                                            int(rng.random() < 0.05)))
        i += 1
    return sched


def id_schedule(case, rng, net):
    """Two messages a tick with ids from the whole uint64 range and distinct
    residues mod 64 (2^63 and 2^64 - 1 among them), topic i % 3; in the dense
    ring the last tick republishes message 0's slot with its id + 64 * 2^40."""
    R, sched = case.rounds, {}
    res = rng.permutation(np.arange(1, 63))
    ids = [(1 << 63), (1 << 64) - 1] + [int(r) + 64 * int(rng.integers(0, 1 << 57)) for r in res]
    i = 0
    for k in case.ticks[:-1]:
        for _ in range(2):
            sched.setdefault(k * R + int(rng.integers(0, R)), []).append((ids[i], i % T, int(rng.integers(0, net.n)), 0))
            i += 1
    if not case.topic_slots:
        sched.setdefault(case.ticks[-1] * R + R - 1, []).append(((1 << 63) + (64 << 40), 0, int(rng.integers(0, net.n)), 0))
    return sched


def setup(case):
    from tickrun import restrict_to_subscriptions, subscribed_schedule
    net = network(case.kind)
    R, hb = case.rounds, case.hb
    rng = np.random.default_rng(sum(map(ord, case.id + case.kind)) + 1000 * case.seed)
    params = beacon_params(T, RetainScore=3 * Second)
    if case.window:
        # a duplicate one round after the first copy: at the window's edge in topic 0, 1 ns
        # outside in topic 1, 1 ns inside in topic 2
        one = round_time(case, R + 1) - round_time(case, R)
        names = sorted(params.Topics)
        params.Topics = {n: replace(params.Topics[n], MeshMessageDeliveriesWindow=one + (0, -1, 1)[q])
                         for q, n in enumerate(names)}
    if case.quiet:
        # three messages in twelve ticks: the mesh-delivery deficit (a threshold of 100 a topic)
        # would put every peer under the graylist within twenty ticks; P3 and P3b are switched off
        params.Topics = {n: replace(tp, MeshMessageDeliveriesWeight=0.0, MeshFailurePenaltyWeight=0.0)
                         for n, tp in params.Topics.items()}
    th = PeerScoreThresholds(**TH)
    gp = GossipSubParams(**{**GP, **case.gp})
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    deg = np.diff(net.row_ptr.astype(np.int64))
    synthetic_state(st, rng, T0 + (case.first - 1) * hb,
                    0.7 if case.kind == "regular" else np.where(deg[net.owner()] <= 65, 0.9, 0.3))
    restrict_to_subscriptions(st, net)
    if case.wrap:
        sched = wrap_schedule(case, rng, net)
    elif case.ids:
        sched = id_schedule(case, rng, net)
    else:
        sched = subscribed_schedule(rng, case.ticks, net, T, case.rate, 0.05, member_only=True, vdelays=case.vdelays,
                                    rounds=R)
    churn = {}
    if case.churn:
        own = net.owner()
        und = np.stack([own, net.col], axis=1)
        und = und[und[:, 0] < und[:, 1]]
        prev = None
        for k in case.ticks:
            down = und[rng.choice(len(und), size=int(len(und) * case.churn), replace=False)]
            churn[k] = ([(prev, True)] if prev is not None else []) + [(down, False)]
            prev = down
    behaviour = (rng.random(net.n) < case.ignore).astype(np.uint8) * ob.ORC_BEHAVE_IGNORE_IWANT
    cuts = {k: rng.choice(net.n, size=case.cut, replace=False) for k in case.ticks} if case.cut else {}
    return dict(net=net, params=params, th=th, gp=gp, st=st, sched=sched, churn=churn, behaviour=behaviour, cuts=cuts)


class Counter:
    """Counts a case's events from the oracle's log, tick by tick."""

    def __init__(self, case, c):
        self.case, self.c = case, c
        self.n = dict(ans_r0=0, ans_lost=0, ans_last=0, first_last=0, ans_down=0, tr_ans=0, tr_iwant=0, lat_1=0, lat_2=0, lat_3=0,
                      lat_4=0, dup_cross=0, broken=0, broken_late=0, repub=0, repub_live=0, serves=0, high_rounds=0,
                      min_gap=1 << 40)
        self.pub_tick, self.used, self.done, self.dups, self.last, self.made = {}, {}, {}, [], {}, {}
        self.down = {k: {(int(a), int(b)) for p, up in v if not up for a, b in p} for k, v in c["churn"].items()}

    def add(self, ev, msgs, kk):
        case, n, R = self.case, self.n, self.case.rounds
        kind, g, x, a, b, mid = ev["kind"], ev["g"], ev["x"], ev["a"], ev["b"], ev["mid"]
        ans = (kind == ob.EV_RPC_MSG) & (x == 1)
        n["ans_r0"] += int((ans & (g % R == 0)).sum())
        n["ans_last"] += int((ans & (g % R == R - 1)).sum())
        n["ans_lost"] += int(((kind == ob.EV_RPC_MSG) & (x == 3)).sum())
        first = (kind == ob.EV_SEEN) & (x == 1) & (b != 0xFFFFFFFF)
        n["first_last"] += int((first & (g % R == R - 1)).sum())
        n["serves"] += int((kind == ob.EV_SERVE).sum())
        iw = kind == ob.EV_RPC_IWANT
        if case.trace:
            lo, hi = case.trace
            inr = ((a >= lo) & (a < hi)) | ((b >= lo) & (b < hi))
            n["tr_ans"] += int((ans & inr & ((g - 1) // R != g // R)).sum())
            n["tr_iwant"] += int((iw & inr & ((g + 1) // R == g // R)).sum())
        for q in np.nonzero(iw)[0] if self.down else []:
            # the answer arrives two rounds after the IWANT was sent
            dn = self.down.get(int(g[q] + 2) // R, set()) if (int(g[q]) + 2) // R != int(g[q]) // R else set()
            pa, pb = int(a[q]), int(b[q])
            n["ans_down"] += (min(pa, pb), max(pa, pb)) in dn
        pub = np.nonzero(kind == ob.EV_PUBLISH)[0]
        promised = int((kind == ob.EV_PROMISE).sum())
        for q in pub:
            self.pub_tick[int(mid[q])] = int(g[q]) // R
        if case.wrap or case.ids:
            fs = (kind == ob.EV_SEEN) & (x == 1)
            um, inv = np.unique(mid[fs], return_inverse=True)
            top = np.full(len(um), -1, dtype=np.int64)
            np.maximum.at(top, inv, g[fs])
            for m_, g_ in zip(um, top):
                self.last[int(m_)] = max(self.last.get(int(m_), -1), int(g_))
            for rnd in range(kk * R, kk * R + R):
                for msg in self.c["sched"].get(rnd, []):
                    slot = self.slot_of(msg)
                    if slot in self.used:
                        n["repub"] += 1
                        n["repub_live"] += promised > 0
                        # the engine's guard: rounds since the last first delivery of the slot's old message
                        n["min_gap"] = min(n["min_gap"], rnd - self.last[self.used[slot]])
                    self.used[slot] = msg[0]
        if case.vdelays:
            for q in np.nonzero(first)[0]:
                off = int(g[q]) // R - self.pub_tick[int(mid[q])]
                if 1 <= off <= 4:
                    n[f"lat_{off}"] += 1
                self.done[(int(a[q]), int(mid[q]))] = int(g[q])
            self.dups += [(int(a[q]), int(mid[q]), int(g[q])) for q in np.nonzero((kind == ob.EV_SEEN) & (x == 0))[0]]
            left = []
            for (p, m, gd) in self.dups:
                if (p, m) in self.done:
                    n["dup_cross"] += gd < self.done[(p, m)] and gd // R < self.done[(p, m)] // R
                else:
                    left.append((p, m, gd))          # (its first copy still validates)
            self.dups = left
        # broken promises, each matched to its AddPromise: EV_PROMISE (router, advertiser, id, made at x)
        # stays outstanding until the router's EV_FULFILL of the id; EV_BROKEN (router, advertiser,
        # count) at the penalty pass of this tick takes the pair's outstanding promises that expired
        # (made + IWantFollowupTime < now), and their number must be its count
        if "broken" in case.reach:
            now, follow = T0 + kk * case.hb, self.c["gp"].IWantFollowupTime
            sel = (kind == ob.EV_BROKEN) | (kind == ob.EV_PROMISE) | (kind == ob.EV_FULFILL)
            for q in np.nonzero(sel)[0]:
                k_, r_, m_ = int(kind[q]), int(a[q]), int(mid[q])
                mine = self.made.setdefault(r_, {})
                if k_ == ob.EV_PROMISE:
                    mine.setdefault((m_, int(b[q])), (int(x[q]), kk))     # (AddPromise keeps an earlier one)
                elif k_ == ob.EV_FULFILL:
                    for key in [key for key in mine if key[0] == m_]:
                        del mine[key]
                else:
                    gone = [key for key, (t_, _) in mine.items() if key[1] == int(b[q]) and t_ + follow < now]
                    assert len(gone) == int(x[q]), f"router {r_}: {int(x[q])} promises of {int(b[q])} broke, {len(gone)} matched"
                    for key in gone:
                        n["broken"] += 1
                        n["broken_late"] += kk - mine.pop(key)[1] >= 30
        n["high_rounds"] = int(((msgs.seen != ob.UNSEEN) & (msgs.seen > (1 << 31) - 64)).sum())

    def slot_of(self, msg):
        if not self.case.topic_slots:
            return msg[0] % self.case.ring
        cnt = self.__dict__.setdefault("tcount", [0] * T)
        cnt[msg[1]] += 1
        return msg[1] * self.case.topic_slots + (cnt[msg[1]] - 1) % self.case.topic_slots


def check_reach(case, counts):
    if case.id == "hb_100ms":
        assert prom_ticks(case.rounds, case.hb, GossipSubParams(**{**GP, **case.gp}).IWantFollowupTime) == 32
    if case.wrap or case.ids:
        guard = reuse_guard(GossipSubParams(**{**GP, **case.gp}), case.rounds, case.hb)
        assert counts["min_gap"] >= guard, f"{case.run_id}: a slot republished {counts['min_gap']} rounds after its last " \
                                           f"first delivery, the guard is {guard}"
    missed = {e: (counts[e], lo) for e, lo in case.reach.items() if counts[e] < lo}
    assert not missed, f"{case.run_id}: events under their minimum (count, minimum): {missed}"


def oracle_run(case):
    """The oracle's half of run_parity alone, with the event log and the score census on."""
    c = setup(case)
    net, st, sched, R, hb = c["net"], c["st"], c["sched"], case.rounds, case.hb
    msgs = ob.Msgs(net.n, T, case.n_ring, R, T0, hb, behaviour=c["behaviour"], topic_slots=case.topic_slots)
    msgs.log()
    lib = ob.load()
    cnt = Counter(case, c)
    with ob.ScoreCensus() as census:
        for kk in case.ticks:
            now = T0 + kk * hb
            for (pairs, up) in c["churn"].get(kk, []):
                st.churn(pairs, up=up, now=now - hb // 2)
            v = st.view()
            lib.orc_refresh_scores(v, now)
            msgs.penalties(st, now)
            lib.orc_ip_colocation(v)
            lib.orc_compute_scores(v)
            msgs.heartbeat(st, kk, now, SEED)
            for p in c["cuts"].get(kk, []) if not case.shards else []:
                cut_mesh(net, st, int(p))
            for g in range(kk * R, kk * R + R):
                for m in sched.get(g, []):
                    msgs.publish(st, m[0], m[1], m[2], m[3], g, vdelay=m[4] if len(m) > 4 else 0)
                msgs.round(st, g)
            cnt.add(msgs.events(), msgs, kk)
            for p in c["cuts"].get(kk + 1, []) if case.shards else []:
                cut_mesh(net, st, int(p))
    cnt.n.update({k: v for k, v in census.table.items() if k.startswith("win_")})
    return cnt.n, msgs


@pytest.mark.parametrize("rid", RUNS)
def test_case_reaches_its_events(rid):
    """The inputs of every case: the oracle alone produces the events the case
    names, each at least as often as stated (no GPU)."""
    case = BY_ID[rid]
    counts, msgs = oracle_run(case)
    print(rid, {k: counts[k] for k in list(case.reach) + ["min_gap"]}, "totals", msgs.stats)
    check_reach(case, counts)
    assert msgs.stats[1] > 0 and msgs.stats[2] > 0, "messages were delivered, with duplicates"


@pytest.mark.gpu
@pytest.mark.parametrize("rid", RUNS)
def test_clock_space_bit_exact(require_gpu, rid):
    """One run_parity at the case's clock and ring: every plane, the seen-set,
    lastput and the totals after every tick (every gsim_step call), the trace
    where the case has one.  What each case reaches, with the oracle's counts:
    the module docstring; test_case_reaches_its_events asserts the minimum."""
    from gsim.engine import Engine
    from tickrun import run_parity
    case = BY_ID[rid]
    c = setup(case)
    net, params, th, gp, st = c["net"], c["params"], c["th"], c["gp"], c["st"]
    if case.shards:
        from gsim.shard import ShardedEngine
        eng = ShardedEngine(params, th, gossip=gp, shards=case.shards)
    else:
        eng = Engine(params, th, gossip=gp)
    eng.load_graph(net)
    eng.set_seed(SEED)
    st.push_to_engine(eng)

    def cut(kk, st_):
        if len(c["cuts"].get(kk, [])):
            for p in c["cuts"][kk]:
                cut_mesh(net, st_, int(p))
            eng.write(_abi.F_TFLAGS, st_.tflags)
            eng.write(_abi.F_CTL, st_.ctl)

    def after_heartbeat(kk, eng_, st_, msgs):
        if not case.shards:
            cut(kk, st_)

    def after_tick(kk, st_, msgs):
        if case.shards:                 # (a shard group takes a written state between ticks only)
            cut(kk + 1, st_)

    msgs, gstats = run_parity(net, params, th, gp, st, case.ticks, c["sched"], ring=case.ring, behaviour=c["behaviour"],
                              churn=c["churn"], eng=eng, after_heartbeat=after_heartbeat, after_tick=after_tick,
                              topic_slots=case.topic_slots,
                              trace=case.trace, trace_every_round=bool(case.trace), step=case.step,
                              rounds=case.rounds, hb=case.hb)
    print(f"{rid}: totals {msgs.stats}, engine gossip {gstats}")
    assert gstats["iwant_ids"] > 0 and gstats["iwant_responses"] > 0, "gossip ran on both sides and was answered"


# ---- the edges of the domain ---------------------------------------------------------

LAST = (1 << 31) - 2         # the last legal round


def small(gp=None, n=30, k=6):
    """A 30-peer network in one topic, dense start: (net, params, th, gp, st)."""
    from gsim.engine import random_regular
    net = random_regular(n, k, seed=5, n_topics=1)
    params = beacon_params(1)
    th = PeerScoreThresholds(**TH)
    gp = GossipSubParams(**{**GP, **(gp or {})})
    st = ob.NetState(net, params, thresholds=th, gossip=gp)
    synthetic_state(st, np.random.default_rng(3), T0, 0.7)
    return net, params, th, gp, st


def small_engine(gp=None):
    from gsim.engine import Engine
    net, params, th, gp, st = small(gp)
    eng = Engine(params, th, gossip=gp)
    eng.load_graph(net)
    eng.set_seed(SEED)
    st.push_to_engine(eng)
    return net, params, th, gp, st, eng


def last_first_delivery(sched, ticks, rounds=2, ring=4):
    """The oracle alone: the last round in which a peer first received message 0."""
    net, params, th, gp, st = small(WRAP_GP)
    msgs = ob.Msgs(net.n, 1, ring, rounds, T0, Second)
    msgs.log()
    lib, last = ob.load(), -1
    for kk in ticks:
        now = T0 + kk * Second
        v = st.view()
        lib.orc_refresh_scores(v, now)
        msgs.penalties(st, now)
        lib.orc_ip_colocation(v)
        lib.orc_compute_scores(v)
        msgs.heartbeat(st, kk, now, SEED)
        for g in range(kk * rounds, kk * rounds + rounds):
            for m in sched.get(g, []):
                msgs.publish(st, m[0], m[1], m[2], m[3], g)
            msgs.round(st, g)
        ev = msgs.events()
        hit = ev[(ev["kind"] == ob.EV_SEEN) & (ev["x"] == 1) & (ev["mid"] == 0)]
        last = max([last] + [int(g) for g in hit["g"]])
    assert (msgs.seen[0] != ob.UNSEEN).all(), "message 0 reached every peer"
    return last


@pytest.mark.gpu
@pytest.mark.parametrize("early", [0, 1])
def test_slot_reuse_at_the_guard(require_gpu, early):
    """One message on a 30-peer network (two rounds a tick, HistoryLength 2,
    HistoryGossip 1, IWantFollowupTime 1 s: 3 promise ticks, a guard G of
    (2 + 3 + 2) * 2 = 14 rounds); L is its last first delivery in the oracle's
    log (round 5: published in round 3).  Republishing its slot in round
    L + G runs bit-exact; in round L + G - 1 the engine answers GSIM_ESTATE
    ("republished ...") no later than the next heartbeat."""
    from gsim.engine import GsimError
    from tickrun import run_parity
    R, ring = 2, 4
    first = {3: [(0, 0, 7, 0)]}
    L = last_first_delivery(first, range(1, 6))
    net, params, th, gp, st = small(WRAP_GP)
    G = (max(gp.HistoryLength, gp.HistoryGossip) + prom_ticks(R, Second, gp.IWantFollowupTime) + 2) * R
    assert G == 14 and L >= 4
    again = L + G - early
    sched = {**first, again: [(ring, 0, 11, 0)]}
    done = []
    ticks = range(1, again // R + 3)
    run = lambda: run_parity(net, params, th, gp, st, ticks, sched, ring=ring, rounds=R,    # noqa: E731
                             after_tick=lambda kk, st_, msgs: done.append(kk))
    if not early:
        msgs, _ = run()
        assert done[-1] == ticks[-1] and msgs.mid[0] == ring and (msgs.seen[0] != ob.UNSEEN).sum() > 1
        return
    with pytest.raises(GsimError) as err:
        run()
    assert err.value.rc == _abi.GSIM_ESTATE and "republished" in str(err.value)
    # reported by the republication's own tick (its totals) or the heartbeat after it
    assert done[-1] in (again // R - 1, again // R), f"ticks completed {done}, republished in tick {again // R}"


@pytest.mark.gpu
def test_heartbeat_too_short_for_the_promise_ring_is_refused(require_gpu):
    """hb_10ms: IWantFollowupTime 3 s at a heartbeat of 10 ms needs 302 promise
    ticks, the ring holds 64: gsim_msgs_init refuses the clock (GSIM_EINVAL,
    naming the bound) instead of failing at tick 65.  The bound itself at
    two rounds a tick: 48 ms needs 64 and is taken, 47 ms needs 66."""
    net, params, th, gp, st, eng = small_engine()
    try:
        assert prom_ticks(2, 10 * MS, gp.IWantFollowupTime) == 302
        with pytest.raises(ValueError, match="64 promise ticks"):
            eng.msgs_init(64, 2, T0, 10 * MS)
        assert prom_ticks(2, 47 * MS, gp.IWantFollowupTime) == 66 and prom_ticks(2, 48 * MS, gp.IWantFollowupTime) == 64
        with pytest.raises(ValueError, match="64 promise ticks"):
            eng.msgs_init(64, 2, T0, 47 * MS)
        eng.msgs_init(64, 2, T0, 48 * MS)
    finally:
        eng.close()


def engine_state(eng, st):
    out = {f: eng.read(st.FIELD_IDS[f]) for f in st.TOPIC_FIELDS + st.EDGE_FIELDS}
    out.update(ctl=eng.read(_abi.F_CTL), seen=eng.read(_abi.F_SEEN), lastput=eng.read(_abi.F_LASTPUT),
               stats=np.array(eng.msg_stats()), gossip=np.array(list(eng.gossip_stats().values())))
    return out


def assert_unchanged(before, eng, st):
    after = engine_state(eng, st)
    for f in before:
        a, b = before[f], after[f]
        if a.dtype.itemsize == 8:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), f"{f} changed"


@pytest.mark.gpu
def test_last_legal_round(require_gpu):
    """gsim_round(2^31 - 2) runs (the heartbeat of its tick, a publication and
    the round, bit-exact); gsim_round(2^31 - 1), and a gsim_step that would
    reach it, return GSIM_ERANGE and change nothing."""
    from gsim.engine import GsimError
    from test_heartbeat import assert_same
    net, params, th, gp, st, eng = small_engine()
    try:
        R, kk = 2, LAST // 2
        eng.msgs_init(8, R, T0, Second)
        msgs = ob.Msgs(net.n, 1, 8, R, T0, Second)
        lib, now = ob.load(), T0 + kk * Second
        before = engine_state(eng, st)
        for tick, n_ticks in ((kk, 1), (kk - 1, 2), (kk + 1, 1), ((1 << 63), 1)):
            with pytest.raises(GsimError) as err:
                eng.step(tick, n_ticks, {LAST - 1: [(1, 0, 3, 0)]} if tick == kk - 1 else None)
            assert err.value.rc == _abi.GSIM_ERANGE
            assert_unchanged(before, eng, st)
        eng.refresh_scores(now)
        eng.heartbeat(kk, now)
        v = st.view()
        lib.orc_refresh_scores(v, now)
        msgs.penalties(st, now)
        lib.orc_ip_colocation(v)
        lib.orc_compute_scores(v)
        msgs.heartbeat(st, kk, now, SEED)
        msgs.publish(st, 5, 0, 3, 0, LAST)
        eng.publish([(5, 0, 3, 0)], LAST)
        msgs.round(st, LAST)
        eng.round(LAST)
        assert eng.msg_stats() == msgs.stats and np.array_equal(eng.read(_abi.F_SEEN), msgs.seen)
        assert msgs.seen[5, 3] == LAST
        gpu = ob.NetState(net, params, thresholds=th, gossip=gp)
        gpu.pull_from_engine(eng)
        assert_same(st, gpu)
        before = engine_state(eng, st)
        for call in (lambda: eng.round(LAST + 1), lambda: eng.publish([(6, 0, 4, 0)], LAST + 1)):
            with pytest.raises(GsimError) as err:
                call()
            assert err.value.rc == _abi.GSIM_ERANGE
            assert_unchanged(before, eng, st)
    finally:
        eng.close()


@pytest.mark.gpu
def test_completion_round_beyond_a_cell_is_refused(require_gpu):
    """far_lat's edge: a copy arriving in round g completes in g + vdelay, and a
    cell holds rounds to 2^31 - 2.  A message with vdelay > 0 is refused
    (GSIM_ERANGE) in a round above 2^31 - 2 - GSIM_MAX_VDELAY, whatever its own
    vdelay (its later copies arrive later); the same message without latency
    is taken; once a latency was published, those rounds are refused too, to
    gsim_round, gsim_step and the publication of any message."""
    from gsim.engine import GsimError
    net, params, th, gp, st, eng = small_engine()
    try:
        eng.msgs_init(8, 2, T0, Second)
        edge = LAST - 7                      # the last round a message with vdelay > 0 may be published in
        before = engine_state(eng, st)
        with pytest.raises(GsimError) as err:
            eng.publish([(1, 0, 3, 0, 1)], edge + 1)
        assert err.value.rc == _abi.GSIM_ERANGE
        assert_unchanged(before, eng, st)
        eng.refresh_scores(T0 + (edge // 2) * Second)
        eng.heartbeat(edge // 2, T0 + (edge // 2) * Second)
        eng.publish([(1, 0, 3, 0, 7)], edge)
        eng.round(edge)
        before = engine_state(eng, st)
        for call in (lambda: eng.round(edge + 1), lambda: eng.step((edge + 1) // 2, 1),
                     lambda: eng.publish([(2, 0, 4, 0)], edge + 1)):     # (no latency of its own)
            with pytest.raises(GsimError) as err:
                call()
            assert err.value.rc == _abi.GSIM_ERANGE
            assert_unchanged(before, eng, st)
    finally:
        eng.close()

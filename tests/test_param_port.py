"""The oracle at the settings of test_param_space.py, against a line-for-line
Python port of the reference (no GPU).

The branch census shows that a case reached a branch, not that the oracle
reads the reference correctly there (PrunePeers = 0 was listed as "nobody" by
oracle and engine alike: parity passed and both were wrong).  The port below
restates, for one (observer, topic),
  mesh maintenance             gossipsub.go:1386-1552
  emitGossip's peer choice     gossipsub.go:1726-1760
  makePrune's PX list          gossipsub.go:1880-1882, getPeers 1908-1928
with every shuffle replaced by "sort by key" (the oracle's exported keys,
orc_select_key / orc_px_key) and the score tracer's Graft / Prune / Score
taken from the oracle's KAT-pinned primitives.  It is driven from the short
network's state at tick 1 (the dense start) and at tick 2, before the
oracle's heartbeat, and must give the oracle's mesh bits, PX-flagged PRUNEs,
IHAVE marks and PX lists for every observer and topic, under every case of
the sweep.

Also here: the settings gsim_create refuses (validated before a device is
asked for, so without a GPU).
"""
import ctypes

import numpy as np
import pytest

import oracle_binding as ob
import test_param_space as ps
from gsim import _abi
from gsim.params import GossipSubParams, Second
from test_delivery import R, T0
from test_heartbeat import SEED, tick_time


class Port:
    """One network's heartbeat, observer by observer, as gossipsub.go writes it."""

    def __init__(self, net, st, gp, th, tick, now, gossip_ids):
        self.net, self.st, self.gp, self.th, self.tick, self.now = net, st, gp, th, tick, now
        self.v = st.view()
        self.lib = ob.load()
        self.has_ids = gossip_ids                      # {(peer, topic)} with a non-empty GetGossipIDs
        self.ihave = np.zeros((st.T, net.e), dtype=np.uint8)
        self.px_lists = {}                             # (pruner, pruned, topic) -> [listed peers]
        self.px_flag = np.zeros((st.T, net.e), dtype=bool)

    # -- helpers ------------------------------------------------------------
    def key(self, i, t, purpose, e, b):
        return ob.select_key(SEED, self.tick, i, t, purpose, int(self.net.col[e]), e - b)

    def topic_peer(self, e, t):                        # gs.p.topics[topic]: connected, announced t
        return bool(self.st.estate[e] & _abi.ES_CONNECTED) and bool((int(self.net.sub[self.net.col[e]]) >> t) & 1)

    def get_peers(self, i, t, b, en, count, filt, purpose):
        peers = [e for e in range(b, en) if self.topic_peer(e, t) and filt(e)]      # :1914-1919
        peers.sort(key=lambda e: self.key(i, t, purpose, e, b))                     # :1921 shufflePeers
        if count > 0 and len(peers) > count:                                        # :1923
            peers = peers[:count]
        return peers

    # -- gossipsub.go:1386-1552 ---------------------------------------------
    def maintain(self, i, t, b, en):
        st, gp, net = self.st, self.gp, self.net
        score = st.score                                                            # :1373-1383 the cached score
        peers = {e for e in range(b, en) if st.tflags[t, e] & _abi.TF_MESH}
        backoff = {e for e in range(b, en) if st.backoff[t, e] != 0}
        toprune, nopx = [], set()

        def prune_peer(e):                                                          # :1387-1393
            self.lib.orc_prune(self.v, e, t)
            peers.discard(e)
            backoff.add(e)
            toprune.append(e)

        def graft_peer(e):                                                          # :1395-1401
            self.lib.orc_graft(self.v, e, t, self.now)
            peers.add(e)

        for e in sorted(peers):                                                     # :1404-1410
            if score[e] < 0:
                prune_peer(e)
                nopx.add(e)
        if len(peers) < gp.Dlo:                                                     # :1413-1427
            ineed = gp.D - len(peers)
            for e in self.get_peers(i, t, b, en, ineed,
                                    lambda e: e not in peers and e not in backoff and score[e] >= 0, ob.P_GRAFT_DLO):
                graft_peer(e)
        if len(peers) > gp.Dhi:                                                     # :1430-1490
            plst = sorted(peers, key=lambda e: self.key(i, t, ob.P_PRUNE_SHUF1, e, b))   # :1434
            plst.sort(key=lambda e: -score[e])                                      # :1435-1437 (ties: shuffle order)
            tail = sorted(plst[gp.Dscore:], key=lambda e: self.key(i, t, ob.P_PRUNE_SHUF2, e, b))   # :1441
            plst = plst[:gp.Dscore] + tail
            outbound = sum(1 for e in plst[:gp.D] if net.outbound[e])               # :1444-1449
            if outbound < gp.Dout:                                                  # :1452
                def rotate(q):                                                      # :1453-1460
                    p = plst[q]
                    for j in range(q, 0, -1):
                        plst[j] = plst[j - 1]
                    plst[0] = p
                if outbound > 0:                                                    # :1463-1472
                    ihave = outbound
                    q = 1
                    while q < gp.D and ihave > 0:
                        if net.outbound[plst[q]]:
                            rotate(q)
                            ihave -= 1
                        q += 1
                ineed = gp.Dout - outbound                                          # :1475-1482
                q = gp.D
                while q < len(plst) and ineed > 0:
                    if net.outbound[plst[q]]:
                        rotate(q)
                        ineed -= 1
                    q += 1
            for e in plst[gp.D:]:                                                   # :1486-1489
                prune_peer(e)
        if len(peers) >= gp.Dlo:                                                    # :1493-1518
            outbound = sum(1 for e in peers if net.outbound[e])
            if outbound < gp.Dout:
                ineed = gp.Dout - outbound
                for e in self.get_peers(i, t, b, en, ineed,
                                        lambda e: e not in peers and e not in backoff and net.outbound[e]
                                        and score[e] >= 0, ob.P_GRAFT_DOUT):
                    graft_peer(e)
        if self.tick % gp.OpportunisticGraftTicks == 0 and len(peers) > 1:         # :1521-1552
            plst = sorted(peers, key=lambda e: score[e])                            # :1530-1533
            median = score[plst[len(peers) // 2]]                                   # :1534-1535
            if median < self.th.OpportunisticGraftThreshold:                        # :1538
                for e in self.get_peers(i, t, b, en, gp.OpportunisticGraftPeers,
                                        lambda e: e not in peers and e not in backoff and score[e] > median,
                                        ob.P_GRAFT_OPP):
                    graft_peer(e)
        # the router's own mesh map and backoff; sendGraftPrune's doPX && !noPX[p] (:1690)
        for e in range(b, en):
            if e in peers:
                st.tflags[t, e] |= _abi.TF_MESH
            else:
                st.tflags[t, e] &= ~np.uint8(_abi.TF_MESH)
        for e in toprune:
            self.px_flag[t, e] = bool(gp.PeerExchange) and e not in nopx
        return peers

    # -- gossipsub.go:1726-1760 ---------------------------------------------
    def emit_gossip(self, i, t, b, en, exclude):
        gp = self.gp
        if (i, t) not in self.has_ids:                                              # :1712-1715
            return
        live = lambda e: self.lib.orc_score_edge(self.v, e)                         # gs.score.Score(p)
        tpeers = [e for e in range(b, en) if self.topic_peer(e, t)]
        peers = [(self.key(i, t, ob.P_GOSSIP, e, b), e) for e in tpeers            # :1730-1737
                 if e not in exclude and live(e) >= self.th.GossipThreshold]
        if len(peers) < gp.Dlo:                                                     # :1739-1748
            for e in sorted(tpeers, key=lambda e: self.key(i, t, ob.P_GOSSIP_FILL, e, b)):   # "map order"
                peers.append((self.key(i, t, ob.P_GOSSIP_DUP, e, b), e))
                if len(peers) >= gp.Dlo:
                    break
        target = gp.Dlazy                                                           # :1749-1753
        factor = int(gp.GossipFactor * float(len(peers)))
        if factor > target:
            target = factor
        if target > len(peers):                                                     # :1755-1759
            target = len(peers)
        else:
            peers.sort()                                                            # shufflePeers
        for _, e in peers[:target]:                                                 # :1760-1774
            self.ihave[t, self.st.rev[e]] = 1

    # -- gossipsub.go:1880-1882 with getPeers ---------------------------------
    def px_list(self, i, t, b, en, ep):
        live = lambda e: self.lib.orc_score_edge(self.v, e)
        peers = [e for e in range(b, en) if self.topic_peer(e, t) and e != ep and live(e) >= 0]
        peers.sort(key=lambda e: ob.px_key(SEED, self.tick, i, t, ob.P_PX, int(self.net.col[e]), ep - b, e - b))
        if self.gp.PrunePeers > 0 and len(peers) > self.gp.PrunePeers:              # :1923
            peers = peers[:self.gp.PrunePeers]
        return [int(self.net.col[e]) for e in peers]

    def heartbeat(self):
        net, st = self.net, self.st
        for i in range(net.n):
            b, en = int(net.row_ptr[i]), int(net.row_ptr[i + 1])
            joined = [t for t in range(st.T) if (int(net.sub[i]) >> t) & 1]
            for t in joined:                                                        # :1386
                mesh = self.maintain(i, t, b, en)
                self.emit_gossip(i, t, b, en, mesh)                                 # :1556
            for t in joined:                                                        # sendGraftPrune :1672-1707
                for e in range(b, en):
                    if self.px_flag[t, e]:
                        self.px_lists[(i, int(net.col[e]), t)] = self.px_list(i, t, b, en, e)


def state_at_tick(case, tick):
    """The short network at `tick` (1: the dense start; 2: after the oracle's
    tick 1), after the tick's refresh and scores, before its heartbeat."""
    net, params, th, gp, st, p5, sched, churn, behaviour = ps.setup(case, "short")
    T = st.T
    ring = T * case.topic_slots if case.topic_slots else 1024
    msgs = ob.Msgs(net.n, T, ring, R, T0, Second, behaviour=behaviour, topic_slots=case.topic_slots)
    lib = ob.load()
    for kk in range(1, tick + 1):
        now = tick_time(kk)
        for (pairs, up) in churn.get(kk, []):
            st.churn(pairs, up=up, now=now - Second // 2)
        v = st.view()
        lib.orc_refresh_scores(v, now)
        msgs.penalties(st, now)
        lib.orc_ip_colocation(v)
        lib.orc_compute_scores(v)
        if kk == tick:
            break
        msgs.heartbeat(st, kk, now, SEED)
        for g in range(kk * R, kk * R + R):
            for (mid, t, o, inv) in sched.get(g, []):
                msgs.publish(st, mid, t, o, inv, g)
            msgs.round(st, g)
        if gp.PeerExchange:
            st.px_connect(now + Second // 2)
    return net, params, st, msgs, gp, th, p5, tick_time(tick)


def copy_state(net, params, st, gp, th, p5):
    c = ob.NetState(net, params, thresholds=th, gossip=gp, p5=p5)
    c.copy_fields_from(st)
    c.ctl[...] = st.ctl
    c.lastpub[...] = st.lastpub
    c.fan_topics[...] = st.fan_topics
    return c


def run_port_and_oracle(case, port_cls=Port, tick=2):
    net, params, st, msgs, gp, th, p5, now = state_at_tick(case, tick)
    st2 = copy_state(net, params, st, gp, th, p5)
    msgs.log()
    msgs.events()
    with ob.Census() as census:
        msgs.heartbeat(st, tick, now, SEED)
    ev = msgs.events()
    ids = ev[ev["kind"] == ob.EV_GOSSIP_ID]
    has_ids = set(zip(ids["a"].tolist(), ids["topic"].tolist()))
    port = port_cls(net, st2, gp, th, tick, now, has_ids)
    port.heartbeat()
    port.census = census.table
    return net, st, st2, msgs, ev, port


@pytest.mark.parametrize("tick", [1, 2])
@pytest.mark.parametrize("cid", [c.id for c in ps.CASES])
def test_oracle_heartbeat_matches_port(cid, tick):
    """tick 1: the dense start (hundreds of Dhi prunes with their rotations and
    PX lists; nothing is published yet, so no gossip); tick 2: the state the
    oracle's tick 1 left, with gossip."""
    case = ps.BY_ID[cid]
    net, st, st2, msgs, ev, port = run_port_and_oracle(case, tick=tick)
    if tick == 1 and not case.sink:
        # what the comparison rests on: the prune in a hundred (observer, topic) events at least
        # (big_d: Dhi = 32 is passed on the long rows only), the PX lists of as many pruners
        floor = 8 if cid == "big_d" else 100
        assert port.census["dhi_prune"].sum() >= floor, port.census["dhi_prune"]
        if cid in ("dout_max", "big_d"):
            assert port.census["rot_pass2"].sum() >= 5 and port.census["rot_pass1"].sum() >= 5
        if case.px:
            assert len(port.px_lists) >= 100
    own = net.owner()
    mesh_o = (st.tflags & _abi.TF_MESH) != 0
    mesh_p = (st2.tflags & _abi.TF_MESH) != 0
    bad = np.argwhere(mesh_o != mesh_p)
    assert len(bad) == 0, f"mesh bits differ at {len(bad)} (topic, edge), first {bad[0]} (observer {own[bad[0][1]]})"
    # PX-flagged PRUNEs: the heartbeat's output inbox, at the receiver's edge
    px_o = (st.ctl[0] & _abi.CTL_PX) != 0
    px_p = np.zeros_like(px_o)
    px_p[:, st.rev] = port.px_flag
    bad = np.argwhere(px_o != px_p)
    assert len(bad) == 0, f"PX-flagged PRUNEs differ at {len(bad)}, first {bad[0]}"
    # IHAVE marks of the joined topics (the fanout topics' emitGossip is not ported)
    joined = np.stack([((net.sub[net.col] >> np.uint64(t)) & np.uint64(1)) != 0 for t in range(st.T)])
    marks = msgs.ihave_marks(net.e).astype(bool) & joined      # (the mark sits at the receiver's edge: col = the sender)
    bad = np.argwhere(marks != (port.ihave.astype(bool) & joined))
    assert len(bad) == 0, f"IHAVE marks differ at {len(bad)}, first {bad[0]} (sender {net.col[bad[0][1]]})"
    assert case.id.startswith("gossip_off") or tick == 1 or marks.any()
    # the PX lists, in list order
    px = ev[ev["kind"] == ob.EV_PX_PEER]
    lists = {}
    for a, b_, t, mid, g in zip(px["a"].tolist(), px["b"].tolist(), px["topic"].tolist(), px["mid"].tolist(),
                                px["g"].tolist()):
        lists.setdefault((a, mid, t), {})[g] = b_
    got = {k: [v[q] for q in range(len(v))] for k, v in lists.items()}
    want = {k: v for k, v in port.px_lists.items() if v}
    assert got == want, f"PX lists differ ({len(got)} vs {len(want)})"
    assert bool(want) == bool(case.px) or (case.sink and not want)


# ---- what gsim_create refuses -------------------------------------------------------

# (every degree refusal ends with all six values, names included: the leading clause is what
# names the field at fault)
REFUSED = [
    (dict(D=6, Dlo=5, Dhi=12, Dout=7), "; Dout must not exceed D (gossipsub.go:90"),
    (dict(D=-1, Dlo=-2, Dhi=12, Dout=-1), "; D must not be negative"),
    (dict(D=6, Dlo=7, Dhi=12), "; Dlo must not exceed D "),
    (dict(D=13, Dlo=5, Dhi=12), "; D must not exceed Dhi"),
    (dict(D=6, Dlo=5, Dhi=12, Dscore=-1), "; Dscore must not be negative"),
    (dict(D=6, Dlo=5, Dhi=12, Dlazy=-1), "; Dlazy must not be negative"),
    (dict(D=6, Dlo=5, Dhi=12, PeerExchange=True, PrunePeers=0), "PrunePeers (0) must be at least 1"),
    (dict(D=6, Dlo=5, Dhi=12, PeerExchange=True, PrunePeers=-3), "PrunePeers (-3) must be at least 1"),
    (dict(HistoryLength=3, HistoryGossip=4), "gossip slots (4) cannot be larger than history slots (3)"),
]


def _create(gp):
    from fixtures import beacon_params, beacon_thresholds
    lib = _abi.load()
    params = beacon_params(1)
    pc, tc, gc = params.to_c(), beacon_thresholds().to_c(), gp.to_c()
    tarr = params.topic_array(sorted(params.Topics))
    h = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(512)
    rc = lib.gsim_create(ctypes.byref(pc), tarr, 1, ctypes.byref(tc), ctypes.byref(gc), 0, ctypes.byref(h), buf, len(buf))
    if rc == 0:
        lib.gsim_destroy(h)
    return rc, buf.value.decode()


@pytest.mark.parametrize("kw,field", REFUSED)
def test_create_refuses(kw, field):
    """gsim_create validates before it asks for a device: GSIM_EINVAL and a
    message whose leading clause names the field."""
    rc, msg = _create(GossipSubParams(**kw))
    assert rc == _abi.GSIM_EINVAL, f"rc {rc}: {msg}"
    assert field in msg, msg


def test_create_accepts_dout_up_to_d():
    """Dout between D / 2 and D stays accepted: the closed form holds there
    (test_dout_rotation_closed_form_matches_go).  Without a device the create
    gets as far as asking for one."""
    for dout in (4, 6):
        rc, msg = _create(GossipSubParams(D=6, Dlo=5, Dhi=12, Dout=dout))
        assert rc in (0, _abi.GSIM_EDEVICE), f"rc {rc}: {msg}"

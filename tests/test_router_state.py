"""Router state (gsim_router_state_*, include/gsim.h): the seen cache and the
gossip tracer's promises of externally driven routers on the device.  The
expectation is the CPU oracle's single-router restatement, pinned by the
reference's own tests (tests/test_oracle_kats.py): one `orc_tcache` and one
`orc_gtracer` per observer, driven in the same order (`Model` below).

The oracle's AddPromise and fulfillPromise return nothing, so the answer bytes
of PROMISE and FULFILL come from a Python shadow of promises[mid][peer]; the
shadow is checked against the oracle at every broken call (same rows) and
against `orc_gtracer_peer_promises`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import REPO
from gsim import _abi, routerstate as rs, tracer
from gsim.engine import Engine, GsimError
from gsim.params import Millisecond, PeerScoreParams, PeerScoreThresholds, Second

STATS = ("seen", "promises", "events", "swept", "fulfilled", "broken")
TH_HUB = PeerScoreThresholds(GossipThreshold=-20, PublishThreshold=-40, GraylistThreshold=-300)


# ---- CPU: layout, builders, to_score_events ---------------------------------------

def _probe(tmp_path, struct, fields):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsim.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({struct}));']
    for f in fields:
        lines.append(f'printf("{f} %zu\\n", offsetof({struct}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / f"{struct}.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / struct
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    return dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())


def test_struct_layouts_match_c(tmp_path):
    """EVENT_DTYPE / BROKEN_DTYPE and the ctypes structs against sizeof / offsetof (a compiled probe)."""
    for struct, ct, dt, size in (("gsim_router_event", _abi.CRouterEvent, rs.EVENT_DTYPE, 32),
                                 ("gsim_broken_row", _abi.CBrokenRow, rs.BROKEN_DTYPE, 16)):
        fields = [f for f, _ in ct._fields_]
        got = _probe(tmp_path, struct, fields)
        assert int(got["size"]) == size == ctypes.sizeof(ct) == dt.itemsize, struct
        for f in fields:
            assert int(got[f]) == getattr(ct, f).offset == dt.fields[f][1], (struct, f)
    hdr = open(os.path.join(REPO, "include", "gsim.h")).read()
    for name in ("SEEN_ADD", "SEEN_HAS", "PROMISE", "FULFILL"):
        assert re.search(rf"#define GSIM_RS_{name}\s+{getattr(rs, 'RS_' + name)}\b", hdr), name


def test_builders():
    ev = rs.batch([rs.seen_add(3, 77, 99), rs.seen_has(4, 78, 100), rs.promise(5, 6, 79, 101), rs.fulfill(7, 80, 102)])
    assert ev.dtype == rs.EVENT_DTYPE and len(ev) == 4
    assert ev["kind"].tolist() == [rs.RS_SEEN_ADD, rs.RS_SEEN_HAS, rs.RS_PROMISE, rs.RS_FULFILL] == [0, 1, 2, 3]
    assert ev["observer"].tolist() == [3, 4, 5, 7] and ev["peer"].tolist() == [0, 0, 6, 0]
    assert ev["mid"].tolist() == [77, 78, 79, 80] and ev["now_ns"].tolist() == [99, 100, 101, 102]
    assert not ev["_pad"].any()
    assert len(rs.batch([])) == 0 and rs.batch([]).dtype == rs.EVENT_DTYPE


def test_to_score_events():
    arrivals = [(0, 1, 0, 10, 5, None),                                  # new: validate + deliver
                (0, 2, 0, 10, 6, None),                                  # seen: duplicate
                (3, 4, 1, 11, 7, tracer.REJECT_INVALID_SIGNATURE),       # new, bad signature: reject alone
                (3, 5, 1, 12, 8, tracer.REJECT_VALIDATION_FAILED),       # new, the validator refused: validate + reject
                (3, 5, 1, 12, 9, tracer.REJECT_VALIDATION_FAILED)]       # seen: duplicate, whatever the reason
    got = rs.to_score_events(arrivals, np.array([1, 0, 1, 1, 0], dtype=np.uint8))
    want = tracer.batch([tracer.validate(0, 1, 0, 10, 5), tracer.deliver(0, 1, 0, 10, 5),
                         tracer.duplicate(0, 2, 0, 10, 6),
                         tracer.reject(3, 4, 1, 11, tracer.REJECT_INVALID_SIGNATURE, 7),
                         tracer.validate(3, 5, 1, 12, 8), tracer.reject(3, 5, 1, 12, tracer.REJECT_VALIDATION_FAILED, 8),
                         tracer.duplicate(3, 5, 1, 12, 9)])
    assert got.dtype == tracer.EVENT_DTYPE and got.tobytes() == want.tobytes()
    assert len(rs.to_score_events([], [])) == 0
    with pytest.raises(ValueError):
        rs.to_score_events(arrivals, [1])


# ---- the oracle model -------------------------------------------------------------------

class Model:
    """One orc_tcache and one orc_gtracer per observer, and the shadow of both."""

    def __init__(self, strategy, ttl, followup):
        self.lib, self.strategy, self.ttl, self.followup = ob.load(), strategy, ttl, followup
        self.tc, self.gt = {}, {}
        self.seen = {}                # (observer, mid) -> expiry
        self.prom = {}                # (observer, mid) -> {peer: expire}
        self.st = dict.fromkeys(STATS, 0)
        self.multi_fulfill = 0        # FULFILLs that dropped promises of two or more peers

    def close(self):
        for c in self.tc.values():
            self.lib.orc_tcache_free(c)
        for g in self.gt.values():
            self.lib.orc_gtracer_free(g)
        self.tc, self.gt = {}, {}

    def _tc(self, o):
        if o not in self.tc:
            self.tc[o] = self.lib.orc_tcache_new(self.strategy, self.ttl)
        return self.tc[o]

    def _gt(self, o):
        if o not in self.gt:
            self.gt[o] = self.lib.orc_gtracer_new(self.followup)
        return self.gt[o]

    def apply(self, events):
        lib, out = self.lib, []
        for (mid, now, o, p, kind, _pad) in np.asarray(events).tolist():
            key = (o, mid)
            if kind == rs.RS_SEEN_ADD:
                r = lib.orc_tcache_add(self._tc(o), mid, now)
                assert r == (key not in self.seen)
                if r or self.strategy == 1:
                    self.seen[key] = now + self.ttl
            elif kind == rs.RS_SEEN_HAS:
                r = lib.orc_tcache_has(self._tc(o), mid, now)
                assert r == (key in self.seen)
                if r and self.strategy == 1:
                    self.seen[key] = now + self.ttl
            elif kind == rs.RS_PROMISE:
                m = ctypes.c_uint64(mid)
                lib.orc_gtracer_add_promise(self._gt(o), p, ctypes.byref(m), 1, 0, now)
                peers = self.prom.setdefault(key, {})
                r = int(p not in peers)
                if r:
                    peers[p] = now + self.followup
            else:
                lib.orc_gtracer_fulfill(self._gt(o), mid)
                r = len(self.prom.pop(key, {}))
                self.st["fulfilled"] += r
                self.multi_fulfill += r >= 2
                r = min(r, 255)
            out.append(r)
        self.st["events"] += len(out)
        return np.array(out, dtype=np.uint8)

    def sweep(self, now):
        for c in self.tc.values():
            self.lib.orc_tcache_sweep(c, now)
        dead = [k for k, x in self.seen.items() if x < now]
        for k in dead:
            del self.seen[k]
        self.st["swept"] += len(dead)

    def throttle(self, pairs):
        gone = 0
        for o, p in pairs:
            self.lib.orc_gtracer_throttle(self._gt(int(o)), int(p))
            for (oo, mid), peers in list(self.prom.items()):
                if oo == o and p in peers:
                    del peers[p]
                    gone += 1
                    if not peers:
                        del self.prom[(oo, mid)]
        self.st["fulfilled"] += gone
        return gone

    def broken(self, now):
        """The oracle's rows of every observer, in (observer, peer) order; the shadow must agree."""
        peers = (ctypes.c_uint32 * 512)()
        counts = (ctypes.c_int32 * 512)()
        rows = []
        for o in sorted(self.gt):
            k = self.lib.orc_gtracer_broken(self.gt[o], now, peers, counts, 512)
            assert k <= 512
            rows += [(o, int(peers[i]), int(counts[i])) for i in range(k)]
        mine = {}
        for (o, mid), ps in list(self.prom.items()):
            for p, x in list(ps.items()):
                if x < now:
                    mine[(o, p)] = mine.get((o, p), 0) + 1
                    del ps[p]
            if not ps:
                del self.prom[(o, mid)]
        assert rows == [(o, p, c) for (o, p), c in sorted(mine.items())]
        self.st["broken"] += sum(c for _, _, c in rows)
        return rows

    def stats(self):
        self.st["seen"] = len(self.seen)
        self.st["promises"] = sum(len(ps) for ps in self.prom.values())
        peers = {}
        for (o, _), ps in self.prom.items():
            peers.setdefault(o, set()).update(ps)
        for o, g in self.gt.items():        # len(peerPromises) of every tracer against the shadow
            assert self.lib.orc_gtracer_peer_promises(g) == len(peers.get(o, ()))
        return dict(self.st)


def rows_of(arr):
    assert not arr["_pad"].any()
    return [(int(r["observer"]), int(r["peer"]), int(r["count"])) for r in arr]


class Pair:
    """The device calls and the model side by side: every call compares its answers and the stats."""

    def __init__(self, eng, seen_cap, promises_cap, strategy, ttl, followup):
        self.eng = eng
        eng.router_state_config(seen_cap, promises_cap, strategy, ttl, followup)
        self.m = Model(strategy, ttl, followup)

    def check(self, what):
        assert self.eng.router_state_stats() == self.m.stats(), what

    def send(self, rows, what=""):
        ev = rs.batch(rows)
        want = self.m.apply(ev)
        got = self.eng.router_state_events(ev)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (what, int(bad[0]), ev[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
        self.check(what)
        return got

    def sweep(self, now, what=""):
        self.m.sweep(now)
        self.eng.router_state_sweep(now)
        self.check(what)

    def throttle(self, pairs, what=""):
        want = self.m.throttle(pairs)
        assert self.eng.router_state_throttle(pairs) == want, what
        self.check(what)
        return want

    def broken(self, now, what=""):
        want = self.m.broken(now)
        got = rows_of(self.eng.router_state_broken(now))
        assert got == want, what
        self.check(what)
        return got

    def close(self):
        self.m.close()
        self.eng.close()


def star_engine():
    """Observer 0 connected to A, B, C, D = peers 1..4 (each of them connected to 0 alone)."""
    from peerscore_harness import star_network
    from test_score_tracer import MY, star_topic
    net, _ = star_network(["A", "B", "C", "D"], 1)
    params = PeerScoreParams(AppSpecificScore=lambda p: 0.0, DecayInterval=Second, DecayToZero=0.01,
                             Topics={MY: star_topic()})
    eng = Engine(params, PeerScoreThresholds(), topics=[MY], validate=False)
    eng.load_graph(net)
    return eng


# ---- GPU 1: the reference's literals on the four-peer star -----------------------------------

def both(rows_for):
    """The rows of a case at observer 0 and at observer 1, interleaved."""
    out = []
    for a, b in zip(rows_for(0), rows_for(1)):
        out += [a, b]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 1])
def test_gpu_timecache_literals(require_gpu, strategy):
    """tests/test_oracle_kats.py's timecache cases (found; expire with 10 / 11
    ids; last-seen slide forward; first-seen does not slide) through the device
    calls, at observers 0 and 1 interleaved in the same batches."""
    # found
    sp = Pair(star_engine(), 64, 64, strategy, 60 * Second, 0)
    try:
        got = sp.send(both(lambda o: [rs.seen_add(o, 42, 0), rs.seen_has(o, 42, 0), rs.seen_has(o, 43, 0)]), "found")
        assert got.tolist() == [1, 1, 1, 1, 0, 0]
    finally:
        sp.close()
    # expire: n ids 100 ms apart, TTL 1 s, the sweeps of the 1 s ticker after 2 s more
    n = 10 if strategy == 0 else 11
    sp = Pair(star_engine(), 64, 64, strategy, Second, 0)
    try:
        now = 0
        for i in range(n):
            assert sp.send(both(lambda o: [rs.seen_add(o, i, now)]), "expire add").tolist() == [1, 1]
            now += 100 * Millisecond
        now += 2 * Second
        sp.sweep(now - Second, "expire sweep 1")
        sp.sweep(now, "expire sweep 2")
        got = sp.send(both(lambda o: [rs.seen_has(o, i, now) for i in range(n)]), "expire has")
        assert not got.any() and sp.eng.router_state_stats()["seen"] == 0
        assert sp.eng.router_state_stats()["swept"] == 2 * n
    finally:
        sp.close()
    # slide forward (last-seen) / no slide (first-seen): the same calls, the model tells them apart
    sp = Pair(star_engine(), 64, 64, strategy, Second, 0)
    try:
        now = 0
        for i in range(8):
            sp.send(both(lambda o: [rs.seen_add(o, i, now)]), "slide add")
            now += 100 * Millisecond
        assert sp.send(both(lambda o: [rs.seen_has(o, 0, now)]), "T800").tolist() == [1, 1]      # slides 0 to 1800
        now += 400 * Millisecond
        sp.sweep(now, "T1200")
        got = sp.send(both(lambda o: [rs.seen_has(o, 0, now), rs.seen_has(o, 1, now)]), "T1200 has")
        assert got.tolist() == ([1, 1, 0, 0] if strategy == 1 else [0, 0, 0, 0])                   # 0 slid to 2200
        now += 1100 * Millisecond
        sp.sweep(now, "T2300")
        assert not sp.send(both(lambda o: [rs.seen_has(o, 0, now), rs.seen_has(o, 0, now)]), "T2300 has").any()
    finally:
        sp.close()
    # Add of an existing id: first-seen keeps the expiry, last-seen renews it; an id re-added after its sweep is new
    sp = Pair(star_engine(), 64, 64, strategy, Second, 0)
    try:
        assert sp.send(both(lambda o: [rs.seen_add(o, 1, 0)])).tolist() == [1, 1]
        assert sp.send(both(lambda o: [rs.seen_add(o, 1, 900 * Millisecond)])).tolist() == [0, 0]
        sp.sweep(1001 * Millisecond)
        got = sp.send(both(lambda o: [rs.seen_has(o, 1, 1001 * Millisecond), rs.seen_add(o, 1, 1001 * Millisecond)]))
        assert got.tolist() == ([0, 0, 1, 1] if strategy == 0 else [1, 1, 0, 0])
    finally:
        sp.close()


@pytest.mark.gpu
def test_gpu_gossip_tracer_literals(require_gpu):
    """gossip_tracer_test.go's two cases (tests/test_oracle_kats.py
    test_broken_promises, test_no_broken_promises) at observer 0, whose peers
    are A, B, C = 1, 2, 3.  Interleaved in the same batches, leaf 1 replays the
    case with the one connection a leaf of the star has (peer 0)."""
    follow = 100 * Millisecond
    sp = Pair(star_engine(), 64, 64, 0, 0, follow)
    try:
        now = 0
        rows = []
        for peer in (1, 2, 3):
            rows += [rs.promise(0, peer, 17, now), rs.promise(1, 0, 17, now)]
        assert sp.send(rows, "promises").tolist() == [1, 1, 1, 0, 1, 0]
        assert sp.broken(now, "nothing broken yet") == []
        assert sp.throttle([(0, 3)], "throttle C") == 1
        # a promise made at t is not broken at t + followup
        assert sp.broken(now + follow, "at the expiry") == []
        now += follow + Millisecond
        assert sp.broken(now, "broken") == [(0, 1, 1), (0, 2, 1), (1, 0, 1)]
        st = sp.eng.router_state_stats()
        assert (st["promises"], st["fulfilled"], st["broken"]) == (0, 1, 3)
    finally:
        sp.close()
    sp = Pair(star_engine(), 64, 256, 0, 0, follow)
    try:
        sp.send([rs.promise(0, 1, 5, 0), rs.promise(1, 0, 5, 0), rs.promise(0, 2, 93, 0), rs.promise(1, 0, 93, 0)])
        got = sp.send(both(lambda o: [rs.fulfill(o, m, 0) for m in range(100)]), "fulfill")
        assert int(got.sum()) == 4 and got[2 * 5] == got[2 * 93] == 1
        assert sp.broken(follow + Millisecond, "none broken") == []
        assert sp.eng.router_state_stats()["promises"] == 0
    finally:
        sp.close()


# ---- GPU 2: random batches on the hub network ---------------------------------------------------

TTL, FOLLOW, STEP, PER_NS = 1500, 700, 1000, 200       # ns; PER_NS events share one nanosecond
T_BASE = 1_000_000
N_BATCH, BATCH, HUB_BATCH, HUB_EVENTS, POOL = 6, 20000, 2, 5000, 24


def make_batch(net, rng, b):
    """20 000 shuffled events of all four kinds; ids from a window of POOL ids
    that moves by half a window per batch, so ids repeat inside a batch and
    between neighbouring batches.  Times grow with the array position (PER_NS
    events per nanosecond): non-decreasing for every observer."""
    from test_score_tracer import HUB
    rp, col = net.row_ptr.astype(np.int64), net.col
    obs = rng.integers(0, net.n - 1, BATCH)
    if b == HUB_BATCH:
        obs[rng.choice(BATCH, HUB_EVENTS, replace=False)] = HUB
    kinds = rng.choice(4, BATCH, p=[0.35, 0.2, 0.3, 0.15])
    mids = b * (POOL // 2) + rng.integers(0, POOL, BATCH)
    rows, named, repeats, seen_events = [], set(), 0, 0
    for k in range(BATCH):
        o, kind, mid = int(obs[k]), int(kinds[k]), int(mids[k])
        now = T_BASE + b * STEP + k // PER_NS
        if kind == rs.RS_SEEN_ADD or kind == rs.RS_SEEN_HAS:
            seen_events += 1
            repeats += (o, mid) in named
            named.add((o, mid))
            rows.append((rs.seen_add if kind == rs.RS_SEEN_ADD else rs.seen_has)(o, mid, now))
        elif kind == rs.RS_PROMISE:
            rows.append(rs.promise(o, int(col[rng.integers(rp[o], rp[o + 1])]), mid, now))
        else:
            rows.append(rs.fulfill(o, mid, now))
    assert 4 * repeats >= seen_events, "a quarter of the seen events name an (observer, id) again"
    return rows


def run_random(require_gpu, hubnet, strategy):
    from test_score_tracer import HUB, TOPICS, hub_params
    net = hubnet
    rng = np.random.default_rng(977 + strategy)
    eng = Engine(hub_params(), TH_HUB, topics=TOPICS)
    eng.load_graph(net)
    sp = Pair(eng, 1 << 15, 1 << 15, strategy, TTL, FOLLOW)
    m = sp.m
    try:
        for b in range(N_BATCH):
            rows = make_batch(net, rng, b)
            if b == HUB_BATCH:
                assert sum(1 for r in rows if r[2] == HUB) >= HUB_EVENTS
            multi = m.multi_fulfill
            got = sp.send(rows, f"batch {b}")
            assert m.multi_fulfill > multi, "a FULFILL hit live promises of two or more peers"
            assert got[rs.batch(rows)["kind"] == rs.RS_FULFILL].max() >= 2
            # a sweep with entries on expiry == now, one above and one below: == and above stay
            now = T_BASE + b * STEP + BATCH // PER_NS // 2 + TTL
            exp = set(m.seen.values())
            assert {now - 1, now, now + 1} <= exp, "entries below, on and above the sweep time"
            n_on = sum(1 for x in m.seen.values() if x >= now)
            sp.sweep(now, f"sweep {b}")
            assert len(m.seen) == n_on and m.st["swept"] > 0
            # broken at expire == now (that promise stays), then at now + 1 (it goes)
            live = sorted(x for ps in m.prom.values() for x in ps.values())
            e0 = live[len(live) // 2]
            sp.broken(e0, f"broken {b} at an expiry")
            assert any(x == e0 for ps in m.prom.values() for x in ps.values())
            assert sp.broken(e0 + 1, f"broken {b} one past it"), "the promises expiring at e0 are broken at e0 + 1"
            # ThrottlePeer of live pairs (one of them twice) and of pairs without promises
            pairs = sorted({(o, p) for (o, _), ps in m.prom.items() for p in ps})
            pick = [pairs[i] for i in rng.choice(len(pairs), 40, replace=False)]
            idle = [(o, int(net.col[net.row_ptr[o]])) for o in rng.integers(0, net.n, 8).tolist()]
            assert sp.throttle(pick + pick[:1] + idle, f"throttle {b}") >= 40
        st = eng.router_state_stats()
        assert st["events"] == N_BATCH * BATCH and min(st.values()) > 0
    finally:
        sp.close()


@pytest.fixture(scope="module")
def hubnet():
    from test_score_tracer import hub_network
    return hub_network()


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 1])
def test_gpu_random_batches_on_a_network(require_gpu, hubnet, strategy):
    """The 301-peer network with a hub row: six shuffled batches of 20 000
    events of all four kinds with ids that repeat inside a batch, the hub
    receiving 5 000 events of one batch; between batches a sweep with entries
    on, above and below its time, broken at an expiry and one past it, and a
    throttle of live pairs.  Every answer byte, every broken row and the stats
    equal the oracle structures driven in the same order."""
    run_random(require_gpu, hubnet, strategy)


def slot_hash(o, mid):
    """rs_hash of csrc/routerstate.hip (the seen table's home slot is its low bits)."""
    M = (1 << 64) - 1
    x = (mid ^ (o * 0x9E3779B97F4A7C15)) & M
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M
    x ^= x >> 33
    return x & 0xFFFFFFFF


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 1])
def test_gpu_seen_table_filled_to_cap(require_gpu, hubnet, strategy):
    """seen_cap = 64: the table (128 slots) is filled to cap exactly.  Four of
    observer 0's ids have the table's last slot as their home, so their probe
    sequences wrap its end; ids that are absent probe up to the first empty
    slot.  Then half is swept and the space is filled again."""
    from test_score_tracer import TOPICS, hub_params
    eng = Engine(hub_params(), TH_HUB, topics=TOPICS)
    eng.load_graph(hubnet)
    sp = Pair(eng, 64, 16, strategy, 1000, 0)
    try:
        last = [mid for mid in range(1, 4000) if slot_hash(0, mid) & 127 == 127][:4]
        assert len(last) == 4
        rng = np.random.default_rng(5)
        keys = [(0, mid) for mid in last] + [(int(o), int(mid)) for o, mid in
                                             zip(rng.integers(0, 8, 60), rng.permutation(60) + 5000)]
        adds = [rs.seen_add(o, mid, 10 + (q >= 32)) for q, (o, mid) in enumerate(keys)]
        assert sp.send(adds, "fill").sum() == 64
        assert eng.router_state_stats()["seen"] == 64
        probe = [rs.seen_has(o, mid, 12) for o, mid in keys] + [rs.seen_has(o, mid + 100000, 12) for o, mid in keys]
        got = sp.send([probe[i] for i in rng.permutation(len(probe))], "has")
        assert int(got.sum()) == 64
        with pytest.raises(GsimError) as ex:
            eng.router_state_events(rs.batch([rs.seen_add(9, 1, 12)]))
        assert ex.value.rc == _abi.GSIM_ERANGE
        if strategy == 0:
            sp.sweep(1011, "sweep the first half")           # expiry 1010 < 1011 <= 1011
            assert eng.router_state_stats()["seen"] == 32
            again = [rs.seen_add(o, mid, 20) for o, mid in keys[:32]]       # 32 live + 32 adds: exactly cap
            assert sp.send(again, "refill").sum() == 32
            assert sp.send([rs.seen_has(o, mid, 20) for o, mid in keys], "all back").all()
        else:
            sp.sweep(1012, "every Has renewed its entry")    # to 12 + 1000
            assert eng.router_state_stats()["seen"] == 64
            sp.sweep(1013, "all gone")
            assert sp.send([rs.seen_add(o, mid, 20) for o, mid in keys], "refill").sum() == 64
        assert eng.router_state_stats()["seen"] == 64
    finally:
        sp.close()


# ---- GPU 3: the network oracle's log through the device -----------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["r10", "wrap32", "r2_lat"])
def test_gpu_network_oracle_log(require_gpu, setting):
    """tests/test_oracle_linkage.py's runs: the network oracle's seen verdicts
    and broken promises against the device structures of a fresh engine on the
    same graph, one batch per round.  EV_VALIDATE and EV_SEEN are SEEN_ADD (a
    verdict whose arrival was logged as EV_VALIDATE marked the id then),
    EV_PROMISE is PROMISE at its logged time, EV_FULFILL is FULFILL,
    EV_PENALTIES is broken(x), whose rows are the EV_BROKEN records that
    follow.  Seen and FULFILL rows carry the observer's last PROMISE time (no
    sweep runs, so only the promises' times matter)."""
    from fixtures import beacon_params
    from test_gossip import TH
    from test_oracle_linkage import SETTINGS, _network_run
    rounds, hb, ring, gpf, vdelays, ticks = SETTINGS[setting]
    net, gp, msgs, ev = _network_run(rounds, hb, ring, gpf, vdelays, ticks)
    eng = Engine(beacon_params(2), TH, gossip=gp)
    eng.load_graph(net)
    eng.router_state_config(1 << 16, 1 << 14)          # followup 0: the engine's IWantFollowupTime
    kinds = ev["kind"]
    clock = np.zeros(net.n, dtype=np.int64)
    validating = set()
    rows, want, cur_g = [], [], None
    answers = {0: 0, 1: 0}
    n_broken = n_calls = 0

    def flush():
        nonlocal rows, want
        if rows:
            got = eng.router_state_events(rs.batch(rows))
            for k, x in want:
                assert got[k] == x, f"seen verdict of {rows[k][0]} at router {rows[k][2]}"
                answers[x] += 1
        rows, want = [], []

    try:
        q = 0
        while q < len(ev):
            e = ev[q]
            kind = int(e["kind"])
            a, b, mid, x, g = int(e["a"]), int(e["b"]), int(e["mid"]), int(e["x"]), int(e["g"])
            if kind == ob.EV_PENALTIES:
                flush()
                q += 1
                expect = []
                while q < len(ev) and kinds[q] == ob.EV_BROKEN:
                    r = ev[q]
                    expect.append((int(r["a"]), int(r["b"]), int(r["x"])))
                    q += 1
                got = rows_of(eng.router_state_broken(x))
                assert got == sorted(expect), f"broken promises at {x}"
                n_broken += len(got)
                n_calls += 1
                continue
            q += 1
            if kind not in (ob.EV_VALIDATE, ob.EV_SEEN, ob.EV_PROMISE, ob.EV_FULFILL):
                continue
            if kind == ob.EV_SEEN and x == 1 and (a, mid) in validating:
                validating.remove((a, mid))              # (its verdict: markSeen happened at the arrival)
                continue
            if kind != ob.EV_FULFILL and g != cur_g:      # (a FULFILL is logged without its round: it joins the batch)
                flush()
                cur_g = g
            if kind == ob.EV_VALIDATE:
                validating.add((a, mid))
                want.append((len(rows), 1))
                rows.append(rs.seen_add(a, mid, clock[a]))
            elif kind == ob.EV_SEEN:
                want.append((len(rows), x))
                rows.append(rs.seen_add(a, mid, clock[a]))
            elif kind == ob.EV_PROMISE:
                assert x >= clock[a]
                clock[a] = x
                rows.append(rs.promise(a, b, mid, x))
            else:
                rows.append(rs.fulfill(a, mid, clock[a]))
        flush()
        assert answers[0] > 0 and answers[1] > 0 and n_broken > 0 and n_calls == ticks
        st = eng.router_state_stats()
        assert st["seen"] == answers[1] and st["broken"] >= n_broken and st["fulfilled"] > 0
    finally:
        eng.close()


# ---- GPU 4: apply_penalty ------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_apply_penalty_is_the_add_penalty_event(require_gpu, hubnet):
    """Two engines on the same written state: broken(apply_penalty=1) on one,
    broken(apply_penalty=0) and its rows as GSIM_EV_ADD_PENALTY events on the
    other.  GSIM_F_BP is bit-equal, every other field bit-equal to before;
    some penalised peers have no peerStats (the silent return)."""
    from gsim.params import GossipSubParams
    from test_score_tracer import STATE_FIELDS, TOPICS, bits, hub_params, hub_state
    net, params = hubnet, hub_params()
    th = TH_HUB
    gp = GossipSubParams(D=6, Dlo=4, Dhi=10, Dscore=3, Dout=2)
    rng = np.random.default_rng(31)
    st = hub_state(net, params, th, gp, rng)
    st.estate[rng.random(net.e) < 0.2] &= ~np.uint8(_abi.ES_TRACKED)       # no peerStats for a fifth of the records
    rp, col = net.row_ptr.astype(np.int64), net.col
    rows = []
    for k in range(3000):
        o = int(rng.integers(0, net.n))
        rows.append(rs.promise(o, int(col[rng.integers(rp[o], rp[o + 1])]), int(rng.integers(0, 6)), 100 + k // 100))
    ev = rs.batch(rows)
    fid = ob.NetState.FIELD_IDS
    engs = []
    try:
        for _ in range(2):
            eng = Engine(params, th, gossip=gp, topics=TOPICS)
            engs.append(eng)
            eng.load_graph(net)
            st.push_to_engine(eng)
            eng.router_state_config(16, 4096, 0, 0, 50)
            eng.router_state_events(ev)
        a, b = engs
        before = {f: a.read(fid[f]) for f in STATE_FIELDS}
        now = 100 + 15 + 50 + 1                          # the promises of the first 1 600 events
        got_a = a.router_state_broken(now, apply_penalty=True)
        got_b = b.router_state_broken(now)
        assert got_a.tobytes() == got_b.tobytes() and len(got_b) > 500 and got_b["count"].max() >= 2
        b.tracer_config(16, 16)
        b.tracer_events(tracer.batch([tracer.add_penalty(int(r["observer"]), int(r["peer"]), int(r["count"]), now)
                                      for r in got_b]))
        bp_a, bp_b = a.read(_abi.F_BP), b.read(_abi.F_BP)
        assert np.array_equal(bits(bp_a), bits(bp_b))
        changed = bits(bp_a) != bits(before["bp"])
        assert 0 < changed.sum() < len(got_b), "some rows changed bp, some met a peer without peerStats"
        for eng in engs:
            for f in STATE_FIELDS:
                if f != "bp":
                    assert np.array_equal(bits(eng.read(fid[f])), bits(before[f])), f
        # without apply_penalty nothing is written
        c_before = b.read(_abi.F_BP)
        assert len(b.router_state_broken(10**6)) > 0
        assert np.array_equal(bits(b.read(_abi.F_BP)), bits(c_before))
    finally:
        for eng in engs:
            eng.close()


# ---- GPU 5: refusals --------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_refusals(require_gpu):
    eng = star_engine()
    try:
        calls = (lambda: eng.router_state_events(rs.batch([rs.seen_add(0, 1, 0)])), lambda: eng.router_state_sweep(0),
                 lambda: eng.router_state_throttle([(0, 1)]), lambda: eng.router_state_broken(0),
                 eng.router_state_stats)
        for call in calls:
            with pytest.raises(GsimError) as ex:
                call()
            assert ex.value.rc == _abi.GSIM_ESTATE
        with pytest.raises(ValueError):
            eng.router_state_config(8, 8, 2)
    finally:
        eng.close()
    sp = Pair(star_engine(), 8, 4, 0, 0, 100)
    eng = sp.eng
    try:
        t0 = 1000
        sp.send([rs.seen_add(0, 1, t0), rs.promise(0, 1, 7, t0), rs.promise(0, 2, 7, t0 + 6), rs.seen_add(1, 1, t0 + 6)])
        stats = eng.router_state_stats()

        def unchanged(what):
            """The stats as before the refusal, and a valid batch that answers as if the refused one had never
            come: its ids (3, 10.., 20..) are unknown, the clocks stand at t0 + 6, what was there is there."""
            nonlocal stats
            assert eng.router_state_stats() == stats, what
            got = sp.send([rs.seen_has(0, 3, t0 + 6), rs.seen_has(0, 10, t0 + 6), rs.seen_has(0, 1, t0 + 6),
                           rs.fulfill(0, 3, t0 + 6), rs.fulfill(0, 20, t0 + 6), rs.seen_has(1, 1, t0 + 6)], what)
            assert got.tolist() == [0, 0, 1, 0, 0, 1], what
            stats = eng.router_state_stats()

        ok = rs.seen_has(0, 1, t0 + 7)
        bad_kind = list(rs.seen_add(0, 3, t0 + 7))
        bad_kind[4] = 4
        bad = {
            "unknown kind": tuple(bad_kind),
            "observer out of range": rs.seen_add(5, 3, t0 + 7),
            "not a connection": rs.promise(1, 2, 3, t0 + 7),               # leaves are connected to 0 alone
            "not a connection of the observer": rs.promise(0, 9, 3, t0 + 7),   # a peer out of range is none either
            "time goes backwards": rs.seen_add(0, 3, t0 + 6),              # within the batch: after `ok` at t0 + 7
            "exceeds the int64 range": rs.seen_add(0, 3, 2**63 - 51),      # now + the 120 s lifetime overflows
        }
        for what, row in bad.items():
            with pytest.raises(ValueError, match=r"^event 2: ") as ex:
                eng.router_state_events(rs.batch([ok, ok, row, rs.seen_add(9, 9, 0)]))
            assert what.split(" of ")[0] in str(ex.value), (what, str(ex.value))
            unchanged(what)
        # against the observer's last event of an earlier batch (t0 + 6); another observer is free; this
        # clock is the router state's own
        with pytest.raises(ValueError, match=r"^event 1: time goes backwards"):
            eng.router_state_events(rs.batch([rs.seen_add(2, 1, 0), rs.seen_add(0, 3, t0 + 5)]))
        unchanged("earlier batch")
        # seen events and FULFILL ignore peer
        row = list(rs.fulfill(0, 99, t0 + 6))
        row[3] = 77
        sp.send([tuple(row)], "peer ignored")
        stats = eng.router_state_stats()
        # throttle's pairs
        for pairs, k in (([(0, 1), (5, 0)], 1), ([(0, 1), (0, 2), (1, 2)], 2)):
            with pytest.raises(ValueError, match=rf"^pair {k}: "):
                eng.router_state_throttle(pairs)
            unchanged("throttle")
        # GSIM_ERANGE at exactly cap + 1: 1 + 1 live seen entries of 8, 2 live promises of 4
        t1 = t0 + 10
        with pytest.raises(GsimError) as ex:
            eng.router_state_events(rs.batch([rs.seen_add(0, 10 + i, t1) for i in range(7)]))
        assert ex.value.rc == _abi.GSIM_ERANGE
        unchanged("seen cap + 1")
        with pytest.raises(GsimError) as ex:
            eng.router_state_events(rs.batch([rs.promise(0, 3, 20 + i, t1) for i in range(3)]))
        assert ex.value.rc == _abi.GSIM_ERANGE
        unchanged("promises cap + 1")
        # broken with too little room: GSIM_ERANGE, *n set, nothing removed
        n = ctypes.c_int64(-1)
        out = np.zeros(1, dtype=rs.BROKEN_DTYPE)
        rc = eng.lib.gsim_router_state_broken(eng.h, 10**9, 1, out.ctypes.data, 1, ctypes.byref(n))
        assert rc == _abi.GSIM_ERANGE and n.value == 2
        unchanged("broken without room")
        # a valid batch answers as if the refused ones had never come: exactly cap of each fits
        got = sp.send([rs.seen_add(0, 10 + i, t1) for i in range(6)] + [rs.promise(0, 3, 20 + i, t1) for i in range(2)] +
                      [rs.seen_has(0, 3, t1)], "at cap")
        assert got.tolist() == [1] * 8 + [0]
        assert (eng.router_state_stats()["seen"], eng.router_state_stats()["promises"]) == (8, 4)
        # fulfilled promises leave their space: live promises count, the batch compacts table and pool
        assert sp.send([rs.fulfill(0, 7, t1), rs.fulfill(0, 20, t1)], "fulfill").tolist() == [2, 1]
        assert sp.send([rs.promise(0, 4, 30 + i, t1) for i in range(3)], "reuse").tolist() == [1, 1, 1]
        with pytest.raises(GsimError) as ex:
            eng.router_state_events(rs.batch([rs.promise(0, 4, 40, t1)]))
        assert ex.value.rc == _abi.GSIM_ERANGE
        assert sp.broken(t1 + 101, "all broken") == [(0, 3, 1), (0, 4, 3)]
        # result == NULL is accepted
        ev = rs.batch([rs.seen_has(0, 10, t1 + 1), rs.promise(0, 2, 50, t1 + 1)])
        sp.m.apply(ev)
        assert eng.lib.gsim_router_state_events(eng.h, ev.ctypes.data, len(ev), None) == 0
        sp.check("no result array")
        # a second config empties both structures (and the observers' clocks)
        eng.router_state_config(8, 4, 1, 0, 100)
        assert eng.router_state_stats() == dict.fromkeys(STATS, 0)
        got = eng.router_state_events(rs.batch([rs.seen_has(0, 10, 0), rs.seen_add(0, 10, 0), rs.fulfill(0, 50, 0),
                                                rs.promise(0, 2, 50, 0)]))
        assert got.tolist() == [0, 1, 0, 1]
        # a new graph drops the configuration
        eng.load_graph(eng.net)
        with pytest.raises(GsimError) as ex:
            eng.router_state_stats()
        assert ex.value.rc == _abi.GSIM_ESTATE
    finally:
        sp.close()


@pytest.mark.gpu
def test_gpu_fulfill_saturates_at_255(require_gpu):
    """300 peers promised one id to the observer of a 300-peer star: fulfillPromise
    drops all 300 and answers 255; 255 and 254 promises answer their number."""
    from peerscore_harness import star_network
    from test_score_tracer import MY, star_topic
    net, _ = star_network([f"p{i}" for i in range(300)], 1)
    params = PeerScoreParams(AppSpecificScore=lambda p: 0.0, DecayInterval=Second, DecayToZero=0.01,
                             Topics={MY: star_topic()})
    eng = Engine(params, PeerScoreThresholds(), topics=[MY], validate=False)
    eng.load_graph(net)
    sp = Pair(eng, 16, 1024, 0, 0, 100)
    try:
        rows = []
        for mid, k in ((1, 300), (2, 255), (3, 254)):
            rows += [rs.promise(0, 1 + p, mid, 5) for p in range(k)]
        assert sp.send(rows, "promises").all()
        assert sp.send([rs.fulfill(0, mid, 6) for mid in (1, 2, 3, 1)], "fulfill").tolist() == [255, 255, 254, 0]
        st = eng.router_state_stats()
        assert (st["promises"], st["fulfilled"]) == (0, 809)
    finally:
        sp.close()


@pytest.mark.gpu
def test_gpu_refused_on_a_shard(require_gpu):
    from fixtures import beacon_params, beacon_thresholds
    from gsim.engine import random_regular
    from gsim.shard import ShardedEngine
    net = random_regular(400, 8, seed=3, n_topics=2)
    grp = ShardedEngine(beacon_params(2), beacon_thresholds(), shards=2)
    try:
        grp.load_graph(net)
        lib, h = grp.lib, grp._shard_handle(0)
        ev = rs.batch([rs.seen_add(0, 1, 1)])
        pairs = np.array([[0, int(net.col[0])]], dtype=np.uint32)
        out = np.zeros(6, dtype=np.int64)
        rows = np.zeros(4, dtype=rs.BROKEN_DTYPE)
        n = ctypes.c_int64(0)
        assert lib.gsim_router_state_config(h, 64, 64, 0, 0, 0) == _abi.GSIM_ESTATE
        assert b"shard" in lib.gsim_last_error(h)
        assert lib.gsim_router_state_events(h, ev.ctypes.data, 1, None) == _abi.GSIM_ESTATE
        assert lib.gsim_router_state_sweep(h, 5) == _abi.GSIM_ESTATE
        assert lib.gsim_router_state_throttle(h, pairs.ctypes.data, 1, None) == _abi.GSIM_ESTATE
        assert lib.gsim_router_state_broken(h, 5, 0, rows.ctypes.data, 4, ctypes.byref(n)) == _abi.GSIM_ESTATE
        assert lib.gsim_router_state_stats(h, out.ctypes.data) == _abi.GSIM_ESTATE
    finally:
        grp.close()

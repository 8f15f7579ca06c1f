"""Host-side engine handle over the C ABI (include/gsim.h).

`Engine` plays the role the reference's GossipSubRouter+peerScore pair plays
for one node (gossipsub.go:420-477, score.go:64-86), but for a whole simulated
network held on one MI355X.  Everything computational runs in libgsim.so's HIP
kernels; this module only marshals arrays.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .params import GossipSubParams, PeerScoreParams, PeerScoreThresholds, TopicScoreParams

_FIELD_DTYPES = {
    _abi.F_FIRST: np.float64, _abi.F_MESHD: np.float64, _abi.F_FAIL: np.float64, _abi.F_INVALID: np.float64,
    _abi.F_GRAFT_TIME: np.int64, _abi.F_MESH_TIME: np.int64, _abi.F_TFLAGS: np.uint8, _abi.F_BP: np.float64,
    _abi.F_ESTATE: np.uint8, _abi.F_EXPIRE: np.int64, _abi.F_P6: np.float64, _abi.F_SCORE: np.float64,
    _abi.F_BACKOFF: np.int64, _abi.F_CTL: np.uint8, _abi.F_SEEN: np.uint32, _abi.F_LASTPUT: np.int32,
    _abi.F_LASTPUB: np.int64, _abi.F_FANOUT_TOPICS: np.uint64,
}
TOPIC_FIELDS = {_abi.F_FIRST, _abi.F_MESHD, _abi.F_FAIL, _abi.F_INVALID, _abi.F_GRAFT_TIME,
                _abi.F_MESH_TIME, _abi.F_TFLAGS, _abi.F_BACKOFF}
PARITY_TOPIC_FIELDS = {_abi.F_CTL}


class GsimError(RuntimeError):
    def __init__(self, rc: int, msg: str):
        super().__init__(f"gsim error {rc}: {msg}")
        self.rc = rc


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@dataclass
class Network:
    """A simulated peer graph: CSR rows = observers, columns = neighbours."""
    n: int
    row_ptr: np.ndarray           # uint32 [n+1]
    col: np.ndarray               # uint32 [E]
    outbound: np.ndarray          # uint8  [E]
    sub: np.ndarray               # uint64 [n] topic bitmask
    ip_ptr: Optional[np.ndarray] = None   # uint32 [n+1]
    ip_ids: Optional[np.ndarray] = None   # uint32
    n_ips: int = 0

    @property
    def e(self) -> int:
        return int(self.row_ptr[-1])

    def rev(self) -> np.ndarray:
        """Reverse-edge index (j->i for every i->j)."""
        owner = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.row_ptr.astype(np.int64)))
        key_fwd = owner * self.n + self.col.astype(np.int64)
        key_rev = self.col.astype(np.int64) * self.n + owner
        order = np.argsort(key_fwd, kind="stable")
        pos = np.searchsorted(key_fwd[order], key_rev)
        return order[pos].astype(np.uint32)

    def owner(self) -> np.ndarray:
        return np.repeat(np.arange(self.n, dtype=np.uint32), np.diff(self.row_ptr.astype(np.int64)))


def random_regular(n: int, k: int, seed: int = 1, n_topics: int = 1, unique_ips: bool = True) -> Network:
    """Seeded random k-regular network; all peers join all topics."""
    lib = _abi.load()
    row_ptr = np.empty(n + 1, dtype=np.uint32)
    col = np.empty(n * k, dtype=np.uint32)
    ob = np.empty(n * k, dtype=np.uint8)
    rc = lib.gsim_gen_random_regular(n, k, seed, _ptr(row_ptr), _ptr(col), _ptr(ob))
    if rc != 0:
        raise GsimError(rc, "gsim_gen_random_regular failed")
    mask = (1 << n_topics) - 1 if n_topics < 64 else (1 << 64) - 1
    sub = np.full(n, mask, dtype=np.uint64)
    ip_ptr = ip_ids = None
    n_ips = 0
    if unique_ips:
        ip_ptr = np.arange(n + 1, dtype=np.uint32)
        ip_ids = np.arange(n, dtype=np.uint32)
        n_ips = n
    return Network(n, row_ptr, col, ob, sub, ip_ptr, ip_ids, n_ips)


def app_scores(fn, n: int) -> np.ndarray:
    """AppSpecificScore(p) for every peer index (score_params.go:78), the array
    gsim_set_app_score installs.  A callback marked ``fn.vectorized = True``
    takes the whole index array at once; any other is called once per peer.
    Every peer's value is evaluated: there is no size above which it is skipped."""
    if getattr(fn, "vectorized", False):
        out = np.asarray(fn(np.arange(n, dtype=np.int64)), dtype=np.float64)
        if out.shape != (n,):
            raise ValueError("a vectorized AppSpecificScore must return one value per peer")
        return np.ascontiguousarray(out)
    return np.fromiter((fn(p) for p in range(n)), dtype=np.float64, count=n)


class Engine:
    """One simulated GossipSub network on one GPU."""

    def __init__(self, params: PeerScoreParams, thresholds: PeerScoreThresholds,
                 gossip: Optional[GossipSubParams] = None, topics: Optional[Sequence[str]] = None,
                 device: int = 0, validate: bool = True):
        """validate=False mirrors newPeerScore (score.go:183) as the reference's
        unit tests use it; the default mirrors WithPeerScore (gossipsub.go:278)."""
        self.lib = _abi.load()
        self.params = params
        self.thresholds = thresholds
        self.gossip = gossip or GossipSubParams()
        self.topics: List[str] = sorted(set(topics or []) | set(params.Topics))
        self.topic_index = {t: i for i, t in enumerate(self.topics)}
        pc = params.to_c()
        self._tarr = params.topic_array(self.topics)
        tc = thresholds.to_c()
        gc = self.gossip.to_c()
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(512)
        create = self.lib.gsim_create if validate else self.lib.gsim_create_unvalidated
        rc = create(ctypes.byref(pc), self._tarr, len(self.topics), ctypes.byref(tc),
                                  ctypes.byref(gc), device, ctypes.byref(h), buf, len(buf))
        if rc != 0:
            if rc == _abi.GSIM_EINVAL:
                raise ValueError(buf.value.decode())
            raise GsimError(rc, buf.value.decode())
        self.h = h
        self.device = device
        self.net: Optional[Network] = None

    # -- lifecycle -----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.gsim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            msg = self.lib.gsim_last_error(self.h)
            msg = msg.decode() if msg else ""
            if rc == _abi.GSIM_EINVAL:
                raise ValueError(msg)
            raise GsimError(rc, msg)

    # -- setup -----------------------------------------------------------------
    def load_graph(self, net: Network):
        self._check(self.lib.gsim_load_graph(
            self.h, net.n, _ptr(net.row_ptr), _ptr(net.col), _ptr(net.outbound), _ptr(net.sub),
            _ptr(net.ip_ptr), _ptr(net.ip_ids), net.n_ips))
        self.net = net
        if self.params.AppSpecificScore is not None:
            self.set_app_score(app_scores(self.params.AppSpecificScore, net.n))

    def set_app_score(self, p5: np.ndarray):
        p5 = np.ascontiguousarray(p5, dtype=np.float64)
        self._check(self.lib.gsim_set_app_score(self.h, _ptr(p5)))

    def set_ips(self, ip_ptr: np.ndarray, ip_ids: np.ndarray, n_ips: int):
        """refreshIPs (score.go:568-585): every peer's IP list replaced (gsim_set_ips)."""
        p = np.ascontiguousarray(ip_ptr, dtype=np.uint32)
        i = np.ascontiguousarray(ip_ids, dtype=np.uint32)
        self._check(self.lib.gsim_set_ips(self.h, _ptr(p), _ptr(i), int(n_ips)))

    def snapshot(self, obs_lo: int = 0, obs_hi: Optional[int] = None):
        """ExtendedPeerScoreInspectFn's view (score.go:127-140, 472-500) of the
        observers [obs_lo, obs_hi): one PeerScoreSnapshot per connection (edge
        order) and its TopicScoreSnapshots [edges, T] (gsim_read_snapshot)."""
        hi = self.net.n if obs_hi is None else obs_hi
        ne = int(self.net.row_ptr[hi]) - int(self.net.row_ptr[obs_lo])
        T = max(1, len(self.topics))
        peers = np.zeros(ne, dtype=_abi.PEER_SNAPSHOT_DTYPE)
        topics = np.zeros((ne, T), dtype=_abi.TOPIC_SNAPSHOT_DTYPE)
        self._check(self.lib.gsim_read_snapshot(self.h, int(obs_lo), int(hi), _ptr(peers), _ptr(topics)))
        return peers, topics

    def set_ip_whitelist(self, white: Optional[np.ndarray]):
        w = None if white is None else np.ascontiguousarray(white, dtype=np.uint8)
        self._check(self.lib.gsim_set_ip_whitelist(self.h, _ptr(w)))

    def set_topic_score_params(self, topic: str, p):
        """Topic.SetScoreParams -> peerScore.SetTopicScoreParams (topic.go:44-82, score.go:201-241)."""
        c = p.to_c(True)
        self._check(self.lib.gsim_set_topic_params(self.h, self.topic_index[topic], ctypes.byref(c)))
        self.params.Topics[topic] = p

    # -- hot path ----------------------------------------------------------------
    def refresh_scores(self, now: int):
        self._check(self.lib.gsim_refresh_scores(self.h, int(now)))

    def compute_scores(self):
        self._check(self.lib.gsim_compute_scores(self.h))

    def compute_ip_colocation(self):
        self._check(self.lib.gsim_compute_ip_colocation(self.h))

    def fill_synthetic(self, seed: int, now: int, p_mesh: float):
        self._check(self.lib.gsim_fill_synthetic(self.h, int(seed), int(now), float(p_mesh)))

    def scores(self) -> np.ndarray:
        out = np.empty(self.net.e, dtype=np.float64)
        self._check(self.lib.gsim_read_scores(self.h, _ptr(out)))
        return out

    # -- raw state ----------------------------------------------------------------
    def field_shape(self, f: int):
        e = self.net.e
        if f in PARITY_TOPIC_FIELDS:
            return (2, max(1, len(self.topics)), e)
        if f == _abi.F_SEEN:
            return (self._msg_cfg.ring, self.net.n)
        if f == _abi.F_LASTPUT:
            return (max(1, len(self.topics)), self.net.n)
        if f == _abi.F_LASTPUB:
            return (self.net.n, max(1, len(self.topics)))
        if f == _abi.F_FANOUT_TOPICS:
            return (self.net.n,)
        return (max(1, len(self.topics)), e) if f in TOPIC_FIELDS else (e,)

    # -- heartbeat / control ------------------------------------------------------
    def census(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.gsim_census(self.h, _ptr(out)))
        keys = ["records", "in_mesh", "nz_first", "nz_meshd", "nz_fail", "nz_invalid", "mesh_links",
                "tracked_edges"]
        return {k: int(v) for k, v in zip(keys, out)}

    def set_seed(self, seed: int):
        self._check(self.lib.gsim_set_seed(self.h, int(seed)))

    def heartbeat(self, tick: int, now: int):
        """GossipSubRouter.heartbeat for every observer (gossipsub.go:1345-1606)."""
        self._check(self.lib.gsim_heartbeat(self.h, int(tick), int(now)))

    def handle_control(self, rnd: int, now: int):
        """handleGraft/handlePrune for the inbox of control round `rnd`."""
        self._check(self.lib.gsim_handle_control(self.h, int(rnd), int(now)))

    # -- message propagation ------------------------------------------------------
    def msgs_init(self, ring: int, rounds: int, t0: int, heartbeat: Optional[int] = None,
                  max_frontier: Optional[int] = None, max_arrivals: Optional[int] = None,
                  topic_slots: int = 0):
        """Allocate the message ring / seen-set (gsim_msgs_init).  topic_slots > 0:
        per-topic sub-rings (a message takes its topic's next slot in publication
        order) with member-compacted seen-set cells."""
        c = _abi.CMsgConfig()
        c.ring, c.rounds, c.t0_ns = int(ring), int(rounds), int(t0)
        c.heartbeat_ns = int(heartbeat if heartbeat is not None else self.gossip.HeartbeatInterval)
        # max_frontier bounds the claim / forwarder lists of member-compacted layouts
        # (0: the default; overflow falls back to the word scans); max_arrivals
        # sizes the IWANT response queue (0: the library default, gsim.h)
        c.max_frontier = int(max_frontier or 0)
        c.max_arrivals = int(max_arrivals or 0)
        # > 0: per-topic sub-rings of this many slots (ring = n_topics * topic_slots),
        # seen-set cells only for each topic's members (gsim.h gsim_msg_config)
        c.topic_slots = int(topic_slots or 0)
        self._check(self.lib.gsim_msgs_init(self.h, ctypes.byref(c)))
        self._msg_cfg = c

    def round_time(self, g: int) -> int:
        c = self._msg_cfg
        return c.t0_ns + (g // c.rounds) * c.heartbeat_ns + (g % c.rounds + 1) * c.heartbeat_ns // (c.rounds + 1)

    def publish(self, msgs, rnd: int):
        """Topic.Publish of each (id, topic, origin, verdict[, vdelay]) at its origin in
        round `rnd` (verdict: _abi.VERDICT_*, the validation result at every receiver;
        vdelay: the validation latency at every receiver in rounds, gsim_msg.vdelay)."""
        arr = np.zeros(len(msgs), dtype=_abi.MSG_DTYPE)
        for k, msg in enumerate(msgs):
            mid, topic, origin, verdict = msg[:4]
            arr[k]["id"], arr[k]["topic"], arr[k]["origin"], arr[k]["verdict"] = mid, topic, origin, verdict
            arr[k]["vdelay"] = msg[4] if len(msg) > 4 else 0
        self._check(self.lib.gsim_publish(self.h, _ptr(arr), len(arr), int(rnd)))

    def publish_array(self, arr: np.ndarray, rnd: int):
        """Like publish() for a prebuilt numpy array of dtype _abi.MSG_DTYPE."""
        a = np.ascontiguousarray(arr)
        self._check(self.lib.gsim_publish(self.h, _ptr(a), len(a), int(rnd)))

    def round(self, rnd: int):
        """One propagation round for the whole network (gsim_round)."""
        self._check(self.lib.gsim_round(self.h, int(rnd)))

    def step(self, tick: int, n_ticks: int = 1, sched: Optional[dict] = None):
        """n_ticks whole heartbeat ticks in one call (gsim_step): refresh,
        heartbeat and the rounds of each tick, with sched[g] (an array of
        dtype _abi.MSG_DTYPE or a list of (id, topic, origin, verdict[, vdelay])
        tuples) published in round g.  The heartbeat timer loop,
        gossipsub.go:1320-1343."""
        R = self._msg_cfg.rounds
        g0 = int(tick) * R
        parts, off = [], [0]
        for q in range(int(n_ticks) * R):
            m = (sched or {}).get(g0 + q)
            if m is not None and len(m):
                if not isinstance(m, np.ndarray):
                    arr = np.zeros(len(m), dtype=_abi.MSG_DTYPE)
                    for k, msg in enumerate(m):
                        arr[k]["id"], arr[k]["topic"], arr[k]["origin"], arr[k]["verdict"] = msg[:4]
                        if len(msg) > 4:
                            arr[k]["vdelay"] = msg[4]
                    m = arr
                parts.append(np.ascontiguousarray(m))
            off.append(off[-1] + (len(parts[-1]) if m is not None and len(m) else 0))
        if off[-1]:
            msgs = np.ascontiguousarray(np.concatenate(parts))
            offs = np.asarray(off, dtype=np.int64)
            self._check(self.lib.gsim_step(self.h, int(tick), int(n_ticks), _ptr(msgs), _ptr(offs)))
        else:
            self._check(self.lib.gsim_step(self.h, int(tick), int(n_ticks), None, None))

    def set_peer_behaviour(self, flags: np.ndarray):
        """Per-peer adversarial behaviour (gsim_set_peer_behaviour)."""
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self.lib.gsim_set_peer_behaviour(self.h, _ptr(f)))

    def set_connections(self, pairs, up: bool, now: int):
        """Connections (a, b) going down or up between ticks, both endpoints
        notified: the router's and the score tracer's RemovePeer / AddPeer
        (gsim_set_connections; gossipsub.go:525-567, score.go:595-644)."""
        p = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
        self._check(self.lib.gsim_set_connections(self.h, _ptr(p), int(p.shape[0]), 1 if up else 0, int(now)))

    def set_subscriptions(self, pairs, join: bool, tick: int, now: int):
        """Join (join=True) or Leave the (peer, topic) pairs between ticks
        (gsim_set_subscriptions; gossipsub.go:1047-1124, pubsub.go:1051-1079),
        before the refresh of `tick`."""
        p = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
        self._check(self.lib.gsim_set_subscriptions(self.h, _ptr(p), int(p.shape[0]), 1 if join else 0, int(tick),
                                                    int(now)))

    def set_peer_gater(self, params, topic_weights=None):
        """WithPeerGater (peer_gater.go:161-186) on every router (gsim_set_peer_gater):
        params is a gsim.PeerGaterParams; its TopicDeliveryWeights (topic index ->
        weight) unless topic_weights ([T]) is given."""
        c = params.to_c()
        T = max(1, len(self.topics))
        w = np.zeros(T, dtype=np.float64)
        for t, x in (params.TopicDeliveryWeights or {}).items():
            w[int(t)] = float(x)
        if topic_weights is not None:
            w = np.ascontiguousarray(topic_weights, dtype=np.float64)
        self._check(self.lib.gsim_set_peer_gater(self.h, ctypes.byref(c), _ptr(w)))

    def gater_throttled(self) -> int:
        """Message copies the peer gater dropped (AcceptControl) so far."""
        n = ctypes.c_int64(0)
        self._check(self.lib.gsim_gater_throttled(self.h, ctypes.byref(n)))
        return n.value

    def gater_read(self) -> dict:
        """The peer gater's state (gsim_gater_read): validate / throttle / last per
        router, and per connection (edge order) the IP group's counters
        [deliver, duplicate, ignore, reject], connected and expire at the group's
        representative position."""
        N, E = self.net.n, self.net.e
        out = {"validate": np.zeros(N), "throttle": np.zeros(N), "last": np.zeros(N, dtype=np.int64),
               "counters": np.zeros((4, E)), "connected": np.zeros(E, dtype=np.int32),
               "expire": np.zeros(E, dtype=np.int64)}
        self._check(self.lib.gsim_gater_read(self.h, _ptr(out["validate"]), _ptr(out["throttle"]), _ptr(out["last"]),
                                             _ptr(out["counters"]), _ptr(out["connected"]), _ptr(out["expire"])))
        return out

    def px_connect(self, now: int, want_pairs: bool = True):
        """The connector for the attempts peer exchange queued this tick
        (gsim_px_connect; pxConnect gossipsub.go:893-973): returns the
        (dialer, peer) pairs that became connections, sorted (want_pairs
        False: only their number, nothing read back or sorted)."""
        n = ctypes.c_int64(0)
        if not want_pairs:
            self._check(self.lib.gsim_px_connect(self.h, int(now), None, 0, ctypes.byref(n)))
            return n.value
        cap = max(1, self.net.e // 2)
        out = np.zeros((cap, 2), dtype=np.uint32)
        self._check(self.lib.gsim_px_connect(self.h, int(now), _ptr(out), int(cap), ctypes.byref(n)))
        return out[:min(n.value, cap)].copy()

    # -- connection tags and the connection manager's trim (gsim.connmgr reads the results) --
    def conn_tags_config(self, bump: int = 1, cap: int = 15, decay_amount: int = 1,
                         decay_interval: Optional[int] = None, t0: Optional[int] = None, off: bool = False):
        """The tag tracer's decaying delivery tags on every router (gsim_conn_tags_config;
        tag_tracer.go): the defaults are GossipSubConnTag*, decay_interval in ns (10 min),
        t0 the phase of the decay instants (the message clock's t0).  After msgs_init.
        Calling it again starts from zero tags; off=True frees them."""
        if off:
            self._check(self.lib.gsim_conn_tags_config(self.h, None))
            return
        c = _abi.CConnTagParams()
        self.lib.gsim_default_conn_tag_params(int(self._msg_cfg.t0_ns if t0 is None else t0), ctypes.byref(c))
        c.bump, c.cap, c.decay_amount = int(bump), int(cap), int(decay_amount)
        if decay_interval is not None:
            c.decay_interval_ns = int(decay_interval)
        self._check(self.lib.gsim_conn_tags_config(self.h, ctypes.byref(c)))

    def conn_tags(self, topic: int) -> np.ndarray:
        """The delivery tags of `topic` per connection, u8 [E] in edge order (gsim_conn_tags_read)."""
        out = np.zeros(self.net.e, dtype=np.uint8)
        self._check(self.lib.gsim_conn_tags_read(self.h, int(topic), _ptr(out)))
        return out

    def conn_values(self, now: int, grace: int = 0):
        """(value i32 [E], flags u8 [E]) per connection in edge order: the sum of its
        delivery tags and _abi.CONN_CONNECTED | CONN_PROTECTED | CONN_GRACE (gsim_conn_values)."""
        value = np.zeros(self.net.e, dtype=np.int32)
        flags = np.zeros(self.net.e, dtype=np.uint8)
        self._check(self.lib.gsim_conn_values(self.h, int(now), int(grace), _ptr(value), _ptr(flags)))
        return value, flags

    def conn_trim(self, tick: int, now: int, low: int, high: int, grace: int = 0, count_only: bool = False):
        """The connection manager's trim on every router at once (gsim_conn_trim): the
        connections closed, as sorted unique (a < b) pairs [n, 2]; they went down as
        through set_connections(pairs, up=False, now).  high = 0 forces the trim of
        every router above low.  count_only: their number, nothing closes."""
        n = ctypes.c_int64(0)
        if count_only:
            self._check(self.lib.gsim_conn_trim(self.h, int(tick), int(now), int(low), int(high), int(grace), None, 0,
                                                ctypes.byref(n)))
            return n.value
        cap = max(1, self.net.e // 2)
        out = np.empty((cap, 2), dtype=np.uint32)             # (untouched beyond the rows the call writes)
        self._check(self.lib.gsim_conn_trim(self.h, int(tick), int(now), int(low), int(high), int(grace), _ptr(out),
                                            int(cap), ctypes.byref(n)))
        return out[:n.value].copy()

    # gsim_trace_event
    TRACE_DTYPE = np.dtype([("timestamp", np.int64), ("msg_id", np.uint64), ("peer", np.uint32),
                            ("other", np.uint32), ("topic", np.int32), ("type", np.uint8), ("reason", np.uint8),
                            ("_pad", np.uint16)])

    def trace_config(self, peer_lo: int, peer_hi: int, cap: int = 1 << 20):
        """Trace the routers [peer_lo, peer_hi) (gsim_trace_config; cap 0 stops)."""
        self._check(self.lib.gsim_trace_config(self.h, int(peer_lo), int(peer_hi), int(cap)))

    def trace_read(self) -> np.ndarray:
        """The traced events since the last read, sorted (gsim_trace_read):
        the pubsubTracer events of trace.go:70-530 as TRACE_DTYPE records."""
        n = ctypes.c_int64(0)
        self._check(self.lib.gsim_trace_read(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=self.TRACE_DTYPE)
        self._check(self.lib.gsim_trace_read(self.h, _ptr(out) if n.value else None, n.value, ctypes.byref(n)))
        return out[:n.value]

    # -- score tracer events (gsim.tracer builds the arrays) ----------------------
    def tracer_config(self, records_cap: int, peers_cap: int, seen_ttl: int = 0):
        """Size the delivery records behind tracer_events: records_cap records
        (one per (observer, message id) alive at a time), peers_cap entries of
        their peers lists, seen_ttl ns of lifetime (0: TimeCacheDuration)
        (gsim_score_tracer_config).  Calling it again drops every record."""
        self._check(self.lib.gsim_score_tracer_config(self.h, int(records_cap), int(peers_cap), int(seen_ttl)))

    def tracer_events(self, events: np.ndarray):
        """Apply a batch of RawTracer calls (an array of gsim.tracer.EVENT_DTYPE;
        the builders of gsim.tracer make its rows): each observer's events in
        array order, observers independently (gsim_score_tracer_events).  A bad
        event fails the whole batch (ValueError naming its index, nothing
        applied); a batch the record space may not hold is a GsimError
        (GSIM_ERANGE, nothing applied)."""
        a = np.ascontiguousarray(events, dtype=np.dtype(_abi.SCORE_EVENT_DTYPE))
        self._check(self.lib.gsim_score_tracer_events(self.h, _ptr(a) if len(a) else None, len(a)))

    def tracer_gc(self, now: int):
        """gcDeliveryRecords (score.go:863-877): drop the records with now > expire (gsim_score_tracer_gc)."""
        self._check(self.lib.gsim_score_tracer_gc(self.h, int(now)))

    def tracer_stats(self) -> dict:
        """Live records, live peers-list entries, events applied, records collected (gsim_score_tracer_stats)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.gsim_score_tracer_stats(self.h, _ptr(out)))
        return dict(zip(["records", "peer_entries", "events", "collected"], (int(x) for x in out)))

    def tracer_settled(self) -> tuple:
        """(records whose pending mesh-delivery increments an event settled so
        far, whether the engine still holds such increments) (gsim_score_tracer_settled)."""
        out = np.zeros(2, dtype=np.int64)
        self._check(self.lib.gsim_score_tracer_settled(self.h, _ptr(out)))
        return int(out[0]), bool(out[1])

    # -- router state: seen cache and IWANT promises (gsim.routerstate builds the arrays) --
    def router_state_config(self, seen_cap: int, promises_cap: int, strategy: int = 0, seen_ttl: int = 0,
                            followup: int = 0):
        """Size the seen cache (seen_cap entries) and the gossip tracer's
        promises (promises_cap), over all observers.  strategy 0: first-seen,
        1: last-seen; seen_ttl 0: TimeCacheDuration; followup 0: the engine's
        IWantFollowupTime (gsim_router_state_config).  Calling it again drops
        everything."""
        self._check(self.lib.gsim_router_state_config(self.h, int(seen_cap), int(promises_cap), int(strategy),
                                                      int(seen_ttl), int(followup)))

    def router_state_events(self, events: np.ndarray) -> np.ndarray:
        """Apply a batch of seen-cache and gossip-tracer calls (an array of
        gsim.routerstate.EVENT_DTYPE): each observer's events in array order,
        observers independently; returns the uint8 answer of every event
        (gsim_router_state_events).  A bad event fails the whole batch
        (ValueError naming its index, nothing applied); a batch the space may
        not hold is a GsimError (GSIM_ERANGE, nothing applied)."""
        a = np.ascontiguousarray(events, dtype=np.dtype(_abi.ROUTER_EVENT_DTYPE))
        res = np.zeros(len(a), dtype=np.uint8)
        self._check(self.lib.gsim_router_state_events(self.h, _ptr(a) if len(a) else None, len(a),
                                                      _ptr(res) if len(a) else None))
        return res

    def router_state_sweep(self, now: int):
        """The time cache's sweep: drop the seen entries with expiry < now (gsim_router_state_sweep)."""
        self._check(self.lib.gsim_router_state_sweep(self.h, int(now)))

    def router_state_throttle(self, pairs) -> int:
        """ThrottlePeer for (observer, peer) pairs: their promises are dropped;
        returns how many (gsim_router_state_throttle)."""
        p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        dropped = ctypes.c_int64(0)
        self._check(self.lib.gsim_router_state_throttle(self.h, _ptr(p) if len(p) else None, len(p),
                                                        ctypes.byref(dropped)))
        return dropped.value

    def router_state_broken(self, now: int, apply_penalty: bool = False) -> np.ndarray:
        """GetBrokenPromises of every observer: the promises with expire < now
        are removed; one (observer, peer, count) row each, sorted, as a
        structured array.  apply_penalty: each row is also AddPenalty(peer,
        count) at the observer's peerScore (gsim_router_state_broken)."""
        n = ctypes.c_int64(0)
        cap = 256
        while True:
            out = np.zeros(cap, dtype=np.dtype(_abi.BROKEN_ROW_DTYPE))
            rc = self.lib.gsim_router_state_broken(self.h, int(now), int(bool(apply_penalty)), _ptr(out), cap,
                                                   ctypes.byref(n))
            if rc == _abi.GSIM_ERANGE and n.value > cap:        # nothing was removed: once more with room
                cap = n.value
                continue
            self._check(rc)
            return out[:n.value]

    def router_state_stats(self) -> dict:
        """Live seen entries and promises, events applied, entries swept,
        promises fulfilled or throttled, promises broken (gsim_router_state_stats)."""
        out = np.zeros(6, dtype=np.int64)
        self._check(self.lib.gsim_router_state_stats(self.h, _ptr(out)))
        return dict(zip(["seen", "promises", "events", "swept", "fulfilled", "broken"], (int(x) for x in out)))

    def set_direct_peers(self, flags):
        """WithDirectPeers as per-edge flags (edge order; None clears)
        (gsim_set_direct_peers; gossipsub.go:352-374)."""
        if flags is None:
            self._check(self.lib.gsim_set_direct_peers(self.h, None))
            return
        f = np.ascontiguousarray(flags, dtype=np.uint8)
        if f.shape != (self.net.e,):
            raise ValueError("direct flags: one byte per edge")
        self._check(self.lib.gsim_set_direct_peers(self.h, _ptr(f)))

    def gossip_stats(self) -> dict:
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.gsim_gossip_stats(self.h, _ptr(out)))
        return dict(zip(["ihave_walks", "iwant_ids", "iwant_responses", "broken_promises"], (int(x) for x in out)))

    def msg_stats(self) -> list:
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.gsim_msg_stats(self.h, _ptr(out)))
        return [int(x) for x in out]

    # struct gsim_msg_report
    MSG_REPORT_DTYPE = np.dtype(_abi.MSG_REPORT_DTYPE)

    def msg_report(self, round_lo: int = 0, round_hi: int | None = None) -> np.ndarray:
        """Reach and latency histogram of every message still in the ring that
        was published in [round_lo, round_hi) (None: no upper bound), as
        MSG_REPORT_DTYPE rows ordered by (pub_round, slot) (gsim_msg_report;
        helpers over the array: gsim.report)."""
        hi = (1 << 63) - 1 if round_hi is None else int(round_hi)
        n = ctypes.c_int64(0)
        self._check(self.lib.gsim_msg_report(self.h, int(round_lo), hi, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=self.MSG_REPORT_DTYPE)
        if n.value:
            self._check(self.lib.gsim_msg_report(self.h, int(round_lo), hi, _ptr(out), n.value, ctypes.byref(n)))
        return out[:n.value]

    # struct gsim_mesh_row / struct gsim_score_row
    MESH_ROW_DTYPE = np.dtype(_abi.MESH_ROW_DTYPE)
    SCORE_ROW_DTYPE = np.dtype(_abi.SCORE_ROW_DTYPE)

    def set_peer_classes(self, cls):
        """One class (< _abi.NET_CLASSES) per peer, None: all class 0; the
        classes key net_report and change nothing else (gsim_set_peer_classes)."""
        if cls is None:
            self._check(self.lib.gsim_set_peer_classes(self.h, None))
            return
        c = np.ascontiguousarray(cls, dtype=np.uint8)
        if c.shape != (self.net.n,):
            raise ValueError("peer classes: one byte per peer")
        self._check(self.lib.gsim_set_peer_classes(self.h, _ptr(c)))

    def net_report(self, edges=None):
        """(mesh_rows, score_rows): per (topic, observer class) the mesh sizes,
        links by the neighbour's class and fanout (MESH_ROW_DTYPE), and per
        (observer class, subject class) the score snapshot's histogram over
        `edges` (at most 15 ascending values; None: gsim.report.threshold_edges
        of the engine's thresholds) with counts, min and max (SCORE_ROW_DTYPE),
        reduced on the device (gsim_net_report; helpers: gsim.report)."""
        from . import report
        ed = report.threshold_edges(self.thresholds) if edges is None else edges
        ed = np.ascontiguousarray(ed, dtype=np.float64).reshape(-1)
        return _net_report_call(self, self.lib.gsim_net_report, self.h, ed)

    # struct gsim_score_part_row / gsim_score_cause_row / gsim_score_topic_row
    SCORE_PART_ROW_DTYPE = np.dtype(_abi.SCORE_PART_ROW_DTYPE)
    SCORE_CAUSE_ROW_DTYPE = np.dtype(_abi.SCORE_CAUSE_ROW_DTYPE)
    SCORE_TOPIC_ROW_DTYPE = np.dtype(_abi.SCORE_TOPIC_ROW_DTYPE)

    def score_report(self, edges=None, params=None, topics=None):
        """(part_rows, cause_rows, topic_rows): the live score of every record
        decomposed into P1..P7 -- per (observer class, subject class, part) a
        fixed signed-log histogram with min, max and NaN count
        (SCORE_PART_ROW_DTYPE; bins: gsim.report.part_bin_bounds), per class
        pair the totals by bin of `edges` (as net_report's) and dominant
        negative part (SCORE_CAUSE_ROW_DTYPE), per (topic, class pair) the
        flag counts (SCORE_TOPIC_ROW_DTYPE) -- reduced on the device from the
        current counters.  What-if: `params`, a PeerScoreParams scored with
        instead of the engine's (its .Topics give the topic table), and / or
        `topics`, a {topic name: TopicScoreParams} laid over that table; the
        engine's own parameters and state stay as they are
        (gsim_score_report; helpers: gsim.report)."""
        from . import report
        ed = report.threshold_edges(self.thresholds) if edges is None else edges
        ed = np.ascontiguousarray(ed, dtype=np.float64).reshape(-1)
        return _score_report_call(self, self.lib.gsim_score_report, self.h, ed, params, topics)

    # struct gsim_peer_row / struct gsim_peer_class_row
    PEER_ROW_DTYPE = np.dtype(_abi.PEER_ROW_DTYPE)
    PEER_CLASS_ROW_DTYPE = np.dtype(_abi.PEER_CLASS_ROW_DTYPE)

    def peer_report(self, round_lo: int = 0, round_hi: int | None = None, peers=None, classes: bool = True):
        """(peer_rows, class_rows) over the messages msg_report(round_lo,
        round_hi) selects: per peer of `peers` (None: every peer; (lo, hi): that
        range) the messages expected, received, missed, its latencies and its
        first deliveries by the first sender's class (PEER_ROW_DTYPE), and per
        (topic, class of the receiving peer) the same over every peer with a
        latency histogram (PEER_CLASS_ROW_DTYPE; classes=False: an empty
        array), reduced on the device from the seen-set cells
        (gsim_peer_report; helpers: gsim.report)."""
        return _peer_report_call(self, self.lib.gsim_peer_report, self.h, self.net.n, round_lo, round_hi, peers, classes)

    # struct gsim_relay_row / struct gsim_relay_class_row / struct gsim_relay_msg_row
    RELAY_ROW_DTYPE = np.dtype(_abi.RELAY_ROW_DTYPE)
    RELAY_CLASS_ROW_DTYPE = np.dtype(_abi.RELAY_CLASS_ROW_DTYPE)
    RELAY_MSG_ROW_DTYPE = np.dtype(_abi.RELAY_MSG_ROW_DTYPE)

    def relay_report(self, round_lo: int = 0, round_hi: int | None = None, peers=None, classes: bool = True,
                     messages: bool = True):
        """(peer_rows, class_rows, msg_rows): the first-delivery forest of the
        messages msg_report(round_lo, round_hi) selects, from the sender's
        side.  Per peer of `peers` (None: every peer; (lo, hi): that range) the
        messages it held and relayed and the first deliveries it gave, by the
        class of the receiving child (RELAY_ROW_DTYPE); per (topic, class of
        the sender) the same over every peer with a fan-out histogram
        (RELAY_CLASS_ROW_DTYPE); per message its relays, widest holder, exact
        depth, depth histogram and per-hop delay histogram
        (RELAY_MSG_ROW_DTYPE).  classes=False / messages=False: an empty array
        in that place.  Reduced on the device from the seen-set cells
        (gsim_relay_report; helpers: gsim.report)."""
        hi = (1 << 63) - 1 if round_hi is None else int(round_hi)
        lo_p, hi_p = (0, int(self.net.n)) if peers is None else (int(peers[0]), int(peers[1]))
        nc, nm = ctypes.c_int64(0), ctypes.c_int64(0)
        fn = self.lib.gsim_relay_report
        self._check(fn(self.h, int(round_lo), hi, lo_p, hi_p, None, None, 0, ctypes.byref(nc), None, 0, ctypes.byref(nm)))
        rows = np.zeros(max(hi_p - lo_p, 0), dtype=Engine.RELAY_ROW_DTYPE)
        cls = np.zeros(nc.value if classes else 0, dtype=Engine.RELAY_CLASS_ROW_DTYPE)
        msg = np.zeros(nm.value if messages else 0, dtype=Engine.RELAY_MSG_ROW_DTYPE)
        if len(rows) or len(cls) or len(msg):
            self._check(fn(self.h, int(round_lo), hi, lo_p, hi_p, _ptr(rows) if len(rows) else None,
                           _ptr(cls) if len(cls) else None, len(cls), ctypes.byref(nc),
                           _ptr(msg) if len(msg) else None, len(msg), ctypes.byref(nm)))
        return rows, cls, msg

    def relay_report_budget(self, nbytes: int = 0):
        """Debug: the byte budget of relay_report's per-batch scratch (0: the default)."""
        self._check(self.lib.gsim_relay_report_budget(self.h, int(nbytes)))

    def relay_report_launch(self) -> dict:
        """How the last relay_report ran (gsim_relay_report_launch)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.gsim_relay_report_launch(self.h, _ptr(out)))
        return dict(zip(["batch", "batches", "depth_passes", "messages"], (int(x) for x in out)))

    # struct gsim_mesh_path_row
    MESH_PATH_ROW_DTYPE = np.dtype(_abi.MESH_PATH_ROW_DTYPE)

    def mesh_paths(self, topic: int, sources, blocked=(), max_hops: int = 0, per_peer: bool = False):
        """Hop distances over the mesh of `topic` from every peer of `sources`
        (a source outside the topic expands once over its fanout), one
        MESH_PATH_ROW_DTYPE row per source in the given order: reached,
        subscribers, the exact largest distance, a distance histogram and the
        reach by peer class.  `blocked`: the peer classes that are reached but
        do not relay (a read-only what-if; a source still forwards its own
        publication); `max_hops` > 0 stops after that many levels.
        per_peer=True: (rows, reach_count, hop_sum), per peer the number of
        sources that reach it and the sum of its distances.  More than 64
        sources run in batches of 64.  A traversal on the device
        (gsim_mesh_paths; helpers: gsim.report)."""
        return _mesh_paths_call(self, self.lib.gsim_mesh_paths, self.h, self.net.n, topic, sources, blocked, max_hops,
                                per_peer)

    def peer_report_launch(self) -> dict:
        """How the last peer_report's reduction was launched (gsim_peer_report_launch)."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.gsim_peer_report_launch(self.h, _ptr(out)))
        return dict(zip(["waves", "parts", "messages"], (int(x) for x in out)))

    def read(self, f: int) -> np.ndarray:
        out = np.empty(self.field_shape(f), dtype=_FIELD_DTYPES[f])
        self._check(self.lib.gsim_read_field(self.h, f, _ptr(out), out.nbytes))
        return out

    def write(self, f: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr, dtype=_FIELD_DTYPES[f]).reshape(self.field_shape(f))
        self._check(self.lib.gsim_write_field(self.h, f, _ptr(a), a.nbytes))

    # -- timing on the engine stream ----------------------------------------------
    def event_record(self, slot: int):
        self._check(self.lib.gsim_event_record(self.h, slot))

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = ctypes.c_float()
        self._check(self.lib.gsim_event_elapsed(self.h, a, b, ctypes.byref(ms)))
        return float(ms.value)

    def synchronize(self):
        self._check(self.lib.gsim_synchronize(self.h))

    def profile(self, enable: bool = True):
        """Record per-kernel-class device time with HIP events (gsim_profile)."""
        self._check(self.lib.gsim_profile(self.h, int(bool(enable))))

    def profile_read(self) -> dict:
        """{class: (ms, launches)} since the last read (synchronizes)."""
        n = len(_abi.KERNEL_CLASSES)
        ms = np.zeros(n, dtype=np.float64)
        cnt = np.zeros(n, dtype=np.int64)
        self._check(self.lib.gsim_profile_read(self.h, _ptr(ms), _ptr(cnt), n))
        return {c: (float(ms[i]), int(cnt[i])) for i, c in enumerate(_abi.KERNEL_CLASSES)}

    def set_kernel_variant(self, which: int, variant: int):
        self._check(self.lib.gsim_set_kernel_variant(self.h, which, variant))


def _mesh_paths_call(eng, fn, handle, n_peers, topic, sources, blocked, max_hops, per_peer):
    """gsim_mesh_paths / gsim_group_mesh_paths in batches of _abi.PATH_SOURCES:
    rows concatenated, the per-peer arrays summed."""
    src = np.ascontiguousarray(sources, dtype=np.uint32).reshape(-1)
    mask = 0
    for c in ([blocked] if np.isscalar(blocked) else blocked):
        if not 0 <= int(c) < 32:
            raise ValueError("mesh_paths: a blocked class must lie in 0..31")
        mask |= 1 << int(c)
    rows = np.zeros(len(src), dtype=Engine.MESH_PATH_ROW_DTYPE)
    reach = np.zeros(n_peers, dtype=np.uint32)
    hops = np.zeros(n_peers, dtype=np.uint32)
    for lo in range(0, len(src), _abi.PATH_SOURCES):
        part = np.ascontiguousarray(src[lo:lo + _abi.PATH_SOURCES])
        out = np.zeros(len(part), dtype=Engine.MESH_PATH_ROW_DTYPE)
        rc = np.zeros(n_peers, dtype=np.uint32) if per_peer else None
        hs = np.zeros(n_peers, dtype=np.uint32) if per_peer else None
        eng._check(fn(handle, int(topic), _ptr(part), len(part), mask, int(max_hops), _ptr(out),
                      _ptr(rc) if per_peer else None, _ptr(hs) if per_peer else None))
        rows[lo:lo + len(part)] = out
        if per_peer:
            reach += rc
            hops += hs
    return (rows, reach, hops) if per_peer else rows


def _peer_report_call(eng, fn, handle, n_peers, round_lo, round_hi, peers, classes):
    """gsim_peer_report / gsim_group_peer_report: count the class rows, then fill."""
    hi = (1 << 63) - 1 if round_hi is None else int(round_hi)
    lo_p, hi_p = (0, int(n_peers)) if peers is None else (int(peers[0]), int(peers[1]))
    nc, nm = ctypes.c_int64(0), ctypes.c_int64(0)
    eng._check(fn(handle, int(round_lo), hi, lo_p, hi_p, None, None, 0, ctypes.byref(nc), ctypes.byref(nm)))
    rows = np.zeros(max(hi_p - lo_p, 0), dtype=Engine.PEER_ROW_DTYPE)
    cls = np.zeros(nc.value if classes else 0, dtype=Engine.PEER_CLASS_ROW_DTYPE)
    if len(rows) or len(cls):
        eng._check(fn(handle, int(round_lo), hi, lo_p, hi_p, _ptr(rows) if len(rows) else None,
                      _ptr(cls) if len(cls) else None, len(cls), ctypes.byref(nc), ctypes.byref(nm)))
    return rows, cls


def _score_what_if(eng, params, topics):
    """struct gsim_score_what_if of a PeerScoreParams and / or a topic overlay
    (None when both are None), with the objects that must outlive the call."""
    if params is None and topics is None:
        return None, ()
    w = _abi.CScoreWhatIf()
    keep = []
    if params is not None:
        pc = params.to_c()
        keep.append(pc)
        w.peer = ctypes.pointer(pc)
    if params is not None or topics:
        table = dict((params if params is not None else eng.params).Topics)
        for name, tp in (topics or {}).items():
            if name not in eng.topic_index:
                raise ValueError(f"score_report: unknown topic {name!r}")
            table[name] = tp
        arr = (_abi.CTopicScoreParams * max(1, len(eng.topics)))()
        for i, name in enumerate(eng.topics):
            arr[i] = table[name].to_c(True) if name in table else TopicScoreParams().to_c(False)
        keep.append(arr)
        w.topics = ctypes.cast(arr, ctypes.POINTER(_abi.CTopicScoreParams))
        w.n_topics = max(1, len(eng.topics))
    return w, keep


def _score_report_call(eng, fn, handle, ed: np.ndarray, params, topics):
    """gsim_score_report / gsim_group_score_report: count, then fill."""
    w, keep = _score_what_if(eng, params, topics)
    wp = ctypes.byref(w) if w is not None else None
    p = _ptr(ed) if len(ed) else None
    n = [ctypes.c_int64(0) for _ in range(3)]

    def call(bufs):
        args = []
        for b, c in zip(bufs, n):
            args += [_ptr(b) if b is not None and len(b) else None, len(b) if b is not None else 0, ctypes.byref(c)]
        eng._check(fn(handle, wp, p, len(ed), *args))

    call((None, None, None))
    rows = (np.zeros(n[0].value, dtype=Engine.SCORE_PART_ROW_DTYPE),
            np.zeros(n[1].value, dtype=Engine.SCORE_CAUSE_ROW_DTYPE),
            np.zeros(n[2].value, dtype=Engine.SCORE_TOPIC_ROW_DTYPE))
    call(rows)
    del keep
    return rows


def _net_report_call(eng, fn, handle, ed: np.ndarray):
    """gsim_net_report / gsim_group_net_report: count, then fill."""
    p = _ptr(ed) if len(ed) else None
    nm, ns = ctypes.c_int64(0), ctypes.c_int64(0)
    eng._check(fn(handle, p, len(ed), None, 0, ctypes.byref(nm), None, 0, ctypes.byref(ns)))
    mesh = np.zeros(nm.value, dtype=Engine.MESH_ROW_DTYPE)
    scores = np.zeros(ns.value, dtype=Engine.SCORE_ROW_DTYPE)
    eng._check(fn(handle, p, len(ed), _ptr(mesh) if nm.value else None, nm.value, ctypes.byref(nm),
                  _ptr(scores) if ns.value else None, ns.value, ctypes.byref(ns)))
    return mesh, scores

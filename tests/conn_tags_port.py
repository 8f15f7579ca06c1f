"""A port of the reference's tag tracer (tag_tracer.go), method by method, over
an in-memory connection manager on a virtual clock (test infrastructure).

`ConnMgr` keeps what go-libp2p's BasicConnMgr keeps per peer as far as the tag
tracer and gossipsub_connmgr_test.go can observe it: Protect / Unprotect by tag
name, decaying tags (RegisterDecayingTag with DecayFixed and BumpSumBounded),
the time a connection was first seen, and a trim.  The connection manager
itself is not part of the reference tree; its trim is the restatement of
include/gsim.h (gsim_conn_trim): candidates connected, unprotected and out of
grace, ascending by (value, key), the first connected - low of them.  Decays
happen at the instants t0 + k * interval of the manager's clock (`advance`),
one shared phase for every tag.

`TagTracer` is tagTracer; `NetPort` holds one per router of a network and is
fed the network oracle's event log (oracle.h ORC_EV_*)."""
from __future__ import annotations

import numpy as np

import oracle_binding as ob
from gsim import _abi

# tag_tracer.go:13-31
GossipSubConnTagBumpMessageDelivery = 1
GossipSubConnTagDecayInterval = 10 * 60 * 1_000_000_000
GossipSubConnTagDecayAmount = 1
GossipSubConnTagMessageDeliveryCap = 15

RejectValidationThrottled = "validation throttled"
RejectValidationFailed = "validation failed"
RejectValidationIgnored = "validation ignored"
RejectInvalidSignature = "invalid signature"
VERDICT_REASON = {_abi.VERDICT_REJECT: RejectValidationFailed, _abi.VERDICT_IGNORE: RejectValidationIgnored,
                  _abi.VERDICT_THROTTLE: RejectValidationThrottled, _abi.VERDICT_SIGNATURE: RejectInvalidSignature}

OLD = -(1 << 61)       # first seen before any grace period


def DecayFixed(minuend):
    """connmgr.DecayFixed: subtract; the tag is removed once it reaches 0."""
    def fn(value):
        v = value - minuend
        return v, v <= 0
    return fn


def BumpSumBounded(lo, hi):
    """connmgr.BumpSumBounded: add within [lo, hi]."""
    def fn(value, delta):
        v = value + delta
        if v >= hi:
            return hi
        if v <= lo:
            return lo
        return v
    return fn


class DecayingTag:
    def __init__(self, mgr, name, interval, decay_fn, bump_fn):
        self.mgr, self.name, self.interval, self.decay_fn, self.bump_fn = mgr, name, interval, decay_fn, bump_fn
        self.closed = False

    def Bump(self, p, delta):
        if self.closed:
            raise RuntimeError(f"decaying tag {self.name} is closed")
        tags = self.mgr.tags.setdefault(p, {})
        tags[self.name] = self.bump_fn(tags.get(self.name, 0), delta)

    def Close(self):
        """The tag is removed from every peer."""
        self.closed = True
        for tags in self.mgr.tags.values():
            tags.pop(self.name, None)
        self.mgr.decaying.pop(self.name, None)


class ConnMgr:
    def __init__(self, low=5, high=10, grace=0, t0=0, interval=None):
        self.low, self.high, self.grace = low, high, grace
        self.interval = interval                       # the decayer's one interval (None: the first tag's)
        self.t0, self.now, self.k = t0, t0, 1          # the next decay instant is t0 + k * interval
        self.protected = {}                            # peer -> set of tag names
        self.tags = {}                                 # peer -> {tag name: value}
        self.decaying = {}                             # name -> DecayingTag
        self.first_seen = {}                           # connected peers -> time

    # -- protection ------------------------------------------------------------
    def Protect(self, p, tag):
        self.protected.setdefault(p, set()).add(tag)

    def Unprotect(self, p, tag):
        s = self.protected.get(p)
        if s is None:
            return False
        s.discard(tag)
        if not s:
            del self.protected[p]
            return False
        return True

    def IsProtected(self, p, tag=""):
        s = self.protected.get(p)
        if not s:
            return False
        return True if tag == "" else tag in s

    # -- decaying tags ---------------------------------------------------------
    def RegisterDecayingTag(self, name, interval, decay_fn, bump_fn):
        if name in self.decaying:
            raise RuntimeError(f"decaying tag with name {name} already exists")
        if self.interval is None:
            self.interval = interval
        assert interval == self.interval, "one decay interval per manager"
        tag = DecayingTag(self, name, interval, decay_fn, bump_fn)
        self.decaying[name] = tag
        return tag

    def advance(self, now):
        """The clock moves to `now`: every decay instant t0 + k * interval it
        reaches decays every tag once (all tags here share one interval)."""
        self.now = max(self.now, now)
        interval = self.interval
        while interval is not None and self.t0 + self.k * interval <= self.now:
            self.k += 1
            for tag in list(self.decaying.values()):
                for tags in self.tags.values():
                    if tag.name in tags:
                        v, rm = tag.decay_fn(tags[tag.name])
                        if rm:
                            del tags[tag.name]
                        else:
                            tags[tag.name] = v

    # -- connections -----------------------------------------------------------
    def Connected(self, p, now=OLD):
        self.first_seen[p] = now

    def Disconnected(self, p):
        """The manager forgets a disconnected peer: its tags go, protection stays by name."""
        self.first_seen.pop(p, None)
        self.tags.pop(p, None)

    def GetTagInfo(self, p):
        if p not in self.first_seen and p not in self.tags:
            return None
        tags = dict(self.tags.get(p, {}))
        return {"Tags": tags, "Value": sum(tags.values()), "FirstSeen": self.first_seen.get(p)}

    def value(self, p):
        return sum(self.tags.get(p, {}).values())

    def trim(self, now, key_fn, low=None, high=None, grace=None):
        """The peers whose connections this manager closes (include/gsim.h
        gsim_conn_trim).  high == 0 is the forced TrimOpenConns."""
        low = self.low if low is None else low
        high = self.high if high is None else high
        grace = self.grace if grace is None else grace
        conns = list(self.first_seen)
        if len(conns) <= (high if high > 0 else low):
            return []
        cands = [p for p in conns if not self.IsProtected(p) and self.first_seen[p] + grace <= now]
        cands.sort(key=lambda p: (self.value(p), key_fn(p)))
        return cands[:len(conns) - low]


class Message:
    def __init__(self, mid, topic, received_from):
        self.mid, self.topic, self.ReceivedFrom = mid, topic, received_from


def topicTag(topic):
    return f"pubsub:{topic}"


class TagTracer:
    """tagTracer (tag_tracer.go:44-259)."""

    def __init__(self, cmgr, bump=GossipSubConnTagBumpMessageDelivery, cap=GossipSubConnTagMessageDeliveryCap,
                 amount=GossipSubConnTagDecayAmount, interval=GossipSubConnTagDecayInterval):
        self.cmgr = cmgr
        self.decayer = cmgr
        self.decaying = {}
        self.direct = None
        self.nearFirst = {}
        self.bump, self.cap, self.amount, self.interval = bump, cap, amount, interval

    def tagPeerIfDirect(self, p):
        if self.direct is None:
            return
        if p in self.direct:
            self.cmgr.Protect(p, "pubsub:<direct>")

    def tagMeshPeer(self, p, topic):
        self.cmgr.Protect(p, topicTag(topic))

    def untagMeshPeer(self, p, topic):
        self.cmgr.Unprotect(p, topicTag(topic))

    def addDeliveryTag(self, topic):
        if self.decayer is None:
            return
        name = f"pubsub-deliveries:{topic}"
        try:
            tag = self.decayer.RegisterDecayingTag(name, self.interval, DecayFixed(self.amount),
                                                   BumpSumBounded(0, self.cap))
        except RuntimeError:
            return
        self.decaying[topic] = tag

    def removeDeliveryTag(self, topic):
        tag = self.decaying.get(topic)
        if tag is None:
            return
        tag.Close()
        del self.decaying[topic]

    def bumpDeliveryTag(self, p, topic):
        tag = self.decaying.get(topic)
        if tag is None:
            return f"no decaying tag registered for topic {topic}"
        tag.Bump(p, self.bump)
        return None

    def bumpTagsForMessage(self, p, msg):
        self.bumpDeliveryTag(p, msg.topic)

    def nearFirstPeers(self, msg):
        peers = self.nearFirst.get(msg.mid)
        return [] if peers is None else list(peers)

    # -- RawTracer -------------------------------------------------------------
    def AddPeer(self, p):
        self.tagPeerIfDirect(p)

    def Join(self, topic):
        self.addDeliveryTag(topic)

    def DeliverMessage(self, msg):
        nearFirst = self.nearFirstPeers(msg)
        self.bumpTagsForMessage(msg.ReceivedFrom, msg)
        for p in nearFirst:
            self.bumpTagsForMessage(p, msg)
        self.nearFirst.pop(msg.mid, None)

    def Leave(self, topic):
        self.removeDeliveryTag(topic)

    def Graft(self, p, topic):
        self.tagMeshPeer(p, topic)

    def Prune(self, p, topic):
        self.untagMeshPeer(p, topic)

    def ValidateMessage(self, msg):
        if msg.mid in self.nearFirst:
            return
        self.nearFirst[msg.mid] = {}

    def DuplicateMessage(self, msg):
        peers = self.nearFirst.get(msg.mid)
        if peers is None:
            return
        peers[msg.ReceivedFrom] = True

    def RejectMessage(self, msg, reason):
        if reason in (RejectValidationThrottled, RejectValidationIgnored, RejectValidationFailed):
            self.nearFirst.pop(msg.mid, None)

    def RemovePeer(self, p):
        pass


def port_topic_tag(topic):
    return topicTag(topic)


def getTagValue(mgr, p, tag):
    info = mgr.GetTagInfo(p)
    if info is None:
        return 0
    return info["Tags"].get(tag, 0)


def tagExists(mgr, p, tag):
    info = mgr.GetTagInfo(p)
    return info is not None and tag in info["Tags"]


class NetPort:
    """One tagTracer and connection manager per router of `net`, started from a
    NetState (its joined topics, connections, direct flags and meshes) and fed
    the oracle's event log.  verdict_of: message id -> GSIM_VERDICT_*."""

    def __init__(self, net, st, t0, verdict_of, bump=1, cap=15, amount=1, interval=GossipSubConnTagDecayInterval):
        self.net, self.T, self.t0, self.interval = net, st.T, t0, interval
        self.verdict_of = verdict_of
        self.own = net.owner().astype(np.int64)
        self.rp = net.row_ptr.astype(np.int64)
        self.tt = []
        for i in range(net.n):
            cm = ConnMgr(t0=t0, interval=interval)
            tt = TagTracer(cm, bump, cap, amount, interval)
            lo, hi = self.rp[i], self.rp[i + 1]
            tt.direct = {int(net.col[e]) for e in range(lo, hi) if st.direct[e]}
            for t in range(st.T):
                if (int(net.sub[i]) >> t) & 1:
                    tt.Join(t)
            for e in range(lo, hi):
                if st.estate[e] & _abi.ES_CONNECTED:
                    cm.Connected(int(net.col[e]))
                    tt.AddPeer(int(net.col[e]))
                for t in range(st.T):
                    if st.tflags[t, e] & _abi.TF_MESH:
                        tt.Graft(int(net.col[e]), t)
            self.tt.append(tt)

    def refresh(self, now):
        for tt in self.tt:
            tt.cmgr.advance(now)

    def feed(self, events):
        for ev in events:
            kind, a, b, t = int(ev["kind"]), int(ev["a"]), int(ev["b"]), int(ev["topic"])
            tt = self.tt[a] if a < len(self.tt) else None
            if kind == ob.EV_SEEN:
                msg = Message(int(ev["mid"]), t, a if b == 0xFFFFFFFF else b)
                if int(ev["x"]):
                    tt.ValidateMessage(msg)
                    vd = self.verdict_of[msg.mid]
                    if vd == _abi.VERDICT_ACCEPT:
                        tt.DeliverMessage(msg)
                    else:
                        tt.RejectMessage(msg, VERDICT_REASON[vd])
                else:
                    tt.DuplicateMessage(msg)
            elif kind == ob.EV_VALIDATE:
                tt.ValidateMessage(Message(int(ev["mid"]), t, b))
            elif kind == ob.EV_REJECT_SIG:
                tt.RejectMessage(Message(int(ev["mid"]), t, b), RejectInvalidSignature)
            elif kind == ob.EV_GRAFT:
                tt.Graft(b, t)
            elif kind == ob.EV_PRUNE:
                tt.Prune(b, t)
            elif kind == ob.EV_ADD_PEER:
                tt.cmgr.Connected(b, int(ev["x"]))
                tt.AddPeer(b)
            elif kind == ob.EV_REMOVE_PEER:
                # the router's RemovePeer takes the peer out of every mesh without a PRUNE
                # (gossipsub.go:554-567), so the reference never unprotects it; the engine derives
                # protection from the meshes (a declared difference): so does this adapter
                for topic in range(self.T):
                    tt.cmgr.Unprotect(b, port_topic_tag(topic))
                tt.cmgr.Disconnected(b)
                tt.RemovePeer(b)
            elif kind == ob.EV_JOIN:
                tt.Join(t)
            elif kind == ob.EV_LEAVE:
                tt.Leave(t)

    def tags(self, topic):
        """u8 [E], edge order: the delivery tag of `topic` each router holds for each connection."""
        out = np.zeros(self.net.e, dtype=np.uint8)
        name = f"pubsub-deliveries:{topic}"
        for i, tt in enumerate(self.tt):
            if not tt.cmgr.tags:
                continue
            lo, hi = self.rp[i], self.rp[i + 1]
            row = self.net.col[lo:hi]
            for p, tags in tt.cmgr.tags.items():
                v = tags.get(name, 0)
                if v and p != i:
                    q = int(np.searchsorted(row, p))
                    assert q < hi - lo and row[q] == p, f"router {i} tagged {p}, which is no neighbour"
                    out[lo + q] = v
        return out

    def values(self):
        out = np.zeros(self.net.e, dtype=np.int32)
        for t in range(self.T):
            out += self.tags(t)
        return out

    def trim(self, seed, tick, now, low, high, grace):
        """Sorted unique (a < b) pairs: the union of every router's trim, keys from orc_select_key."""
        pairs = set()
        for i, tt in enumerate(self.tt):
            lo, hi = self.rp[i], self.rp[i + 1]
            if len(tt.cmgr.first_seen) <= (high if high > 0 else low):
                continue
            row = self.net.col[lo:hi]

            def key(p, i=i, row=row):
                return ob.select_key(seed, tick, i, 0, _abi.P_TRIM, p, int(np.searchsorted(row, p)))
            for p in tt.cmgr.trim(now, key, low, high, grace):
                pairs.add((min(i, p), max(i, p)))
        return np.array(sorted(pairs), dtype=np.uint32).reshape(-1, 2)

"""Propagation figures from the array Engine.msg_report returns (rows of
Engine.MSG_REPORT_DTYPE, struct gsim_msg_report): pure numpy, no device.

hist[d] counts the peers a message reached d rounds after its publication,
d < REPORT_BINS - 1; the last bin holds every later one (its exact extent is
max_latency).  Further down: the network report's, the peer delivery
report's, the relay report's, the mesh path report's and the score report's
rows (Engine.net_report, Engine.peer_report, Engine.relay_report,
Engine.mesh_paths, Engine.score_report)."""
import numpy as np

from ._abi import (NET_CLASSES, NET_DEG_BINS, NET_OUT_BINS, NET_SCORE_BINS, RELAY_DELAY_BINS, REPORT_BINS, SR_BINS,
                   SR_CAUSES, SR_PARTS)


def coverage(rep: np.ndarray) -> np.ndarray:
    """reached / subscribers per message (nan where nobody announces the topic)."""
    reached = rep["reached"].astype(np.float64)
    subs = rep["subscribers"].astype(np.float64)
    out = np.full(len(rep), np.nan)
    np.divide(reached, subs, out=out, where=subs > 0)
    return out


def latency_quantile(rep: np.ndarray, q: float):
    """Per message the smallest latency d with at least q of its reached peers
    at latency <= d, read from hist.  Returns (latency, overflow): overflow is
    True where the quantile falls in the last bin, whose latency reads
    REPORT_BINS - 1 (a lower bound); a message that reached nobody reads 0."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    hist = rep["hist"].astype(np.int64).reshape(len(rep), REPORT_BINS)
    cum = np.cumsum(hist, axis=1)
    total = cum[:, -1]
    need = np.maximum(np.ceil(q * total).astype(np.int64), 1)     # peers the quantile must cover
    lat = (cum < need[:, None]).sum(axis=1).astype(np.int64)
    lat[total == 0] = 0
    return lat, (lat == REPORT_BINS - 1) & (total > 0)


def by_topic(rep: np.ndarray) -> dict:
    """Histograms summed per topic: {topic: {"messages", "reached", "hist"}}."""
    out = {}
    for t in np.unique(rep["topic"]):
        rows = rep[rep["topic"] == t]
        out[int(t)] = {"messages": int(len(rows)), "reached": int(rows["reached"].astype(np.int64).sum()),
                       "hist": rows["hist"].astype(np.int64).reshape(len(rows), REPORT_BINS).sum(axis=0)}
    return out


def cdf(rep: np.ndarray) -> np.ndarray:
    """Network-wide cumulative reach by round: cdf[d] = share of all
    (message, subscriber) pairs reached within d rounds of publication, d <
    REPORT_BINS (the last entry includes every later arrival).  nan when no
    message has a subscriber."""
    hist = rep["hist"].astype(np.int64).reshape(len(rep), REPORT_BINS).sum(axis=0)
    denom = int(rep["subscribers"].astype(np.int64).sum())
    if denom == 0:
        return np.full(REPORT_BINS, np.nan)
    return np.cumsum(hist) / float(denom)


# ---- network report (Engine.net_report: struct gsim_mesh_row / gsim_score_row) ----

def threshold_edges(thresholds) -> np.ndarray:
    """The default score histogram edges: the sorted distinct values of the
    graylist, publish, gossip, accept-PX and opportunistic-graft thresholds
    (a gsim.PeerScoreThresholds) and 0."""
    vals = [thresholds.GraylistThreshold, thresholds.PublishThreshold, thresholds.GossipThreshold, 0.0,
            thresholds.AcceptPXThreshold, thresholds.OpportunisticGraftThreshold]
    return np.unique(np.asarray(vals, dtype=np.float64))


def mesh_health(mesh_rows: np.ndarray, gossip_params) -> dict:
    """Per mesh row the share of its members whose mesh is smaller than Dlo
    ("below_dlo"), larger than Dhi ("above_dhi"), or holds fewer than Dout
    outbound links ("below_dout"), from deg_hist / out_hist (a
    gsim.GossipSubParams gives the bounds).  nan where a row has no members.
    Bounds the histograms cannot resolve (Dlo or Dhi + 1 past the last degree
    bin, Dout past the last outbound bin) raise ValueError."""
    dlo, dhi, dout = int(gossip_params.Dlo), int(gossip_params.Dhi), int(gossip_params.Dout)
    if dlo > NET_DEG_BINS - 1 or dhi + 1 > NET_DEG_BINS - 1 or dout > NET_OUT_BINS - 1:
        raise ValueError("mesh bounds lie past the report's last exact bin")
    deg = mesh_rows["deg_hist"].astype(np.int64).reshape(len(mesh_rows), NET_DEG_BINS)
    out = mesh_rows["out_hist"].astype(np.int64).reshape(len(mesh_rows), NET_OUT_BINS)
    members = mesh_rows["members"].astype(np.float64)

    def share(count):
        res = np.full(len(mesh_rows), np.nan)
        np.divide(count.astype(np.float64), members, out=res, where=members > 0)
        return res

    return {"below_dlo": share(deg[:, :dlo].sum(axis=1)), "above_dhi": share(deg[:, dhi + 1:].sum(axis=1)),
            "below_dout": share(out[:, :dout].sum(axis=1))}


def class_share(mesh_rows: np.ndarray) -> np.ndarray:
    """share[a, b]: the fraction of class a's mesh links, over every topic, that
    point into class b ([C, C], C = the classes the rows name; a row of nan
    for a class without mesh links)."""
    C = int(mesh_rows["cls"].max()) + 1 if len(mesh_rows) else 0
    links = np.zeros((C, NET_CLASSES), dtype=np.float64)
    ml = mesh_rows["mesh_links"].astype(np.float64).reshape(len(mesh_rows), NET_CLASSES)
    np.add.at(links, mesh_rows["cls"].astype(np.int64), ml)
    tot = links.sum(axis=1, keepdims=True)
    res = np.full((C, C), np.nan)
    np.divide(links[:, :C], tot, out=res, where=tot > 0)
    return res


# ---- peer delivery report (Engine.peer_report: struct gsim_peer_row / gsim_peer_class_row) ----

def delivery_ratio(peer_rows: np.ndarray) -> np.ndarray:
    """Per row the share of the expected messages that arrived, (expected -
    missed) / expected; nan where nothing was expected.  Works on per-peer rows
    and on class rows alike."""
    exp = peer_rows["expected"].astype(np.float64)
    got = exp - peer_rows["missed"].astype(np.float64)
    out = np.full(len(peer_rows), np.nan)
    np.divide(got, exp, out=out, where=exp > 0)
    return out


def starved(peer_rows: np.ndarray, below: float) -> np.ndarray:
    """Indices of the rows whose delivery_ratio lies under `below` (rows that
    expected nothing are never starved)."""
    ratio = delivery_ratio(peer_rows)
    return np.nonzero(np.less(ratio, below, where=~np.isnan(ratio), out=np.zeros(len(ratio), dtype=bool)))[0]


def source_share(rows: np.ndarray) -> np.ndarray:
    """first_from normalised per row, [len(rows), NET_CLASSES]: the share of a
    peer's (or a class row's) first deliveries that came from each sender
    class, the eclipse measure; a row of nan where nothing was delivered by
    another peer."""
    ff = rows["first_from"].astype(np.float64).reshape(len(rows), NET_CLASSES)
    tot = ff.sum(axis=1, keepdims=True)
    out = np.full((len(rows), NET_CLASSES), np.nan)
    np.divide(ff, tot, out=out, where=tot > 0)
    return out


def class_latency_quantile(class_rows: np.ndarray, q: float):
    """latency_quantile over the class rows' histograms: per (topic, class) the
    smallest latency d with at least q of its received deliveries at latency
    <= d, and the overflow flag (True where the quantile falls in the last bin,
    whose latency reads REPORT_BINS - 1, a lower bound)."""
    return latency_quantile(class_rows, q)


# ---- relay report (Engine.relay_report: struct gsim_relay_row / _class_row / _msg_row) ----

def _bin_quantile(hist: np.ndarray, q: float):
    """latency_quantile's rule on an [n, bins] histogram: (bin, overflow)."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    hist = hist.astype(np.int64)
    cum = np.cumsum(hist, axis=1)
    total = cum[:, -1] if hist.shape[1] else np.zeros(len(hist), dtype=np.int64)
    need = np.maximum(np.ceil(q * total).astype(np.int64), 1)
    k = (cum < need[:, None]).sum(axis=1).astype(np.int64)
    k[total == 0] = 0
    return k, (k == hist.shape[1] - 1) & (total > 0)


def relay_share(class_rows: np.ndarray) -> np.ndarray:
    """share[t, c]: of the first deliveries of topic t's selected messages, the
    fraction given by senders of class c ([topics, classes] as the rows name
    them; a row of nan for a topic without any first delivery)."""
    T = int(class_rows["topic"].max()) + 1 if len(class_rows) else 0
    C = int(class_rows["cls"].max()) + 1 if len(class_rows) else 0
    ch = np.zeros((T, C), dtype=np.float64)
    np.add.at(ch, (class_rows["topic"].astype(np.int64), class_rows["cls"].astype(np.int64)),
              class_rows["children"].astype(np.float64))
    tot = ch.sum(axis=1, keepdims=True)
    out = np.full((T, C), np.nan)
    np.divide(ch, tot, out=out, where=tot > 0)
    return out


def leaf_share(class_rows: np.ndarray) -> np.ndarray:
    """Per class row the share of its holders (q, m) that gave nobody a first
    delivery, fanout[0] / held; nan where the row holds nothing."""
    held = class_rows["held"].astype(np.float64)
    leaves = class_rows["fanout"].astype(np.float64).reshape(len(class_rows), REPORT_BINS)[:, 0]
    out = np.full(len(class_rows), np.nan)
    np.divide(leaves, held, out=out, where=held > 0)
    return out


def fanout_quantile(class_rows: np.ndarray, q: float):
    """Per class row the smallest k with at least q of its holders at a fan-out
    <= k, read from fanout.  Returns (fanout, overflow): overflow is True where
    the quantile falls in the last bin (>= REPORT_BINS - 1 children, a lower
    bound; max_children is exact); a row that holds nothing reads 0."""
    return _bin_quantile(class_rows["fanout"].reshape(len(class_rows), REPORT_BINS), q)


def top_relays(peer_rows: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k rows with the most children, most first, the lower index
    first among equals; rows without children are left out."""
    ch = peer_rows["children"].astype(np.int64)
    order = np.lexsort((np.arange(len(ch)), -ch))
    return order[ch[order] > 0][:max(int(k), 0)]


def depth_quantile(msg_rows: np.ndarray, q: float):
    """Per message the smallest depth d with at least q of its placed holders
    (reached - orphans) at depth <= d, read from depth_hist.  Returns (depth,
    overflow) as latency_quantile does; depth_max is exact."""
    return _bin_quantile(msg_rows["depth_hist"].reshape(len(msg_rows), REPORT_BINS), q)


def pulled_share(msg_rows: np.ndarray) -> np.ndarray:
    """Per message the share of its first deliveries whose hop took more than
    1 + vdelay rounds: those came by IWANT, not by eager push.  nan where a
    message has no timed delivery.  The last delay bin holds every delay >=
    RELAY_DELAY_BINS, so a message with 1 + vdelay >= RELAY_DELAY_BINS cannot be
    answered from the bins: ValueError."""
    push = 1 + msg_rows["vdelay"].astype(np.int64)
    if (push >= RELAY_DELAY_BINS).any():
        raise ValueError("pulled_share: 1 + vdelay reaches the overflow bin (delays >= %d)" % RELAY_DELAY_BINS)
    hist = msg_rows["delay_hist"].astype(np.float64).reshape(len(msg_rows), RELAY_DELAY_BINS)
    delay = np.arange(1, RELAY_DELAY_BINS + 1)[None, :]               # bin k holds delay k + 1
    late = np.where(delay > push[:, None], hist, 0.0).sum(axis=1)
    tot = hist.sum(axis=1)
    out = np.full(len(msg_rows), np.nan)
    np.divide(late, tot, out=out, where=tot > 0)
    return out


# ---- mesh path report (Engine.mesh_paths: struct gsim_mesh_path_row) ----

def hop_quantile(rows: np.ndarray, q: float) -> np.ndarray:
    """Per source the smallest distance d with at least q of its reached peers
    within d hops, read from hist (a source that reaches nobody reads 0).  A
    quantile that falls in the last bin, which holds every distance >=
    REPORT_BINS - 1, cannot be answered from the bins: ValueError (as
    mesh_health refuses bounds past its last exact bin)."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    hops, overflow = latency_quantile(rows, q)
    if overflow.any():
        raise ValueError("hop_quantile: the quantile lies in the overflow bin (distances >= %d)" % (REPORT_BINS - 1))
    return hops


def reach_ratio(rows: np.ndarray) -> np.ndarray:
    """reached / subscribers per source (nan where nobody announces the topic)."""
    return coverage(rows)


def censored_share(rows_plain: np.ndarray, rows_blocked: np.ndarray, blocked=()) -> np.ndarray:
    """Per source the share of the peers outside the classes `blocked` that the
    plain traversal reaches and the one with those classes blocked does not:
    1 - reached_cls(blocked run) / reached_cls(plain run), both summed over the
    other classes.  The two arrays hold the same sources in the same order
    (ValueError otherwise); nan where the plain run reaches no such peer."""
    if len(rows_plain) != len(rows_blocked) or (rows_plain["source"] != rows_blocked["source"]).any() \
            or (rows_plain["topic"] != rows_blocked["topic"]).any():
        raise ValueError("censored_share: the two runs must hold the same sources and topic, in the same order")
    keep = np.ones(NET_CLASSES, dtype=bool)
    for c in ([blocked] if np.isscalar(blocked) else blocked):
        keep[int(c)] = False
    plain = rows_plain["reached_cls"].astype(np.float64).reshape(len(rows_plain), NET_CLASSES)[:, keep].sum(axis=1)
    cut = rows_blocked["reached_cls"].astype(np.float64).reshape(len(rows_blocked), NET_CLASSES)[:, keep].sum(axis=1)
    out = np.full(len(rows_plain), np.nan)
    np.divide(plain - cut, plain, out=out, where=plain > 0)
    return out


def unreachable(reach_count: np.ndarray, n_sources: int) -> np.ndarray:
    """Indices of the peers that fewer than n_sources sources reach (per-peer
    reach_count of Engine.mesh_paths(..., per_peer=True)); peers outside the
    topic are among them, no source reaches those."""
    return np.nonzero(np.asarray(reach_count).astype(np.int64) < int(n_sources))[0]


# ---- score report (Engine.score_report: struct gsim_score_part_row / _cause_row / _topic_row) ----

def part_bin_bounds() -> np.ndarray:
    """[SR_BINS, 2]: (lo, hi) of each bin of a part row's hist.  The negative
    bins 0..15 hold lo < x <= hi (bin 0: -inf .. -2^22, bin 15: -2^-6 .. 0,
    zero excluded), bin 16 holds zero of either sign (lo = hi = 0), the
    positive bins 17..32 hold lo <= x < hi (bin 17: 0 .. 2^-6, zero excluded;
    bin 32: 2^22 .. +inf); in between the edges are the even powers 2^(2m - 8).
    The infinities themselves fall in the end bins."""
    pos = np.empty((16, 2))
    for m in range(16):
        pos[m] = (0.0 if m == 0 else 2.0 ** (2 * m - 8), np.inf if m == 15 else 2.0 ** (2 * m - 6))
    out = np.zeros((SR_BINS, 2))
    out[17:] = pos
    out[:16] = -pos[::-1, ::-1]
    return out


def part_bin(x) -> np.ndarray:
    """The hist bin of each value of x under gsim_score_report's rule (integer
    arithmetic on the f64 bits); -1 for NaN, which a part row counts in `nan`."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = x.view(np.uint64)
    mag = u & np.uint64(0x7FFFFFFFFFFFFFFF)
    k = (mag >> np.uint64(52)).astype(np.int64) - 1023
    m = np.clip((k + 8) >> 1, 0, 15)
    b = np.where((u >> np.uint64(63)) != 0, 15 - m, 17 + m)
    b = np.where(mag == 0, 16, b)
    return np.where(np.isnan(x), -1, b).astype(np.int64)


def _class_count(rows) -> int:
    return int(max(rows["obs_cls"].max(), rows["subj_cls"].max())) + 1 if len(rows) else 0


def cause_below(cause_rows: np.ndarray, edges, threshold: float) -> np.ndarray:
    """[C, C, SR_CAUSES]: per (observer class, subject class) the connected
    records whose total lies under `threshold`, by dominant negative part
    (_abi.SR_CAUSE_NAMES).  `edges` are the edges the report was taken with and
    `threshold` must be one of them (only there does a bin boundary fall on
    it), else ValueError."""
    ed = np.asarray(edges, dtype=np.float64).reshape(-1)
    hit = np.nonzero(ed == float(threshold))[0]
    if len(hit) == 0:
        raise ValueError("cause_below: the threshold is not one of the report's edges")
    C = _class_count(cause_rows)
    out = np.zeros((C, C, SR_CAUSES), dtype=np.int64)
    cause = cause_rows["cause"].astype(np.int64).reshape(len(cause_rows), NET_SCORE_BINS, SR_CAUSES)
    # bins 0 .. k hold the totals under edges[k]
    np.add.at(out, (cause_rows["obs_cls"].astype(np.int64), cause_rows["subj_cls"].astype(np.int64)),
              cause[:, :int(hit[0]) + 1].sum(axis=1))
    return out


def part_share_negative(part_rows: np.ndarray) -> np.ndarray:
    """[C, C, SR_PARTS]: per (observer class, subject class) and part
    (_abi.SR_PART_NAMES) the fraction of the connected records whose value of
    the part is negative (NaN values count as connected, not as negative);
    nan where a pair has no connected record."""
    C = _class_count(part_rows)
    hist = part_rows["hist"].astype(np.float64).reshape(len(part_rows), SR_BINS)
    neg = np.zeros((C, C, SR_PARTS))
    tot = np.zeros((C, C, SR_PARTS))
    idx = (part_rows["obs_cls"].astype(np.int64), part_rows["subj_cls"].astype(np.int64), part_rows["part"].astype(np.int64))
    np.add.at(neg, idx, hist[:, :16].sum(axis=1))
    np.add.at(tot, idx, hist.sum(axis=1) + part_rows["nan"].astype(np.float64))
    out = np.full((C, C, SR_PARTS), np.nan)
    np.divide(neg, tot, out=out, where=tot > 0)
    return out

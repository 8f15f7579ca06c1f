"""Propagation figures from the array Engine.msg_report returns (rows of
Engine.MSG_REPORT_DTYPE, struct gsim_msg_report): pure numpy, no device.

hist[d] counts the peers a message reached d rounds after its publication,
d < REPORT_BINS - 1; the last bin holds every later one (its exact extent is
max_latency).  Further down: the network report's and the peer delivery
report's rows (Engine.net_report, Engine.peer_report)."""
import numpy as np

from ._abi import NET_CLASSES, NET_DEG_BINS, NET_OUT_BINS, REPORT_BINS


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

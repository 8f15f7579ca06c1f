"""Propagation figures from the array Engine.msg_report returns (rows of
Engine.MSG_REPORT_DTYPE, struct gsim_msg_report): pure numpy, no device.

hist[d] counts the peers a message reached d rounds after its publication,
d < REPORT_BINS - 1; the last bin holds every later one (its exact extent is
max_latency)."""
import numpy as np

from ._abi import REPORT_BINS


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

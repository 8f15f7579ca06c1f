"""numpy helpers over the connection tags' read-outs (Engine.conn_values,
Engine.conn_trim; include/gsim.h gsim_conn_*): what a sybil or churn scenario
under connection limits asks of them.  Nothing here touches the device."""
from __future__ import annotations

import numpy as np

from . import _abi


def _owner(net) -> np.ndarray:
    return np.repeat(np.arange(net.n, dtype=np.int64), np.diff(net.row_ptr.astype(np.int64)))


def protected_share(net, flags) -> np.ndarray:
    """Per router, the share of its connected connections that the connection
    manager may not trim (direct or mesh peers); NaN for a router without
    connections.  flags: Engine.conn_values()[1]."""
    flags = np.asarray(flags, dtype=np.uint8)
    own = _owner(net)
    conn = (flags & _abi.CONN_CONNECTED) != 0
    prot = conn & ((flags & _abi.CONN_PROTECTED) != 0)
    nconn = np.bincount(own[conn], minlength=net.n).astype(np.float64)
    nprot = np.bincount(own[prot], minlength=net.n).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(nconn > 0, nprot / nconn, np.nan)


def trimmed_by_class(pairs, cls, n_classes: int = _abi.NET_CLASSES) -> np.ndarray:
    """The closed connections by the classes of their two ends (the classes of
    Engine.set_peer_classes): out[c][d], c <= d, counts the pairs (a, b) with
    {cls[a], cls[b]} = {c, d}.  pairs: Engine.conn_trim()."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    cls = np.asarray(cls, dtype=np.int64)
    ca, cb = cls[pairs[:, 0]], cls[pairs[:, 1]]
    lo, hi = np.minimum(ca, cb), np.maximum(ca, cb)
    out = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(out, (lo, hi), 1)
    return out


def survivors(net, flags_before, pairs) -> np.ndarray:
    """Edge mask [E]: the connections that were connected before the trim and
    were not closed by it.  flags_before: Engine.conn_values()[1] read before
    Engine.conn_trim() returned `pairs`."""
    conn = (np.asarray(flags_before, dtype=np.uint8) & _abi.CONN_CONNECTED) != 0
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return conn
    own, col = _owner(net), net.col.astype(np.int64)
    key = own * net.n + col
    closed = np.concatenate([pairs[:, 0] * net.n + pairs[:, 1], pairs[:, 1] * net.n + pairs[:, 0]])
    return conn & ~np.isin(key, closed)

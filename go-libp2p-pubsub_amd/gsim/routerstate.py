"""Router state: the seen cache's and the gossip tracer's calls as rows for
``Engine.router_state_events`` (struct gsim_router_event, include/gsim.h).

A caller that owns its routers keeps, besides every router's peerScore
(``gsim.tracer``), the two id-keyed structures the router consults around it
on the GPU: the seen cache (timecache/, pubsub.go:986-995, 1150-1162) and the
gossip tracer's promises (gossip_tracer.go:48-200)::

    eng.router_state_config(seen_cap=1 << 20, promises_cap=1 << 16)
    new = eng.router_state_events(routerstate.batch([routerstate.seen_add(o, mid, now)]))
    eng.tracer_events(routerstate.to_score_events([(o, p, t, mid, now, None)], new))

The events of one observer take effect in array order; observers are
independent, so rows of different observers may interleave freely.
"""
from __future__ import annotations

import numpy as np

from . import _abi, tracer
from ._abi import RS_FULFILL, RS_PROMISE, RS_SEEN_ADD, RS_SEEN_HAS  # noqa: F401

# numpy views of struct gsim_router_event (32 bytes) and struct gsim_broken_row (16 bytes)
EVENT_DTYPE = np.dtype(_abi.ROUTER_EVENT_DTYPE)
BROKEN_DTYPE = np.dtype(_abi.BROKEN_ROW_DTYPE)

_PAD = (0,) * 7


def _row(kind, observer, peer, mid, now):
    return (int(mid), int(now), int(observer), int(peer), int(kind), _PAD)


def seen_add(observer, mid, now):
    """markSeen = TimeCache.Add (pubsub.go:1150-1162): answer 1 a new id, 0 already there."""
    return _row(RS_SEEN_ADD, observer, 0, mid, now)


def seen_has(observer, mid, now):
    """seenMessage = TimeCache.Has (pubsub.go:986-995): answer 1 there, 0 not."""
    return _row(RS_SEEN_HAS, observer, 0, mid, now)


def promise(observer, peer, mid, now):
    """AddPromise (gossip_tracer.go:48-77) with the id already picked: `peer`
    promised `mid`; answer 1 a new promise, 0 it existed."""
    return _row(RS_PROMISE, observer, peer, mid, now)


def fulfill(observer, mid, now):
    """fulfillPromise (gossip_tracer.go:119-141): the id arrived; answer = promises dropped (at most 255)."""
    return _row(RS_FULFILL, observer, 0, mid, now)


def batch(rows) -> np.ndarray:
    """The builders' rows as one EVENT_DTYPE array."""
    rows = list(rows)
    return np.array(rows, dtype=EVENT_DTYPE) if rows else np.zeros(0, dtype=EVENT_DTYPE)


# the reasons a validator returns: the message entered validation first
_VALIDATED = (tracer.REJECT_VALIDATION_THROTTLED, tracer.REJECT_VALIDATION_FAILED, tracer.REJECT_VALIDATION_IGNORED)


def to_score_events(arrivals, results) -> np.ndarray:
    """Raw copies plus the seen cache's answers as ``gsim.tracer`` rows.

    arrivals: one (observer, from, topic, mid, now, reason) per copy, reason a
    tracer.REJECT_* or None; results: the answer of that copy's ``seen_add``
    (1 new, 0 seen).  A new id is validated and delivered / rejected
    (ValidateMessage, then DeliverMessage or RejectMessage; a reason that
    precedes validation -- a bad signature, a blacklisted peer or source, a
    full queue, a self-originated message -- is the RejectMessage alone,
    validation.go:274-343); a seen id is a DuplicateMessage."""
    arrivals = list(arrivals)
    results = np.asarray(results)
    if len(arrivals) != len(results):
        raise ValueError(f"{len(arrivals)} arrivals, {len(results)} seen answers")
    rows = []
    for (o, p, t, mid, now, reason), new in zip(arrivals, results.tolist()):
        if not new:
            rows.append(tracer.duplicate(o, p, t, mid, now))
        elif reason is None:
            rows.append(tracer.validate(o, p, t, mid, now))
            rows.append(tracer.deliver(o, p, t, mid, now))
        else:
            if reason in _VALIDATED:
                rows.append(tracer.validate(o, p, t, mid, now))
            rows.append(tracer.reject(o, p, t, mid, reason, now))
    return tracer.batch(rows) if rows else np.zeros(0, dtype=tracer.EVENT_DTYPE)


"""Score tracer events: peerScore's RawTracer calls (trace.go:27-60, score.go:88)
as rows for ``Engine.tracer_events`` (struct gsim_score_event, include/gsim.h).

A caller that owns its routers -- an event-driven simulator, a replay of a
recorded TraceEvent stream -- builds rows with the one-line builders below,
packs them with ``batch`` and hands them to the engine, which keeps every
router's peerStats and delivery records on the GPU::

    eng.tracer_config(records_cap=1 << 20, peers_cap=1 << 20)
    eng.tracer_events(tracer.batch([tracer.validate(o, p, t, mid, now),
                                    tracer.deliver(o, p, t, mid, now)]))

The events of one observer take effect in array order; observers are
independent, so rows of different observers may interleave freely.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from ._abi import (EV_ADD_PENALTY, EV_DELIVER, EV_DUPLICATE, EV_GRAFT, EV_PRUNE, EV_REJECT,  # noqa: F401
                   EV_VALIDATE, REJECT_BLACKLISTED_PEER, REJECT_BLACKLISTED_SOURCE, REJECT_INVALID_SIGNATURE,
                   REJECT_MISSING_SIGNATURE, REJECT_SELF_ORIGIN, REJECT_UNEXPECTED_AUTH_INFO,
                   REJECT_UNEXPECTED_SIGNATURE, REJECT_VALIDATION_FAILED, REJECT_VALIDATION_IGNORED,
                   REJECT_VALIDATION_QUEUE_FULL, REJECT_VALIDATION_THROTTLED)

# numpy view of struct gsim_score_event (32 bytes)
EVENT_DTYPE = np.dtype(_abi.SCORE_EVENT_DTYPE)

_PAD = (0, 0, 0, 0)


def _row(kind, observer, peer, topic, mid, arg, now):
    return (int(mid), int(now), int(observer), int(peer), int(arg), int(topic), int(kind), _PAD)


def validate(observer, peer, topic, mid, now):
    """ValidateMessage (score.go:693-700): the message entered validation at `observer`."""
    return _row(EV_VALIDATE, observer, peer, topic, mid, 0, now)


def deliver(observer, peer, topic, mid, now):
    """DeliverMessage (score.go:702-726): first valid delivery, received from `peer`."""
    return _row(EV_DELIVER, observer, peer, topic, mid, 0, now)


def reject(observer, peer, topic, mid, reason, now):
    """RejectMessage (score.go:728-793) with one of the REJECT_* reasons."""
    return _row(EV_REJECT, observer, peer, topic, mid, reason, now)


def duplicate(observer, peer, topic, mid, now):
    """DuplicateMessage (score.go:795-827): another copy, from `peer`."""
    return _row(EV_DUPLICATE, observer, peer, topic, mid, 0, now)


def graft(observer, peer, topic, now):
    """Graft (score.go:649-667): `peer` joined the observer's mesh of `topic`."""
    return _row(EV_GRAFT, observer, peer, topic, 0, 0, now)


def prune(observer, peer, topic, now):
    """Prune (score.go:669-691): `peer` left the observer's mesh of `topic`."""
    return _row(EV_PRUNE, observer, peer, topic, 0, 0, now)


def add_penalty(observer, peer, count, now):
    """AddPenalty (score.go:391-405): `count` behaviour penalties for `peer`."""
    return _row(EV_ADD_PENALTY, observer, peer, 0, 0, count, now)


def batch(rows) -> np.ndarray:
    """The builders' rows as one EVENT_DTYPE array."""
    return np.array(list(rows), dtype=EVENT_DTYPE)


# gsim_trace_event.reason of a REJECT_MESSAGE (GSIM_VERDICT_*) -> RejectMessage reason
_VERDICT_REASON = {1: REJECT_VALIDATION_FAILED, 2: REJECT_VALIDATION_IGNORED, 3: REJECT_VALIDATION_THROTTLED,
                   4: REJECT_INVALID_SIGNATURE}


def from_trace(events: np.ndarray) -> np.ndarray:
    """The score events of traced routers: ``Engine.trace_read`` records
    (DELIVER_MESSAGE, REJECT_MESSAGE, DUPLICATE_MESSAGE, GRAFT, PRUNE; the
    other types carry nothing for the score tracer) as an EVENT_DTYPE array.
    A traced first reception is validated and delivered / rejected at its
    timestamp (ValidateMessage then DeliverMessage / RejectMessage; a
    bad-signature REJECT never entered validation).  Rows are ordered by
    (timestamp, router); within one of those, trace_read lists REJECT and
    DUPLICATE before DELIVER, while a router sees the first reception before
    its duplicates: every DELIVER / REJECT comes before the DUPLICATEs, and the
    GRAFTs / PRUNEs keep their place after the messages."""
    ev = np.asarray(events)
    ty = ev["type"]
    first = (ty == _abi.TRACE_DELIVER_MESSAGE) | (ty == _abi.TRACE_REJECT_MESSAGE)
    dup = ty == _abi.TRACE_DUPLICATE_MESSAGE
    ctl = (ty == _abi.TRACE_GRAFT) | (ty == _abi.TRACE_PRUNE)
    keep = np.flatnonzero(first | dup | ctl)
    cls = np.where(first[keep], 0, np.where(dup[keep], 1, 2))
    keep = keep[np.lexsort((cls, ev["peer"][keep], ev["timestamp"][keep]))]     # (stable)
    rows = []
    for x in ev[keep]:
        o, p, t, mid, now = int(x["peer"]), int(x["other"]), int(x["topic"]), int(x["msg_id"]), int(x["timestamp"])
        k = int(x["type"])
        if k == _abi.TRACE_DELIVER_MESSAGE:
            rows.append(validate(o, p, t, mid, now))
            rows.append(deliver(o, p, t, mid, now))
        elif k == _abi.TRACE_REJECT_MESSAGE:
            reason = _VERDICT_REASON.get(int(x["reason"]))
            if reason is None:
                raise ValueError(f"REJECT_MESSAGE with the unknown verdict {int(x['reason'])}")
            if reason != REJECT_INVALID_SIGNATURE:
                rows.append(validate(o, p, t, mid, now))
            rows.append(reject(o, p, t, mid, reason, now))
        elif k == _abi.TRACE_DUPLICATE_MESSAGE:
            rows.append(duplicate(o, p, t, mid, now))
        elif k == _abi.TRACE_GRAFT:
            rows.append(graft(o, p, t, now))
        else:
            rows.append(prune(o, p, t, now))
    return batch(rows) if rows else np.zeros(0, dtype=EVENT_DTYPE)

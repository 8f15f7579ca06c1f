"""The oracle pinned at the score-space settings (no GPU).

The oracle is the checker of tests/test_score_space.py, and the reference's
known-answer tests pin it at their own parameters only.  This module restates
peerScore over numpy float64 arrays, from the reference's score.go and in its
operation order (every product and sum rounded on its own, topics ascending as
DESIGN.md §3.2 fixes the map order):

  refresh          refreshScores        score.go:504-565
  ip_colocation    ipColocationFactor   score.go:344-388
  score            score                score.go:265-342
  graft / prune    Graft / Prune        score.go:649-691
  mark_invalid / mark_first / mark_duplicate            score.go:901-981

For every case of test_score_space, at every tick, the port starts from the
oracle's state before its refresh and must give the planes of
orc_refresh_scores bit for bit; then, from the oracle's planes after the
heartbeat's IWANT penalties, the P6 plane of orc_ip_colocation and the scores
of orc_compute_scores bit for bit.  The bookkeeping functions are compared with
the oracle's on the records of each case's start state, under its parameters.
(The replay of the oracle's event log through the mark functions is not here.)
"""
import numpy as np
import pytest

import oracle_binding as ob
import test_score_space as space
from gsim import _abi
from test_heartbeat import tick_time

TRACKED, CONNECTED = _abi.ES_TRACKED, _abi.ES_CONNECTED
IN_MESH, ACTIVE = _abi.TF_IN_MESH, _abi.TF_ACTIVE
ROUTER = _abi.TF_MESH | _abi.TF_FANOUT           # router membership: not score state
PLANES = ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time", "tflags", "bp", "estate", "expire")


def snapshot(st):
    return {f: getattr(st, f).copy() for f in PLANES}


def topic_params(params, names):
    return [params.Topics.get(n) for n in names]                     # None: not scored


def refresh(S, params, names, now):
    """refreshScores on every record at once."""
    tracked = (S["estate"] & TRACKED) != 0
    connected = tracked & ((S["estate"] & CONNECTED) != 0)
    purge = tracked & ~connected & (now > S["expire"])                # now.After(expire)
    for f in ("first", "meshd", "fail", "invalid", "graft_time", "mesh_time"):
        S[f][:, purge] = 0
    S["tflags"][:, purge] &= np.uint8(ROUTER)
    S["bp"][purge] = 0.0
    S["expire"][purge] = 0
    S["estate"][purge] = 0
    dtz = params.DecayToZero
    for t, tp in enumerate(topic_params(params, names)):
        if tp is None:
            continue
        for f, decay in (("first", tp.FirstMessageDeliveriesDecay), ("meshd", tp.MeshMessageDeliveriesDecay),
                         ("fail", tp.MeshFailurePenaltyDecay), ("invalid", tp.InvalidMessageDeliveriesDecay)):
            x = S[f][t] * decay
            x[x < dtz] = 0.0
            S[f][t] = np.where(connected, x, S[f][t])
        mesh = connected & ((S["tflags"][t] & IN_MESH) != 0)
        mt = now - S["graft_time"][t]
        # (a record outside the mesh: meshTime is never read there and the oracle keeps it 0)
        S["mesh_time"][t] = np.where(mesh, mt, np.where(connected, 0, S["mesh_time"][t]))
        S["tflags"][t] |= np.where(mesh & (mt > tp.MeshMessageDeliveriesActivation), ACTIVE, 0).astype(np.uint8)
    b = S["bp"] * params.BehaviourPenaltyDecay
    b[b < dtz] = 0.0
    S["bp"] = np.where(connected, b, S["bp"])
    return S


def ip_colocation(net, estate, params, white):
    """ipColocationFactor of every record: per IP of the peer, the number of
    the observer's tracked peers holding it."""
    own = net.owner()
    tracked = (estate & TRACKED) != 0
    n_ip = np.diff(net.ip_ptr.astype(np.int64))
    e_idx = np.repeat(np.arange(net.e), n_ip[net.col])                # one entry per (record, IP of its peer)
    start = np.repeat(net.ip_ptr[net.col].astype(np.int64), n_ip[net.col])
    within = np.arange(len(e_idx)) - np.repeat(np.cumsum(n_ip[net.col]) - n_ip[net.col], n_ip[net.col])
    ip = net.ip_ids[start + within].astype(np.int64)
    live = tracked[e_idx]
    key = own[e_idx].astype(np.int64) * int(net.n_ips) + ip
    uniq, inv, cnt = np.unique(key[live], return_inverse=True, return_counts=True)
    peers_in_ip = np.zeros(len(e_idx), dtype=np.int64)
    peers_in_ip[live] = cnt[inv]
    thr = int(params.IPColocationFactorThreshold)
    counted = live & (peers_in_ip > thr)
    if white is not None:
        counted &= white[ip] == 0
    surplus = (peers_in_ip - thr).astype(np.float64)
    out = np.zeros(net.e)
    for q in np.nonzero(counted)[0]:                                  # in the peer's IP order
        out[e_idx[q]] += surplus[q] * surplus[q]
    return out


def score(S, p6, p5, net, params, names):
    """score(p) of every record."""
    total = np.zeros(net.e)
    for t, tp in enumerate(topic_params(params, names)):
        if tp is None:
            continue
        ts = np.zeros(net.e)
        mesh = (S["tflags"][t] & IN_MESH) != 0
        if tp.TimeInMeshQuantum != 0:
            mt = S["mesh_time"][t]
            quot = np.sign(mt) * (np.abs(mt) // tp.TimeInMeshQuantum)  # Go's integer division truncates
            p1 = np.minimum(quot.astype(np.float64), tp.TimeInMeshCap)
        else:
            p1 = np.zeros(net.e)
        ts = np.where(mesh, ts + p1 * tp.TimeInMeshWeight, ts)
        ts = ts + S["first"][t] * tp.FirstMessageDeliveriesWeight
        deficit = tp.MeshMessageDeliveriesThreshold - S["meshd"][t]
        p3 = ((S["tflags"][t] & ACTIVE) != 0) & (S["meshd"][t] < tp.MeshMessageDeliveriesThreshold)
        ts = np.where(p3, ts + (deficit * deficit) * tp.MeshMessageDeliveriesWeight, ts)
        ts = ts + S["fail"][t] * tp.MeshFailurePenaltyWeight
        ts = ts + (S["invalid"][t] * S["invalid"][t]) * tp.InvalidMessageDeliveriesWeight
        total = total + ts * tp.TopicWeight
    if params.TopicScoreCap > 0:
        total = np.where(total > params.TopicScoreCap, params.TopicScoreCap, total)
    total = total + p5[net.col] * params.AppSpecificWeight
    total = total + p6 * params.IPColocationFactorWeight
    excess = S["bp"] - params.BehaviourPenaltyThreshold
    total = np.where(S["bp"] > params.BehaviourPenaltyThreshold, total + (excess * excess) * params.BehaviourPenaltyWeight,
                     total)
    return np.where((S["estate"] & TRACKED) != 0, total, 0.0)


# ---- the bookkeeping, one record at a time ---------------------------------------

def graft(S, tp, t, e, now):
    if not (S["estate"][e] & TRACKED) or tp is None:
        return
    S["tflags"][t, e] = (int(S["tflags"][t, e]) | IN_MESH) & ~ACTIVE & 0xFF
    S["graft_time"][t, e] = now
    S["mesh_time"][t, e] = 0


def prune(S, tp, t, e):
    if not (S["estate"][e] & TRACKED) or tp is None:
        return
    if (S["tflags"][t, e] & ACTIVE) and S["meshd"][t, e] < tp.MeshMessageDeliveriesThreshold:
        deficit = tp.MeshMessageDeliveriesThreshold - S["meshd"][t, e]
        S["fail"][t, e] += deficit * deficit
    if S["tflags"][t, e] & IN_MESH:
        S["mesh_time"][t, e] = 0                                     # (normalised outside the mesh)
    S["tflags"][t, e] = int(S["tflags"][t, e]) & ~IN_MESH & 0xFF


def mark_invalid(S, tp, t, e):
    if (S["estate"][e] & TRACKED) and tp is not None:
        S["invalid"][t, e] += 1


def mark_first(S, tp, t, e):
    if not (S["estate"][e] & TRACKED) or tp is None:
        return
    S["first"][t, e] = min(S["first"][t, e] + 1, tp.FirstMessageDeliveriesCap)
    if S["tflags"][t, e] & IN_MESH:
        S["meshd"][t, e] = min(S["meshd"][t, e] + 1, tp.MeshMessageDeliveriesCap)


def mark_duplicate(S, tp, t, e, validated, now):
    """validated: the time the message was validated, None while it is not."""
    if not (S["estate"][e] & TRACKED) or tp is None or not (S["tflags"][t, e] & IN_MESH):
        return
    if validated is not None and now - validated > tp.MeshMessageDeliveriesWindow:
        return
    S["meshd"][t, e] = min(S["meshd"][t, e] + 1, tp.MeshMessageDeliveriesCap)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.itemsize == 8:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return np.array_equal(a, b)


def first_diff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    av, bv = (a.view(np.uint64), b.view(np.uint64)) if a.dtype.itemsize == 8 else (a, b)
    idx = tuple(np.argwhere(av != bv)[0])
    return f"{int((av != bv).sum())} differ, first at {idx}: oracle {a[idx]!r}, port {b[idx]!r}"


@pytest.mark.parametrize("rid", space.RUNS)
def test_oracle_matches_the_port_every_tick(rid):
    case = space.BY_ID[rid]
    box = {}

    def before_refresh(kk, now, st):
        box["S"] = refresh(snapshot(st), st.params, space.NAMES, now)

    def after_refresh(kk, now, st):
        for f in PLANES:
            assert same(getattr(st, f), box["S"][f]), f"{rid} tick {kk}: refresh, {f}: {first_diff(getattr(st, f), box['S'][f])}"

    def after_scores(kk, now, st):
        S = snapshot(st)                                             # (with the tick's IWANT penalties in bp)
        p6 = ip_colocation(st.net, S["estate"], st.params, st.ip_white)
        assert same(st.p6, p6), f"{rid} tick {kk}: P6: {first_diff(st.p6, p6)}"
        sc = score(S, p6, st.p5, st.net, st.params, space.NAMES)
        assert same(st.score, sc), f"{rid} tick {kk}: score: {first_diff(st.score, sc)}"
        box["ticks"] = box.get("ticks", 0) + 1

    space.oracle_run(case, before_refresh=before_refresh, after_refresh=after_refresh, after_scores=after_scores)
    assert box["ticks"] == len(case.ticks)


@pytest.mark.parametrize("rid", [r for r in space.RUNS if r.endswith("/regular")])
def test_oracle_bookkeeping_matches_the_port(rid):
    """Graft, Prune and the three mark functions on 400 records of the case's
    start state (after one refresh: activations set), each record through a
    random sequence of six calls, under the case's parameters."""
    case = space.BY_ID[rid]
    c = space.setup(case)
    st, params = c["st"], c["params"]
    lib = ob.load()
    lib.orc_refresh_scores(st.view(), tick_time(1))
    S = snapshot(st)
    tps = topic_params(params, space.NAMES)
    rng = np.random.default_rng(5)
    now = tick_time(1)
    for e in rng.choice(st.net.e, size=400, replace=False):
        e = int(e)
        for _ in range(6):
            t = int(rng.integers(0, space.T))
            op = int(rng.integers(0, 6))
            now += int(rng.integers(0, 3)) * space.ONE_ROUND
            if op == 0:
                lib.orc_graft(st.view(), e, t, now)
                graft(S, tps[t], t, e, now)
            elif op == 1:
                lib.orc_prune(st.view(), e, t)
                prune(S, tps[t], t, e)
            elif op == 2:
                lib.orc_mark_invalid(st.view(), e, t)
                mark_invalid(S, tps[t], t, e)
            elif op == 3:
                lib.orc_mark_first(st.view(), e, t)
                mark_first(S, tps[t], t, e)
            else:
                # validated a whole number of rounds ago (0-3), or not yet: the window's edge among them
                ago = int(rng.integers(0, 4)) * space.ONE_ROUND
                has = op == 4
                lib.orc_mark_duplicate(st.view(), e, t, 1 if has else 0, now - ago if has else 0, now)
                mark_duplicate(S, tps[t], t, e, now - ago if has else None, now)
    for f in PLANES:
        assert same(getattr(st, f), S[f]), f"{rid}: {f}: {first_diff(getattr(st, f), S[f])}"

"""The numpy truth of the fixed-point personalized-PageRank push (include/eps_abi.h, csrc/ppr_push.hip), and the exact PPR
vectors it is bounded against.

Mass is in units of 2^-48.  Per source s: r[s] = ONE; a source without entries keeps everything (p[s] = ONE, no rounds).  A round
reads the frontier F = { u : d(u) > 0 and r[u] >= T d(u) } off the state at its start (exact integers: T d(u) is formed in
Python ints wherever it could pass 2^63), every u of F keeps (r[u] * a16) >> 16 in p[u], hands floor(spread / d(u)) to each
entry of its row and keeps the remainder; the shares are added after every frontier node has been reset.  Everything is integer
arithmetic on arrays (np.add.at): r <= 2^48 and a16 <= 2^15, so r * a16 fits 64 unsigned bits and everything else int64."""
import os

import numpy as np

ONE = 1 << 48
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYMMETRIC_GOLDEN = ("clique20", "path30", "star50", "isolated_deg1", "er500", "collab_like", "rmat10")


def golden_graph(name):
    """(rowptr int64, col int32, val float32) of tests/golden/pairs_<name>.npz."""
    d = np.load(os.path.join(GOLDEN, f"pairs_{name}.npz"))
    return d["rowptr"].astype(np.int64), d["col"].astype(np.int32), d["val"]


def parameters(alpha, eps):
    """(a16, thr) as heuristics.ppr_parameters forms them, without the package."""
    return int(round(float(alpha) * 65536)), int(np.ceil(float(eps) * 2.0 ** 48))


def thresholds(deg, thr):
    """int64[n]: T d(u) saturated at ONE + 1 (r never exceeds ONE), ONE + 1 for a node without entries; exact integers."""
    return np.array([min(int(thr) * int(d), ONE + 1) if d > 0 else ONE + 1 for d in deg], dtype=np.int64)


def push(rowptr, col, s, a16, thr, max_rounds, bars=None):
    """-> (p int64[n], r int64[n], rounds, pushes, steps, capped) of source s."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    bars = thresholds(deg, thr) if bars is None else bars
    p, r = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if deg[s] == 0:
        p[s] = ONE
        return p, r, 0, 0, 0, 0
    r[s] = ONE
    rounds = pushes = steps = 0
    capped = 0
    while True:
        F = np.flatnonzero(r >= bars)
        if rounds >= max_rounds:
            capped = int(len(F) > 0)
            break
        if len(F) == 0:
            break
        rounds += 1
        R = r[F]
        d = deg[F]
        keep = ((R.astype(np.uint64) * np.uint64(a16)) >> np.uint64(16)).astype(np.int64)    # (2^48 * 2^15 = 2^63: unsigned)
        spread = R - keep
        share = spread // d
        p[F] += keep
        r[F] = spread - share * d
        # every entry of every frontier row receives its row's share
        starts = np.repeat(rowptr[F] - np.r_[0, np.cumsum(d)[:-1]], d)
        targets = col[starts + np.arange(int(d.sum()))]
        np.add.at(r, targets, np.repeat(share, d))
        pushes += len(F)
        steps += int(d.sum())
    assert int(p.sum()) + int(r.sum()) == ONE, "mass is not conserved"
    return p, r, rounds, pushes, steps, capped


def push_queries(rowptr, col, sources, qptr, qnode, a16, thr, max_rounds):
    """What eps_ppr_push returns: (mass int64[Q], rounds int32[S], pushes int64[S], steps int64[S], capped int32[S]); equal
    sources are pushed once."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    bars = thresholds(deg, thr)
    sources, qptr, qnode = np.asarray(sources), np.asarray(qptr), np.asarray(qnode)
    mass = np.zeros(len(qnode), dtype=np.int64)
    rounds = np.zeros(len(sources), dtype=np.int32)
    pushes, steps = np.zeros(len(sources), dtype=np.int64), np.zeros(len(sources), dtype=np.int64)
    capped = np.zeros(len(sources), dtype=np.int32)
    memo = {}
    for i, s in enumerate(sources.tolist()):
        if s not in memo:
            memo[s] = push(rowptr, col, s, a16, thr, max_rounds, bars)
        p, _, rounds[i], pushes[i], steps[i], capped[i] = memo[s]
        mass[qptr[i]:qptr[i + 1]] = p[qnode[qptr[i]:qptr[i + 1]]]
    return mass, rounds, pushes, steps, capped


def all_sources(rowptr, col, a16, thr, max_rounds):
    """(P int64[n, n] with row s = p of source s, rounds, pushes, steps, capped): every node a source."""
    n = len(rowptr) - 1
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    bars = thresholds(deg, thr)
    out = [push(rowptr, col, s, a16, thr, max_rounds, bars) for s in range(n)]
    return (np.stack([o[0] for o in out]), np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int64),
            np.array([o[4] for o in out], np.int64), np.array([o[5] for o in out], np.int32))


def exact_ppr(rowptr, col, alpha):
    """float64[n, n]: row s = pi_s, the stationary vector of "teleport to s with probability alpha, else step to a uniform entry
    of the current row": pi_s = alpha e_s (I - (1 - alpha) P)^-1 with P = D^-1 A on the pattern, by one dense solve.  A node
    without entries keeps its mass (the push's convention for an isolated source): its row of P is e_u."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    P = np.zeros((n, n))
    rows = np.repeat(np.arange(n), deg)
    np.add.at(P, (rows, np.asarray(col, dtype=np.int64)), 1.0 / deg[rows])
    for u in np.flatnonzero(deg == 0):
        P[u, u] = 1.0
    return alpha * np.linalg.inv(np.eye(n) - (1.0 - alpha) * P)


def pair_score(m_uv, m_vu):
    """The pair entry's formula: float32(float64(M[u->v] + M[v->u]) * 2^-48)."""
    return ((np.asarray(m_uv, np.int64) + np.asarray(m_vu, np.int64)).astype(np.float64) * 2.0 ** -48).astype(np.float32)


def column_score(m_vu, du, dv):
    """The column entry's formula, in its order: float32(float64(M[v->u]) * float64(d(u) + d(v)) / float64(d(u)) * 2^-48)."""
    du, dv = np.asarray(du, np.float64), np.asarray(dv, np.float64)
    return (np.asarray(m_vu, np.int64).astype(np.float64) * (du + dv) / du * 2.0 ** -48).astype(np.float32)

"""The truth of the degree-normalised local indices (helper of the local-index tests, no test itself).

c = the number of common STORED neighbours of rows u and v of the SciPy matrix (its pattern: stored values are ignored),
a, b = the numbers of stored entries of the two rows (indptr differences):

    salton c/sqrt(ab)   jaccard c/(a+b-c)   sorensen 2c/(a+b)   hpi c/min(a,b)   hdi c/max(a,b)   lhn c/(ab)   pa ab

with a zero denominator scoring 0 -- float64 numpy on the integers, then one rounding to float32.

The bar of the tests is ONE float32 ulp, derived: the kernel forms the same float64 expression and rounds it once; sqrt and the
division are correctly rounded on both sides as IEEE 754 asks, so the float64 values agree except where an implementation's last
float64 bit differs, and such a pair of neighbouring float64 values rounds to the same float32 or to two adjacent ones.  In
practice the comparison sees equality."""
import numpy as np
import scipy.sparse as ssp

INDICES = ("salton", "jaccard", "sorensen", "hpi", "hdi", "lhn", "pa")


def pattern(A):
    """The stored pattern of A as an int64 CSR matrix of ones (explicit zeros stay stored), indices sorted."""
    A = ssp.csr_matrix(A)
    P = ssp.csr_matrix((np.ones(A.indices.size, np.int64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    P.sort_indices()
    return P


def degrees(A):
    return np.diff(ssp.csr_matrix(A).indptr).astype(np.int64)


def common_counts(A, u, v, chunk=1 << 18):
    """c of the pairs (u[i], v[i]) from the SciPy pattern product, row by row of P[u] * P[v]."""
    P = pattern(A)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    out = np.zeros(len(u), np.int64)
    for s in range(0, len(u), chunk):
        out[s:s + chunk] = np.asarray(P[u[s:s + chunk]].multiply(P[v[s:s + chunk]]).sum(axis=1)).ravel()
    return out


def index_scores(index, c, a, b):
    """float32 scores of (c, a, b) integer arrays."""
    c, a, b = (np.asarray(x, np.int64).astype(np.float64) for x in (c, a, b))
    num = c
    if index == "salton":
        den = np.sqrt(a * b)
    elif index == "jaccard":
        den = a + b - c
    elif index == "sorensen":
        num, den = 2.0 * c, a + b
    elif index == "hpi":
        den = np.minimum(a, b)
    elif index == "hdi":
        den = np.maximum(a, b)
    elif index == "lhn":
        den = a * b
    elif index == "pa":
        return (a * b).astype(np.float32)
    else:
        raise KeyError(index)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
    return s.astype(np.float32)


def truth(A, u, v, index, c=None):
    """float32 truth of the pairs; ``c`` may be passed when it is at hand (one product for the seven indices)."""
    deg = degrees(A)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    c = common_counts(A, u, v) if c is None else c
    return index_scores(index, c, deg[u], deg[v])


def two_hop_candidates(A):
    """(u, v, c) of every 2-hop non-edge of a SYMMETRIC pattern -- (P P^T)[u, v] != 0, u != v, A[u, v] not stored -- column-major
    (v ascending, then u ascending), with c = (P P^T)[u, v]."""
    P = pattern(A)
    n = P.shape[0]
    C = (P @ P.T).tocoo()
    u, v, c = C.row.astype(np.int64), C.col.astype(np.int64), C.data.astype(np.int64)
    Pc = P.tocoo()
    stored = np.isin(u * n + v, Pc.row.astype(np.int64) * n + Pc.col)
    keep = (c != 0) & (u != v) & ~stored
    u, v, c = u[keep], v[keep], c[keep]
    order = np.lexsort((u, v))
    return u[order], v[order], c[order]


def assert_within_one_ulp(got, want, what=""):
    """|got - want| <= one float32 ulp of want, elementwise (both float32); NaN nowhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    assert not np.isnan(got).any(), f"{what}: NaN scores"
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
    assert not bad.any(), f"{what}: {int(bad.sum())} scores off by more than one float32 ulp, e.g. {got[bad][:3]} vs {want[bad][:3]}"

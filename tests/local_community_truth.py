"""The truth of the local-community indices (Cannistraci, Alanis-Lobato, Ravasi, Sci. Rep. 3:1613) -- helper of the
local-community tests, no test itself.  SciPy / numpy float64 only.

For a pair (u, v) of the SciPy matrix A (its PATTERN: stored values are ignored): L = the ascending common stored neighbours of
rows u and v (``cn_list_truth.cn_lists``), c = |L|, a, b, d_w the stored entries of rows u, v, w,

    gamma(w) = |{z in L : z != w, z stored in row w}|,   G = sum of gamma over L,   CAR = c G / 2
    car CAR   cpa e_u e_v + e_u CAR + e_v CAR + CAR^2 (e = a - c, b - c)   caa sum gamma/log2 d_w   cra sum gamma/d_w
    cjc CAR / (a + b - c), 0 over 0

a term with gamma == 0 skipped.  gamma comes from ONE sparse product: with C the [lists x nodes] incidence of the lists and P0 the
pattern without its diagonal, gamma = ((C P0^T) o C) read at C's entries (P0^T = P0 on a symmetric pattern; "z stored in row w"
is P0[w, z], so the transpose is what holds on any pattern).  ``gammas`` takes ANY ascending segments, not only common-neighbour
lists.  ``gammas_by_pair`` / ``scores_by_pair`` restate both with np.intersect1d and Python sums, one list at a time.

The bar of the score tests is ONE float32 ulp (``local_index_truth.assert_within_one_ulp``): kernel and truth form the same
float64 expression; their sums associate differently, which moves a float64 sum of n positive terms by at most n 2^-53 relative
-- 4e-12 at the longest list of the tests, 40,000 entries, against the 6e-8 of a float32 ulp -- so the two float64 values round to
the same float32 or to neighbours."""
import numpy as np
import scipy.sparse as ssp

import cn_list_truth as ct
import local_index_truth as lit

INDICES = ("car", "cpa", "caa", "cra", "cjc")


def pattern_without_diagonal(A):
    P = lit.pattern(A).tocoo()
    keep = P.row != P.col
    return ssp.csr_matrix((np.ones(int(keep.sum()), np.int64), (P.row[keep], P.col[keep])), shape=P.shape)


def gammas(A, ptr, w, chunk=1 << 15):
    """int64[M]: for entry i of the segments (ptr, w), the stored entries of row w[i] among the OTHER members of its segment."""
    ptr, w = np.asarray(ptr, np.int64), np.asarray(w, np.int64)
    n = ssp.csr_matrix(A).shape[0]
    P0t = pattern_without_diagonal(A).T.tocsr()
    out = np.zeros(len(w), np.int64)
    for s in range(0, len(ptr) - 1, chunk):
        e = min(len(ptr) - 1, s + chunk)
        lo, hi = ptr[s], ptr[e]
        if hi == lo:
            continue
        C = ssp.csr_matrix((np.ones(hi - lo, np.int64), w[lo:hi], ptr[s:e + 1] - lo), shape=(e - s, n))
        R = (C @ P0t).multiply(C).tocoo()                       # the non-zero gammas, at (list, w)
        b_of = np.repeat(np.arange(e - s, dtype=np.int64), np.diff(ptr[s:e + 1]))
        keys = b_of * n + w[lo:hi]                              # ascending: lists in order, w ascending inside a list
        at = np.searchsorted(keys, R.row.astype(np.int64) * n + R.col)
        out[lo + at] = R.data
    return out


def gammas_by_pair(A, ptr, w):
    """The same, one segment at a time with np.intersect1d."""
    A = ssp.csr_matrix(A)
    A.sort_indices()
    ip, ix = A.indptr, A.indices
    out = np.zeros(len(w), np.int64)
    for b in range(len(ptr) - 1):
        L = np.asarray(w[ptr[b]:ptr[b + 1]], np.int64)
        for k, x in enumerate(L):
            row = ix[ip[x]:ip[x + 1]]
            out[ptr[b] + k] = len(np.intersect1d(row, L, assume_unique=True)) - int(x in row)
    return out


def scores(A, u, v, ptr, w, gamma, index):
    """float32 scores of the pairs from their lists and gammas."""
    deg = lit.degrees(A).astype(np.float64)
    u, v, ptr, w = (np.asarray(x, np.int64) for x in (u, v, ptr, w))
    g = np.asarray(gamma, np.int64).astype(np.float64)
    nb = len(ptr) - 1
    b_of = np.repeat(np.arange(nb, dtype=np.int64), np.diff(ptr))
    c = np.diff(ptr).astype(np.float64)
    a, b = deg[u], deg[v]
    G = np.bincount(b_of, weights=g, minlength=nb)              # integers below 2^53: exact
    car = c * (G / 2.0)
    if index == "car":
        s = car
    elif index == "cpa":
        eu, ev = a - c, b - c
        s = eu * ev + eu * car + ev * car + car * car
    elif index in ("caa", "cra"):
        d = deg[w]
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.log2(d) if index == "caa" else d
            term = np.where(g == 0.0, 0.0, g / np.where(g == 0.0, 1.0, den))
        s = np.bincount(b_of, weights=term, minlength=nb)
    elif index == "cjc":
        den = a + b - c
        s = np.where(den == 0.0, 0.0, car / np.where(den == 0.0, 1.0, den))
    else:
        raise KeyError(index)
    return s.astype(np.float32)


def scores_by_pair(A, u, v, index):
    """The same from nothing but the matrix, one pair at a time, Python floats."""
    A = ssp.csr_matrix(A)
    A.sort_indices()
    ip, ix = A.indptr, A.indices
    out = np.zeros(len(u), np.float64)
    for p, (x, y) in enumerate(zip(u, v)):
        rx, ry = ix[ip[x]:ip[x + 1]], ix[ip[y]:ip[y + 1]]
        L = np.intersect1d(rx, ry, assume_unique=True)
        c, a, b = len(L), len(rx), len(ry)
        gam = [len(np.intersect1d(ix[ip[z]:ip[z + 1]], L, assume_unique=True)) - int(z in ix[ip[z]:ip[z + 1]]) for z in L]
        car = c * sum(gam) / 2.0
        if index == "car":
            out[p] = car
        elif index == "cpa":
            out[p] = (a - c) * (b - c) + (a - c) * car + (b - c) * car + car * car
        elif index == "caa":
            out[p] = sum(gm / np.log2(float(ip[z + 1] - ip[z])) for gm, z in zip(gam, L) if gm)
        elif index == "cra":
            out[p] = sum(gm / float(ip[z + 1] - ip[z]) for gm, z in zip(gam, L) if gm)
        else:
            out[p] = car / (a + b - c) if a + b - c else 0.0
    return out.astype(np.float32)


def pair_truth(A, u, v):
    """-> (ptr, w, gamma) of the pairs: the lists of ``cn_list_truth.cn_lists`` and their gammas."""
    ptr, w = ct.cn_lists(A, u, v)
    return ptr, w, gammas(A, ptr, w)


def clique(n):
    """K_n as a SciPy CSR pattern."""
    return ssp.csr_matrix(np.ones((n, n)) - np.eye(n))

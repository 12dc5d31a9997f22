"""CPU: the truth of tests/pair_score_truth.py against a triple loop over explicit sets, its dyadic licence, the three host-only
limit queries, and -- at the limits the library reports -- that every builder really contains every class of case the GPU test
(tests/test_gpu_pair_paths.py) is there for.  A builder that stops reaching a boundary fails here, before any GPU is involved."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as ssp

import pair_score_truth as pt
from conftest import ROOT


@pytest.fixture(scope="module")
def lim(eps):
    from eps_amd import ops
    S, C, Q, R, T, STRIDE = ops.pair_scores_limits()
    K, GQ, B, RING = ops.pair_scores_grouped_limits()
    return dict(S=S, C=C, Q=Q, R=R, T=T, STRIDE=STRIDE, K=K, GQ=GQ, B=B, RING=RING)


@pytest.fixture(scope="module")
def generic(lim):
    return pt.generic_graph(lim["S"], lim["C"], lim["Q"], lim["R"])


@pytest.fixture(scope="module")
def grouped(lim):
    return pt.grouped_graph(lim["GQ"])


# ---------------------------------------------------------------------------------------------------------- the truth itself
def test_scores_equal_a_triple_loop_over_sets():
    rng = np.random.default_rng(1)
    n = 50
    D = (rng.random((n, n)) < 0.25) * rng.choice([0.5, 1.0, 1.5, -2.0], (n, n))
    D[::9] = 0                                                                     # empty rows
    A = ssp.csr_matrix(D.astype(np.float32))
    A.sort_indices()
    w = rng.standard_normal(n)
    u, v = np.concatenate([rng.integers(0, n, 300), np.arange(n)]), np.concatenate([rng.integers(0, n, 300), np.arange(n)])
    t = pt.scores(A, w, u, v)
    nbr = [set(np.flatnonzero(D[i]).tolist()) for i in range(n)]
    for i, (a, b) in enumerate(zip(u, v)):
        count, cn, ws, ab = 0, 0.0, 0.0, 0.0
        for x in nbr[a]:
            for y in nbr[b]:
                if x == y:
                    count += 1
                    cn += D[a, x] * D[b, x]
                    ws += D[a, x] * D[b, x] * w[x]
                    ab += abs(D[a, x] * D[b, x] * w[x])
        assert t["count"][i] == count
        assert abs(t["cn"][i] - cn) <= 1e-12 and abs(t["ws"][i] - ws) <= 1e-12 and abs(t["abs"][i] - ab) <= 1e-12
    assert t["count"].dtype.kind == "i" and t["ws"].dtype == np.float64 and (t["count"][300:] == [len(s) for s in nbr]).all()
    assert (t["abs"] >= np.abs(t["ws"])).all() and (t["count"][300:][::9] == 0).all()       # (the empty rows against themselves)
    ones = pt.scores(pt.unit(A), np.ones(n), u, v)
    assert np.array_equal(ones["cn"], ones["count"]) and np.array_equal(ones["ws"], ones["count"])


def test_the_dyadic_licence_refuses_what_would_round():
    A, info = pt.generic_graph(128, 1024, 256, 32)
    u, v = pt.grid_pairs(info)
    w = pt.dyadic_weights(A.shape[0])
    assert pt.require_exact(A, w, u, v) == 2 * 1 + 5 and pt.require_exact(pt.unit(A), w, u, v) == 5
    with pytest.raises(AssertionError, match="not dyadic"):
        pt.require_exact(A, pt.real_weights(A, "aa", np.float32), u, v)           # 1 / log: no multiple of a power of two
    third = w.copy()
    third[7] = 1.0 / 3.0
    with pytest.raises(AssertionError, match="not dyadic"):
        pt.require_exact(A, third, u, v)
    with pytest.raises(AssertionError, match="could round"):                      # dyadic, but the hub's sums pass 2^(24 - q)
        pt.require_exact(A, w * 64.0 + 2.0 ** -10, u, v)
    with pytest.raises(AssertionError, match="could round"):                      # 12 fraction bits: the hub's own sum leaves 2^10
        pt.require_exact(A, w + 2.0 ** -12, u, v)
    assert pt.frac_bits([0.5, 1.5, 3.0]) == 1 and pt.frac_bits([2.0, 7.0]) == 0


def test_limit_queries(eps):
    from eps_amd import ops
    lib, sig, pi32 = eps.load(), eps._lib.SIGNATURES, ctypes.POINTER(ctypes.c_int32)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eps_abi.h")).read(), flags=re.S)
    for name, k in (("eps_pair_scores_limits", 6), ("eps_pair_scores_grouped_limits", 4), ("eps_rescore_limits", 3)):
        assert re.search(r"\bint %s\s*\(" % name, text) and sig[name] == (ctypes.c_int, [pi32] * k) and hasattr(lib, name)
        assert getattr(lib, name)(*[None] * k) == 0                                # (a NULL pointer skips that value)
    assert lib.eps_version() == eps._lib.ABI_VERSION == 7
    src = {f: open(os.path.join(ROOT, "edge-proposal-sets_amd", "csrc", f)).read() for f in ("pair_intersect.hip", "row_intersect.h", "pair_grouped.hip", "rescore.hip")}

    def define(f, name):
        return int(eval(re.search(r"^#define %s\s+(\(?[0-9 <]+\)?)" % name, src[f], flags=re.M).group(1)))          # noqa: S307
    assert ops.pair_scores_limits() == (define("pair_intersect.hip", "PI_SMALL"), define("row_intersect.h", "ROW_CAP"),
                                        define("pair_intersect.hip", "PI_QCAP"), define("row_intersect.h", "ROW_INPLACE_RATIO"),
                                        define("pair_intersect.hip", "PI_TICKET"), define("pair_intersect.hip", "PI_CLS_STRIDE"))
    assert ops.pair_scores_grouped_limits() == (define("pair_grouped.hip", "PG_CHUNK"), define("pair_grouped.hip", "PG_QCAP"),
                                                define("pair_grouped.hip", "PG_MAX_WORDS") * 32, define("pair_grouped.hip", "PG_RING"))
    assert ops.rescore_limits() == tuple(define("rescore.hip", d) for d in ("RS_BITS", "RS_SHORT", "RS_CHUNK"))


# ---------------------------------------------------------------------------------------------------------- the generic builders
def test_generic_graph_has_every_row_and_route(lim, generic):
    A, info = generic
    S, C, Q, R = lim["S"], lim["C"], lim["Q"], lim["R"]
    deg = np.diff(A.indptr)
    for L in pt.long_lengths(S, C) + pt.short_lengths() + [(C + 1) // R, (C + 1) // R + 1]:
        assert deg[info["row"][L]] == L
    hub, stranger = info["node"]["hub"], info["node"]["stranger"]
    assert deg[hub] >= 40000 and deg[stranger] == 64
    # the ends of col[]: the first and the last stored row are boundary rows, the last one a staged row with a one-entry tail load
    assert info["first_stored"] == info["row"][1] and info["last_stored"] == info["row"][513] == A.shape[0] - 1
    assert A.indptr[-1] == A.nnz and deg[-1] == 513
    u, v = pt.grid_pairs(info)
    k = len(info["specials"]) + 2
    assert len(u) == k * k and (u.reshape(k, k).diagonal() == v.reshape(k, k).diagonal()).all()          # u == v is there
    routes = np.array([pt.route(deg[a], deg[b], S, C, R) for a, b in zip(u, v)])
    t = pt.scores(A, np.ones(A.shape[0]), u, v)
    for r in ("small", "one", "multi", "inplace"):
        sel = (routes == r) & (u != stranger) & (v != stranger)
        assert (t["count"][sel] > 0).any(), r
        assert (t["count"][(routes == r) & ((u == stranger) ^ (v == stranger))] == 0).all() and (routes[(u == stranger) ^ (v == stranger)] == r).any(), r
    assert (t["count"][routes == "empty"] == 0).all() and (routes == "empty").sum() == 2 * k - 1
    # any two non-empty boundary rows share entries; the diagonal lists the whole row
    g = t["count"].reshape(k, k)
    assert (g[1:k - 1, 1:k - 1] > 0).all() and (g.diagonal() == deg[u.reshape(k, k).diagonal()]).all()
    # the in-place switch: C + 1 against the two lengths around (C + 1) / R, C against 1 (staged), the hub against everyone
    lo = (C + 1) // R
    assert pt.route(C + 1, lo, S, C, R) == "inplace" and pt.route(C + 1, lo + 1, S, C, R) == "multi" and pt.route(C, 1, S, C, R) == "one"
    assert all(pt.route(deg[hub], L, S, C, R) in ("inplace", "multi") for L in info["lens"] if L)
    assert {pt.route(deg[hub], L, S, C, R) for L in info["lens"] if L} == {"inplace", "multi"}
    # a last pass of exactly one entry
    assert {C + 1, 2 * C + 1, 3 * C + 1} <= set(info["lens"])


def test_merge_family_sits_on_the_first_pass_end(lim, generic):
    A, info = generic
    S, C, R = lim["S"], lim["C"], lim["R"]
    M = A.indices[A.indptr[info["node"]["M"]]:A.indptr[info["node"]["M"] + 1]]
    assert len(M) == 2 * C + 1 and M[C - 1] == info["last1"] and M[2 * C - 1] == info["last2"]
    cls = pt.merge_classes(A, info)
    for nm, (below, total, holds) in cls.items():
        assert pt.route(total, len(M), S, C, R) == "multi", nm                     # staged in passes, never searched in place
    assert cls["below"][0] == cls["below"][1] and cls["above"][0] == 0
    assert 0 < cls["straddle"][0] < 64 and cls["straddle"][1] > cls["straddle"][0] and not cls["straddle"][2]
    assert 64 < cls["straddle2"][0] < 128 < cls["straddle2"][1]                  # ... inside the SECOND slice of the shorter row
    eq = A.indices[A.indptr[info["node"]["equal"]]:A.indptr[info["node"]["equal"] + 1]]
    assert cls["equal"][2] and info["last2"] in eq and M[-1] in eq and eq[cls["equal"][0] - 1] == info["last1"]
    u, v, names = pt.merge_pairs(info)
    t = pt.scores(A, np.ones(A.shape[0]), u, v)
    assert (t["count"] > 0).all() and np.array_equal(t["count"][:5], t["count"][5:])


def test_queue_chunks_reach_every_queue_edge(lim, generic):
    A, info = generic
    Q = lim["Q"]
    u, v, chunks = pt.queue_chunks(info, Q)
    deg = np.diff(A.indptr)
    t = pt.scores(A, np.ones(A.shape[0]), u, v)
    assert len(u) == 64 * len(chunks) and t["count"].tolist() == [c for ch in chunks for c in ch]
    assert all(pt.route(deg[a], deg[b], lim["S"], lim["C"], lim["R"]) == "one" for a, b in zip(u, v))   # staged: the queue's route
    assert (u != info["node"]["H"]).any() and (v != info["node"]["H"]).any()                           # both ways round
    events = [pt.queue_events(ch, Q) for ch in chunks]
    seen = set().union(*events)
    assert seen >= {"slice_on_Q-64", "flush_on_Q-63", "open_1", "open_2", "pair_restarts_at_0", "ends_full"}
    assert "ends_full" in events[4] and chunks[4][-1] > 0                                                 # the LAST pair fills it
    # the model itself: nothing below Q - 64 flushes, one slice too many does
    assert pt.queue_events([64] * (Q // 64), Q) == {"slice_on_Q-64", "ends_full"}
    assert "pair_restarts_at_0" in pt.queue_events([64] * (Q // 64) + [1], Q)


def test_split_lists_sit_on_both_sides_of_the_choice(lim, generic):
    A, info = generic
    S, C, stride = lim["S"], lim["C"], lim["STRIDE"]
    deg = np.diff(A.indptr)
    lists = pt.split_lists(A, info, S, C, stride)
    dec = {k: pt.split_decision(deg, a, b, S, stride) for k, (a, b) in lists.items()}
    n_chunks = sorted(len(dec["chunks_%d" % c][1]) for c in (1, 2, 4, 5, stride, stride + 1, 2 * stride + 1))
    assert n_chunks == [1, 2, 4, 5, stride, stride + 1, 2 * stride + 1]
    assert all(len(lists["chunks_%d" % c][0]) % 64 for c in n_chunks)                                    # ragged last chunks
    assert {dec["chunks_%d" % c][0] for c in n_chunks} == {True, False}
    # the sample decides against the majority, both ways
    for name, want in (("sampled_small_rest_long", True), ("sampled_long_rest_small", False)):
        split, per = dec[name]
        assert split is want and (per[::stride] == (64 if want else 0))[:-1].all()
        rest = np.delete(per, np.arange(0, len(per), stride))
        assert (rest == (0 if want else 64)).all()
    # the threshold itself: 5 small > 3 pairs
    below, at = dec["one_chunk_below"], dec["one_chunk_at"]
    assert not below[0] and at[0] and at[1][0] == below[1][0] + 1 and at[1][0] * 5 > 64 * 3 >= below[1][0] * 5
    assert lim["STRIDE"] >= 2 and (below[1][0], at[1][0]) == (38, 39)                               # 60 % of 64
    # chunks with no, one, four (one round of the four-pair kernel) and five small pairs, under both decisions
    assert dec["counts_split"][0] and not dec["counts_whole"][0]
    assert dec["counts_split"][1].tolist()[1:] == dec["counts_whole"][1].tolist()[1:] == [0, 1, 4, 5]
    # a small row against an empty one is no small pair, and sits in a list that splits
    u, v = lists["empty_partner"]
    e = info["row"][0]
    small = pt.small_flags(deg, u, v, S)
    one_empty = (u == e) ^ (v == e)
    assert dec["empty_partner"][0] and one_empty.sum() >= 10 and not small[one_empty].any() and ((u == e) & (v == e)).any()
    assert ((deg[u] <= S) & (deg[v] <= S) & one_empty).sum() >= 5
    assert (u[one_empty] == e).any() and (v[one_empty] == e).any()


# ---------------------------------------------------------------------------------------------------------- the column-run builders
def test_grouped_graph_and_lists_hold_every_case(lim, grouped):
    A, info = grouped
    K, Q = lim["K"], lim["GQ"]
    deg = np.diff(A.indptr)
    nd = info["node"]
    assert info["n_stored"] < lim["B"] and A.shape[0] == info["n_stored"]
    assert [deg[i] for i in info["row_u"].values()] == pt.row_u_lengths() and deg[nd["hub"]] >= 40000 and deg[nd["empty"]] == 0
    lists = pt.grouped_lists(A, info, K)
    ones = np.ones(A.shape[0])
    # runs of equal v
    u, v = lists["runs"]
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1], [True]]))
    assert np.diff(starts).tolist() == pt.run_lengths() and (pt.scores(A, ones, u, v)["count"] > 0).any()
    # row u against the column that holds it all and the one that holds nothing; empty rows as u and as v
    u, v = lists["row_u"]
    t = pt.scores(A, ones, u, v)["count"]
    full, none = v == nd["full"], v == nd["none"]
    assert sorted(deg[u[full]]) == sorted(pt.row_u_lengths() + [deg[nd["hub"]], 0, deg[0]]) and (t[none] == 0).all()
    long_u = full & (deg[u] >= 255)
    assert (t[long_u] == deg[u[long_u]]).all()                                   # every unit of 256 entries: 256 hits
    assert (deg[u] == 0).any() and (deg[v] == 0).any() and (t[(deg[u] == 0) | (deg[v] == 0)] == 0).all()
    assert ((deg[u] > 512) & (deg[v] == 0)).any()
    # node 0: its five roles
    row = lambda i: set(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist())          # noqa: E731
    u, v = lists["node0"]
    roles = set()
    for a, b in zip(u, v):
        common = row(a) & row(b)
        roles.add((0 in row(a), 0 in row(b), common == {0}))
    assert {(True, True, False), (True, True, True), (False, True, False), (True, False, False), (False, False, False)} <= roles
    assert (u == 0).any() and (v == 0).any()                                       # node 0 as an endpoint too
    # ... and the queue exactly full when node 0 is appended: the two pairs head the run of vq, in this order
    at = int(np.flatnonzero(v == nd["vq"])[0])
    assert (u[at], u[at + 1]) == (nd["u_one"], nd["u_full"]) and v[at - 1] != nd["vq"] and v[at + 1] == nd["vq"]
    assert pt.grouped_queue_fill(A, info, Q) == Q and 0 in row(nd["u_full"]) and 0 in row(nd["vq"])
    # chunk edges
    assert len(lists["K"][0]) == K and len(lists["K+1"][0]) == K + 1
    v = lists["run_across_K"][1]
    assert v[K - 1] == v[K] and len(v) > K and (np.diff(np.flatnonzero(v == v[K]))[:] == 1).all() and v[K - 150] != v[K]
    v = lists["unsorted"][1]
    assert 200 <= len(v) <= 999 and (np.diff(v) < 0).any() and (np.diff(v) > 0).any()


def test_padded_and_hashed_graphs(lim, grouped):
    B = lim["B"]
    A, info = grouped
    for n in (B, B + 1):
        P, pinfo = pt.grouped_graph(lim["GQ"], n=n)
        assert P.shape == (n, n) and P.nnz == A.nnz and np.array_equal(P.indices, A.indices) and np.array_equal(P.data, A.data)
        assert np.array_equal(P.indptr[:info["n_stored"] + 1], A.indptr) and (np.diff(P.indptr)[info["n_stored"]:] == 0).all()
    H, hinfo, (u, v, names) = pt.hashed_graph(B)
    assert H.shape[0] == B + 4096
    row = lambda i: set(H.indices[H.indptr[i]:H.indptr[i + 1]].tolist())          # noqa: E731
    t = pt.scores(H, np.ones(H.shape[0]), u, v)["count"]
    seen = set()
    for a, b, (x, ku, cu, kv, cv), c in zip(u, v, names, t):
        ra, rb = row(a), row(b)
        assert c == len(ra & rb)
        collide = {(p, q) for p in ra for q in rb if p != q and (p - q) % B == 0}
        if collide and not (ra & rb):
            seen.add((x, ku, kv, "false_positive_only"))
        seen.add((x, ku, kv))
    for x in (0, 777):
        assert {(x, "hi", "lo", "false_positive_only"), (x, "lo", "hi", "false_positive_only"), (x, "both", "both")} <= seen
    assert 0 in row(u[[n[0] == 0 and n[1] == "lo" for n in names].index(True)]) and any(B in row(a) for a in u)
    assert (np.diff(v) >= 0).all()

"""GPU: ops.pair_scores (csrc/pair_intersect.hip, csrc/pair_grouped.hip) against the truth of tests/pair_score_truth.py on graphs
and pair lists built around the kernels' own switch points, every one of them read from the library (ops.pair_scores_limits,
ops.pair_scores_grouped_limits); tests/test_pair_score_truth_host.py holds the builders to the classes they promise.

Every list goes through both kernels (grouped False / True), float32 and float64 weights, unit and stored values, and the outputs
asked for singly and together.  Counts are exact.  With the dyadic tables every float32 sum is exact in any association
(pair_score_truth.require_exact, asserted per case), so cn and wsum must have the truth's BITS on every route -- which makes all
routes agree with each other, and (u, v) with (v, u).  With the real AA / RA tables |got - truth| <= gamma(count + 2) sum|terms|
in the kernel's accumulation precision: two roundings per term at most (the two products), count - 1 additions in whatever
association, and one unit for the truth's own rounding to float64; each test prints the largest error / bound it saw."""
import numpy as np
import pytest
import torch

import pair_score_truth as pt

pytestmark = pytest.mark.gpu

SPLIT_NAMES = ["chunks_1", "chunks_2", "chunks_4", "chunks_5", "chunks_stride", "chunks_stride+1", "chunks_2stride+1",
               "sampled_small_rest_long", "sampled_long_rest_small", "one_chunk_below", "one_chunk_at", "counts_split", "counts_whole",
               "empty_partner"]
GROUPED_NAMES = ["runs", "row_u", "node0", "K", "K+1", "run_across_K", "unsorted"]


class World:
    """A graph on the device with its weight tables, and the truths of the lists scored on it (computed once, never written to)."""

    def __init__(self, A, dev):
        self.A = {"val": A, "unit": pt.unit(A)}
        self.n, self.dev = A.shape[0], dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                   # noqa: E731
        self.rowptr, self.col = t(A.indptr.astype(np.int64)), t(A.indices.astype(np.int32))
        self.val = {"val": t(A.data.astype(np.float32)), "unit": None}
        dy = pt.dyadic_weights(self.n)
        self.w = {("dy", k, d): dy.astype(d) for k in ("val", "unit") for d in (np.float32, np.float64)}
        for mode in ("aa", "ra"):
            for k in ("val", "unit"):
                for d in (np.float32, np.float64):
                    self.w[(mode, k, d)] = pt.real_weights(self.A[k], mode, d)
        self.w_dev = {key: t(w) for key, w in self.w.items()}
        self._truth = {}

    def truth(self, table, kind, dtype, u, v):
        key = (table, kind, dtype if table != "dy" else None, u.tobytes(), v.tobytes())
        if key not in self._truth:
            self._truth[key] = pt.scores(self.A[kind], self.w[(table, kind, dtype)], u, v)
        return self._truth[key]

    def run(self, table, kind, dtype, u, v, grouped, **want):
        from eps_amd import ops
        nw = None if table is None else self.w_dev[(table, kind, dtype)]
        return ops.pair_scores(self.rowptr, self.col, self.val[kind], nw, self.n, u, v, grouped=grouped, **want)


def _bits(x, dtype):
    return np.ascontiguousarray(x, dtype).view(np.int32 if dtype == np.float32 else np.int64)


def _same(got, want, dtype):
    return got.dtype == (torch.float32 if dtype == np.float32 else torch.float64) and np.array_equal(_bits(got.cpu().numpy(), dtype),
                                                                                                     _bits(want, dtype))


def check_exact(W, u, v):
    """The dyadic family: the truth's bits from every variant."""
    dev = W.dev
    du, dv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    for kind in ("unit", "val"):
        t = W.truth("dy", kind, np.float32, u, v)
        pt.require_exact(W.A[kind], W.w[("dy", kind, np.float64)], u, v, truth=t)
        for grouped in (False, True):
            where = (kind, "grouped" if grouped else "generic")
            count, cn, ws = W.run("dy", kind, np.float32, du, dv, grouped)
            assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), t["count"]), where
            assert _same(cn, t["cn"], np.float32), where
            assert _same(ws, t["ws"], np.float32), where
            c2, cn2, ws2 = W.run("dy", kind, np.float32, dv, du, grouped)                                 # (v, u): the same bits
            assert torch.equal(c2, count) and torch.equal(cn2, cn) and torch.equal(ws2, ws), where
            c64, none, ws64 = W.run("dy", kind, np.float64, du, dv, grouped)
            assert none is None and torch.equal(c64, count) and _same(ws64, t["ws"], np.float64), where
            # the outputs asked for one at a time: other instantiations (no weights: no queue), the same results
            only = W.run("dy", kind, np.float32, du, dv, grouped, want_count=True, want_cn=False, want_wsum=False)
            assert only[1] is None and only[2] is None and torch.equal(only[0], count), where
            only = W.run("dy", kind, np.float32, du, dv, grouped, want_count=False, want_cn=True, want_wsum=False)
            assert only[0] is None and only[2] is None and torch.equal(only[1], cn), where
            only = W.run("dy", kind, np.float32, du, dv, grouped, want_count=False, want_cn=False, want_wsum=True)
            assert only[0] is None and only[1] is None and torch.equal(only[2], ws), where
            only = W.run(None, kind, np.float32, du, dv, grouped)                                          # no table at all
            assert only[2] is None and torch.equal(only[0], count) and torch.equal(only[1], cn), where
            only = W.run("dy", kind, np.float64, du, dv, grouped, want_count=False)
            assert only[0] is None and torch.equal(only[2], ws64), where


def check_real(W, u, v):
    """The real AA / RA tables: the derived bound; -> the largest error / bound."""
    dev = W.dev
    du, dv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    worst = 0.0
    for mode in ("aa", "ra"):
        for kind in ("unit", "val"):
            for dtype, gam in ((np.float32, pt.gamma), (np.float64, pt.gamma64)):
                t = W.truth(mode, kind, dtype, u, v)
                bound = gam(t["count"] + 2) * t["abs"]
                for grouped in (False, True):
                    count, cn, ws = W.run(mode, kind, dtype, du, dv, grouped)
                    where = (mode, kind, dtype.__name__, "grouped" if grouped else "generic")
                    assert np.array_equal(count.cpu().numpy(), t["count"]), where
                    err = np.abs(ws.cpu().numpy().astype(np.float64) - t["ws"])
                    ratio = float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))
                    worst = max(worst, ratio)
                    print("error / bound", where, "%.4f" % ratio)
                    assert (err <= bound).all(), where
                    if cn is not None:
                        assert (np.abs(cn.cpu().numpy().astype(np.float64) - t["cn"]) <= pt.gamma(t["count"] + 1) * t["abs_cn"]).all(), where
    print("largest error / bound: %.4f" % worst)
    return worst


# ---------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def lim(eps):
    from eps_amd import ops
    S, C, Q, R, T, STRIDE = ops.pair_scores_limits()
    K, GQ, B, RING = ops.pair_scores_grouped_limits()
    return dict(S=S, C=C, Q=Q, R=R, T=T, STRIDE=STRIDE, K=K, GQ=GQ, B=B, RING=RING)


@pytest.fixture(scope="module")
def generic(eps, dev, lim):
    A, info = pt.generic_graph(lim["S"], lim["C"], lim["Q"], lim["R"])
    W = World(A, dev)
    lists = pt.split_lists(A, info, lim["S"], lim["C"], lim["STRIDE"])
    s = lim["STRIDE"]
    named = dict(zip(SPLIT_NAMES[:7], [lists["chunks_%d" % c] for c in (1, 2, 4, 5, s, s + 1, 2 * s + 1)]))
    named.update({k: lists[k] for k in SPLIT_NAMES[7:]})
    return W, info, named


@pytest.fixture(scope="module")
def grouped(eps, dev, lim):
    A, info = pt.grouped_graph(lim["GQ"])
    return World(A, dev), info, pt.grouped_lists(A, info, lim["K"])


# ---------------------------------------------------------------------------------------------------------- the generic kernel's cases
def test_boundary_rows_every_ordered_pair(generic):
    """Every ordered pair of the rows at the path boundaries, the hub and the stranger, u == v included; the first and the last
    stored row of col[] among them; the in-place switch on both sides."""
    W, info, _ = generic
    u, v = pt.grid_pairs(info)
    check_exact(W, u, v)
    check_real(W, u, v)


def test_merge_cursor_over_several_passes(generic):
    W, info, _ = generic
    u, v, _names = pt.merge_pairs(info)
    check_exact(W, u, v)
    check_real(W, u, v)


def test_hit_queue_edges(generic, lim):
    """64-pair chunks whose hit counts put the queue of deferred weight gathers on Q - 64 (no flush), Q - 63 (flush), leave a pair
    open across one and two flushes, restart a pair at slot 0 and end a chunk on a full queue (unit values, float32 weights are the
    variant with a queue; the others run the same lists)."""
    W, info, _ = generic
    u, v, chunks = pt.queue_chunks(info, lim["Q"])
    assert W.truth("dy", "unit", np.float32, u, v)["count"].tolist() == [c for ch in chunks for c in ch]
    check_exact(W, u, v)
    check_real(W, u, v)
    # one chunk at a time: the queue starts empty, and a one-chunk list is classified on that chunk alone
    for c in range(len(chunks)):
        check_exact(W, u[64 * c:64 * c + 64].copy(), v[64 * c:64 * c + 64].copy())


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_device_side_split(generic, name):
    """Lists on both sides of the classifier's choice.  Which launch ran cannot be seen from here: the truth's bits either way."""
    W, info, lists = generic
    u, v = lists[name]
    check_exact(W, u, v)
    check_real(W, u, v)


# ---------------------------------------------------------------------------------------------------------- the column-run kernel's cases
@pytest.mark.parametrize("name", GROUPED_NAMES)
def test_column_runs(grouped, name):
    W, info, lists = grouped
    u, v = lists[name]
    check_exact(W, u, v)
    check_real(W, u, v)


def _switch_lists(lists):
    u = np.concatenate([lists[k][0] for k in ("runs", "row_u", "node0", "unsorted")])
    v = np.concatenate([lists[k][1] for k in ("runs", "row_u", "node0", "unsorted")])
    return u, v


@pytest.mark.parametrize("where", ["B", "B+1", "7B/8", "7B/8+1"])
def test_bitmap_switch_exact_to_hashed(eps, dev, lim, grouped, where):
    """The same stored graph padded with isolated nodes to n = B (the last id space the bitmap holds one bit per id for) and to
    n = B + 1 (hashed, every positive verified): the truth's bits from both, and the bits of the unpadded graph.  The same around
    7 B / 8: above it the bitmap alone fills the last sweep of the LDS a workgroup has and leaves no room for the hit queues, and
    the launch goes hashed as well (before this test that band could not be launched at all)."""
    W0, info, lists = grouped
    B = lim["B"]
    n = {"B": B, "B+1": B + 1, "7B/8": B - B // 8, "7B/8+1": B - B // 8 + 1}[where]
    u, v = _switch_lists(lists)
    du, dv = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    A, _ = pt.grouped_graph(lim["GQ"], n=n)
    assert A.shape[0] == n and np.array_equal(A.indices, W0.A["val"].indices) and np.array_equal(A.data, W0.A["val"].data)
    W = World(A, dev)
    assert np.array_equal(W.w[("dy", "val", np.float64)][:W0.n], W0.w[("dy", "val", np.float64)])
    check_exact(W, u, v)
    check_real(W, u, v)
    for kind in ("unit", "val"):
        for a, b in zip(W.run("dy", kind, np.float32, du, dv, True), W0.run("dy", kind, np.float32, du, dv, True)):
            assert torch.equal(a, b)


def test_hashed_bitmap_colliding_ids(eps, dev, lim):
    """n = B + 4096: ids x and x + B share a bit.  Row u holding only the one against a column holding only the other is a false
    positive the verification must reject; x = 0 puts node 0 and node B on bit 0.  With and without stored values (check_exact
    runs both)."""
    A, info, (u, v, names) = pt.hashed_graph(lim["B"])
    assert A.shape[0] == lim["B"] + 4096
    W = World(A, dev)
    t = W.truth("dy", "unit", np.float32, u, v)["count"]
    assert (t == 0).any() and (t > 0).any()
    check_exact(W, u, v)
    check_real(W, u, v)

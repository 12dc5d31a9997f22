"""GPU: the common-neighbour list kernel (csrc/pair_cn_list.hip: count, fill) and the transpose against the numpy truths of
tests/cn_list_truth.py, on a graph whose rows sit at the sizes where the kernel changes its path (read from the library)."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import cn_list_truth as ct

pytestmark = pytest.mark.gpu


def _dev_csr(A, dev):
    A = ssp.csr_matrix(A)
    A.sort_indices()
    return (torch.from_numpy(A.indptr.astype(np.int64)).to(dev), torch.from_numpy(A.indices.astype(np.int32)).to(dev))


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


@pytest.fixture(scope="module")
def case(eps, dev):
    """The boundary graph, its pairs and their true lists: computed once, shared, never written to."""
    from eps_amd import ops
    cap, ratio = ops.pair_cn_list_limits()
    A, special, stranger = ct.boundary_graph(cap, ratio)
    u, v = ct.boundary_pairs(A, special, stranger)
    ptr, w = ct.cn_lists(A, u, v)
    rowptr, col = _dev_csr(A, dev)
    return dict(cap=cap, ratio=ratio, A=A, n=A.shape[0], special=special, stranger=stranger, u=u, v=v, ptr=ptr, w=w,
                rowptr=rowptr, col=col, du=_i32(u, dev), dv=_i32(v, dev))


def test_boundary_pairs_cover_every_path(case):
    """Asserted on the CPU side, before anything is launched: every length class shows up in a pair with matches and in a pair
    of two non-empty rows without any, and the three ways through the kernel (one pass, several passes, in place) are taken."""
    c = case
    deg = np.diff(c["A"].indptr)
    cnt = np.diff(c["ptr"])
    k = len(c["special"])
    grid = cnt[:(k + 1) * (k + 1)].reshape(k + 1, k + 1)                          # [u class, v class], the stranger last
    assert deg[c["special"]].tolist() == ct.boundary_lengths(c["cap"], c["ratio"])
    for i, L in enumerate(deg[c["special"]]):
        if L == 0:
            assert grid[i].max() == 0 and grid[:, i].max() == 0
            continue
        assert grid[i, :k].max() > 0 and grid[:k, i].max() > 0, L                # matches, as u and as v
        assert grid[i, k] == 0 and grid[k, i] == 0, L                             # none with the stranger (64 entries elsewhere)
        assert grid[i, i] == L                                                    # u == v lists the whole row
    assert grid[k, k] == 64
    du, dv = deg[c["u"]], deg[c["v"]]
    lo, hi = np.minimum(du, dv), np.maximum(du, dv)
    inplace = (hi > c["cap"]) & (hi >= lo * c["ratio"]) & (lo > 0)
    multi = (hi > c["cap"]) & ~inplace & (lo > 0)
    single = (hi <= c["cap"]) & (lo > 0)
    for path in (inplace, multi, single):
        assert (cnt[path] > 0).any() and (cnt[path] == 0).any()
    assert (cnt[(k + 1) * (k + 1):] > 0).any()                                   # the random pairs find common neighbours too


def test_count_and_lists_equal_the_truth(eps, case):
    from eps_amd import ops
    c = case
    count = ops.pair_cn_list_count(c["rowptr"], c["col"], c["n"], c["du"], c["dv"])
    assert count.dtype == torch.int32 and count.cpu().numpy().tolist() == np.diff(c["ptr"]).tolist()
    ptr, w = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["du"], c["dv"])
    assert ptr.dtype == torch.int64 and w.dtype == torch.int32
    assert np.array_equal(ptr.cpu().numpy(), c["ptr"]) and np.array_equal(w.cpu().numpy(), c["w"])
    # list(u, v) == list(v, u): the same array
    ptr2, w2 = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["dv"], c["du"])
    assert torch.equal(ptr2, ptr) and torch.equal(w2, w)
    # two runs, the same bits
    ptr3, w3 = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["du"], c["dv"])
    assert torch.equal(ptr3, ptr) and torch.equal(w3, w)


@pytest.mark.parametrize("b", [0, 1, 63, 64, 65, 129])
def test_list_lengths_around_a_chunk(eps, case, b):
    """Lists of B pairs around the 64-pair chunk a wave takes; the pairs are the heaviest of the boundary set first."""
    from eps_amd import ops
    c = case
    order = np.argsort(-np.diff(c["ptr"]), kind="stable")[:b]
    u, v = c["u"][order], c["v"][order]
    want_ptr, want_w = ct.cn_lists(c["A"], u, v)
    ptr, w = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], _i32(u, c["rowptr"].device), _i32(v, c["rowptr"].device))
    assert ptr.shape == (b + 1,) and np.array_equal(ptr.cpu().numpy(), want_ptr) and np.array_equal(w.cpu().numpy(), want_w)


def test_a_list_without_matches(eps, case):
    from eps_amd import ops
    c = case
    dev = c["rowptr"].device
    u = np.concatenate([c["special"], [c["special"][0]] * 3])                     # everyone against the stranger, and the empty row
    v = np.concatenate([np.full(len(c["special"]), c["stranger"]), c["special"][:3]])
    ptr, w = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], _i32(u, dev), _i32(v, dev))
    assert w.numel() == 0 and ptr.cpu().numpy().tolist() == [0] * (len(u) + 1)
    tptr, tb = ops.cn_list_transpose(ptr, w, c["n"])
    assert tb.numel() == 0 and tptr.shape == (c["n"] + 1,) and int(tptr.abs().max()) == 0


def test_stored_values_are_ignored(eps, case):
    """The graph carries values in 1..3 (collab-like); its lists are those of the pattern, however the values are stored."""
    from eps_amd import ops
    c = case
    assert c["A"].data.max() > 1
    g = eps.CSRGraph.from_scipy(c["A"], device=c["rowptr"].device)
    assert g.val is not None and torch.equal(g.col, c["col"]) and torch.equal(g.rowptr, c["rowptr"])
    ptr, w = ops.pair_cn_list(g.rowptr, g.col, g.n_rows, c["du"], c["dv"])
    assert np.array_equal(ptr.cpu().numpy(), c["ptr"]) and np.array_equal(w.cpu().numpy(), c["w"])


def test_ids_out_of_range(eps, case):
    from eps_amd import ops
    c = case
    dev = c["rowptr"].device
    u, v = c["u"][:200].copy(), c["v"][:200].copy()
    bad = [3, 64, 65, 130, 199]
    u[3], v[64], u[65], v[130], u[199] = -1, c["n"], c["n"] + 7, -5, np.iinfo(np.int32).max
    for call in (ops.pair_cn_list, ops.pair_cn_list_count):
        with pytest.raises(eps.EpsError, match="node ids"):
            call(c["rowptr"], c["col"], c["n"], _i32(u, dev), _i32(v, dev))
    ptr, w = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], _i32(u, dev), _i32(v, dev), check=False)
    want_ptr, want_w = ct.cn_lists(c["A"], u, v)                                  # (the truth lists nothing for such a pair)
    assert all(want_ptr[b] == want_ptr[b + 1] for b in bad)
    assert np.array_equal(ptr.cpu().numpy(), want_ptr) and np.array_equal(w.cpu().numpy(), want_w)
    # every other segment is what it was
    full_ptr, full_w = c["ptr"], c["w"]
    got_w, got_ptr = w.cpu().numpy(), ptr.cpu().numpy()
    for b in range(200):
        if b not in bad:
            assert np.array_equal(got_w[got_ptr[b]:got_ptr[b + 1]], full_w[full_ptr[b]:full_ptr[b + 1]])


def test_host_checks(eps, case):
    from eps_amd import ops
    c = case
    with pytest.raises(eps.EpsError, match="int32"):
        ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["du"].long(), c["dv"])
    with pytest.raises(eps.EpsError, match="rowptr must hold"):
        ops.pair_cn_list(c["rowptr"], c["col"], c["n"] - 1, c["du"], c["dv"])
    with pytest.raises(eps.EpsError, match="one length"):
        ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["du"], c["dv"][:-1])
    with pytest.raises(eps.EpsError, match="ptr must hold"):
        ops.pair_cn_list_fill(c["rowptr"], c["col"], c["n"], c["du"], c["dv"], torch.zeros(3, dtype=torch.int64, device=c["du"].device),
                              torch.zeros(8, dtype=torch.int32, device=c["du"].device))


@pytest.mark.parametrize("ptr_kind", ["zero", "short"])
def test_fill_never_leaves_its_segments(eps, case, ptr_kind):
    """The clamp, not a fault: a ptr built from counts that are too small -- all zero, or every count one short -- on an out_w with
    guard words on both sides.  Nothing is stored outside the segments (so never in the guards) and the call raises."""
    from eps_amd import ops
    c = case
    dev = c["rowptr"].device
    cnt = np.diff(c["ptr"])
    small = np.zeros_like(cnt) if ptr_kind == "zero" else np.maximum(cnt - 1, 0)
    ptr = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(small, out=ptr[1:])
    m, guard, mark = int(ptr[-1]), 4096, -77
    buf = torch.full((guard + m + guard,), mark, dtype=torch.int32, device=dev)
    out_w = buf[guard:guard + m]
    with pytest.raises(eps.EpsError, match="not as long as its pair's list"):
        ops.pair_cn_list_fill(c["rowptr"], c["col"], c["n"], c["du"], c["dv"], torch.from_numpy(ptr).to(dev), out_w)
    got = buf.cpu().numpy()
    assert (got[:guard] == mark).all() and (got[guard + m:] == mark).all()
    if ptr_kind == "short":
        # what was stored inside a segment is the head of that pair's list
        for b in np.flatnonzero(small)[:300]:
            assert np.array_equal(got[guard + ptr[b]:guard + ptr[b + 1]], c["w"][c["ptr"][b]:c["ptr"][b] + small[b]])
    # the right ptr on the same guarded buffer: accepted, guards untouched
    m = int(c["ptr"][-1])
    buf = torch.full((guard + m + guard,), mark, dtype=torch.int32, device=dev)
    ops.pair_cn_list_fill(c["rowptr"], c["col"], c["n"], c["du"], c["dv"], torch.from_numpy(c["ptr"]).to(dev), buf[guard:guard + m])
    got = buf.cpu().numpy()
    assert (got[:guard] == mark).all() and (got[guard + m:] == mark).all() and np.array_equal(got[guard:guard + m], c["w"])


def test_transpose_equals_the_stable_truth(eps, case):
    from eps_amd import ops
    c = case
    dev = c["rowptr"].device
    ptr, w = torch.from_numpy(c["ptr"]).to(dev), torch.from_numpy(c["w"]).to(dev)
    want_tptr, want_tb = ct.transpose_stable(c["ptr"], c["w"], c["n"])
    tptr, tb = ops.cn_list_transpose(ptr, w, c["n"])
    assert tptr.dtype == torch.int64 and tb.dtype == torch.int32
    assert np.array_equal(tptr.cpu().numpy(), want_tptr) and np.array_equal(tb.cpu().numpy(), want_tb)
    tptr2, tb2 = ops.cn_list_transpose(ptr, w, c["n"])
    assert torch.equal(tptr2, tptr) and torch.equal(tb2, tb)
    # one node listed by every pair (and by some twice over other nodes), empty segments in between
    b = 5000
    rng = np.random.default_rng(8)
    extra = rng.integers(0, 3, b)
    extra[::11] = 0
    hub = 17
    segs = [np.sort(np.concatenate([[hub], rng.choice(np.setdiff1d(np.arange(40), [hub]), e, replace=False)])) for e in extra]
    segs[7] = segs[4000] = np.zeros(0, np.int64)                                  # ... but for two pairs that list nothing
    p = np.zeros(b + 1, np.int64)
    np.cumsum([len(s) for s in segs], out=p[1:])
    ww = np.concatenate(segs).astype(np.int32)
    want_tptr, want_tb = ct.transpose_stable(p, ww, 40)
    tptr, tb = ops.cn_list_transpose(torch.from_numpy(p).to(dev), torch.from_numpy(ww).to(dev), 40)
    assert np.array_equal(tptr.cpu().numpy(), want_tptr) and np.array_equal(tb.cpu().numpy(), want_tb)
    assert want_tptr[hub + 1] - want_tptr[hub] == b - 2
    with pytest.raises(eps.EpsError, match="w must lie in"):
        ops.cn_list_transpose(torch.from_numpy(p).to(dev), torch.from_numpy(ww).to(dev), 30)
    with pytest.raises(eps.EpsError, match="ptr must ascend"):
        ops.cn_list_transpose(torch.from_numpy(p[:-1].copy()).to(dev), torch.from_numpy(ww).to(dev), 40)

"""GPU: the local-community indices (csrc/local_community.hip; ops.local_community_degrees / local_community_scores,
heuristics.local_community, filter_stage.local_community_blocks, filter.py / rank.py --model car | cpa | caa | cra | cjc) against
the SciPy truth of tests/local_community_truth.py: gamma bit-exact, scores within one float32 ulp, and bit-identical between
orientations, batch cuts, routes and block splits.  On the parent of this change the symbols and the model names do not exist."""
import argparse
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import cn_list_truth as ct
import local_community_truth as lct
import local_index_truth as lit
from conftest import GOLDEN
from test_gpu_katz_filter import CASES, _graph, _stand_in

pytestmark = pytest.mark.gpu

NAMES = lct.INDICES
SENTINEL = -77
GOLDENS = ("pairs_clique20", "pairs_collab_like", "pairs_er500", "pairs_isolated_deg1", "pairs_path30", "pairs_rmat10",
           "pairs_rmat12", "pairs_star50")
_CASES = {}


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)


def _dev_csr(A, dev):
    A = ssp.csr_matrix(A)
    A.sort_indices()
    return _i64(A.indptr, dev), _i32(A.indices, dev)


def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = len(d["rowptr"]) - 1
    A = ssp.csr_matrix((np.ones(len(d["col"])), d["col"], d["rowptr"]), shape=(n, n))
    A.sort_indices()
    return A


def _case(key, dev):
    """(A, u, v, ptr, w, gamma) of a named pair set: the truth computed once, shared, never written to."""
    if key not in _CASES:
        name, _, kind = key.partition(":")
        if name == "boundary":
            from eps_amd import ops
            _, cap, ratio = ops.local_community_limits()
            A, special, stranger = ct.boundary_graph(cap, ratio)
            u, v = ct.boundary_pairs(A, special, stranger)
        else:
            A = _golden(name)
            n = A.shape[0]
            if kind == "edges":                                  # the stored edges: long lists
                coo = A.tocoo()
                u, v = coo.row, coo.col
            elif name == "pairs_clique20":                       # no candidates: every node pair
                u, v = np.nonzero(np.ones((n, n)) - np.eye(n))
            else:                                                # every ordered pair of the 2-hop candidates
                u, v, _ = lit.two_hop_candidates(A)
                if len(u) > 200_000:
                    pick = np.sort(np.random.default_rng(12).choice(len(u), 200_000, replace=False))
                    u, v = u[pick], v[pick]
        ptr, w, gamma = lct.pair_truth(A, u, v)
        rowptr, col = _dev_csr(A, dev)
        _CASES[key] = dict(A=A, n=A.shape[0], u=np.asarray(u, np.int64), v=np.asarray(v, np.int64), ptr=ptr, w=w, gamma=gamma,
                           rowptr=rowptr, col=col, du=_i32(u, dev), dv=_i32(v, dev))
    return _CASES[key]


def _gamma(ops, c, ptr, w, **kw):
    """local_community_degrees into a buffer prefilled with a sentinel, guard words on both sides."""
    dev = c["rowptr"].device
    m, guard = len(w), 64
    buf = torch.full((guard + m + guard,), SENTINEL, dtype=torch.int32, device=dev)
    out = ops.local_community_degrees(c["rowptr"], c["col"], c["n"], _i64(ptr, dev), _i32(w, dev), out=buf[guard:guard + m], **kw)
    got = buf.cpu().numpy()
    assert (got[:guard] == SENTINEL).all() and (got[guard + m:] == SENTINEL).all(), "stored outside gamma"
    assert m == 0 or out.data_ptr() == buf[guard:].data_ptr()
    return got[guard:guard + m]


# ---------------------------------------------------------------------------------------------------------- gamma
@pytest.mark.parametrize("key", GOLDENS + ("pairs_rmat10:edges",))
def test_gamma_and_scores_on_the_golden_graphs(eps, dev, key):
    from eps_amd import heuristics, ops
    c = _case(key, dev)
    ptr, w = ops.pair_cn_list(c["rowptr"], c["col"], c["n"], c["du"], c["dv"])
    assert np.array_equal(ptr.cpu().numpy(), c["ptr"]) and np.array_equal(w.cpu().numpy(), c["w"])
    got = _gamma(ops, c, c["ptr"], c["w"])
    assert np.array_equal(got, c["gamma"]), key
    if key == "pairs_clique20":
        assert len(c["u"]) == 380 and (np.diff(c["ptr"]) == 18).all() and (got == 17).all()
    if key == "pairs_rmat10:edges":
        assert np.diff(c["ptr"]).max() > 64 and c["gamma"].max() > 0
    g = eps.CSRGraph(c["rowptr"], c["col"], None, c["n"], c["n"])
    e = torch.stack([c["du"], c["dv"]]).long()
    for index in NAMES:
        want = lct.scores(c["A"], c["u"], c["v"], c["ptr"], c["w"], c["gamma"], index)
        fwd = heuristics.local_community(g, e, index)
        assert fwd.dtype == torch.float32 and fwd.device == c["rowptr"].device
        lit.assert_within_one_ulp(fwd.cpu().numpy(), want, f"{key} {index}")
        rev = heuristics.local_community(g, e.flip(0), index)
        assert torch.equal(fwd.view(torch.int32), rev.view(torch.int32)), f"{key} {index}: score(u, v) != score(v, u)"
        if index == "cpa":                                       # no link among fewer than two: (a - c)(b - c), exactly
            deg, cnt = lit.degrees(c["A"]), np.diff(c["ptr"])
            few = cnt < 2
            assert np.array_equal(fwd.cpu().numpy()[few], ((deg[c["u"]] - cnt) * (deg[c["v"]] - cnt))[few].astype(np.float32))
    if key == "pairs_path30":
        assert (np.diff(c["ptr"]) < 2).all() and len(c["w"]) > 0


def test_gamma_and_scores_on_the_boundary_graph(eps, dev, monkeypatch):
    """Lists of cap - 1, cap, cap + 1, 2 cap + 1 and 40,000 entries, entries whose own row is a 40,000-entry hub, empty lists --
    the graph of the list kernel's tests built from THIS unit's limits; then the same batch under an entry budget of 1000."""
    from eps_amd import heuristics, ops
    short, cap, ratio = ops.local_community_limits()
    c = _case("boundary", dev)
    cnt, deg = np.diff(c["ptr"]), lit.degrees(c["A"])
    b_of = np.repeat(np.arange(len(cnt)), cnt)
    for length in (cap - 1, cap, cap + 1, 2 * cap + 1, 40000):
        assert (c["gamma"][np.isin(b_of, np.flatnonzero(cnt == length))] > 0).any(), length
    assert (cnt == 0).any() and (cnt == 1).any()
    hub = deg[c["w"]] > cap                                      # entries whose own row is a long special row, in 2-entry lists too
    assert hub.sum() >= 100 and (cnt[b_of][hub] == 2).any()
    got = _gamma(ops, c, c["ptr"], c["w"])
    assert np.array_equal(got, c["gamma"])
    g = eps.CSRGraph(c["rowptr"], c["col"], None, c["n"], c["n"])
    e = torch.stack([c["du"], c["dv"]]).long()
    whole = {}
    for index in NAMES:
        whole[index] = heuristics.local_community(g, e, index)
        want = lct.scores(c["A"], c["u"], c["v"], c["ptr"], c["w"], c["gamma"], index)
        lit.assert_within_one_ulp(whole[index].cpu().numpy(), want, f"boundary {index}")
    monkeypatch.setattr(heuristics, "LOCAL_COMMUNITY_BUDGET", 1000)
    assert cnt.max() > 1000 and len(heuristics._budget_cuts(c["du"].new_tensor(cnt[cnt >= 2]), 1000)) > 10
    for index in NAMES:
        cut = heuristics.local_community(g, e, index)
        assert torch.equal(cut.view(torch.int32), whole[index].view(torch.int32)), f"{index}: the cuts of the batch changed a score"


@pytest.fixture(scope="module")
def loops(dev):
    """An ASYMMETRIC pattern with self loops on a third of the nodes, and random ordered pairs on it."""
    rng = np.random.default_rng(21)
    n = 300
    M = rng.random((n, n)) < 0.12
    np.fill_diagonal(M, rng.random(n) < 0.33)
    A = ssp.csr_matrix(M.astype(np.float64))
    A.sort_indices()
    u, v = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    ptr, w, gamma = lct.pair_truth(A, u, v)
    rowptr, col = _dev_csr(A, dev)
    return dict(A=A, n=n, u=u, v=v, ptr=ptr, w=w, gamma=gamma, rowptr=rowptr, col=col, du=_i32(u, dev), dv=_i32(v, dev))


def test_self_loops_and_an_asymmetric_pattern(eps, dev, loops):
    from eps_amd import heuristics, ops
    c = loops
    cnt = np.diff(c["ptr"])
    G = np.bincount(np.repeat(np.arange(len(cnt)), cnt), weights=c["gamma"], minlength=len(cnt)).astype(np.int64)
    assert (G % 2 == 1).any(), "expected an odd sum of gamma somewhere"
    assert c["A"].diagonal()[c["w"]].any(), "expected common neighbours with a self loop"
    assert np.array_equal(_gamma(ops, c, c["ptr"], c["w"]), c["gamma"])
    g = eps.CSRGraph(c["rowptr"], c["col"], None, c["n"], c["n"])
    e = torch.stack([c["du"], c["dv"]]).long()
    for index in NAMES:
        want = lct.scores(c["A"], c["u"], c["v"], c["ptr"], c["w"], c["gamma"], index)
        assert np.isfinite(want).all()
        lit.assert_within_one_ulp(heuristics.local_community(g, e, index).cpu().numpy(), want, index)


def _segments(n, lengths, rng):
    segs = [np.sort(rng.choice(n, L, replace=False)) for L in lengths]
    ptr = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([len(s) for s in segs], out=ptr[1:])
    return ptr, np.concatenate(segs).astype(np.int32)


def test_arbitrary_segments_of_every_length_class(eps, dev, loops):
    """Ascending segments that are no common-neighbour lists: lengths 0, 1, 2, 3, the short-list bound and one past it, and
    63 / 64 / 65, thirty of each in a random order (so a 64-segment chunk mixes them)."""
    from eps_amd import ops
    short, _, _ = ops.local_community_limits()
    c = loops
    rng = np.random.default_rng(3)
    lengths = rng.permutation(np.repeat([0, 1, 2, 3, short, short + 1, 63, 64, 65], 30))
    ptr, w = _segments(c["n"], lengths, rng)
    want = lct.gammas(c["A"], ptr, w)
    assert want.max() > 3 and np.array_equal(want, lct.gammas_by_pair(c["A"], ptr, w))
    assert np.array_equal(_gamma(ops, c, ptr, w), want)
    # ... and one segment alone, of each length
    for L in (1, 2, 3, short, short + 1, 63, 64, 65):
        p1, w1 = _segments(c["n"], [L], rng)
        assert np.array_equal(_gamma(ops, c, p1, w1), lct.gammas(c["A"], p1, w1)), L


def test_hubs_searched_in_place_around_the_ratio(eps, dev):
    """Three hubs of exactly ratio * 40 stored entries (one with a self loop) among 4000 low-degree nodes, in segments of 9 ..
    100 entries: a hub's row is searched in place up to 40 staged entries and streamed from 41 on; then lists beyond the staging
    capacity whose later passes are short enough for the in-place search again."""
    from eps_amd import ops
    short, cap, ratio = ops.local_community_limits()
    rng = np.random.default_rng(31)
    n, hubs = 4000, np.array([5, 1999, 3777])
    ring = np.arange(n)                                          # (every row holds two entries at least: log2 d_w > 0)
    r = np.concatenate([rng.integers(0, n, 20000), ring, ring])
    cidx = np.concatenate([rng.integers(0, n, 20000), (ring + 1) % n, (ring + 2) % n])
    M = ssp.coo_matrix((np.ones(len(r)), (r, cidx)), shape=(n, n)).tolil()
    M[hubs, :] = 0
    for h in hubs:
        M[h, rng.choice(np.setdiff1d(np.arange(n), [h]), ratio * 40 - (h == 5), replace=False)] = 1
    M[5, 5] = 1
    A = ssp.csr_matrix(M)
    A = ssp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=(n, n))
    A.sort_indices()
    deg = lit.degrees(A)
    assert (deg[hubs] == ratio * 40).all() and A[5, 5] == 1
    c = dict(rowptr=_dev_csr(A, dev)[0], col=_dev_csr(A, dev)[1], n=n)
    lengths = [short + 1, 20, 39, 40, 41, 64, 100] * 6 + [cap + 3, 2 * cap + 40]
    segs = []
    for k, L in enumerate(lengths):
        mine = hubs[:1 + k % 3]                                  # one, two or three hubs in the segment
        pool = A[5].indices if L <= 100 else np.arange(n)        # (neighbours of hub 5: its gamma is every other member)
        rest = rng.choice(np.setdiff1d(pool, hubs), L - len(mine), replace=False)
        segs.append(np.sort(np.concatenate([mine, rest])))
    ptr = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([len(x) for x in segs], out=ptr[1:])
    w = np.concatenate(segs).astype(np.int32)
    want = lct.gammas(A, ptr, w)
    b_of = np.repeat(np.arange(len(lengths)), lengths)
    is_hub = np.isin(w, hubs)
    staged = np.minimum(np.asarray(lengths)[b_of], cap)
    inplace = is_hub & (deg[w] >= ratio * staged)
    assert inplace.sum() >= 40 and (is_hub & ~inplace).sum() >= 20 and (want[inplace & (w != 5)] > 0).any()
    small = (w == 5) & (np.asarray(lengths)[b_of] <= 100)        # hub 5: every other member, its self loop not counted
    assert (want[small] >= np.asarray(lengths)[b_of][small] - 3).all() and (want[small] < np.asarray(lengths)[b_of][small]).all()
    assert np.array_equal(_gamma(ops, c, ptr, w), want)
    u = _i32(rng.integers(0, n, len(lengths)), dev)
    v = _i32(rng.integers(0, n, len(lengths)), dev)
    for index in NAMES:
        got = ops.local_community_scores(c["rowptr"], n, u, v, _i64(ptr, dev), _i32(w, dev), _i32(want, dev), index)
        lit.assert_within_one_ulp(got.cpu().numpy(), lct.scores(A, u.cpu().numpy(), v.cpu().numpy(), ptr, w, want, index), index)


def test_refused_segments_get_zeros_and_leave_their_neighbours_alone(eps, dev, loops):
    from eps_amd import ops
    short, _, _ = ops.local_community_limits()
    c = loops
    rng = np.random.default_rng(4)
    lengths = np.tile([3, 64, short, 20, 2, short + 1], 20)
    ptr, w = _segments(c["n"], lengths, rng)
    want = lct.gammas(c["A"], ptr, w)
    stats = {}
    assert np.array_equal(_gamma(ops, c, ptr, w, stats=stats), want) and stats["status"] == 0
    bad = w.copy()
    spoiled = {0: "descending", 1: "descending", 8: "too large", 13: "negative", 21: "repeated", 61: "too large", 119: "descending"}
    for s, how in spoiled.items():
        lo, hi = ptr[s], ptr[s + 1]
        if how == "descending":
            bad[lo], bad[lo + 1] = max(bad[lo], bad[lo + 1]), min(bad[lo], bad[lo + 1])
            bad[hi - 1], bad[hi - 2] = bad[hi - 2], bad[hi - 1]
        elif how == "too large":
            bad[hi - 1] = c["n"] if s == 8 else np.iinfo(np.int32).max
        elif how == "negative":
            bad[lo] = -1
        else:
            bad[lo + 1] = bad[lo]
    got = _gamma(ops, c, ptr, bad, stats=stats)
    assert stats["status"] == 1
    for s in range(len(lengths)):
        lo, hi = ptr[s], ptr[s + 1]
        assert np.array_equal(got[lo:hi], np.zeros(hi - lo, np.int32) if s in spoiled else want[lo:hi]), s
    with pytest.raises(eps.EpsError, match="does not ascend strictly"):
        _gamma(ops, c, ptr, bad)
    with pytest.raises(eps.EpsError, match="ptr must ascend"):
        _gamma(ops, c, ptr[:-1], w)


def test_nothing_to_do(eps, dev, loops):
    from eps_amd import heuristics, ops
    c = loops
    none = _gamma(ops, c, np.zeros(1, np.int64), np.zeros(0, np.int32))                      # n_pairs = 0
    assert none.shape == (0,)
    assert _gamma(ops, c, np.zeros(6, np.int64), np.zeros(0, np.int32)).shape == (0,)       # M = 0
    z = torch.zeros(0, dtype=torch.int32, device=dev)
    out = ops.local_community_scores(c["rowptr"], c["n"], z, z, _i64([0], dev), z, z, "cra")
    assert out.shape == (0,) and out.dtype == torch.float32
    g = eps.CSRGraph(c["rowptr"], c["col"], None, c["n"], c["n"])
    assert heuristics.local_community(g, torch.zeros((2, 0), dtype=torch.long), "car").shape == (0,)
    # five pairs that list nothing: closed forms
    u = _i32([0, 1, 2, 3, 4], dev)
    got = ops.local_community_scores(c["rowptr"], c["n"], u, u.flip(0), _i64(np.zeros(6), dev), z, z, "cpa").cpu().numpy()
    deg = lit.degrees(c["A"])
    assert np.array_equal(got, (deg[:5] * deg[:5][::-1]).astype(np.float32))
    with pytest.raises(eps.EpsError, match="node ids"):
        heuristics.local_community(g, torch.tensor([[0], [c["n"]]]), "cra")


# ---------------------------------------------------------------------------------------------------------- the filter's route
def _blocks(eps, dev, g, index, bounds):
    from eps_amd import filter_stage
    args, data = argparse.Namespace(model=index), argparse.Namespace(adj_t=g)
    pairs, scores = [], []
    for v_lo, v_hi, blk, score in filter_stage.local_community_blocks(args, data, bounds):
        if isinstance(blk, torch.Tensor):
            if blk.shape[1]:
                pairs.append(blk.long()); scores.append(score)
            continue
        assert score is blk.score and not blk.padded
        pairs.append(blk.pairs()); scores.append(score)
    return torch.cat(pairs, 1), torch.cat(scores)


def test_blocks_equal_the_pair_entry_under_any_split(eps, dev):
    from eps_amd import heuristics
    A = _golden("pairs_er500")
    n = A.shape[0]
    g = eps.CSRGraph(*_dev_csr(A, dev), None, n, n)
    cu, cv, cc = lit.two_hop_candidates(A)
    thirds = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    for index in NAMES:
        pairs, one = _blocks(eps, dev, g, index, [(0, n)])
        assert np.array_equal(pairs[0].cpu().numpy(), cu) and np.array_equal(pairs[1].cpu().numpy(), cv)
        ref = heuristics.local_community(g, pairs, index)
        assert torch.equal(one.view(torch.int32), ref.view(torch.int32)), f"{index}: filter route != pair entry"
        p3, three = _blocks(eps, dev, g, index, thirds)
        assert torch.equal(p3, pairs) and torch.equal(three.view(torch.int32), one.view(torch.int32)), f"{index}: three blocks"
        if index == "cra":
            pn, each = _blocks(eps, dev, g, index, [(v, v + 1) for v in range(n)])
            assert torch.equal(pn, pairs) and torch.equal(each.view(torch.int32), one.view(torch.int32)), "one block per column"
            ptr, w, gamma = lct.pair_truth(A, cu, cv)
            lit.assert_within_one_ulp(one.cpu().numpy(), lct.scores(A, cu, cv, ptr, w, gamma, index), "blocks cra")
            assert (cc >= 2).any() and (cc < 2).any()


def test_padding_slots_of_a_count_free_block_keep_the_sentinel(eps, dev):
    from eps_amd import filter_stage, heuristics
    A = _golden("pairs_rmat10")
    n = A.shape[0]
    g = eps.CSRGraph(*_dev_csr(A, dev), None, n, n)
    blk = filter_stage._counted_block(g, 0, n, count_free=True)
    assert blk.padded
    out = torch.full((blk.cand_u.numel(),), float(SENTINEL), dtype=torch.float32, device=dev)
    got = heuristics.local_community_columns(g, 0, n, blk, "cra", out=out)
    assert got is out
    colptr, counts = blk.colptr.cpu().numpy(), blk.counts.cpu().numpy()
    live = np.zeros(out.numel(), bool)
    for s in range(n):                                           # the counted entries of every column
        live[colptr[s]:colptr[s] + counts[s]] = True
    cu, cv, _ = lit.two_hop_candidates(A)
    assert live.sum() == len(cu) and (~live).sum() > 0
    live = torch.from_numpy(live).to(dev)
    assert bool((out[~live] == float(SENTINEL)).all()), "a padding slot was written"
    got_v = np.repeat(np.arange(n), counts)
    order = np.lexsort((blk.cand_u[live].cpu().numpy(), got_v))  # (whatever the order inside a column)
    assert np.array_equal(blk.cand_u[live].cpu().numpy()[order], cu) and np.array_equal(got_v[order], cv)
    ref = heuristics.local_community(g, torch.from_numpy(np.stack([cu, cv])).to(dev), "cra")
    assert torch.equal(out[live][torch.from_numpy(order).to(dev)].view(torch.int32), ref.view(torch.int32)) and float(ref.max()) > 0
    assert bool(torch.isinf(heuristics.local_community_columns(g, 0, n, blk, "cra")[~live]).all())


# ---------------------------------------------------------------------------------------------------------- command lines
def _filter(dataset, model, run, *flags):
    from eps_amd import filter_stage
    return torch.load(filter_stage.main(["--dataset", dataset, "--model", model, "--checkpoint", f"{dataset}_{model}||0|{run}.pt",
                                         "--synthetic", *flags]))


@pytest.mark.parametrize("dataset", sorted(CASES))
def test_filter_cli_cra(eps, dev, oracle, tmp_path, dataset, monkeypatch):
    """filter.py --model cra: the full file is the candidate set scored and ordered; --keep_top K is its first K rows and
    --keep_per_node 3 every node's first three, bit for bit (several column blocks)."""
    from eps_amd import candidates
    from oracle import eps_oracle
    with _stand_in(dataset, tmp_path):
        rows = _filter(dataset, "cra", 0)
        A = _graph(oracle, dataset)
        monkeypatch.setattr(candidates, "DEFAULT_BLOCK_PATHS", 30_000)
        top = _filter(dataset, "cra", 1, "--keep_top", "1000")
        cut = _filter(dataset, "cra", 2, "--keep_per_node", "3")
    n = A.shape[0]
    assert rows.shape == (CASES[dataset][2], 3) and rows.dtype == torch.float32
    r = rows.numpy()
    u, v, s = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), r[:, 2]
    want = eps_oracle.candidates_scipy(A)[0]
    assert np.array_equal(np.sort(v * n + u), np.sort(want[:, 1] * n + want[:, 0])), "not the 2-hop non-edge set"
    pick = np.random.default_rng(5).choice(len(u), 4000, replace=False)          # (the SciPy truth of a dense graph is slow)
    ptr, w, gamma = lct.pair_truth(A, u[pick], v[pick])
    lit.assert_within_one_ulp(s[pick], lct.scores(A, u[pick], v[pick], ptr, w, gamma, "cra"), f"{dataset} cra")
    assert np.array_equal(np.lexsort((u, v, -s.astype(np.float64))), np.arange(len(s))), "rows out of the declared order"
    assert s.max() > 0
    assert top.shape == (1000, 3) and torch.equal(top, rows[:1000])
    order = np.argsort(v, kind="stable")
    start = np.r_[0, np.flatnonzero(np.diff(v[order])) + 1]
    rank = np.arange(len(v)) - np.repeat(start, np.diff(np.r_[start, len(v)]))
    keep = np.zeros(len(v), bool)
    keep[order[rank < 3]] = True
    assert 0 < keep.sum() < len(v) and torch.equal(cut, rows[torch.from_numpy(keep)])


def test_rank_cli_car(eps, dev, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", CASES["collab"][0])
    from eps_amd import rank_stage
    curves = rank_stage.main(["--dataset", "collab", "--model", "car", "--synthetic", "--runs", "1"])
    assert len(curves) == 1 and int(curves[0][0]) == 0
    for x in curves[0][1:]:
        assert np.isfinite(float(x)) and 0.0 <= float(x) <= 100.0
    assert "Hits@" in capsys.readouterr().out

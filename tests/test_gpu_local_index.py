"""GPU: the local-index kernels (csrc/local_index.hip) against the float64 truth of tests/local_index_truth.py, to one float32
ulp (derived there; in practice equality), and bit for bit between the routes of this build: the golden graphs with every 2-hop
candidate of every column in both layouts and both count forms and under three splits into blocks; the pair entry; the
survivor lists."""
import os

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import local_index_truth as lit
from conftest import golden_pair_files

pytestmark = pytest.mark.gpu


def _graphs(eps, A):
    """(the graph without stored values -> float32 counts from the list kernels, the same pattern with values -> int32 counts
    from the fused expansion).  The values must not matter: ones are stored as 2.0."""
    P = ssp.csr_matrix(A, dtype=np.float32)
    P.sum_duplicates()
    P.sort_indices()
    g = eps.CSRGraph.from_scipy(P, device="cuda:0", keep_values=False)
    val = torch.from_numpy(np.where(P.data == 1.0, np.float32(2.0), P.data).astype(np.float32)).to("cuda:0")
    return g, eps.CSRGraph(g.rowptr, g.col, val, g.n_rows, g.n_cols)


def _live(blk):
    """Positions of a block's counted slots, ascending, and the column of each (numpy)."""
    colptr = blk.colptr.cpu().numpy()
    width = np.diff(colptr)
    cnt = width if blk.counts is None else blk.counts.cpu().numpy()
    assert np.all(cnt >= 0) and np.all(cnt <= width)
    col = np.repeat(np.arange(len(cnt)), cnt)
    start = np.repeat(colptr[:-1], cnt)
    rank = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return start + rank, col


SENTINEL = -1          # the bits of a slot nobody wrote (0xFFFFFFFF: what a poisoned allocator block holds)


def _scores(eps, g, v_lo, v_hi, blk, name, **kw):
    """Scores per slot through ops, into an array prefilled with the sentinel bits: -> (float32 numpy, int32 view of it)."""
    out = torch.full((blk.cand_u.numel(),), SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)
    got = eps.ops.local_index_columns(g.rowptr, g.n_rows, v_lo, v_hi, blk.colptr, blk.cand_u, blk.cn, name, counts=blk.counts,
                                      out=out, **kw)
    assert got is out
    s = out.cpu().numpy()
    return s, s.view(np.int32)


@pytest.mark.parametrize("path", golden_pair_files(), ids=lambda p: os.path.basename(p)[6:-4])
def test_every_candidate_of_the_golden_graphs(eps, dev, path):
    from eps_amd import filter_stage
    d = np.load(path)
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    assert (lit.pattern(A) != lit.pattern(A).T).nnz == 0
    cu, cv, cc = lit.two_hop_candidates(A)
    name_of = os.path.basename(path)
    if "clique20" in name_of:
        assert len(cu) == 0
    deg = lit.degrees(A)
    g_unit, g_val = _graphs(eps, A)
    assert g_unit.val is None and g_val.val is not None
    blocks = {}
    for form, g in (("f32", g_unit), ("i32", g_val)):
        for layout, count_free in (("exact", False), ("padded", True)):
            blk = filter_stage._counted_block(g, 0, n, count_free)
            assert blk.cn.dtype == (torch.float32 if form == "f32" else torch.int32) and (blk.counts is not None) == count_free
            pos, col = _live(blk)
            # the candidates and their counts are the truth's, in its order
            assert np.array_equal(blk.cand_u.cpu().numpy()[pos], cu) and np.array_equal(col, cv), (form, layout)
            assert np.array_equal(blk.cn.cpu().numpy()[pos].astype(np.int64), cc), (form, layout)
            blocks[form, layout] = (g, blk, pos)
    # (u, v) -> (v, u) among the candidates
    key = cv * n + cu
    mirror = np.searchsorted(key, cu * n + cv)
    assert np.array_equal(key[mirror], cu * n + cv)
    rng = np.random.default_rng(n)
    cut = int(rng.integers(1, n))
    for k, name in enumerate(lit.INDICES):
        want = lit.index_scores(name, cc, deg[cu], deg[cv])
        ref = None
        for (form, layout), (g, blk, pos) in blocks.items():
            s, bits = _scores(eps, g, 0, n, blk, name)
            pad = np.ones(len(s), bool)
            pad[pos] = False
            assert np.all(bits[pad] == SENTINEL), f"{name} {form} {layout}: a padding slot was written"
            got = s[pos]
            lit.assert_within_one_ulp(got, want, f"{name_of} {name} {form} {layout}")
            if ref is None:
                ref = got
            assert got.tobytes() == ref.tobytes(), f"{name} {form} {layout}: differs from the first route"
        assert np.array_equal(ref[mirror].view(np.int32), ref.view(np.int32)), f"{name}: score(u, v) != score(v, u)"
        if "star50" in name_of:
            assert np.all(ref == 1.0)
        # one block per column: slices of the one-block arrays (odd offsets: the 16-byte accesses do not apply), both count forms in turn
        g, blk, pos = blocks["f32" if k % 2 else "i32", "exact"]
        colptr = blk.colptr.cpu().numpy()
        lens = torch.stack([torch.zeros(n, dtype=torch.int64), torch.from_numpy(np.diff(colptr))], 1).to(dev)
        parts = []
        for v in np.flatnonzero(np.diff(colptr)):
            lo, hi = int(colptr[v]), int(colptr[v + 1])
            parts.append(eps.ops.local_index_columns(g.rowptr, n, int(v), int(v) + 1, lens[v], blk.cand_u[lo:hi], blk.cn[lo:hi], name,
                                                     check=False))
        per_col = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.float32)
        assert per_col.tobytes() == ref.tobytes(), f"{name}: one block per column differs"
        # two blocks cut at a seeded column, each expanded on its own
        g = blocks["i32" if k % 2 else "f32", "exact"][0]
        halves = []
        for lo, hi in ((0, cut), (cut, n)):
            b2 = filter_stage._counted_block(g, lo, hi, bool(k & 2))
            s2, _ = _scores(eps, g, lo, hi, b2, name)
            halves.append(s2[_live(b2)[0]])
        assert np.concatenate(halves).tobytes() == ref.tobytes(), f"{name}: two blocks cut at column {cut} differ"


def test_pair_entry_on_rmat10(eps, dev):
    from eps_amd import heuristics
    d = np.load([p for p in golden_pair_files() if "rmat10" in p][0])
    n = d["rowptr"].size - 1
    A = ssp.csr_matrix((d["val"].astype(np.float64), d["col"], d["rowptr"]), shape=(n, n))
    g = _graphs(eps, A)[0]
    deg = lit.degrees(A)
    isolated, rows = np.flatnonzero(deg == 0), A.tocoo()
    assert len(isolated) > 10
    rng = np.random.default_rng(10)
    for m in (0, 1, 63, 64, 65, 1000):
        u, v = rng.integers(0, n, m), rng.integers(0, n, m)
        k = m // 4
        pick = rng.integers(0, rows.nnz, k)
        u[:k], v[:k] = rows.row[pick], rows.col[pick]                       # stored edges
        u[k:2 * k] = v[k:2 * k]                                             # u == v
        u[2 * k:3 * k] = isolated[rng.integers(0, len(isolated), k)]        # isolated nodes
        if m == 1:
            u[0] = isolated[0]
        c = lit.common_counts(A, u, v)
        e = torch.from_numpy(np.stack([u, v]))
        for name in lit.INDICES:
            got = heuristics.local_index(g, e, name)
            assert got.dtype == torch.float32 and got.is_cuda and got.shape == (m,)
            got = got.cpu().numpy()
            lit.assert_within_one_ulp(got, lit.truth(A, u, v, name, c=c), f"{name}, {m} pairs")
            assert np.all(got[2 * k:3 * k] == 0.0), f"{name}: an isolated node scores 0"
            assert np.array_equal(got, heuristics.local_index(g, e.flip(0), name).cpu().numpy()), f"{name}: not symmetric"
            # a slice off the 16-byte grid takes the scalar path: the same bits
            if m == 1000:
                cnt = eps.ops.pair_scores(g.rowptr, g.col, None, None, n, e[0].to(dev, torch.int32), e[1].to(dev, torch.int32),
                                          want_count=True, want_cn=False)[0]
                odd = eps.ops.local_index_pairs(g.rowptr, n, e[0].to(dev, torch.int32)[1:], e[1].to(dev, torch.int32)[1:], cnt[1:], name)
                assert np.array_equal(odd.cpu().numpy(), got[1:])
    with pytest.raises(eps.EpsError, match="node ids"):
        heuristics.local_index(g, torch.tensor([[0], [n]]), "jaccard")
    with pytest.raises(eps.EpsError, match="one of salton"):
        heuristics.local_index(g, torch.tensor([[0], [1]]), "cosine")


def test_an_id_outside_the_graph_scores_nan_and_nothing_else(eps, dev):
    """The kernels index rowptr with ids they have checked: a slot with a bad id is NaN, its neighbours are untouched."""
    rowptr = torch.tensor([0, 2, 3, 5, 5], dtype=torch.int64, device=dev)
    u = torch.tensor([0, -1, 2, 4, 1, 3, 2, 0, 1], dtype=torch.int32, device=dev)
    cn = torch.ones(9, dtype=torch.int32, device=dev)
    colptr = torch.tensor([0, 3, 5, 9, 9], dtype=torch.int64, device=dev)
    got = eps.ops.local_index_columns(rowptr, 4, 0, 4, colptr, u, cn, "pa", check=False).cpu().numpy()
    deg, col = np.array([2, 1, 2, 0]), np.array([0, 0, 0, 1, 1, 2, 2, 2, 2])
    bad = np.array([False, True, False, True, False, False, False, False, False])
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], (deg[u.cpu().numpy()[~bad]] * deg[col[~bad]]).astype(np.float32))
    with pytest.raises(eps.EpsError, match="node ids"):
        eps.ops.local_index_columns(rowptr, 4, 0, 4, colptr, u, cn, "pa")
    with pytest.raises(eps.EpsError, match="colptr must ascend"):
        eps.ops.local_index_columns(rowptr, 4, 0, 4, colptr - 1, u.clamp(0, 3), cn, "pa")
    v = torch.tensor([0, 9, 2], dtype=torch.int32, device=dev)
    got = eps.ops.local_index_pairs(rowptr, 4, u[:3], v, cn[:3], "pa").cpu().numpy()
    assert got[0] == 4.0 and np.isnan(got[1]) and got[2] == 4.0
    # a NaN never exceeds a bar
    assert eps.ops.local_index_columns(rowptr, 4, 0, 4, colptr, u, cn, "pa", bar=-1.0, capacity=9, check=False)[0].tolist() == \
        [i for i in range(9) if not bad[i]]


# ---------------------------------------------------------------------------------------------------------- survivors
def _hub_graph():
    """n = 6000: node 0 with 75 neighbours of 70 leaves each (column 0 holds 5250 candidates: more than one slice of the slot
    array), nodes 100 .. 399 isolated (300 consecutive empty columns), some seeded leaf-leaf edges for a spread of scores."""
    n, mids, per = 6000, 75, 70
    mid_ids = np.arange(1, mids + 1)
    leaf_ids = np.arange(400, 400 + mids * per)
    e = [(0, m) for m in mid_ids] + [(mid_ids[i // per], leaf) for i, leaf in enumerate(leaf_ids)]
    rng = np.random.default_rng(6000)
    extra = rng.choice(leaf_ids, (3000, 2))
    e += [(a, b) for a, b in extra if a != b]
    r, c = np.array([a for a, b in e]), np.array([b for a, b in e])
    A = ssp.csr_matrix((np.ones(2 * len(e)), (np.r_[r, c], np.r_[c, r])), shape=(n, n))
    A.data[:] = 1.0
    return A


@pytest.fixture(scope="module")
def hub(eps, dev):
    from eps_amd import filter_stage
    A = _hub_graph()
    n = A.shape[0]
    g_unit, g_val = _graphs(eps, A)
    cu, cv, cc = lit.two_hop_candidates(A)
    per_col = np.bincount(cv, minlength=n)
    assert per_col[0] > 5000 and np.all(per_col[100:400] == 0)
    blocks = {"f32 exact": (g_unit, filter_stage._counted_block(g_unit, 0, n, False)),
              "f32 padded": (g_unit, filter_stage._counted_block(g_unit, 0, n, True)),
              "i32 padded": (g_val, filter_stage._counted_block(g_val, 0, n, True))}
    return A, (cu, cv, cc), blocks


@pytest.mark.parametrize("name", ["jaccard", "salton", "pa"])
@pytest.mark.parametrize("which", ["f32 exact", "f32 padded", "i32 padded"])
def test_survivors(eps, dev, hub, name, which):
    A, (cu, cv, cc), blocks = hub
    n = A.shape[0]
    g, blk = blocks[which]
    pos, _ = _live(blk)
    assert blk.cand_u.numel() > len(pos) or blk.counts is None
    deg = lit.degrees(A)
    kw = dict(counts=blk.counts)
    args = (g.rowptr, n, 0, n, blk.colptr, blk.cand_u, blk.cn, name)
    full = torch.full((blk.cand_u.numel(),), float("-inf"), dtype=torch.float32, device=dev)      # (padding never exceeds a bar)
    eps.ops.local_index_columns(*args, out=full, **kw)
    lit.assert_within_one_ulp(full.cpu().numpy()[pos], lit.index_scores(name, cc, deg[cu], deg[cv]), f"{name} {which}")
    live = full[torch.from_numpy(pos).to(dev)]
    lo, hi = float(live.min()), float(live.max())
    mid = float(live.sort().values[len(pos) // 2])
    assert lo < mid < hi and int((live == mid).sum()) >= 1
    for bar in (np.nextafter(np.float32(lo), np.float32(-np.inf)).item(), hi, mid):
        want_pos = torch.nonzero(full > bar).squeeze(1)
        m = want_pos.numel()
        assert m == {hi: 0}.get(bar, m) and (bar != mid or 0 < m < len(pos)) and (bar >= lo or m == len(pos))
        st = {}
        got = eps.ops.local_index_columns(*args, bar=bar, capacity=m, stats=st, **kw)
        assert st["n_surv"] == m and got is not None
        assert torch.equal(got[0], want_pos) and torch.equal(got[1], full[want_pos]), (name, which, bar)
        again = eps.ops.local_index_columns(*args, bar=torch.tensor([bar], dtype=torch.float32, device=dev), capacity=m + 7, **kw)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))
        if m > 0:
            st = {}
            assert eps.ops.local_index_columns(*args, bar=bar, capacity=m - 1, stats=st, **kw) is None and st["n_surv"] == m
        if m > 1:
            st = {}
            assert eps.ops.local_index_columns(*args, bar=bar, capacity=1, stats=st, **kw) is None and st["n_surv"] == m
    # scores and survivors out of one call: the same bits in both
    out = torch.full_like(full, float("-inf"))
    got = eps.ops.local_index_columns(*args, bar=mid, capacity=len(pos), out=out, **kw)
    assert torch.equal(out.view(torch.int32), full.view(torch.int32)) and torch.equal(got[0], torch.nonzero(full > mid).squeeze(1))

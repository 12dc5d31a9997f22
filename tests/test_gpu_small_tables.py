"""Three small kernels that the suite only ever handed bad arguments (tests/test_gpu_ops_call.py, tests/test_katz_host.py), each
against the model its own comment states, in numpy / torch, exactly:

  ops.two_path_counts     paths[x] = sum over the entries w of row x of the length of row w   (csrc/katz_pairs.hip; a wrong
                          value only changes the end Katz expands a pair from -- no end-to-end result shows it)
  ops.row_window_splits   splits[k * N + w] = entries of row w below id (k + 1) * win_ids     (csrc/filter_scan.hip)
  ops.compact_at_least    the slots with key >= 0 and score >= *cut, in any order; a NULL cut keeps every survivor
                          (csrc/topk_select.hip; ops.compact_between, the same kernel with an upper end, its chunk edges and
                          its second grid-stride trip: tests/test_gpu_shard_kernels.py)"""
import numpy as np
import pytest
import torch

import weighted_truth as W

pytestmark = pytest.mark.gpu


def _csr(n, r, c):
    """(rowptr, col) of the directed pattern with the distinct entries (r, c); rows sorted."""
    key = np.unique(np.asarray(r, np.int64) * n + np.asarray(c, np.int64))
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(key // n, minlength=n), out=rowptr[1:])
    return rowptr, key % n


def _up(dev, rowptr, col):
    return torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(dev)


def _cus(eps, dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == eps.ops.device_info()[0]
    return cus


# ------------------------------------------------------------------------------------------------- two_path_counts
def _two_path_graphs(eps, dev, name):
    from eps_amd import synth
    rng = np.random.default_rng(5)
    if name == "rmat11":
        n, lo, hi = W.patterns(synth)["rmat11"]
        return _csr(n, np.concatenate([lo, hi]), np.concatenate([hi, lo]))
    if name == "empty_rows":                          # 40 edges among 500 nodes: most rows are empty, the last one too
        r, c = rng.integers(0, 499, 40), rng.integers(0, 499, 40)
        return _csr(500, np.concatenate([r, c]), np.concatenate([c, r]))
    if name in ("asymmetric", "asymmetric_transposed"):
        r, c = rng.integers(0, 700, 6000), rng.integers(0, 700, 6000) ** 2 // 700          # (skewed columns: in- and out-degrees differ)
        return _csr(700, c, r) if name.endswith("transposed") else _csr(700, r, c)
    if name == "no_nodes":
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    assert name == "ring"                             # more nodes than the grid has threads: every thread takes a second node
    n = 256 * 16 * _cus(eps, dev) + 1000
    i = np.arange(n, dtype=np.int64)
    nb = np.sort(np.stack([(i - 1) % n, (i + 1) % n], 1), 1)
    return 2 * np.arange(n + 1, dtype=np.int64), nb.reshape(-1)


@pytest.mark.parametrize("name", ("rmat11", "empty_rows", "asymmetric", "asymmetric_transposed", "no_nodes", "ring"))
def test_two_path_counts(eps, dev, name):
    rowptr, col = _two_path_graphs(eps, dev, name)
    n, deg = len(rowptr) - 1, np.diff(rowptr)
    want = np.zeros(n, np.int64)
    np.add.at(want, np.repeat(np.arange(n, dtype=np.int64), deg), deg[col])
    got = eps.ops.two_path_counts(*_up(dev, rowptr, col))
    assert got.dtype == torch.int64 and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), want)
    if name == "ring":
        assert n > 256 * 16 * _cus(eps, dev) and (want == 4).all()
    if name == "empty_rows":
        assert (deg == 0).sum() > 400 and deg[-1] == 0 and want.any()
    if name.startswith("asymmetric"):
        other, _ = _two_path_graphs(eps, dev, "asymmetric" if name.endswith("transposed") else "asymmetric_transposed")
        assert not np.array_equal(np.diff(other), deg) and np.diff(other).sum() == deg.sum()


# ------------------------------------------------------------------------------------------------- row_window_splits
def _splits_truth(rowptr, col, win_ids, n_win):
    n = len(rowptr) - 1
    bounds = (np.arange(n_win - 1, dtype=np.int64) + 1) * win_ids
    out = np.zeros((n_win - 1, n), np.int64)
    for w in range(n):
        out[:, w] = np.searchsorted(col[rowptr[w]:rowptr[w + 1]], bounds, side="left")
    return out.reshape(-1)


def _special_rows(n, win_ids, n_win):
    """A directed pattern over n ids: random rows, and rows 0 .. 3 = every entry in the last window, entries exactly at the
    window boundaries (and one id either side), no entry at all, every id."""
    rng = np.random.default_rng(win_ids)
    r, c = rng.integers(4, n, 8 * n), rng.integers(0, n, 8 * n)
    last = min((n_win - 1) * win_ids, n - 1)
    row0 = np.arange(last, n)
    edge = (np.arange(n_win - 1) + 1) * win_ids
    row1 = np.concatenate([edge, edge - 1, edge + 1])
    row1 = row1[(row1 >= 0) & (row1 < n)]
    row3 = np.arange(n)
    r = np.concatenate([r, np.zeros(len(row0), np.int64), np.ones(len(row1), np.int64), np.full(n, 3)])
    c = np.concatenate([c, row0, row1, row3])
    rowptr, col = _csr(n, r, c)
    assert rowptr[3] == rowptr[2] and len(row1)
    return rowptr, col


@pytest.mark.parametrize("win_ids,n_win", ((32, 2), (100, 7), (1, 720)))
def test_row_window_splits(eps, dev, win_ids, n_win):
    n = 720
    rowptr, col = _special_rows(n, win_ids, n_win)
    got = eps.ops.row_window_splits(*_up(dev, rowptr, col), win_ids, n_win)
    want = _splits_truth(rowptr, col, win_ids, n_win)
    assert got.dtype == torch.int32 and got.shape == ((n_win - 1) * n,)
    assert np.array_equal(got.cpu().numpy(), want)
    by_window = want.reshape(n_win - 1, n)
    assert not by_window[:, 2].any() and (by_window[:, 0] == 0).all()                   # the empty row; nothing below the last window
    assert np.array_equal(by_window[:, 3], np.minimum((np.arange(n_win - 1) + 1) * win_ids, n))
    assert (np.diff(by_window, axis=0) >= 0).all()
    assert eps.ops.row_window_splits(*_up(dev, rowptr, col), n, 1) is None


def test_row_window_splits_of_a_wide_id_space(eps, dev):
    """The windows eps_filter_scan really uses, on the 1.3 M-node graph of test_scan_wide_id_space_in_windows."""
    from eps_amd import synth
    n = 1_300_000
    g = synth.rmat_graph(21, 1, 13, dev, n_nodes=n)
    win_ids, n_win = eps.ops.filter_scan_windows(n)
    assert n_win >= 2 and win_ids * n_win >= n
    got = eps.ops.row_window_splits(g.rowptr, g.col, win_ids, n_win).cpu().numpy().reshape(n_win - 1, n)
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy().astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    assert (np.diff(row * n + col) > 0).all()                          # rows ascend: "below the boundary" is a prefix of the row
    for k in range(n_win - 1):
        assert np.array_equal(got[k], np.bincount(row[col < (k + 1) * win_ids], minlength=n)), k
    assert 0 < got[0].sum() < len(col)


# ------------------------------------------------------------------------------------------------- compact_at_least
LEVELS = np.array([-2.5, 0.0, 0.25, 1.0, 1.0 + 2.0 ** -23, 7.0], np.float32)


@pytest.mark.parametrize("n", (0, 1, 255, 256, 100_003))
def test_compact_at_least(eps, dev, n):
    rng = np.random.default_rng(n)
    keys = rng.permutation(n).astype(np.int64) + (np.int64(1) << 33) * (np.arange(n) % 3 == 1)          # (distinct, some beyond 32 bits)
    vals = LEVELS[rng.integers(0, len(LEVELS), n)]
    dead = rng.random(n) < 1 / 3
    keys[dead], vals[dead] = -1, -np.inf
    if n > 100:
        keys[5], vals[5] = -1, 7.0                    # an untouched key with a stale score of the highest level: still no survivor
        keys[6], vals[6] = n + 10, -np.inf            # a survivor that scores -inf: kept under no cut and under a cut of -inf
        vals[7] = 7.0
    d_keys, d_vals = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)
    top = float(vals[keys >= 0].max()) if (keys >= 0).any() else 0.0
    for cut in (None, float("-inf"), float("inf"), top, 1.0, 0.25, float(np.float32(1.0 + 2.0 ** -23)), 0.5):
        d_cut = None if cut is None else torch.tensor([cut], dtype=torch.float32, device=dev)
        out_k, out_v, n_out = eps.ops.compact_at_least(d_keys, d_vals, d_cut)
        keep = (d_keys >= 0) if cut is None else (d_keys >= 0) & (d_vals >= d_cut)
        m = int(n_out)
        assert n_out.dtype == torch.int64 and m == int(keep.sum()), cut
        got_k, got_v = out_k[:m].cpu().numpy(), out_v[:m].cpu().numpy()
        assert (got_k >= 0).all()
        o, w = np.argsort(got_k), np.argsort(keys[keep.cpu().numpy()])
        assert np.array_equal(got_k[o], keys[keep.cpu().numpy()][w]), cut                      # (the keys are distinct: the multiset is the sorted list)
        assert np.array_equal(got_v[o].view(np.int32), vals[keep.cpu().numpy()][w].view(np.int32)), cut
        if cut == float("inf"):
            assert m == 0
        if cut in (None, float("-inf")) and n:
            assert m == int((keys >= 0).sum())
        if n > 100 and cut == top:
            assert 0 < m < int((keys >= 0).sum()) and (got_v == np.float32(top)).all()        # many tie at the cut

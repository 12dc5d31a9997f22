"""GPU: adding proposal edges to a resident graph by the HIP merge (eps_csr_merge_count / _fill, CSRGraph.with_edges,
add_edges(..., base=)) against the yardstick -- add_edges WITHOUT ``base``, the rebuild from the concatenated edge list.

Exact equality throughout: rowptr and col are integers, and every weight here is a whole number (as collab's are), so each
float32 sum stays below 2**24 and is exact whatever order the rebuild's float atomics arrive in."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _same(got, want):
    assert torch.equal(got.rowptr, want.rowptr)
    assert torch.equal(got.col, want.col)
    assert (got.val is None) == (want.val is None)
    if want.val is not None:
        assert torch.equal(got.val, want.val)
    assert got.sparse_sizes() == want.sparse_sizes()


def _both_routes(eps, dataset, ei, ew, extra, n):
    """(merge route, rebuild) of one batch; the merge route twice -- through add_edges(base=) and through with_edges."""
    base = eps.add_edges(dataset, ei, ew, ei.new_zeros((2, 0)), n)
    want = eps.add_edges(dataset, ei, ew, extra, n)
    got = eps.add_edges(dataset, ei, ew, extra, n, base=base)
    _same(got, want)
    again = base.with_edges(extra, dataset == "collab")
    _same(again, want)
    assert got.uid != base.uid and again.uid != got.uid and not got._cache
    return base, got, want


# ---------------------------------------------------------------------------------------------------------------- N = 50
N50 = 50


def _graph50(dev):
    """Random weighted edge list on nodes 0..39 plus (49, 0): rows 40..48 are empty, row N - 1 is not."""
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, 40, (2, 150), generator=gen)
    ei = torch.cat([ei, torch.tensor([[49], [0]])], 1)
    ew = torch.randint(1, 6, (ei.shape[1],), generator=gen).float()
    return ei.to(dev), ew.to(dev)


def _extras50(ei):
    gen = torch.Generator().manual_seed(12)
    rnd = torch.randint(0, N50, (2, 40), generator=gen)
    special = torch.tensor([[7, 7, 7, 12, 30, 3, 3, 44, 41, 5, 49, 2, 49, 49],
                            [30, 30, 30, 30, 12, 3, 3, 44, 5, 42, 3, 49, 49, 48]])
    # (7, 30) three times; one pair in both orientations, (12, 30) and (30, 12); the self pair (3, 3) twice and (44, 44) on an
    # empty row; (41, 5) and (5, 42) touch empty rows; (49, 3), (2, 49), (49, 49), (49, 48) touch row N - 1
    already = ei[:, :12].cpu()                                  # pairs the graph holds
    return torch.cat([rnd, special, already, already[:, :4].flip(0)], 1).to(ei.device)


@pytest.mark.parametrize("dataset", ["collab", "ddi"])
def test_n50_every_kind_of_extra(eps, dev, dataset):
    ei, ew = _graph50(dev)
    extra = _extras50(ei)
    base, got, _ = _both_routes(eps, dataset, ei, ew, extra, N50)
    assert int(base.degree()[41]) == 0 and int(got.degree()[41]) > 0 and int(got.degree()[N50 - 1]) > int(base.degree()[N50 - 1])
    assert (got.val is not None) == (dataset == "collab")


@pytest.mark.parametrize("dataset", ["collab", "ddi"])
def test_n50_against_scipy(eps, dev, dataset):
    """The same result restated without torch: coo_matrix of the concatenated list, A + A.T, duplicates summed."""
    import scipy.sparse as ssp
    ei, ew = _graph50(dev)
    extra = _extras50(ei)
    base = eps.add_edges(dataset, ei, ew, ei.new_zeros((2, 0)), N50)
    got = base.with_edges(extra, dataset == "collab")
    rows = np.concatenate([ei[0].cpu().numpy(), extra[0].cpu().numpy()])
    cols = np.concatenate([ei[1].cpu().numpy(), extra[1].cpu().numpy()])
    w = np.concatenate([ew.cpu().numpy().astype(np.float64), np.ones(extra.shape[1])])
    A = ssp.coo_matrix((w, (rows, cols)), shape=(N50, N50)).tocsr()
    S = (A + A.T).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    assert np.array_equal(got.rowptr.cpu().numpy(), S.indptr.astype(np.int64))
    assert np.array_equal(got.col.cpu().numpy(), S.indices.astype(np.int32))
    if dataset == "collab":
        assert got.val is not None and np.array_equal(got.val.cpu().numpy().astype(np.float64), S.data)
    else:
        assert got.val is None


def test_empty_batch_returns_the_base(eps, dev):
    ei, ew = _graph50(dev)
    for dataset in ("collab", "ddi"):
        base = eps.add_edges(dataset, ei, ew, ei.new_zeros((2, 0)), N50)
        got = base.with_edges(ei.new_zeros((2, 0)), dataset == "collab")
        _same(got, base)
        assert got.uid != base.uid
    rp, c, v = eps.ops.csr_merge(base.rowptr, base.col, None, N50, torch.zeros(0, dtype=torch.int64, device=dev), False)
    assert torch.equal(rp, base.rowptr) and torch.equal(c, base.col) and v is None


def test_same_inputs_same_bits(eps, dev):
    ei, ew = _graph50(dev)
    extra = _extras50(ei)
    base = eps.add_edges("collab", ei, ew, ei.new_zeros((2, 0)), N50)
    a, b = base.with_edges(extra, True), base.with_edges(extra, True)
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
    assert torch.equal(a.val.view(torch.int32), b.val.view(torch.int32))


def test_chaining_equals_one_batch(eps, dev):
    ei, ew = _graph50(dev)
    extra = _extras50(ei)
    a, b = extra[:, :30], extra[:, 30:]
    base = eps.add_edges("ddi", ei, ew, ei.new_zeros((2, 0)), N50)
    _same(base.with_edges(a, False).with_edges(b, False), base.with_edges(torch.cat([a, b], 1), False))


def test_bad_batches_raise(eps, dev):
    ei, ew = _graph50(dev)
    base = eps.add_edges("ddi", ei, ew, ei.new_zeros((2, 0)), N50)
    for bad in ([[3], [N50]], [[N50], [3]], [[3, 4], [5, -1]]):
        with pytest.raises(eps.EpsError, match="outside"):
            base.with_edges(torch.tensor(bad, device=dev), False)
    keys = torch.tensor([(5 << 32) | 3, (2 << 32) | 9, (9 << 32) | 2], dtype=torch.int64, device=dev)
    with pytest.raises(eps.EpsError, match="sorted"):
        eps.ops.csr_merge(base.rowptr, base.col, None, N50, keys, False)
    with pytest.raises(eps.EpsError):
        eps.ops.csr_merge(base.rowptr, base.col, None, N50, keys.cpu(), False)
    ok = eps.ops.csr_merge(base.rowptr, base.col, None, N50, torch.sort(keys).values, False)       # (the same keys, sorted)
    assert ok[0][-1] == ok[1].numel()


# --------------------------------------------------------------------------------------------------- a hub and empty rows
N_STAR = 3000


@pytest.fixture(scope="module")
def star(dev):
    """Node 0 is joined to 1..2000 (a row far longer than 1024), noise among 1..2899; rows 2900.. are empty."""
    gen = torch.Generator().manual_seed(21)
    hub = torch.stack([torch.zeros(2000, dtype=torch.int64), torch.arange(1, 2001)])
    noise = torch.randint(1, 2900, (2, 6000), generator=gen)
    ei = torch.cat([hub, noise], 1)
    ew = torch.randint(1, 4, (ei.shape[1],), generator=gen).float()
    return ei.to(dev), ew.to(dev)


def _star_batches():
    z = torch.zeros
    return {
        "hub70": torch.stack([z(70, dtype=torch.int64), torch.arange(1966, 2036)]),                 # half of them present
        "hub1500": torch.stack([torch.arange(1500, 3000), z(1500, dtype=torch.int64)]),             # hub as the SECOND end
        "empty70": torch.stack([torch.full((70,), 2950), torch.cat([torch.arange(0, 60), torch.arange(2940, 2950)])]),
        "all_present": torch.stack([z(64, dtype=torch.int64), torch.arange(1, 65)]),
    }


@pytest.mark.parametrize("dataset", ["collab", "ddi"])
@pytest.mark.parametrize("batch", sorted(_star_batches()))
def test_star_hub_and_empty_rows(eps, dev, star, dataset, batch):
    ei, ew = star
    extra = _star_batches()[batch].to(dev)
    base, got, _ = _both_routes(eps, dataset, ei, ew, extra, N_STAR)
    assert int(base.degree()[0]) >= 2000 and int(base.degree()[2950]) == 0
    if batch == "all_present":
        assert torch.equal(got.rowptr, base.rowptr)
    if batch == "hub1500":
        assert int(got.degree()[0]) - int(base.degree()[0]) == 999               # 2001..2999 are new to the hub


# ---------------------------------------------------------------------------------------------------------------- R-MAT
@pytest.mark.parametrize("dataset", ["collab", "ddi"])
def test_rmat_20k_extras(eps, dev, dataset):
    from eps_amd import synth
    g = synth.rmat_graph(12, 8, 5, dev)
    n = g.n_rows
    row, col, _ = g.coo()
    ei = torch.stack([row, col])
    gen = torch.Generator(device=dev).manual_seed(6)
    ew = torch.randint(1, 4, (ei.shape[1],), generator=gen, device=dev).float()
    extra = torch.randint(0, n, (2, 20_000), generator=gen, device=dev)
    extra[:, :2000] = ei[:, torch.randint(0, ei.shape[1], (2000,), generator=gen, device=dev)]      # a tenth are stored pairs
    _both_routes(eps, dataset, ei, ew, extra, n)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_rank_cli_with_and_without_the_merge(eps, dev, tmp_path, monkeypatch, capsys):
    """rank.py --model adamic_ogb over a sweep of three points on the ddi stand-in: the default route (base graph once,
    proposals merged per point) and --no_incremental_graph print and save the same curve points."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.02")
    from eps_amd import filter_stage, rank_stage
    filter_stage.main(["--dataset", "ddi", "--model", "adamic_ogb", "--checkpoint", "ddi_adamic_ogb||0|0.pt", "--synthetic"])
    capsys.readouterr()
    curves, printed, saved = {}, {}, {}
    for name, flags in (("merge", []), ("rebuild", ["--no_incremental_graph"])):
        torch.manual_seed(3)
        curves[name] = rank_stage.main(["--dataset", "ddi", "--model", "adamic_ogb", "--sorted_edge_path",
                                        "ddi_adamic_ogb__0_0_sorted_edges.pt", "--sweep_num", "2", "--sweep_min", "0",
                                        "--sweep_max", "200", "--runs", "1", "--synthetic", "--out_name", name] + flags)
        printed[name] = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[")]
        files = sorted(glob.glob(os.path.join("curves", name + "|*.pt")), key=lambda f: int(os.path.basename(f).split("|")[2]))
        saved[name] = [torch.load(f) for f in files]
    assert [c[0] for c in curves["merge"]] == [0, 100, 200]
    assert len(printed["merge"]) == 3 and printed["merge"] == printed["rebuild"]
    for a, b in ((curves["merge"], curves["rebuild"]), (saved["merge"], saved["rebuild"]), (saved["merge"], curves["merge"])):
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            assert x[0] == y[0] and float(x[1]) == float(y[1]) and float(x[2]) == float(y[2])

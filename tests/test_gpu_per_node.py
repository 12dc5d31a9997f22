"""GPU: the per-node cut -- eps_segment_topk alone against the host restatement (tests/per_node_cases.py; positions exactly
equal), and filter.py --keep_per_node k through the command line against "the first k rows per v" of the whole file the same
build writes without the flag (bit for bit), for heuristic, GNN and cosine filters."""
import os

import numpy as np
import pytest
import torch

import per_node_cases as cases

pytestmark = pytest.mark.gpu

KS = (1, 2, 64, 65, 300)


def _lengths(eps):
    base = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 70000]
    for edge in (eps.ops.SEGMENT_TOPK_WAVE_MAX, eps.ops.SEGMENT_TOPK_LDS_MAX):
        base += [edge - 1, edge, edge + 1]
    lens = np.array(sorted(set(base)) + [0, 3, 300, 64], np.int64)      # (a few repeats: two empty segments, two of one class in a row)
    # shuffled, then interleaved short / long so that neighbours differ in class
    rng = np.random.default_rng(11)
    lens = lens[rng.permutation(len(lens))]
    order = np.argsort(lens, kind="stable")
    half = (len(order) + 1) // 2
    mixed = np.empty_like(order)
    mixed[0::2], mixed[1::2] = order[:half], order[half:][::-1]
    return lens[mixed]


def _scores(pattern, n, rng):
    if pattern == "distinct":
        return rng.permutation(n).astype(np.float32) * np.float32(0.37) - np.float32(1000.0)     # distinct float32 values
    if pattern == "small_ints":
        return rng.integers(0, 4, n).astype(np.float32)
    if pattern == "all_equal":
        return np.full(n, 2.5, np.float32)
    pool = np.array([np.inf, -np.inf, 0.0, -0.0, 1.5, -2.0, 3.25, 1e-30, -1e-30], np.float32)
    x = pool[rng.integers(0, len(pool), n)]
    some = rng.random(n) < 0.3
    x[some] = rng.standard_normal(int(some.sum())).astype(np.float32)
    return x


def _layout(lens, pattern, rng, padded):
    """(colptr, counts | None, score): segments of ``lens`` entries; ``padded``: each in a room 0..40 entries wider, the padding
    +inf -- a kernel that reads past ``counts`` selects padding."""
    room = lens + (rng.integers(0, 41, len(lens)) if padded else 0)
    colptr = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    score = np.full(int(colptr[-1]), np.inf, np.float32)
    for s, n in enumerate(lens):
        score[colptr[s]:colptr[s] + n] = _scores(pattern, int(n), rng)
    return colptr, (lens.copy() if padded else None), score


def _run(eps, dev, colptr, counts, score, k):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)      # noqa: E731
    return eps.ops.segment_topk(t(colptr), t(score), k, counts=t(counts)).cpu().numpy()


@pytest.mark.parametrize("pattern", ["distinct", "small_ints", "all_equal", "specials"])
def test_segment_topk_against_the_host_restatement(eps, dev, pattern):
    rng = np.random.default_rng(5)
    lens = _lengths(eps)
    colptr, counts, score = _layout(lens, pattern, rng, padded=True)
    # the same segments in reverse order (another hand-out, other neighbours), same padding per segment
    room = np.diff(colptr)
    r_colptr = np.concatenate([[0], np.cumsum(room[::-1])]).astype(np.int64)
    r_score = np.concatenate([score[colptr[s]:colptr[s + 1]] for s in range(len(lens))][::-1]) if len(lens) else score
    # the plain layout (no counts): the same data without the padding
    p_colptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p_score = np.concatenate([score[colptr[s]:colptr[s] + lens[s]] for s in range(len(lens))])
    for k in KS:
        want = cases.segment_topk_ref(colptr, score, k, counts)
        got = _run(eps, dev, colptr, counts, score, k)
        assert got.dtype == np.int64 and np.array_equal(got, want), (pattern, k)
        assert np.array_equal(_run(eps, dev, colptr, counts, score, k), got), "the same call twice"
        rev = _run(eps, dev, r_colptr, counts[::-1].copy(), r_score, k)
        kept = np.minimum(lens, k)
        outptr, r_outptr = np.concatenate([[0], np.cumsum(kept)]), np.concatenate([[0], np.cumsum(kept[::-1])])
        n = len(lens)
        for s in range(n):
            back = rev[r_outptr[n - 1 - s]:r_outptr[n - s]] - r_colptr[n - 1 - s] + colptr[s]
            assert np.array_equal(back, got[outptr[s]:outptr[s + 1]]), (pattern, k, s)
        assert np.array_equal(_run(eps, dev, p_colptr, None, p_score, k), cases.segment_topk_ref(p_colptr, p_score, k)), (pattern, k)


def test_segment_topk_edges(eps, dev):
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    assert eps.ops.segment_topk(z, torch.zeros(0, device=dev), 3).numel() == 0                  # no segment
    colptr = torch.tensor([0, 0, 0], dtype=torch.int64, device=dev)
    assert eps.ops.segment_topk(colptr, torch.zeros(0, device=dev), 3).numel() == 0             # empty segments only
    with pytest.raises(eps.EpsError, match="k=0"):
        eps.ops.segment_topk(colptr, torch.zeros(0, device=dev), 0)
    with pytest.raises(eps.EpsError, match="span"):
        eps.ops.segment_topk(torch.tensor([0, 9], dtype=torch.int64, device=dev), torch.zeros(4, device=dev), 2)
    with pytest.raises(eps.EpsError, match="int64"):
        eps.ops.segment_topk(colptr.to(torch.int32), torch.zeros(0, device=dev), 2)


# ---- through the command line -------------------------------------------------------------------------------------------
@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", "0.004")
    return tmp_path


def _cli(argv, run, *extra):
    from eps_amd import filter_stage
    argv = list(argv)
    at = argv.index("--checkpoint") + 1
    argv[at] = argv[at].replace("|0.pt", f"|{run}.pt")
    return torch.load(filter_stage.main(argv + list(extra)))


def _check_per_node(argv, ks=(1, 7), keep_top=500):
    whole = _cli(argv, 0)
    assert whole.shape[0] > 1000
    for k in ks:
        want = cases.first_k_rows_per_v(whole, k)
        assert 0 < want.shape[0] < whole.shape[0]
        got = _cli(argv, k, "--keep_per_node", str(k))
        assert got.dtype == torch.float32 and torch.equal(got, want), f"k = {k}"
        if keep_top:
            top = _cli(argv, 100 + k, "--keep_per_node", str(k), "--keep_top", str(keep_top))
            assert torch.equal(top, want[:keep_top]), f"k = {k} with --keep_top {keep_top}"
    return whole


@pytest.mark.parametrize("dataset,model", [("ppa", "adamic_ogb"), ("ppa", "simple"), ("ppa", "resource_allocation"),
                                           ("collab", "adamic_ogb"), ("collab", "simple")])
def test_cli_matches_first_k_rows_per_node(eps, dev, workdir, dataset, model):
    argv = ["--dataset", dataset, "--model", model, "--checkpoint", f"{dataset}_{model}||0|0.pt", "--synthetic"]
    whole = _check_per_node(argv)
    if (dataset, model) == ("ppa", "adamic_ogb"):
        # the stand-in reaches every work class: columns beyond the one-wave class and ties at the cut
        per_v = torch.bincount(whole[:, 1].long())
        assert int(per_v.max()) > eps.ops.SEGMENT_TOPK_WAVE_MAX and int(per_v.min()) < 7
        # ... and the file assembled from many blocks
        from eps_amd import candidates
        candidates.DEFAULT_BLOCK_PATHS = 20_000
        try:
            got = _cli(argv, 50, "--keep_per_node", "7")
        finally:
            candidates.DEFAULT_BLOCK_PATHS = (1 << 31) - 1
        assert torch.equal(got, cases.first_k_rows_per_v(whole, 7))


def test_cli_gcn_filter(eps, dev, workdir):
    """A GNN filter (list + decode; a pair tensor per block, its column pointers from a search of the v row)."""
    import argparse
    from eps_amd import datasets, models
    args = models.default_model_configs(argparse.Namespace(
        dataset="collab", model="gcn", synthetic=True, num_layers=None, hidden_channels=32, dropout=None,
        batch_size=None, lr=None, epochs=None, use_feature=None, use_learnable_embedding=None))
    _, _, _, data = datasets.get_data(args)
    torch.manual_seed(0)
    os.makedirs("models", exist_ok=True)
    sd = models.build_model(args, data, torch.device("cpu")).state_dict()
    for run in (0, 3):
        torch.save(sd, f"models/collab_gcn||0|{run}.pt")
    argv = ["--dataset", "collab", "--model", "gcn", "--checkpoint", "collab_gcn||0|0.pt", "--synthetic", "--hidden_channels", "32"]
    _check_per_node(argv, ks=(3,), keep_top=0)


def test_cli_simplecos_filter(eps, dev, workdir):
    """A cosine filter (signed fused expansion, sigmoid scores: saturated ties) on the ppa stand-in with features."""
    argv = ["--dataset", "ppa", "--model", "simplecos", "--checkpoint", "ppa_simplecos||0|0.pt", "--synthetic", "--use_feature", "True"]
    _check_per_node(argv, ks=(3,), keep_top=0)

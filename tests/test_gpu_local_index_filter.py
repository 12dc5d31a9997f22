"""GPU: filter.py / rank.py --model jaccard | salton | hdi | pa end to end on the scaled stand-ins (N = 943 / 426, the scale of the
Katz filter tests) -- the candidate set against the oracle's, every score against tests/local_index_truth.py to one float32 ulp,
the declared row order (score descending, then v, then u ascending: these indices tie a lot), and --keep_top (through the
kernel's survivor lists, and through their overflow) / --keep_per_node / proposal edges / two ranks against the full
single-process file, bit for bit.  On the parent of this change build_model refuses the names."""
import argparse

import numpy as np
import pytest
import torch

import local_index_truth as lit
from test_gpu_katz_filter import CASES, _graph, _stand_in

pytestmark = pytest.mark.gpu

MODELS = ("jaccard", "salton", "hdi", "pa")
_RUNS = {}


def _filter(dataset, model, run, *flags, checkpoint=None):
    from eps_amd import filter_stage
    return torch.load(filter_stage.main(["--dataset", dataset, "--model", model, "--checkpoint",
                                         checkpoint or f"{dataset}_{model}||0|{run}.pt", "--synthetic", *flags]))


def _check_file(rows, A, model, what):
    from oracle import eps_oracle
    n = A.shape[0]
    rows = rows.numpy()
    assert rows.dtype == np.float32 and rows.shape[1] == 3
    u, v, s = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2]
    want = eps_oracle.candidates_scipy(A)[0]
    keys = np.sort(v * n + u)
    assert np.array_equal(keys, np.sort(want[:, 1] * n + want[:, 0])), f"{what}: not the 2-hop non-edge set"
    lit.assert_within_one_ulp(s, lit.truth(A, u, v, model), what)
    # score descending, then v ascending, then u ascending -- by the file's own scores
    assert np.array_equal(np.lexsort((u, v, -s.astype(np.float64))), np.arange(len(s))), f"{what}: rows out of the declared order"
    assert len(np.unique(s)) < len(s), f"{what}: expected tied scores"


def _full(dataset, model, tmp_path_factory):
    if (dataset, model) not in _RUNS:
        workdir = tmp_path_factory.mktemp(f"li_{dataset}_{model}")
        with _stand_in(dataset, workdir):
            _RUNS[dataset, model] = (workdir, _filter(dataset, model, 0))
    return (dataset, model) + _RUNS[dataset, model]


@pytest.fixture(params=[(d, m) for d in sorted(CASES) for m in MODELS], ids=lambda p: f"{p[0]}-{p[1]}")
def full_run(request, eps, dev, oracle, tmp_path_factory):
    return _full(*request.param, tmp_path_factory)


def test_full_file_is_the_candidate_set_scored_and_ordered(full_run, oracle):
    dataset, model, workdir, rows = full_run
    with _stand_in(dataset, workdir):
        A = _graph(oracle, dataset)
    assert A.shape[0] == CASES[dataset][1] and rows.shape[0] == CASES[dataset][2]
    assert (dataset == "collab") == bool(np.any(A.data != 1.0))             # collab is weighted (int32 counts), ddi unit-valued (float32)
    _check_file(rows, A, model, f"{dataset} {model}")


def test_keep_top_is_the_head_of_the_full_file(full_run, monkeypatch):
    """Several column blocks, so that the later ones run against the streaming top-K's bar: the kernel's survivor lists -- and,
    with a capacity of 8, their overflow and the block scored in full instead."""
    from eps_amd import candidates, filter_stage
    dataset, model, workdir, rows = full_run
    monkeypatch.setattr(candidates, "DEFAULT_BLOCK_PATHS", 30_000)
    with _stand_in(dataset, workdir):
        top = _filter(dataset, model, 1, "--keep_top", "1000")
        cuts = [c[3] for c in filter_stage.LAST_LOCAL_INDEX_CUTS]
        assert len(cuts) >= 3 and cuts[0] == "scored" and "cut" in cuts
        monkeypatch.setattr(filter_stage, "CUT_CAPACITY", 8)
        small = _filter(dataset, model, 2, "--keep_top", "1000")
        assert len(filter_stage.LAST_LOCAL_INDEX_CUTS) == len(cuts)
    assert top.shape == (1000, 3) and torch.equal(top, rows[:1000])
    assert torch.equal(small, rows[:1000])


def test_keep_per_node_is_every_nodes_head_of_the_full_file(full_run):
    dataset, model, workdir, rows = full_run
    with _stand_in(dataset, workdir):
        cut = _filter(dataset, model, 3, "--keep_per_node", "3")
    v = rows[:, 1].numpy().astype(np.int64)
    order = np.argsort(v, kind="stable")                     # rows of one v, in the file's order
    start = np.r_[0, np.flatnonzero(np.diff(v[order])) + 1]
    rank = np.arange(len(v)) - np.repeat(start, np.diff(np.r_[start, len(v)]))
    keep = np.zeros(len(v), bool)
    keep[order[rank < 3]] = True
    assert 0 < keep.sum() < len(v) and torch.equal(cut, rows[torch.from_numpy(keep)])


def test_filter_on_a_graph_with_proposal_edges(eps, dev, oracle, tmp_path):
    """An AA filter run, then the jaccard filter on the graph with its 200 best proposals added: candidates and scores against
    the augmented SciPy matrix."""
    from eps_amd import filter_stage
    with _stand_in("collab", tmp_path):
        filter_stage.main(["--dataset", "collab", "--model", "adamic_ogb", "--checkpoint", "collab_adamic_ogb||0|0.pt",
                           "--synthetic"])
        rows = _filter("collab", "jaccard", 0, checkpoint="collab_jaccard|collab_adamic_ogb__0_0_sorted_edges|200|0.pt")
        props = torch.load("filtered_edges/collab_adamic_ogb__0_0_sorted_edges.pt")
        A = _graph(oracle, "collab", props[:200, :2].t().long().numpy())
        assert A.nnz > _graph(oracle, "collab").nnz
    _check_file(rows, A, "jaccard", "collab + 200 proposals")


def test_two_ranks_write_the_single_process_file(eps, dev, oracle, tmp_path_factory):
    """Column shards on two ranks (several blocks each), gathered in rank order and sorted: the same file, bit for bit."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _rank_main
    dataset, model, workdir, rows = _full("collab", "jaccard", tmp_path_factory)
    with _stand_in(dataset, workdir):
        argv = ["--dataset", dataset, "--model", model, "--checkpoint", f"{dataset}_{model}||0|4.pt", "--synthetic"]
        mp.spawn(_rank_main, args=(2, _free_port(), str(workdir), argv), nprocs=2, join=True)
        multi = torch.load(f"filtered_edges/{dataset}_{model}__0_4_sorted_edges.pt")
    assert torch.equal(multi, rows)


def test_rank_cli_and_module_forward(eps, dev, tmp_path, monkeypatch):
    """rank.py --model jaccard --dataset collab --synthetic --runs 1: one curve point with finite Hits in [0, 100]; the module's
    forward on the evaluation lists is heuristics.local_index, bit for bit."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("EPS_SYNTH_SCALE", CASES["collab"][0])
    from eps_amd import datasets, heuristics, models, rank_stage
    curves = rank_stage.main(["--dataset", "collab", "--model", "jaccard", "--synthetic", "--runs", "1"])
    assert len(curves) == 1 and int(curves[0][0]) == 0
    for x in curves[0][1:]:
        assert np.isfinite(float(x)) and 0.0 <= float(x) <= 100.0
    args = models.default_model_configs(argparse.Namespace(
        dataset="collab", model="jaccard", synthetic=True, num_layers=None, hidden_channels=None, dropout=None, batch_size=None,
        lr=None, epochs=None, use_feature=None, use_learnable_embedding=None))
    _, _, split_edge, data = datasets.get_data(args)
    data = data.to(dev)
    model = models.build_model(args, data, dev)
    assert sum(p.numel() for p in model.parameters()) == 0
    A = data.adj_t.to_scipy()
    for edges in (split_edge["valid"]["edge"], split_edge["valid"]["edge_neg"], split_edge["test"]["edge"]):
        e = edges.t().to(dev)
        out = model(data.x, e, data.adj_t)
        ref = heuristics.local_index(data.adj_t, e, "jaccard")
        assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), ref.view(torch.int32))
        en = edges.numpy()
        lit.assert_within_one_ulp(out.cpu().numpy(), lit.truth(A, en[:, 0], en[:, 1], "jaccard"), "module forward")

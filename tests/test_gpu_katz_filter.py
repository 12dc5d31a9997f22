"""GPU: filter.py --model katz end to end on the scaled stand-ins -- the candidate set, every score against the float64 truth
(test_katz_host.truncated_truth) to one float32 ulp, the declared row order, and --keep_top / --keep_per_node / proposal edges /
two ranks against the full single-process file, bit for bit.  (On the parent of this change the command crashed: the block
route handed the model's None to the streaming top-K.)"""
import argparse
import contextlib
import os

import numpy as np
import pytest
import torch

from test_gpu_katz import assert_within_one_ulp
from test_katz_host import truncated_truth

pytestmark = pytest.mark.gpu

COEFFS = (0.05, 0.005, 0.000125)
CASES = {"collab": ("0.004", 943, 64_734), "ddi": ("0.1", 426, 76_162)}     # EPS_SYNTH_SCALE, N, directed 2-hop non-edges
_RUNS = {}


@contextlib.contextmanager
def _stand_in(dataset, workdir):
    old_env, old_cwd = os.environ.get("EPS_SYNTH_SCALE"), os.getcwd()
    os.environ["EPS_SYNTH_SCALE"] = CASES[dataset][0]
    os.chdir(workdir)
    try:
        yield
    finally:
        os.chdir(old_cwd)
        if old_env is None:
            os.environ.pop("EPS_SYNTH_SCALE", None)
        else:
            os.environ["EPS_SYNTH_SCALE"] = old_env


def _filter(dataset, run, *flags, checkpoint=None):
    from eps_amd import filter_stage
    return torch.load(filter_stage.main(["--dataset", dataset, "--model", "katz", "--checkpoint",
                                         checkpoint or f"{dataset}_katz||0|{run}.pt", "--synthetic", *flags]))


def _graph(oracle, dataset, extra=None):
    """The SciPy adjacency the filter scores on (oracle.add_edges_scipy), as float64."""
    from eps_amd import datasets
    edge_index, edge_weight, _, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=False))
    extra = np.zeros((2, 0), np.int64) if extra is None else extra
    return oracle.add_edges_scipy(dataset, edge_index.numpy(), edge_weight.numpy(), extra, data.num_nodes).astype(np.float64)


def _check_file(rows, A, what):
    """Candidate set (both orientations), scores, and the declared order of a full [E,3] file against the SciPy matrix."""
    from oracle import eps_oracle
    n = A.shape[0]
    rows = rows.numpy()
    assert rows.dtype == np.float32 and rows.shape[1] == 3
    u, v, s = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2]
    want = eps_oracle.candidates_scipy(A)[0]
    keys = np.sort(v * n + u)
    assert np.array_equal(keys, np.sort(want[:, 1] * n + want[:, 0])), f"{what}: not the 2-hop non-edge set"
    assert np.array_equal(keys, np.sort(u * n + v)), f"{what}: an orientation is missing"
    assert_within_one_ulp(s, truncated_truth(A, np.stack([u, v], 1), COEFFS), what)
    # score descending, then v ascending, then u ascending
    assert np.array_equal(np.lexsort((u, v, -s.astype(np.float64))), np.arange(len(s))), f"{what}: rows out of the declared order"


def _full(dataset, tmp_path_factory):
    """(dataset, work directory, the full file of the bare command): one run per dataset, shared by the tests below."""
    if dataset not in _RUNS:
        workdir = tmp_path_factory.mktemp(f"katz_{dataset}")
        with _stand_in(dataset, workdir):
            _RUNS[dataset] = (workdir, _filter(dataset, 0))
    return (dataset,) + _RUNS[dataset]


@pytest.fixture(params=sorted(CASES))
def full_run(request, eps, dev, oracle, tmp_path_factory):
    return _full(request.param, tmp_path_factory)


def test_full_file_is_the_candidate_set_scored_and_ordered(full_run, oracle):
    dataset, workdir, rows = full_run
    with _stand_in(dataset, workdir):
        A = _graph(oracle, dataset)
    assert A.shape[0] == CASES[dataset][1] and rows.shape[0] == CASES[dataset][2]
    assert (dataset == "collab") == bool(np.any(A.data != 1.0))             # collab is weighted, ddi dense and unit-valued
    _check_file(rows, A, dataset)


def test_keep_top_is_the_head_of_the_full_file(full_run):
    dataset, workdir, rows = full_run
    with _stand_in(dataset, workdir):
        top = _filter(dataset, 1, "--keep_top", "1000")
    assert top.shape == (1000, 3) and torch.equal(top, rows[:1000])


def test_keep_per_node_is_every_nodes_head_of_the_full_file(full_run):
    dataset, workdir, rows = full_run
    with _stand_in(dataset, workdir):
        cut = _filter(dataset, 2, "--keep_per_node", "3")
    v = rows[:, 1].numpy().astype(np.int64)
    order = np.argsort(v, kind="stable")                     # rows of one v, in the file's order
    start = np.r_[0, np.flatnonzero(np.diff(v[order])) + 1]
    rank = np.arange(len(v)) - np.repeat(start, np.diff(np.r_[start, len(v)]))
    keep = np.zeros(len(v), bool)
    keep[order[rank < 3]] = True
    assert 0 < keep.sum() < len(v) and torch.equal(cut, rows[torch.from_numpy(keep)])


def test_katz_filter_on_a_graph_with_proposal_edges(eps, dev, oracle, tmp_path, monkeypatch):
    """An AA filter run, then the Katz filter on the graph with its 200 best proposals added: candidates and scores against the
    augmented SciPy matrix (built as test_gpu_katz.test_rank_cli_katz_matches_host_restatement builds it)."""
    from eps_amd import filter_stage
    with _stand_in("collab", tmp_path):
        filter_stage.main(["--dataset", "collab", "--model", "adamic_ogb", "--checkpoint", "collab_adamic_ogb||0|0.pt",
                           "--synthetic"])
        rows = _filter("collab", 0, checkpoint="collab_katz|collab_adamic_ogb__0_0_sorted_edges|200|0.pt")
        props = torch.load("filtered_edges/collab_adamic_ogb__0_0_sorted_edges.pt")
        A = _graph(oracle, "collab", props[:200, :2].t().long().numpy())
        assert A.nnz > _graph(oracle, "collab").nnz
    _check_file(rows, A, "collab + 200 proposals")


def test_two_ranks_write_the_single_process_file(eps, dev, tmp_path_factory):
    """Column shards on two ranks (several blocks each), gathered in rank order and sorted: the same file, bit for bit."""
    import torch.multiprocessing as mp
    from test_gpu_multirank import _free_port, _rank_main
    dataset, workdir, rows = _full("collab", tmp_path_factory)
    with _stand_in(dataset, workdir):
        argv = ["--dataset", dataset, "--model", "katz", "--checkpoint", f"{dataset}_katz||0|3.pt", "--synthetic"]
        mp.spawn(_rank_main, args=(2, _free_port(), str(workdir), argv), nprocs=2, join=True)
        multi = torch.load(f"filtered_edges/{dataset}_katz__0_3_sorted_edges.pt")
    assert torch.equal(multi, rows)

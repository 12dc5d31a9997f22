"""CPU: the host side of filter.py --keep_per_node k -- the flag and its refusals (raised before the dataset is read), the ABI
surface of csrc/segment_topk.hip and its domain errors (which return before any pointer is touched), and the host restatement
the GPU tests compare against (tests/per_node_cases.py), held to a brute-force lexsort."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import per_node_cases as cases


def _args(*extra):
    from eps_amd import filter_stage, models
    argv = ["--dataset", "collab", "--checkpoint", "x||0|0.pt", "--synthetic"] + list(extra)
    return models.default_model_configs(filter_stage.make_parser().parse_args(argv))


def _check(args):
    from eps_amd import filter_stage
    filter_stage.check_per_node_args(args)
    filter_stage.check_decode_args(args)


def test_parser_flag_and_default():
    bare = _args("--model", "adamic_ogb")
    assert bare.keep_per_node == 0
    _check(bare)
    for model in ("adamic_ogb", "gcn"):
        a = _args("--model", model, "--keep_per_node", "5")
        assert a.keep_per_node == 5
        _check(a)
    _check(_args("--model", "simple", "--keep_per_node", "5", "--keep_top", "100"))


@pytest.mark.parametrize("extra,match", [
    (["--model", "adamic_ogb", "--keep_per_node", "-3"], r"--keep_per_node -3"),
    (["--model", "gcn", "--keep_per_node", "4", "--keep_top", "100", "--decode_precision", "bf16"], r"--keep_per_node 4 with --decode_precision bf16"),
    (["--model", "gcn", "--keep_per_node", "4", "--decode_precision", "bf16"], r"--keep_per_node 4 with --decode_precision bf16"),
])
def test_refusals_name_the_value_before_the_dataset_is_read(monkeypatch, extra, match):
    from eps_amd import filter_stage

    def boom(*a, **k):
        raise AssertionError("the dataset was read")
    monkeypatch.setattr(filter_stage, "get_data", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    with pytest.raises(ValueError, match=match):
        filter_stage.main(["--dataset", "collab", "--checkpoint", "x||0|0.pt", "--synthetic"] + extra)


def test_exports_and_version(eps):
    lib = eps.load()
    for name in ("eps_segment_topk", "eps_segment_topk_class_max"):
        assert name in eps._lib.SIGNATURES and hasattr(lib, name)
    assert lib.eps_version() == 7
    assert "segment_topk.hip" in open(os.path.join(ROOT, "edge-proposal-sets_amd", "csrc", "Makefile")).read()
    assert callable(eps.ops.segment_topk)
    # the class boundaries ops shows are the library's
    assert lib.eps_segment_topk_class_max(0) == eps.ops.SEGMENT_TOPK_WAVE_MAX
    assert lib.eps_segment_topk_class_max(1) == eps.ops.SEGMENT_TOPK_LDS_MAX
    assert lib.eps_segment_topk_class_max(2) == -1
    assert 64 <= eps.ops.SEGMENT_TOPK_WAVE_MAX < eps.ops.SEGMENT_TOPK_LDS_MAX


def test_domain_errors_without_gpu(eps):
    """k <= 0 and n_seg < 0 return EPS_EINVAL with the value named, before any pointer is touched (the pointers here are not
    device memory); n_seg == 0 launches nothing."""
    import ctypes
    lib = eps.load()
    one = ctypes.c_void_p(8)
    for k in (0, -3):
        assert lib.eps_segment_topk(one, None, one, 5, k, one, None, one, None) == -1
        assert f"eps_segment_topk: k={k} " in lib.eps_last_error().decode()
    assert lib.eps_segment_topk(one, None, one, -1, 4, one, None, one, None) == -1
    assert "eps_segment_topk: n_seg=-1 " in lib.eps_last_error().decode()
    assert lib.eps_segment_topk(None, None, one, 3, 4, one, None, one, None) == -1
    assert "eps_segment_topk: colptr is null with n_seg=3" in lib.eps_last_error().decode()
    assert lib.eps_segment_topk(None, None, None, 0, 4, None, None, None, None) == 0
    with pytest.raises(eps.EpsError):                # ops: CPU tensors are refused like everywhere else
        eps.ops.segment_topk(torch.zeros(2, dtype=torch.int64), torch.zeros(3), 2)


def test_helper_against_bruteforce_tie_straddling_k():
    #          seg 0: the 2nd place falls inside a run of three 5s     seg 1: empty   seg 2: shorter than k    seg 3: both zeros tie
    score = np.array([1, 5, 9, 5, 5, 0,                                               7, 3,                   -0.0, 0.0, -1, 0.0], np.float32)
    colptr = np.array([0, 6, 6, 8, 12])
    got = cases.segment_topk_ref(colptr, score, 3)
    assert got.tolist() == [1, 2, 3, 6, 7, 8, 9, 11]        # 9 and the FIRST two 5s; both of seg 2; the zeros in position order
    for k in (1, 2, 3, 4, 100):
        assert np.array_equal(cases.segment_topk_ref(colptr, score, k), cases.segment_topk_bruteforce(colptr, score, k))
    # the padded layout: counts below the room, padding never selected
    counts = np.array([4, 0, 1, 3])
    got = cases.segment_topk_ref(colptr, score, 2, counts)
    assert got.tolist() == [1, 2, 6, 8, 9]
    assert np.array_equal(got, cases.segment_topk_bruteforce(colptr, score, 2, counts))
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 40, 50)
    cp = np.concatenate([[0], np.cumsum(lens)])
    sc = rng.integers(0, 4, cp[-1]).astype(np.float32)
    for k in (1, 5, 39, 40):
        assert np.array_equal(cases.segment_topk_ref(cp, sc, k), cases.segment_topk_bruteforce(cp, sc, k))


def test_file_level_restatement():
    #                       u  v  score     (a whole file in its declared order: score descending)
    rows = torch.tensor([[3, 1, 9.0], [0, 2, 8.0], [4, 1, 8.0], [5, 1, 8.0], [6, 2, 7.0], [7, 1, 7.0], [8, 0, 1.0]])
    assert torch.equal(cases.first_k_rows_per_v(rows, 2), rows[[0, 1, 2, 4, 6]])
    assert torch.equal(cases.first_k_rows_per_v(rows, 1), rows[[0, 1, 6]])
    assert torch.equal(cases.first_k_rows_per_v(rows, 10), rows)
    assert cases.first_k_rows_per_v(rows[:0], 3).shape == (0, 3)

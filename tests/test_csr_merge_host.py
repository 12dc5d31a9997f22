"""CPU: the host side of adding edges to a resident graph -- the ABI surface of csrc/csr_merge.hip, its argument checks (which
return before any launch), rank.py's flag, the batch CSRGraph.with_edges builds, and add_edges without a base."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("eps_csr_merge_workspace_bytes", "eps_csr_merge_count", "eps_csr_merge_fill")


def test_symbols_in_signatures_header_and_library(eps):
    header = open(os.path.join(ROOT, "include", "eps_abi.h")).read()
    lib = eps.load()
    for s in SYMBOLS:
        assert s in eps._lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % s, header)
        assert hasattr(lib, s)
    assert "csr_merge.hip" in open(os.path.join(ROOT, "edge-proposal-sets_amd", "csrc", "Makefile")).read()
    assert callable(eps.ops.csr_merge) and callable(eps.CSRGraph.with_edges)


def test_argument_checks_come_before_any_launch(eps):
    """EPS_EINVAL (-1) with the value named: n >= 2**31, a null rowptr, a negative m -- checkable without a device."""
    lib = eps.load()
    one = ctypes.c_void_p(8)          # (any non-null address: a refused call never reads through it)
    rc = lib.eps_csr_merge_count(one, one, 1 << 31, one, 1, one, one, one, one, 1 << 20, None)
    assert rc == -1 and b"n=2147483648" in lib.eps_last_error()
    rc = lib.eps_csr_merge_count(None, one, 10, one, 1, one, one, one, one, 1 << 20, None)
    assert rc == -1 and b"rowptr" in lib.eps_last_error()
    rc = lib.eps_csr_merge_count(one, one, 10, one, -1, one, one, one, one, 1 << 20, None)
    assert rc == -1 and b"m=-1" in lib.eps_last_error()
    rc = lib.eps_csr_merge_count(one, one, 10, one, 4, one, one, one, None, 0, None)
    assert rc == -1 and b"workspace" in lib.eps_last_error()
    rc = lib.eps_csr_merge_fill(one, one, None, 1 << 31, one, 1, one, one, 5, one, None, None)
    assert rc == -1 and b"n=2147483648" in lib.eps_last_error()
    rc = lib.eps_csr_merge_fill(None, one, None, 10, one, 1, one, one, 5, one, None, None)
    assert rc == -1 and b"rowptr" in lib.eps_last_error()
    rc = lib.eps_csr_merge_fill(one, one, None, 10, one, -3, one, one, 5, one, None, None)
    assert rc == -1 and b"m=-3" in lib.eps_last_error()
    assert lib.eps_csr_merge_workspace_bytes(0) == 256 and lib.eps_csr_merge_workspace_bytes(1000) >= 4000


def test_rank_parser_has_the_ab_flag(eps):
    from eps_amd import rank_stage
    p = rank_stage.make_parser()
    assert p.parse_args(["--dataset", "ddi"]).no_incremental_graph is False
    assert p.parse_args(["--dataset", "ddi", "--no_incremental_graph"]).no_incremental_graph is True


def test_merge_keys_mirrors_sorts_and_keeps_repeats(eps):
    from eps_amd.graph import merge_keys
    extra = torch.tensor([[5, 2, 5, 7, 9],
                          [2, 5, 2, 7, 0]])                    # (5, 2) twice and once mirrored, a self pair, (9, 0)
    keys = merge_keys(extra)
    assert keys.dtype == torch.int64 and keys.shape == (10,)
    pairs = [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in keys]
    assert pairs == sorted(pairs)
    assert pairs == [(0, 9), (2, 5), (2, 5), (2, 5), (5, 2), (5, 2), (5, 2), (7, 7), (7, 7), (9, 0)]
    assert merge_keys(torch.zeros((2, 0), dtype=torch.int64)).shape == (0,)
    assert merge_keys(extra.to(torch.int32)).tolist() == keys.tolist()


def test_add_edges_without_base_is_unchanged(eps):
    """``base=None`` is the rebuild from the edge list, on CPU tensors as before; a CPU graph cannot take the merge route."""
    ei = torch.tensor([[0, 1, 1, 3], [1, 2, 2, 0]])
    ew = torch.tensor([2.0, 1.0, 3.0, 1.0])
    extra = torch.tensor([[4, 0], [0, 1]])
    for dataset in ("collab", "ddi"):
        a = eps.add_edges(dataset, ei, ew, extra, 5)
        b = eps.add_edges(dataset, ei, ew, extra, 5, base=None)
        assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
        assert a.rowptr.tolist() == [0, 3, 5, 6, 7, 8] and a.col.tolist() == [1, 3, 4, 0, 2, 1, 0, 0]
        if dataset == "collab":
            assert a.val.tolist() == b.val.tolist() == [3.0, 1.0, 1.0, 3.0, 4.0, 4.0, 1.0, 1.0]
        else:
            assert a.val is None and b.val is None
    base = eps.add_edges("ddi", ei, ew, extra[:, :0], 5)
    with pytest.raises(eps.EpsError):
        eps.add_edges("ddi", ei, ew, extra, 5, base=base)

"""CPU: the host side of the fused training decode (--fused_decode): the flag, its refusals, the mask packing, the signature
table, and the float32 dense formulation on the cases the GPU tests use."""
import numpy as np
import pytest
import torch

import decode_train_cases as dc
import training_truth as tt


def test_parser_has_the_flag_off_by_default(eps):
    from eps_amd import rank_stage
    p = rank_stage.make_parser()
    assert p.parse_args(["--dataset", "ddi"]).fused_decode is False
    assert p.parse_args(["--dataset", "ddi", "--fused_decode"]).fused_decode is True
    from eps_amd import models
    assert models.LinkGNN.fused_decode is False


@pytest.mark.parametrize("model", ["adamic_ogb", "dea", "mlpcos"])
def test_flag_refuses_other_models_before_data_is_read(eps, model, monkeypatch):
    from eps_amd import rank_stage

    def no_data(*a, **k):
        raise AssertionError("the dataset was read")

    monkeypatch.setattr(rank_stage, "get_data", no_data)
    with pytest.raises(ValueError, match="BatchNorm"):
        rank_stage.main(["--dataset", "ddi", "--model", model, "--synthetic", "--fused_decode"])


@pytest.mark.parametrize("H", [36, 256])
def test_mask_packing_round_trips(eps, H):
    g = torch.Generator().manual_seed(H)
    mask = torch.rand(3, 37, H, generator=g) >= 0.5
    words = eps.ops.pack_mask(mask)
    nw = (H + 31) // 32
    assert words.dtype == torch.int32 and tuple(words.shape) == (3, 37, nw)
    padded = np.zeros((3, 37, nw * 32), dtype=np.uint8)
    padded[..., :H] = mask.numpy()
    truth = np.packbits(padded, axis=-1, bitorder="little").view("<u4").reshape(3, 37, nw)
    assert np.array_equal(words.numpy().view(np.uint32), truth)
    assert torch.equal(eps.ops.unpack_mask(words, H), mask)


def test_signatures_hold_the_new_entry_points(eps):
    sig = eps._lib.SIGNATURES
    for name in ("eps_mlp_decode_train", "eps_mlp_decode_backward", "eps_mlp_decode_backward_workspace_bytes"):
        assert name in sig and hasattr(eps.load(), name)
    lib = eps.load()
    assert lib.eps_mlp_decode_backward_workspace_bytes(64, 64, 3) >= (2 * 2 + 1) * 64 * 64 * 4
    assert lib.eps_version() == 7


def test_domain_errors_name_the_value_without_a_gpu(eps):
    lib = eps.load()
    for H, L, word in [(20, 2, b"hdim=20"), (260, 2, b"hdim=260"), (64, 1, b"n_layers=1")]:
        rc = lib.eps_mlp_decode_train(None, 8, H, None, None, 4, None, None, L, None, 1.0, 1, None, None, None)
        assert rc == -1 and word in lib.eps_last_error() and b"eps_mlp_decode_train" in lib.eps_last_error()
        rc = lib.eps_mlp_decode_backward(None, 8, H, None, None, 4, None, None, None, L, None, 1.0, 1, None, None, None, None, None,
                                         None, None, 0, None)
        assert rc == -1 and word in lib.eps_last_error() and b"eps_mlp_decode_backward" in lib.eps_last_error()
    assert lib.eps_mlp_decode_train(None, 8, 64, None, None, 0, None, None, 2, None, 1.0, 1, None, None, None) == 0


def test_restatement_without_masks_is_the_truth_module(eps):
    h, edges, ws, bs, _ = dc.make_case(36, 3, 65, 5)
    a = dc.decode_forward(h.double(), edges, [w.double() for w in ws], [b.double() for b in bs])
    b = tt.link_predictor(h.double(), edges, [w.double() for w in ws], [b.double() for b in bs])
    assert torch.equal(a, b)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,L,B", [(H, L, B) for H in (36, 64, 256) for L in (2, 3) for B in (1, 63, 64, 65, 200)])
def test_float32_dense_formulation_passes_the_protocol(eps, H, L, B, masked):
    """The seeds of the GPU cases: on float64's own ReLU branch the float32 dense formulation is inside the gradient gate."""
    h, edges, ws, bs, keep = dc.make_case(H, L, B, seed=1000 * H + 10 * B + L)
    keep, scale = (keep, 2.0) if masked else (None, 1.0)
    pre = []
    with torch.no_grad():
        dc.decode_forward(h.double(), edges, [w.double() for w in ws], [b.double() for b in bs], keep, scale, pre=pre)
    branch = [z > 0 for z in pre]
    g64 = dc.reference_grads(h, edges, ws, bs, keep, scale, branch, torch.float64)
    g32 = dc.reference_grads(h, edges, ws, bs, keep, scale, branch, torch.float32)
    for k in g64:
        err = float((g32[k].double() - g64[k]).abs().max())
        assert err <= dc.GATE * max(1e-6, float(g64[k].abs().max())), (k, err)

"""CPU: the host side of dea's fused training decode (--fused_decode_bn): the flag, its refusals, the signature table, the
library's domain errors without a GPU, the float64 restatement against torch's own batch_norm, the backward's decomposition in
float64, and the float32 dense formulation on the cases the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

import decode_bn_cases as bc
import decode_train_cases as dc
import training_truth as tt


def test_parser_has_the_flag_off_by_default(eps):
    from eps_amd import models, rank_stage
    p = rank_stage.make_parser()
    assert p.parse_args(["--dataset", "ddi"]).fused_decode_bn is False
    assert p.parse_args(["--dataset", "ddi", "--fused_decode_bn"]).fused_decode_bn is True
    assert models.DEA_GNN_JK.fused_decode is False


@pytest.mark.parametrize("extra,word", [
    (["--model", "gcn"], "--model dea"),                                  # a model other than dea
    (["--model", "mlpcos"], "--model dea"),
    (["--model", "dea_512"], "dea_512"),
    (["--model", "dea", "--hidden_channels", "20"], "hidden_channels 20"),
    (["--model", "dea", "--hidden_channels", "30"], "hidden_channels 30"),
    (["--model", "dea", "--hidden_channels", "260"], "hidden_channels 260"),
    (["--model", "dea", "--fused_decode"], "BatchNorm"),                  # both flags: --fused_decode's own refusal of dea comes first
    (["--model", "gcn", "--fused_decode"], "exclude each other"),
])
def test_flag_refusals_come_before_the_data_is_read(eps, monkeypatch, extra, word):
    from eps_amd import rank_stage

    def no_data(*a, **k):
        raise AssertionError("the dataset was read")

    monkeypatch.setattr(rank_stage, "get_data", no_data)
    with pytest.raises(ValueError, match=word):
        rank_stage.main(["--dataset", "ddi", "--synthetic", "--fused_decode_bn"] + extra)


def test_default_width_passes_the_flag_check(eps, monkeypatch):
    """ddi's default width for dea (256, filled in by default_model_configs) is inside the domain: the run gets as far as the data."""
    from eps_amd import rank_stage

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    monkeypatch.setattr(rank_stage, "get_data", stop)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises((Reached, RuntimeError)) as ei:
        rank_stage.main(["--dataset", "ddi", "--synthetic", "--fused_decode_bn", "--model", "dea"])
    assert not isinstance(ei.value, ValueError)


def test_signatures_hold_the_new_entry_points(eps):
    sig = eps._lib.SIGNATURES
    lib = eps.load()
    for name in ("eps_mlp_decode_bn_stats", "eps_mlp_decode_bn_backward", "eps_mlp_decode_bn_workspace_bytes"):
        assert name in sig and hasattr(lib, name)
    assert lib.eps_mlp_decode_bn_workspace_bytes(64, 64, 2) >= 3 * 64 * 64 * 4
    assert lib.eps_mlp_decode_bn_workspace_bytes(64, 64, 3) == 0 and lib.eps_mlp_decode_bn_workspace_bytes(1, 64, 2) == 0
    assert lib.eps_version() == 7


def test_domain_errors_name_the_value_without_a_gpu(eps):
    lib = eps.load()
    for H, L, B, word in [(20, 2, 4, b"hdim=20"), (260, 2, 4, b"hdim=260"), (64, 3, 4, b"n_layers=3"), (64, 2, 1, b"n_pairs=1")]:
        rc = lib.eps_mlp_decode_bn_stats(None, 8, H, None, None, B, None, None, L, None, None, None, 0, None)
        assert rc == -1 and word in lib.eps_last_error() and b"eps_mlp_decode_bn_stats" in lib.eps_last_error()
        rc = lib.eps_mlp_decode_bn_backward(None, 8, H, None, None, B, None, None, None, L, None, None, None, None, None, 1e-5, None,
                                            1.0, None, None, None, None, None, None, None, None, None, 0, None)
        assert rc == -1 and word in lib.eps_last_error() and b"eps_mlp_decode_bn_backward" in lib.eps_last_error()


def _f64(xs):
    return [x.double() for x in xs]


@pytest.mark.parametrize("masked", [False, True])
def test_restatement_is_torch_batch_norm(eps, masked):
    """bn_forward writes the BatchNorm out; in float64 its logits and every gradient are F.batch_norm(training=True)'s."""
    h, edges, ws, bs, gamma, beta, keep = bc.make_case(36, 65, 5)
    kp, scale = (keep, 2.0) if masked else (None, 1.0)
    ours = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, None, torch.float64)
    leaf = lambda x: x.detach().double().clone().requires_grad_(True)   # noqa: E731
    hh, w, b, ga, be = leaf(h), [leaf(x) for x in ws], [leaf(x) for x in bs], leaf(gamma), leaf(beta)
    z = (hh[edges[0]] * hh[edges[1]]) @ w[0].t() + b[0]
    rm, rv = torch.zeros(36, dtype=torch.float64), torch.ones(36, dtype=torch.float64)
    a = torch.relu(F.batch_norm(z, rm, rv, ga, be, training=True, momentum=0.1, eps=tt.BN_EPS))
    if masked:
        a = a * (keep.double() * scale)
    out = (a @ w[1].t() + b[1]).squeeze(1)
    with torch.no_grad():
        mine = bc.bn_forward(h.double(), edges, _f64(ws), _f64(bs), gamma.double(), beta.double(), kp, scale)
        mean, var = bc.statistics(h.double(), edges, _f64(ws), _f64(bs))
    assert float((mine - out.detach()).abs().max()) <= 1e-13
    # the running statistics torch keeps: momentum 0.1, the UNBIASED variance
    assert float((rm - 0.1 * mean).abs().max()) <= 1e-14 and float((rv - (0.9 + 0.1 * var * 65 / 64)).abs().max()) <= 1e-14
    tt.bce_logits_loss(out, bc.labels(65)).backward()
    theirs = {"h": hh.grad, "w0": w[0].grad, "w1": w[1].grad, "b0": b[0].grad, "b1": b[1].grad, "gamma": ga.grad, "beta": be.grad}
    for k in ours:
        assert float((ours[k] - theirs[k]).abs().max()) <= 1e-13 * max(1.0, float(theirs[k].abs().max())), k
    assert float(ours["b0"].abs().max()) <= 1e-15        # a bias in front of batch statistics: a true gradient of 0


@pytest.mark.parametrize("masked", [False, True])
def test_backward_decomposition_in_float64(eps, masked):
    """What eps_mlp_decode_bn_backward computes, step by step in float64: the backward of the FOLDED decoder up to dy and g' =
    sum dy, G' = dy^T x0, grad gamma = (W0 . G' + (b0 - mu) g') / sigma, dz = s (dy - g' / B - zhat grad_gamma / B),
    dx0 = dz W0, grad W0 = dz^T x0, grad b0 = 0 -- against autograd through the BatchNorm."""
    H, B = 36, 65
    h, edges, ws, bs, gamma, beta, keep = bc.make_case(H, B, 5)
    kp, scale = (keep, 2.0) if masked else (None, 1.0)
    ref = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, None, torch.float64)
    d = torch.float64
    h, gamma, beta, (W0, w1), (b0, b1) = h.to(d), gamma.to(d), beta.to(d), _f64(ws), _f64(bs)
    x0 = h[edges[0]] * h[edges[1]]
    mu, var = bc.statistics(h, edges, [W0, w1], [b0, b1])
    sig = torch.sqrt(var + tt.BN_EPS)
    s = gamma / sig
    Wf, bf = (W0 * s[:, None]).requires_grad_(True), (s * (b0 - mu) + beta).requires_grad_(True)
    y = x0 @ Wf.t() + bf
    y.retain_grad()
    a = torch.relu(y) * (keep.to(d) * scale if masked else 1.0)
    out = (a @ w1.t() + b1).squeeze(1)
    tt.bce_logits_loss(out, bc.labels(B)).backward()
    dy, g1, G1 = y.grad, bf.grad, Wf.grad
    dgamma = ((W0 * G1).sum(1) + (b0 - mu) * g1) / sig
    zhat = (x0 @ W0.t() + b0 - mu) / sig
    dz = s * (dy - g1 / B - zhat * dgamma / B)
    dx0 = dz @ W0
    gh = torch.zeros_like(h)
    gh.index_add_(0, edges[0], dx0 * h[edges[1]])
    gh.index_add_(0, edges[1], dx0 * h[edges[0]])
    got = {"h": gh, "w0": dz.t() @ x0, "gamma": dgamma, "beta": g1, "b0": torch.zeros(H, dtype=d)}
    for k, g in got.items():
        assert float((g - ref[k]).abs().max()) <= 1e-13 * max(1.0, float(ref[k].abs().max())), k


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,B", bc.SHAPES)
def test_float32_dense_formulation_passes_the_protocol(eps, H, B, masked):
    """The seeds of the GPU cases, on float64's own ReLU branch: the float32 dense formulation goes through check_grads, and
    from one tile of edges on it is inside the 2e-4 gate outright.  (At B = 2 the normalised values are +-1 up to eps / sigma^2,
    so what reaches W0 and h is the O(eps) remainder of a cancellation: float32 resolves it to a few 1e-3 of its size, which
    is why the protocol's second clause -- 4 x this formulation's own distance -- exists.)"""
    h, edges, ws, bs, gamma, beta, keep = bc.make_case(H, B, bc.seed_of(H, B))
    kp, scale = (keep, 2.0) if masked else (None, 1.0)
    branch = bc.own_branch(h, edges, ws, bs, gamma, beta, kp, scale)
    g64 = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, branch, torch.float64)
    g32 = bc.reference_grads(h, edges, ws, bs, gamma, beta, kp, scale, branch, torch.float32)
    dc.check_grads(f"f32 dense H={H} B={B} masks={masked}", g32, g64, g32)
    if B >= 63:
        for k in g64:
            if k == "b0":         # (a true gradient of 0: float32 noise is all the dense formulation has for it; the kernels write zeros)
                continue
            err = float((g32[k].double() - g64[k]).abs().max())
            assert err <= dc.GATE * max(1e-6, float(g64[k].abs().max())), (k, err)

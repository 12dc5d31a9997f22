"""What tests/test_decode_train_host.py (CPU) and tests/test_gpu_decode_train.py (GPU) share: the small decode cases, the
restatement of LinkPredictor's training forward WITH dropout masks in the dtype of its inputs (float64 = the truth, float32 =
the plain dense torch formulation), and the project's gradient protocol (tests/test_gpu_training.py::_check_grads, restated).
A plain helper module, no fixtures."""
import torch

import training_truth as tt

GATE = 2e-4          # the project's gradient gate: per output, of max|grad|
N_NODES = 50         # few nodes: the endpoints of a batch collide


def make_case(H, L, B, seed, p_drop=0.5):
    """CPU float32 case: h [50, H], edges int64 [2, B] with a self pair and a duplicated pair, Linear-initialised layers,
    keep masks bool [L - 1, B, H] drawn at p_drop."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N_NODES, H, generator=g)
    edges = torch.randint(0, N_NODES, (2, B), generator=g)
    edges[1, 0] = edges[0, 0]                      # a self pair u == v
    if B >= 3:
        edges[:, 2] = edges[:, 1]                  # the same pair twice
    bound = 1.0 / H ** 0.5
    ws = [(torch.rand(H, H, generator=g) * 2 - 1) * bound for _ in range(L - 1)] + [(torch.rand(1, H, generator=g) * 2 - 1) * bound]
    bs = [(torch.rand(H, generator=g) * 2 - 1) * bound for _ in range(L - 1)] + [(torch.rand(1, generator=g) * 2 - 1) * bound]
    keep = torch.rand(L - 1, B, H, generator=g) >= p_drop
    return h, edges, ws, bs, keep


def decode_forward(h, edges, ws, bs, keep=None, scale=1.0, branch=None, pre=None):
    """training_truth.link_predictor plus dropout: after every ReLU the units are multiplied by keep[l] * scale.  ``branch`` /
    ``pre``: as in training_truth._relu (masks in layer order).  Without keep it is training_truth.link_predictor itself."""
    branch = None if branch is None else iter(branch)
    z = h[edges[0]] * h[edges[1]]
    for l, (w, b) in enumerate(zip(ws[:-1], bs[:-1])):
        z = tt._relu(z @ w.t() + b, branch, pre)
        if keep is not None:
            z = z * (keep[l].to(z.dtype) * scale)
    return torch.sigmoid(z @ ws[-1].t() + bs[-1]).squeeze(1)


def loss_of(out):
    """training_truth.log_loss with the first half of the batch as positives; a batch of one edge is one positive."""
    if out.numel() == 1:
        return -torch.log(out + 1e-8).mean()
    return tt.log_loss(out, out.numel() // 2)


def reference_grads(h, edges, ws, bs, keep, scale, branch, dtype):
    """{name: grad} of loss_of(decode_forward(...)) in ``dtype`` on the given ReLU branch: 'h', 'w0'.., 'b0'.."""
    hh = h.detach().to(dtype).clone().requires_grad_(True)
    w = [x.detach().to(dtype).clone().requires_grad_(True) for x in ws]
    b = [x.detach().to(dtype).clone().requires_grad_(True) for x in bs]
    loss_of(decode_forward(hh, edges, w, b, keep, scale, branch=branch)).backward()
    out = {"h": hh.grad}
    out.update({f"w{i}": x.grad for i, x in enumerate(w)})
    out.update({f"b{i}": x.grad for i, x in enumerate(b)})
    return out


def check_grads(tag, got, g64, g32, floor=1e-6):
    """Per output: |got - f64| <= GATE * max(floor, max|f64|); an output past that gate is held to 4 x the distance of the
    float32 dense torch formulation from float64."""
    for k, g in got.items():
        err = float((g.double().cpu() - g64[k].cpu()).abs().max())
        d32 = float((g32[k].double().cpu() - g64[k].cpu()).abs().max())
        gate = GATE * max(floor, float(g64[k].abs().max()))
        print(f"{tag} {k}: |got - f64| = {err:.3g}, gate {gate:.3g}, |f32 dense - f64| = {d32:.3g}")
        if err > gate:
            assert err <= 4.0 * d32, (tag, k, err, gate, d32)

#!/usr/bin/env python3
"""Time the DEA_GNN_JK model ('dea' / 'dea_512') on the HIP kernels; one JSON line.

  forward: the eval-mode TAG forward (3 layers: hop buffer + one GEMM each, BatchNorm folded, JK max) on the ddi-like and
      collab-like stand-ins, median of --reps after --warmup (the embeddings cache is cleared before each call).
  decode: eps_mlp_decode at H = 256 and 512 (L = 2: the DEA decoder) on --edges random edges, as edges/s and as a fraction of
      157.3 TFLOP/s f32 MFMA under the FLOP model of BASELINE.md (H + 2 H^2 (L - 1) + 2 H per edge).
  filter: filter.py --dataset ddi --model dea --synthetic --keep_top K with a freshly initialised checkpoint (wall time of the
      whole command, data set-up included).

Run:  python tools/dea_bench.py [--edges 4194304 --keep_top 530000 --reps 10 --warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def forward_ms(dataset, model_name, reps, warmup, dev):
    from eps_amd import datasets, models
    os.environ.pop("EPS_SYNTH_SCALE", None)
    use_feature = dataset == "collab"
    _, _, _, data = datasets.get_data(argparse.Namespace(dataset=dataset, synthetic=True, use_feature=use_feature))
    data = data.to(dev)
    args = models.default_model_configs(argparse.Namespace(dataset=dataset, model=model_name,
                                                      **{k: None for k in models._KEYS}))
    m = models.build_model(args, data, dev).eval()

    def run():
        m._h_key = None
        m.embeddings(data.x, data.adj_t)
    return {"ms": round(timed(run, reps, warmup), 3), "nodes": data.num_nodes, "nnz": data.adj_t.nnz(),
            "H": args.hidden_channels}


def decode_rate(H, n_edges, reps, warmup, dev):
    import torch
    from eps_amd import ops
    g = torch.Generator(device=dev).manual_seed(H)
    n = 100_000
    h = torch.randn(n, H, device=dev, generator=g)
    u = torch.randint(0, n, (n_edges,), device=dev, dtype=torch.int32, generator=g)
    v = torch.randint(0, n, (n_edges,), device=dev, dtype=torch.int32, generator=g)
    ws = [torch.randn(H, H, device=dev, generator=g) / H ** 0.5, torch.randn(1, H, device=dev, generator=g) / H ** 0.5]
    bs = [torch.zeros(H, device=dev), torch.zeros(1, device=dev)]
    ms = timed(lambda: ops.mlp_decode(h, u, v, ws, bs, apply_sigmoid=False), reps, warmup)
    flop = n_edges * (H + 2 * H * H * 1 + 2 * H)
    return {"ms": round(ms, 3), "edges_per_s": round(n_edges / (ms * 1e-3), 1),
            "frac_f32_mfma_peak": round(flop / (ms * 1e-3) / PEAK_F32_MFMA, 3)}


def filter_s(keep, dev):
    import torch
    from eps_amd import datasets, filter_stage, models
    os.environ.pop("EPS_SYNTH_SCALE", None)
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            _, _, _, data = datasets.get_data(argparse.Namespace(dataset="ddi", synthetic=True, use_feature=False))
            args = models.default_model_configs(argparse.Namespace(dataset="ddi", model="dea", **{k: None for k in models._KEYS}))
            m = models.build_model(args, data, "cpu")
            os.makedirs("models")
            torch.save(m.state_dict(), "models/ddi_dea||0|0.pt")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            filter_stage.main(["--dataset", "ddi", "--model", "dea", "--checkpoint", "ddi_dea||0|0.pt", "--synthetic",
                               "--keep_top", str(keep)])
            torch.cuda.synchronize()
            return round(time.perf_counter() - t0, 3)
        finally:
            os.chdir(cwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=1 << 22)
    ap.add_argument("--keep_top", type=int, default=530_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dea_bench: no GPU (the figures are GPU timings; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"forward": {f"{ds}/{mn}": forward_ms(ds, mn, a.reps, a.warmup, dev)
                       for ds in ("ddi", "collab") for mn in ("dea", "dea_512")},
           "decode": {f"H{H}": decode_rate(H, a.edges, a.reps, a.warmup, dev) for H in (256, 512)},
           "filter_ddi_dea_s": filter_s(a.keep_top, dev)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time one mlpcos training step (train_and_eval.py:31-96 through the cosine common-neighbour score) piece by piece on the
ddi-like stand-in (embedding only, F = 256, batch 64 k positive edges) and the collab-like one (F = 256 + 128, batch 16 k);
one JSON line.

  pieces (median of --reps after --warmup, HIP events): node features (+ norms), edge cosines, pair forward, pair backward
      (eps_pair_cn_backward), feature backward (eps_cos_features_backward), the smoothing's SpMM over the 256 embedding columns,
      and the whole step (model forward, loss, backward, clip, Adam) as training.train runs it.
  byte models of the two backward kernels:
      pair backward:    both rows of every pair once (4 B per entry) + 12 B of list per pair + 16 B of 64-bit
                        atomic traffic per hit (two adds of 8 B); "atomic_tbs" = the atomic bytes alone / time, to set against
                        the chip-wide rate of float atomics (about 1.3 TB/s of added bytes).
      feature backward: nnz x (4 F + 12) + N x 8 F bytes (one xhat row, col, revpos and gc per entry; xhat_r in, two rows out).

Run:  python tools/cosine_train_bench.py [--datasets ddi,collab --reps 10 --warmup 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cosine_cn_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="ddi,collab")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import eps_amd  # noqa: F401
    from eps_amd import datasets, heuristics, models, ops, scan
    from eps_amd.graph import CSRGraph
    from eps_amd.rank_helpers import to_undirected

    dev = torch.device("cuda:0")
    out = {}
    for name in a.datasets.split(","):
        args = models.default_model_configs(argparse.Namespace(
            dataset=name, model="mlpcos", synthetic=True, **dict.fromkeys(models._KEYS)))
        _, _, split_edge, data = datasets.get_data(args)
        data = data.to(dev)
        g = data.adj_t
        model = models.build_model(args, data, dev)
        feat = data.x if args.use_feature else None
        hidden = args.hidden_channels
        torch.manual_seed(0)
        pos = to_undirected(split_edge["train"]["edge"][:args.batch_size].t().to(dev))
        neg = torch.stack([pos[0], torch.randint(0, data.num_nodes, (pos.shape[1],), device=dev)])
        edges = torch.cat([pos, neg], 1)
        u, v = heuristics._as_pairs(edges, dev, g.n_rows)
        w = model.emb.weight.detach()
        x = heuristics._aligned_rows(w if feat is None else torch.cat([w, feat], 1))
        f = x.shape[1]
        rev = scan.reverse_positions(g)
        xhat, nrm = ops.cos_node_features(g.rowptr, g.col, g.val, x, want_norm=True)
        c = ops.edge_cosines(g.rowptr, g.col, xhat, rev)
        cg = CSRGraph(g.rowptr, g.col, c, g.n_rows, g.n_cols)
        count, raw, _ = ops.pair_scores(g.rowptr, g.col, c, None, g.n_rows, u, v, want_count=True, want_cn=True, grouped=False)
        graw = (torch.sigmoid(raw) - 0.5) / u.numel()
        gc = ops.pair_cn_backward(g.rowptr, g.col, c, u, v, graw)
        gxp, gxs = ops.cos_features_backward(g.rowptr, g.col, g.val, xhat, nrm, rev, gc, want_scaled=True)
        t = {
            "node_features_ms": timed(lambda: ops.cos_node_features(g.rowptr, g.col, g.val, x, want_norm=True), a.reps, a.warmup),
            "edge_cosines_ms": timed(lambda: ops.edge_cosines(g.rowptr, g.col, xhat, rev), a.reps, a.warmup),
            "pair_forward_ms": timed(lambda: heuristics.pair_scores_streamed(cg, u, v, None, want_cn=True), a.reps, a.warmup),
            "pair_backward_ms": timed(lambda: ops.pair_cn_backward(g.rowptr, g.col, c, u, v, graw), a.reps, a.warmup),
            "feature_backward_ms": timed(lambda: ops.cos_features_backward(g.rowptr, g.col, g.val, xhat, nrm, rev, gc,
                                                                           want_scaled=True), a.reps, a.warmup),
            "spmm_ms": timed(lambda: ops.spmm_csr(g.rowptr, g.col, g.val, gxs[:, :hidden]), a.reps, a.warmup),
        }
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        model.train()

        def step():
            opt.zero_grad()
            o = model(feat, edges, g)
            n_pos = pos.shape[1]
            loss = -torch.log(o[:n_pos] + 1e-8).mean() - torch.log(1 - o[n_pos:] + 1e-8).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()

        t["train_step_ms"] = timed(step, a.reps, a.warmup)
        deg = (g.rowptr[1:] - g.rowptr[:-1])
        hits = int(count.sum().item())
        row_bytes = int((deg[u.long()] + deg[v.long()]).sum().item()) * 4 + 12 * u.numel()
        atomic_bytes = 16 * hits
        nnz = g.nnz()
        fb_bytes = nnz * (4 * f + 12) + g.n_rows * 8 * f
        r = {"nodes": g.n_rows, "nnz": nnz, "f": f, "pairs": u.numel(), "hits": hits}
        r.update({k: round(val, 3) for k, val in t.items()})
        r.update({"pair_backward_model_gb": round((row_bytes + atomic_bytes) / 1e9, 3),
                  "pair_backward_tbs": round((row_bytes + atomic_bytes) / t["pair_backward_ms"] / 1e9, 3),
                  "pair_backward_atomic_gb": round(atomic_bytes / 1e9, 3),
                  "pair_backward_atomic_tbs": round(atomic_bytes / t["pair_backward_ms"] / 1e9, 3),
                  "feature_backward_model_gb": round(fb_bytes / 1e9, 3),
                  "feature_backward_tbs": round(fb_bytes / t["feature_backward_ms"] / 1e9, 3)})
        out[name] = r
        print(name, json.dumps(r), flush=True)
        del model, opt, data, g, cg, xhat, gxp, gxs
        torch.cuda.empty_cache()
    print(json.dumps({"cosine_train_bench": out}))


if __name__ == "__main__":
    main()

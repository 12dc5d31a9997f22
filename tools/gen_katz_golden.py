#!/usr/bin/env python3
"""Generate tests/golden/katz_{collab,ddi}_like.npz by running the reference's own test_katz (build machine only).

Run:  python tools/gen_katz_golden.py            (needs the reference checkout; never runs on the GPU box)

test_katz (train_and_eval.py:272-343) is called with stand-in ``data`` / ``args`` and an evaluator that records every
``y_pred_pos`` / ``y_pred_neg`` it is handed (and computes ogb's Hits@K, restated as in evaluate.Evaluator).  Only the
emitted vectors travel: the two CSR adjacencies, the five pair lists, the five prediction vectors in the reference's
dtypes (float32 on the collab branch, float64 on the inverse branch), the Hits table and, for the inverse branch,
cond(I - beta*A).  Seeds are drawn until cond <= 1e6 and no positive lies within 2e-5 relative of a nonzero Hits@K cut,
so a one-ulp difference cannot flip a hit.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import scipy.sparse as ssp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (the reference's third-party stubs and graph helpers, read-only)

OUT = os.path.join(ROOT, "tests", "golden")
BETA = 0.05
SIZES = dict(eval_train=150, valid=150, valid_neg=600, test=150, test_neg=600)


class Adj:
    """The slice of torch_sparse.SparseTensor get_A touches (adamic_utils.py:8-11): ``coo()``."""

    def __init__(self, A):
        self.A = A.tocoo()

    def coo(self):
        a = self.A
        return (torch.from_numpy(a.row.astype(np.int64)), torch.from_numpy(a.col.astype(np.int64)),
                torch.from_numpy(a.data.astype(np.float32)))


class RecordingEvaluator:
    """ogb's Hits@K (kth = topk(neg, K)[-1]; mean(pos > kth); 1.0 below K negatives) that keeps what it was given."""

    def __init__(self):
        self.K = None
        self.seen = []

    def eval(self, d):
        pos, neg = d["y_pred_pos"], d["y_pred_neg"]
        self.seen.append((pos, neg))
        if len(neg) < self.K:
            return {f"hits@{self.K}": 1.0}
        kth = torch.topk(neg.reshape(-1), self.K)[0][-1]
        return {f"hits@{self.K}": float(torch.sum(pos.reshape(-1) > kth)) / len(pos)}


def edges_of(A):
    """Upper-triangle (u < v) stored edges of a symmetric matrix, [E,2]."""
    c = ssp.triu(A, 1).tocoo()
    return np.stack([c.row, c.col], 1).astype(np.int64)


def make_case(kind, seed):
    rng = np.random.default_rng(seed)
    n = 1000
    r, c = gg.rmat_edges(10, 5000, rng, a=0.45, b=0.22, c=0.22)
    r, c = r % n, c % n
    w = rng.integers(1, 6, size=len(r)).astype(np.float32) if kind == "collab" else None
    A_all = gg.sym_csr(r, c, n, w)
    und = edges_of(A_all)
    und = und[rng.permutation(len(und))]
    valid, test, train = und[:SIZES["valid"]], und[SIZES["valid"]:SIZES["valid"] + SIZES["test"]], und[SIZES["valid"] + SIZES["test"]:]
    wt = np.asarray(A_all[train[:, 0], train[:, 1]]).ravel() if kind == "collab" else None
    A_train = gg.sym_csr(train[:, 0], train[:, 1], n, wt)
    if kind == "collab":       # rank.py's collab graphs: the validation edges (weight 1, both directions) join the test graph
        A_full = gg.sym_csr(np.concatenate([train[:, 0], valid[:, 0]]), np.concatenate([train[:, 1], valid[:, 1]]), n,
                            np.concatenate([wt, np.ones(len(valid), np.float32)]))
    else:
        A_full = A_train
    split = {"eval_train": {"edge": train[rng.choice(len(train), SIZES["eval_train"], replace=False)]},
             "valid": {"edge": valid, "edge_neg": rng.integers(0, n, (SIZES["valid_neg"], 2))},
             "test": {"edge": test, "edge_neg": rng.integers(0, n, (SIZES["test_neg"], 2))}}
    return n, A_train, A_full, split


def cut_margin_ok(table_preds, ks, margin=2e-5):
    for pos, neg in table_preds:
        srt = np.sort(np.asarray(neg, np.float64))[::-1]
        for K in ks:
            if len(srt) < K:
                continue
            kth = srt[K - 1]
            if kth == 0:
                continue            # zero is exact on both sides
            if np.any(np.abs(np.asarray(pos, np.float64) - kth) <= margin * abs(kth)):
                return False
    return True


def emit(kind, train_and_eval, first_seed):
    dataset = "collab" if kind == "collab" else "ddi"
    for seed in range(first_seed, first_seed + 200):
        n, A_train, A_full, split = make_case(kind, seed)
        cond = float(np.linalg.cond(np.eye(n) - BETA * A_full.toarray().astype(np.float64)))
        if kind != "collab" and cond > 1e6:
            continue
        split_t = {k: {kk: torch.from_numpy(vv) for kk, vv in v.items()} for k, v in split.items()}
        data = SimpleNamespace(adj_t=Adj(A_train), full_adj_t=Adj(A_full), num_nodes=n)
        args = SimpleNamespace(dataset=dataset, model="katz")
        ev = RecordingEvaluator()
        results = train_and_eval.test_katz(None, data, split_t, ev, 64, args, "cpu")
        ks = train_and_eval.hits[dataset]
        # the evaluator saw (train, valid, test) per K, in that order: train = (pos_train, neg_valid) ...
        pos_train, neg_valid = ev.seen[0]
        pos_valid, _ = ev.seen[1]
        pos_test, neg_test = ev.seen[2]
        if not cut_margin_ok([(pos_train, neg_valid), (pos_valid, neg_valid), (pos_test, neg_test)], ks):
            continue
        table = np.array([results[f"Hits@{K}"] for K in ks], np.float64)
        out = dict(dataset=np.array(dataset), seed=np.array(seed), n=np.array(n), beta=np.array(BETA), ks=np.array(ks),
                   hits=table, cond=np.array(cond))
        for tag, A in (("train", A_train), ("full", A_full)):
            A = A.tocsr()
            A.sort_indices()
            out[f"{tag}_rowptr"], out[f"{tag}_col"] = A.indptr.astype(np.int64), A.indices.astype(np.int32)
            out[f"{tag}_val"] = A.data.astype(np.float32)
        for name, (sp, key) in dict(pos_train=("eval_train", "edge"), pos_valid=("valid", "edge"),
                                    neg_valid=("valid", "edge_neg"), pos_test=("test", "edge"),
                                    neg_test=("test", "edge_neg")).items():
            out[f"{name}_edge"] = split[sp][key].astype(np.int64)
        for name, t in dict(pos_train=pos_train, pos_valid=pos_valid, neg_valid=neg_valid, pos_test=pos_test,
                            neg_test=neg_test).items():
            out[f"{name}_pred"] = t.numpy()
        path = os.path.join(OUT, f"katz_{kind}_like.npz")
        np.savez_compressed(path, **out)
        print(f"{os.path.basename(path)}: seed={seed} N={n} nnz train/full={A_train.nnz}/{A_full.nnz} cond={cond:.3g} "
              f"pred dtype={pos_test.dtype} hits={table.tolist()}")
        return
    raise SystemExit(f"no seed in [{first_seed}, {first_seed + 200}) meets the fixture's conditions for {kind}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("EPS_REFERENCE", gg.REF))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    gg.install_stubs()
    import train_and_eval
    train_and_eval.tqdm = lambda x: x
    emit("collab", train_and_eval, 1)
    emit("ddi", train_and_eval, 1)


if __name__ == "__main__":
    main()

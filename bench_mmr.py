"""MMR diversified re-ranking (ops.mmr_rerank / tt_mmr_rerank_f32: one launch per batch) against a torch-eager equivalent
(gather, bmm, per-pick max / arg-max), both timed in the same run on the pool the same BruteForce call returned.  One JSON
line per shape:

    python bench_mmr.py [--iters 20] [--warmup 3] [--out profiles/mmr.jsonl]

Shapes: nq in {1, 16, 1024, 8192} x (k, k1) in {(10, 40), (100, 256)} at D = 128 over a 1M-row corpus (the seeded clustered
corpus of bench_ivf.py, generated on the device); lambda = 0.7, no group cap.

Fields: mmr_ms (the launch, device events around --iters calls), eager_ms (the eager equivalent, same events), speedup =
eager_ms / mmr_ms, brute_ms (the tt_retrieval_topk_f32 call for k1 candidates that feeds it), frac_of_brute = mmr_ms /
brute_ms, us_per_pick = mmr_ms / k (the k picks of a query are sequential; the queries of a batch run side by side), agree =
the fraction of output positions where the eager list names the same item (its cosines come from a bmm over normalised rows,
so near-ties may resolve differently).
"""
import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from bench_ivf import _time, corpus, queries  # noqa: E402

N, D, NCLUSTERS, LAMBDA = 1_000_000, 128, 5_000, 0.7
SHAPES = [(nq, k, k1) for nq in (1, 16, 1024, 8192) for k, k1 in ((10, 40), (100, 256))]


def eager_mmr(scores, idx, c, k: int, lam: float):
    """The same greedy selection in torch eager: a [nq, k1, D] gather, a [nq, k1, k1] Gram matrix and ~7 launches per pick."""
    nq, k1 = scores.shape
    valid = (idx >= 0) & torch.isfinite(scores)
    rows = torch.nn.functional.normalize(c[idx.clamp(min=0)], dim=2)
    sim = torch.bmm(rows, rows.transpose(1, 2))
    inf = torch.full_like(scores, float("inf"))
    lo = torch.where(valid, scores, inf).amin(1, keepdim=True)
    hi = torch.where(valid, scores, -inf).amax(1, keepdim=True)
    rel = torch.where(hi > lo, (scores - lo) / (hi - lo), torch.zeros_like(scores))
    pen = torch.zeros_like(scores)
    avail = valid.clone()
    out_s = torch.full((nq, k), float("-inf"), device=scores.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int64, device=scores.device)
    ar = torch.arange(nq, device=scores.device)
    for t in range(k):
        val = torch.where(avail, lam * rel - (1.0 - lam) * pen, -inf)
        best, p = val.max(1)
        ok = best > float("-inf")
        out_s[:, t] = torch.where(ok, scores[ar, p], out_s[:, t])
        out_i[:, t] = torch.where(ok, idx[ar, p], out_i[:, t])
        avail[ar, p] = False
        pen = torch.maximum(pen, sim[ar, p])
    return out_s, out_i


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-iters", type=int, default=5, help="timed calls of the eager baseline (it is slow at large nq)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args(argv)
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    x, g = corpus(N, D, NCLUSTERS, 2024, dev)
    lines = []
    for nq, k, k1 in SHAPES:
        q = queries(x, nq, g)
        ws = torch.empty(max(ops.retrieval_topk_workspace_bytes(nq, N, D, k1), 1), dtype=torch.uint8, device=dev)
        pool = (torch.empty(nq, k1, device=dev), torch.empty(nq, k1, dtype=torch.int64, device=dev))
        t_brute = _time(lambda: ops.retrieval_topk(q, x, k1, workspace=ws, out=pool), args.iters, args.warmup)
        out = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
        t_mmr = _time(lambda: ops.mmr_rerank(pool[0], pool[1], x, k, LAMBDA, out=out), args.iters, args.warmup)
        t_eager = _time(lambda: eager_mmr(pool[0], pool[1], x, k, LAMBDA), args.eager_iters, 1)
        agree = float((eager_mmr(pool[0], pool[1], x, k, LAMBDA)[1] == out[1]).float().mean())
        line = json.dumps({"nq": nq, "n": N, "d": D, "k": k, "k1": k1, "lambda": LAMBDA, "mmr_ms": round(t_mmr, 4),
                           "eager_ms": round(t_eager, 4), "speedup": round(t_eager / t_mmr, 2), "brute_ms": round(t_brute, 4),
                           "frac_of_brute": round(t_mmr / t_brute, 4), "us_per_pick": round(t_mmr * 1e3 / k, 3),
                           "agree": round(agree, 4)})
        print(line, flush=True)
        lines.append(line)
        del ws, pool, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

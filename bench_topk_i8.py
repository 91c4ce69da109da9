"""Int8-quantised top-k (serving.Int8BruteForce / tt_retrieval_topk_i8_f32) against exact BruteForce
(tt_retrieval_topk_f32), both timed in the same run on the same corpus.  One JSON line per (shape, k1, re-rank or not):

    python bench_topk_i8.py [--iters 20] [--warmup 3] [--shapes 0,1,2,3,4]

Shapes: the five of the exact top-K table (bench_topk.py), each with k1 = k and the default k1 = min(256, n, max(4 k, 32)),
with the f32 re-rank (``rerank`` true) and, at k1 = k, without it (stage 1 only; without c the call requires k1 = k).
Corpus: the seeded clustered corpus of bench_ivf.py, generated on the device.

Fields: i8_ms and brute_ms (per call), speedup = brute_ms / i8_ms, recall = mean |i8_r & exact_r| / k against the exact
answer of the same run, bytes = what the call streams (n * (D + 4) code and scale bytes per 32-query row block, plus the
re-ranked f32 rows nq * k1 * D * 4), frac_hbm = bytes / t / 8.0e12, quant_s = quantising the corpus, in seconds.
"""
import argparse
import json
import pathlib
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from bench_ivf import PEAK_HBM, _time, corpus, queries, recall  # noqa: E402

# (nq, n, D, k, nclusters)
SHAPES = [(1, 10_000_000, 128, 10, 20_000), (16, 10_000_000, 128, 100, 20_000), (1000, 1_000_000, 128, 100, 5_000),
          (8192, 1_000_000, 128, 100, 5_000), (1024, 10_000_000, 128, 100, 20_000)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
    args = ap.parse_args(argv)
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    built = {}
    for si in (int(v) for v in args.shapes.split(",")):
        nq, n, d, k, ncl = SHAPES[si]
        key = (n, d)
        if key not in built:
            built.clear()
            torch.cuda.empty_cache()
            x, g = corpus(n, d, ncl, 2024, dev)
            out = (torch.empty(n, d, dtype=torch.int8, device=dev), torch.empty(n, device=dev))
            ops.quantize_rows_i8(x[:1024].contiguous())                     # first-launch costs stay out of the timing
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codes, scales = ops.quantize_rows_i8(x, out=out)
            torch.cuda.synchronize()
            built[key] = (x, g, codes, scales, time.perf_counter() - t0)
        x, g, codes, scales, quant_s = built[key]
        q = queries(x, nq, g)
        ws = torch.empty(max(ops.retrieval_topk_workspace_bytes(nq, n, d, k), 1), dtype=torch.uint8, device=dev)
        out = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
        t_brute = _time(lambda: ops.retrieval_topk(q, x, k, workspace=ws, out=out), args.iters, args.warmup)
        exact = out[1].clone()
        del ws
        k1_default = ops.default_k1(k, n)
        for k1, rerank in ((k, False), (k, True), (k1_default, True)):
            c = x if rerank else None
            iws = torch.empty(max(ops.retrieval_topk_i8_workspace_bytes(nq, n, d, k, k1), 1), dtype=torch.uint8, device=dev)
            iout = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
            t_i8 = _time(lambda: ops.retrieval_topk_i8(q, codes, scales, k, c=c, k1=k1, workspace=iws, out=iout),
                         args.iters, args.warmup)
            nbytes = (nq + 31) // 32 * n * (d + 4) + (nq * k1 * d * 4 if rerank else 0)
            print(json.dumps({"nq": nq, "n": n, "d": d, "k": k, "k1": k1, "rerank": rerank, "i8_ms": round(t_i8, 4),
                              "brute_ms": round(t_brute, 4), "speedup": round(t_brute / t_i8, 2),
                              "recall": round(recall(iout[1], exact), 4), "bytes": nbytes,
                              "frac_hbm": round(nbytes / (t_i8 * 1e-3) / PEAK_HBM, 4), "quant_s": round(quant_s, 4)}),
                  flush=True)
            del iws, iout
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Exact top-k retrieval (tt_retrieval_topk_f32) timed on the shapes of serving and of offline recommendation, with the
rank pass (tt_retrieval_rank_f32: the same dot products, one count per query, no selection) timed on the same shape in the
same run as the yardstick.  One JSON line per shape:

    python bench_topk.py [--iters 20] [--warmup 3] [--shapes 0,1,2,3,4]

frac_mfma = 2 nq nc D / t / 157.3e12 (f32 MFMA peak), frac_hbm = nc D 4 / t / 8.0e12 (one read of the corpus).
"""
import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = [(1, 10_000_000, 128, 10), (16, 10_000_000, 128, 100), (1000, 1_000_000, 128, 100), (8192, 1_000_000, 128, 100),
          (1024, 10_000_000, 128, 100)]
PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


def _time(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
    args = ap.parse_args(argv)
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    corpus = {}
    for si in (int(x) for x in args.shapes.split(",")):
        nq, nc, d, k = SHAPES[si]
        if (nc, d) not in corpus:
            corpus.clear()
            torch.cuda.empty_cache()
            c = torch.empty(nc, d, device=dev)
            ops.fill_uniform_(c, 2024, 1, -1.0, 2.0)
            corpus[(nc, d)] = c
        c = corpus[(nc, d)]
        q = torch.empty(nq, d, device=dev)
        ops.fill_uniform_(q, 2024, 2, -1.0, 2.0)
        ws = torch.empty(ops.retrieval_topk_workspace_bytes(nq, nc, d, k), dtype=torch.uint8, device=dev)
        out = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
        t_topk = _time(lambda: ops.retrieval_topk(q, c, k, workspace=ws, out=out), args.iters, args.warmup)
        rws = torch.empty(ops.retrieval_rank_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=dev)
        pos = torch.zeros(nq, dtype=torch.int64, device=dev)
        rank = torch.empty(nq, dtype=torch.int32, device=dev)
        t_rank = _time(lambda: ops.retrieval_rank(q, c, 1.0, pos, workspace=rws, out=rank), args.iters, args.warmup)
        s = t_topk * 1e-3
        print(json.dumps({"nq": nq, "nc": nc, "d": d, "k": k, "topk_ms": round(t_topk, 4), "rank_ms": round(t_rank, 4),
                          "topk_over_rank": round(t_topk / t_rank, 3),
                          "frac_mfma": round(2.0 * nq * nc * d / s / PEAK_F32_MFMA, 4),
                          "frac_hbm": round(nc * d * 4 / s / PEAK_HBM, 4)}), flush=True)
        del ws, out, rws
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""IVF approximate top-k (serving.IVF / tt_ivf_search_f32) against exact BruteForce (tt_retrieval_topk_f32), both timed in
the same run on the same corpus.  One JSON line per (shape, nprobe):

    python bench_ivf.py [--iters 20] [--warmup 3] [--shapes 0,1,2,3] [--nprobe 8,32,128]

Corpus (seeded, generated on the device): `nclusters` unit directions d_c ~ normalize(N(0, I)); item j = d_{lab_j} +
1.5 / sqrt(D) * N(0, I) with lab_j uniform; queries = random items + 0.75 / sqrt(D) * N(0, I).  Uniform random vectors
would have no structure for an inverted file to use.

Fields: ivf_ms and brute_ms (per call), speedup = brute_ms / ivf_ms, recall = mean |ivf_r & exact_r| / k, rows_scanned =
the list rows the select kernel streams (each probed list once per 32-query tile that probes it), frac_hbm = rows_scanned
* D * 4 / t / 8.0e12, build_s = the index build (k-means + placement + reorder) in seconds.
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# (nq, n, D, k, nlist, nclusters)
SHAPES = [(1, 10_000_000, 128, 10, 4096, 20_000), (16, 10_000_000, 128, 100, 4096, 20_000),
          (1024, 10_000_000, 128, 100, 4096, 20_000), (8192, 1_000_000, 128, 100, 1024, 5_000)]
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


def corpus(n: int, d: int, nclusters: int, seed: int, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(nclusters, d, device=dev, generator=g), dim=1)
    x = torch.empty(n, d, device=dev)
    for s in range(0, n, 1 << 21):
        e = min(n, s + (1 << 21))
        lab = torch.randint(0, nclusters, (e - s,), device=dev, generator=g)
        x[s:e] = dirs[lab] + 1.5 / d ** 0.5 * torch.randn(e - s, d, device=dev, generator=g)
    return x, g


def queries(x, nq: int, g):
    n, d = x.shape
    pick = torch.randint(0, n, (nq,), device=x.device, generator=g)
    return (x[pick] + 0.75 / d ** 0.5 * torch.randn(nq, d, device=x.device, generator=g)).contiguous()


def rows_scanned(ivf, q, nprobe: int) -> int:
    from two_tower_amazon_recommender_amd import ops
    probes = ops.retrieval_topk(q, ivf.centroids, nprobe)[1].reshape(-1)
    per_list = torch.bincount(probes, minlength=ivf.nlist)
    lens = ivf.list_offsets.diff()
    return int((((per_list + 31) // 32) * lens).sum())


def recall(got: torch.Tensor, exact: torch.Tensor) -> float:
    g, e = got.cpu().numpy(), exact.cpu().numpy()
    return float(np.mean([len(np.intersect1d(a[a >= 0], b)) / b.shape[0] for a, b in zip(g, e)]))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
    ap.add_argument("--nprobe", default="8,32,128")
    args = ap.parse_args(argv)
    from two_tower_amazon_recommender_amd import ops
    from two_tower_amazon_recommender_amd.serving import IVF
    dev = torch.device("cuda:0")
    built = {}
    for si in (int(v) for v in args.shapes.split(",")):
        nq, n, d, k, nlist, ncl = SHAPES[si]
        key = (n, d, nlist)
        if key not in built:
            built.clear()
            torch.cuda.empty_cache()
            x, g = corpus(n, d, ncl, 2024, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ivf = IVF(k=k, nlist=nlist, nprobe=1, seed=0).index(x)
            torch.cuda.synchronize()
            built[key] = (x, g, ivf, time.perf_counter() - t0)
        x, g, ivf, build_s = built[key]
        q = queries(x, nq, g)
        ws = torch.empty(max(ops.retrieval_topk_workspace_bytes(nq, n, d, k), 1), dtype=torch.uint8, device=dev)
        out = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
        t_brute = _time(lambda: ops.retrieval_topk(q, x, k, workspace=ws, out=out), args.iters, args.warmup)
        exact = out[1].clone()
        del ws
        arrays = (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids)
        for nprobe in (int(v) for v in args.nprobe.split(",")):
            iws = torch.empty(max(ops.ivf_search_workspace_bytes(nq, nlist, n, d, k, nprobe), 1), dtype=torch.uint8, device=dev)
            iout = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
            t_ivf = _time(lambda: ops.ivf_search(q, *arrays, k, nprobe, workspace=iws, out=iout, check_offsets=False),
                          args.iters, args.warmup)
            rows = rows_scanned(ivf, q, nprobe)
            print(json.dumps({"nq": nq, "n": n, "d": d, "k": k, "nlist": nlist, "nprobe": nprobe, "ivf_ms": round(t_ivf, 4),
                              "brute_ms": round(t_brute, 4), "speedup": round(t_brute / t_ivf, 2),
                              "recall": round(recall(iout[1], exact), 4), "rows_scanned": rows,
                              "frac_hbm": round(rows * d * 4 / (t_ivf * 1e-3) / PEAK_HBM, 4),
                              "build_s": round(build_s, 3)}), flush=True)
            del iws, iout
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Int8 IVF (serving.Int8IVF / tt_ivf_search_i8_f32) against the f32 IVF (serving.IVF / tt_ivf_search_f32) over the same
lists and against exact BruteForce, all timed in the same run on bench_ivf.py's corpus and shapes.  One JSON line per
(shape, nprobe, k1, re-rank or not):

    python bench_ivf_i8.py [--iters 20] [--warmup 3] [--shapes 0,1,2,3] [--nprobe 8,32,128] [--variants stage1,k,default]
                           [--i8-only]

Both indexes are built with the same seed, and so hold the same lists (checked).  Per (shape, nprobe) the int8 search runs
with k1 = k without the re-rank (stage 1 only), with k1 = k and the re-rank, and with the default k1 = min(256, n,
max(4 k, 32)) and the re-rank.

Fields: ivf_i8_ms, ivf_ms and brute_ms (per call), vs_ivf = ivf_ms / ivf_i8_ms, vs_brute = brute_ms / ivf_i8_ms, recall =
mean |ivf_i8_r & exact_r| / k against the exact answer of the same run, agree_ivf = the same against IVF's answer, bytes =
what the call streams (rows_scanned * (D + 8): codes, scale and id of every list row, each probed list once per 32-query
tile that probes it; plus the re-ranked f32 rows nq * k1 * D * 4), frac_hbm = bytes / t / 8.0e12, build_s = the Int8IVF
build (k-means + placement + batched quantisation) and ivf_build_s = the IVF build, in seconds.

``--variants`` picks among the three (stage1: k1 = k, no re-rank; k: k1 = k; default: the default k1).  ``--i8-only`` times
the int8 search alone (the other fields are null): a kernel profile of such a run holds no launch of the other two paths,
which share the merge and coarse-probe kernels with it.
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

from bench_ivf import PEAK_HBM, SHAPES, _time, corpus, queries, recall, rows_scanned  # noqa: E402


def _timed_build(index, x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index.index(x)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
    ap.add_argument("--nprobe", default="8,32,128")
    ap.add_argument("--variants", default="stage1,k,default")
    ap.add_argument("--i8-only", action="store_true")
    args = ap.parse_args(argv)
    variants = args.variants.split(",")
    if not variants or any(v not in ("stage1", "k", "default") for v in variants):
        ap.error("--variants: a comma list of stage1, k, default")
    from two_tower_amazon_recommender_amd import ops
    from two_tower_amazon_recommender_amd.serving import IVF, Int8IVF
    dev = torch.device("cuda:0")
    built = {}
    for si in (int(v) for v in args.shapes.split(",")):
        nq, n, d, k, nlist, ncl = SHAPES[si]
        key = (n, d, nlist)
        if key not in built:
            built.clear()
            torch.cuda.empty_cache()
            x, g = corpus(n, d, ncl, 2024, dev)
            ivf = IVF(k=k, nlist=nlist, nprobe=1, seed=0)
            ivf_build_s = _timed_build(ivf, x)
            i8 = Int8IVF(k=k, nlist=nlist, nprobe=1, seed=0)
            build_s = _timed_build(i8, x)
            assert torch.equal(ivf.list_ids, i8.list_ids) and torch.equal(ivf.centroids, i8.centroids)
            built[key] = (x, g, ivf, i8, ivf_build_s, build_s)
        x, g, ivf, i8, ivf_build_s, build_s = built[key]
        q = queries(x, nq, g)
        t_brute = exact = None
        if not args.i8_only:
            ws = torch.empty(max(ops.retrieval_topk_workspace_bytes(nq, n, d, k), 1), dtype=torch.uint8, device=dev)
            out = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
            t_brute = _time(lambda: ops.retrieval_topk(q, x, k, workspace=ws, out=out), args.iters, args.warmup)
            exact = out[1].clone()
            del ws
        f32_arrays = (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids)
        i8_arrays = (i8.centroids, i8.list_offsets, i8.list_codes, i8.list_scales, i8.list_ids)
        k1_default = ops.default_k1(k, n)
        for nprobe in (int(v) for v in args.nprobe.split(",")):
            t_ivf = fout = None
            if not args.i8_only:
                fws = torch.empty(max(ops.ivf_search_workspace_bytes(nq, nlist, n, d, k, nprobe), 1), dtype=torch.uint8, device=dev)
                fout = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
                t_ivf = _time(lambda: ops.ivf_search(q, *f32_arrays, k, nprobe, workspace=fws, out=fout, check_offsets=False),
                              args.iters, args.warmup)
                del fws
            rows = rows_scanned(ivf, q, nprobe)
            for name, k1, rerank in (("stage1", k, False), ("k", k, True), ("default", k1_default, True)):
                if name not in variants:
                    continue
                c = x if rerank else None
                iws = torch.empty(max(ops.ivf_search_i8_workspace_bytes(nq, nlist, n, d, k, k1, nprobe), 1), dtype=torch.uint8,
                                  device=dev)
                iout = (torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev))
                t_i8 = _time(lambda: ops.ivf_search_i8(q, *i8_arrays, k, nprobe, c=c, k1=k1, workspace=iws, out=iout,
                                                       check_offsets=False), args.iters, args.warmup)
                nbytes = rows * (d + 8) + (nq * k1 * d * 4 if rerank else 0)
                print(json.dumps({"nq": nq, "n": n, "d": d, "k": k, "nlist": nlist, "nprobe": nprobe, "k1": k1, "rerank": rerank,
                                  "ivf_i8_ms": round(t_i8, 4), "ivf_ms": t_ivf and round(t_ivf, 4),
                                  "brute_ms": t_brute and round(t_brute, 4), "vs_ivf": t_ivf and round(t_ivf / t_i8, 2),
                                  "vs_brute": t_brute and round(t_brute / t_i8, 2),
                                  "recall": None if exact is None else round(recall(iout[1], exact), 4),
                                  "agree_ivf": None if fout is None else round(recall(iout[1], fout[1]), 4),
                                  "rows_scanned": rows, "bytes": nbytes,
                                  "frac_hbm": round(nbytes / (t_i8 * 1e-3) / PEAK_HBM, 4), "build_s": round(build_s, 3),
                                  "ivf_build_s": round(ivf_build_s, 3)}), flush=True)
                del iws, iout
            del fout
    return 0


if __name__ == "__main__":
    sys.exit(main())

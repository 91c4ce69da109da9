"""L2 normalisation of the tower outputs (tt_l2_normalize_fwd_f32 / tt_l2_normalize_bwd_f32) against a plain copy of the
same bytes, and the train step with cfg.normalize_embeddings off and on.  JSON lines, printed and appended to --out:

    python bench_l2norm.py [--iters 200] [--warmup 20] [--steps 300] [--rounds 3] [--out profiles/l2norm.jsonl]

Kernel lines ("what": "kernel"), for two towers of 8192 x 128 and 8192 x 256 in one launch:
  fwd_us / bwd_us        per launch, from replays of a HIP graph of `iters` back-to-back launches (no host time between them)
  copy_fwd_us / copy_bwd_us   one torch copy_ moving the same bytes (fwd: 2 towers x (4 read + 4 written) x rows x dim; bwd:
                         2 x (8 + 4) x rows x dim), timed the same way in the same run
  fwd_kernel_us / bwd_kernel_us   the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  fwd_to_copy / bwd_to_copy, and bytes / time as a fraction of 8.0e12 B/s
Step lines ("what": "step"): trainer.step at cfg3's batch, dims and towers (8192, 128, [256, 128], SGD, uniform ids) with small
tables, switch off and on alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise);
the median round of each, and their ratio.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PEAK_HBM = 8.0e12
SHAPES = [(8192, 128), (8192, 256)]


def _graph_us(fn, iters: int, warmup: int, replays: int = 5) -> float:
    """Microseconds per call of fn inside a replayed HIP graph of `iters` calls (the best of `replays`)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def _kernel_us(tag: str, fn, iters: int) -> float:
    from two_tower_amazon_recommender_amd import _lib
    _lib.profile_enable(tag, iters)
    for _ in range(iters):
        fn()
    ms, _ = _lib.profile_read(tag, iters)
    _lib.profile_enable("")
    return statistics.median(ms) * 1e3


def kernels(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    for rows, dim in SHAPES:
        g = torch.Generator(device=dev).manual_seed(rows + dim)
        xs = tuple(torch.randn(rows, dim, device=dev, generator=g) for _ in range(2))
        dys = tuple(torch.randn(rows, dim, device=dev, generator=g) for _ in range(2))
        ys = tuple(torch.empty_like(x) for x in xs)
        dxs = tuple(torch.empty_like(x) for x in xs)
        src2, dst2 = torch.randn(2 * rows, dim, device=dev, generator=g), torch.empty(2 * rows, dim, device=dev)
        src3, dst3 = torch.randn(3 * rows, dim, device=dev, generator=g), torch.empty(3 * rows, dim, device=dev)
        fwd = lambda: ops.l2_normalize2(xs, ys)                      # noqa: E731
        bwd = lambda: ops.l2_normalize_bwd2(xs, dys, dxs)            # noqa: E731
        t = {"fwd_us": _graph_us(fwd, args.iters, args.warmup), "bwd_us": _graph_us(bwd, args.iters, args.warmup),
             "copy_fwd_us": _graph_us(lambda: dst2.copy_(src2), args.iters, args.warmup),
             "copy_bwd_us": _graph_us(lambda: dst3.copy_(src3), args.iters, args.warmup),
             "fwd_kernel_us": _kernel_us("l2norm_fwd", fwd, args.iters), "bwd_kernel_us": _kernel_us("l2norm_bwd", bwd, args.iters)}
        fwd_bytes, bwd_bytes = 2 * 8 * rows * dim, 2 * 12 * rows * dim
        emit({"what": "kernel", "rows": rows, "dim": dim, "towers": 2, **{k: round(v, 3) for k, v in t.items()},
              "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
              "fwd_to_copy": round(t["fwd_us"] / t["copy_fwd_us"], 3), "bwd_to_copy": round(t["bwd_us"] / t["copy_bwd_us"], 3),
              "fwd_frac_hbm": round(fwd_bytes / (t["fwd_kernel_us"] * 1e-6) / PEAK_HBM, 4),
              "bwd_frac_hbm": round(bwd_bytes / (t["bwd_kernel_us"] * 1e-6) / PEAK_HBM, 4)})


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    n_users = n_items = 100_000
    batch, dim, towers = 8192, 128, [256, 128]
    trainers = {}
    for on in (False, True):
        cfg = TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=towers, temperature=0.1,
                             l2_regularization=1e-6, learning_rate=0.001, optimizer="sgd", batch_size=batch,
                             normalize_embeddings=on)
        trainers[on] = TwoTowerTrainer(cfg, dev, seed=1001)
    batches = [trainers[False].synthetic_batch(1001, s) for s in range(16)]
    times = {False: [], True: []}
    for rnd in range(args.rounds + 1):                                # round 0 warms both up
        for on in (False, True):
            tr = trainers[on]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                tr.step(*batches[s % len(batches)])
            torch.cuda.synchronize()
            if rnd:
                times[on].append((time.perf_counter() - t0) * 1e3 / args.steps)
    for tr in trainers.values():
        tr.check_ids()
    off, on = statistics.median(times[False]), statistics.median(times[True])
    emit({"what": "step", "batch": batch, "dim": dim, "tower_dims": towers, "table_rows": n_users, "optimizer": "sgd",
          "steps": args.steps, "rounds": args.rounds, "step_ms_off": round(off, 4), "step_ms_on": round(on, 4),
          "on_to_off": round(on / off, 4), "rounds_ms_off": [round(v, 4) for v in times[False]],
          "rounds_ms_on": [round(v, 4) for v in times[True]]})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "l2norm.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_l2norm.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    kernels(args, emit)
    steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

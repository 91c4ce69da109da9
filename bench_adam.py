"""Lazy Adam (tt_adam_step_f32: two launches) against Adagrad and SGD through the same sort-plan path (tt_optimizer_step_f32: one
launch), and the train step with the three optimizers.  JSON lines, printed and appended to --out:

    python bench_adam.py [--iters 200] [--warmup 20] [--steps 200] [--rounds 3] [--out profiles/adam.jsonl]

Optimizer lines ("what": "optimizer"), at cfg3's shape - 2 tables (5M and 10M rows) x 8192 ids x dim 128 plus the 8 segments of
two [256, 128] towers with 32 gradient slabs each - for uniform ("U") and power-law ("Z") ids; the sort plans run once, outside:
  adam_us / adagrad_us / sgd_us     per call, from replays of a HIP graph of `iters` back-to-back calls (no host time between them)
  adam_sparse_kernel_us, adam_finish_kernel_us, adagrad_kernel_us   the dispatches' own begin-to-end times (the library's built-in
                         timing, eager launches)
  adam_to_adagrad, target_us = 1.4 * adagrad_us + 4 (28*dim against 20*dim bytes per distinct row, one more launch at the
                         platform's 4.0 us floor), and algorithmic bytes / call time as a fraction of 8.0e12 B/s
Step lines ("what": "step"): trainer.step at cfg3 for sgd, adagrad and adam, alternating for `rounds` rounds of `steps` steps
(host clock around steps that end in a synchronise); the median round of each.
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
LAUNCH_FLOOR_US = 4.0                      # profiles/r04_launch_floor.txt
CFG3 = dict(n_users=5_000_000, n_items=10_000_000, dim=128, towers=[256, 128], batch=8192)


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


def _kernel_us(tags, fn, iters: int) -> dict:
    from two_tower_amazon_recommender_amd import _lib
    _lib.profile_enable(",".join(tags), iters)
    for _ in range(iters):
        fn()
    out = {t: statistics.median(_lib.profile_read(t, iters)[0]) * 1e3 for t in tags}
    _lib.profile_enable("")
    return out


def optimizer_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, batch, towers = CFG3["dim"], CFG3["batch"], CFG3["towers"]
    rows = (args.users, args.items)
    tables = [torch.empty(r, dim, device=dev).uniform_(-0.05, 0.05) for r in rows]
    accum = [torch.full_like(t, 0.1) for t in tables]
    mom = [torch.zeros_like(t) for t in tables]
    var = [torch.zeros_like(t) for t in tables]
    g = torch.Generator(device=dev).manual_seed(7)
    grads = [torch.randn(batch, dim, device=dev, generator=g) * 0.01 for _ in rows]
    n_slabs = ops.dense_bwd_num_slabs(batch)
    counts = []
    for _ in range(2):
        k = dim
        for n in towers:
            counts += [k * n, n]
            k = n
    prm = [torch.randn(c, device=dev, generator=g) * 0.1 for c in counts]
    acc_d = [torch.full_like(p, 0.1) for p in prm]
    m_d, v_d = [torch.zeros_like(p) for p in prm], [torch.zeros_like(p) for p in prm]
    slabs = [torch.randn(n_slabs, c, device=dev, generator=g) * 0.01 for c in counts]
    l2 = [1e-6 if i % 2 == 0 else 0.0 for i in range(len(counts))]
    segs = {opt: [ops.make_dense_seg(p, a if opt == "adagrad" else None, s, n_slabs, r) for p, a, s, r in zip(prm, acc_d, slabs, l2)]
            for opt in ("sgd", "adagrad")}
    adam_segs = [ops.make_adam_seg(p, m, v, s, n_slabs, r) for p, m, v, s, r in zip(prm, m_d, v_d, slabs, l2)]
    plans = [ops.SparsePlan(batch, dev) for _ in rows]
    hyper = ops.AdamHyper(lr=0.001, step=100)
    for variant in ("U", "Z"):
        ids = [torch.empty(batch, dtype=torch.int64, device=dev) for _ in rows]
        for i, r in enumerate(rows):
            ops.fill_ids_(ids[i], 1001, 3 + i, r, variant)
        ops.sparse_plan_batched(plans, ids, rows)
        distinct = [int(torch.unique(i).numel()) for i in ids]

        def adam():
            ops.adam_step_([(t, m, v, gr, p) for t, m, v, gr, p in zip(tables, mom, var, grads, plans)], adam_segs, hyper)

        def plan_path(opt):
            return lambda: ops.optimizer_step_(opt, [(t, a if opt == "adagrad" else None, gr, p)
                                                     for t, a, gr, p in zip(tables, accum, grads, plans)], segs[opt], 0.001)
        t = {"adam_us": _graph_us(adam, args.iters, args.warmup)}
        for opt in ("adagrad", "sgd"):
            t[f"{opt}_us"] = _graph_us(plan_path(opt), args.iters, args.warmup)
        t["adam_us_again"] = _graph_us(adam, args.iters, args.warmup)          # the spread of the method: the first figure, repeated
        k = _kernel_us(["adam_sparse", "adam_finish"], adam, args.iters)
        t["adam_sparse_kernel_us"], t["adam_finish_kernel_us"] = k["adam_sparse"], k["adam_finish"]
        t["adagrad_kernel_us"] = _kernel_us(["optimizer"], plan_path("adagrad"), args.iters)["optimizer"]
        # algorithmic bytes: every gradient row, sorted id and position once; per distinct row w (+ state) read and written;
        # per dense element the slabs, and the parameter (+ state) read and written
        def nbytes(state_rows):
            sparse = sum(batch * (4 * dim + 12) + d * 8 * dim * (1 + state_rows) for d in distinct)
            return sparse + sum(c * (4 * n_slabs + 8 * (1 + state_rows)) for c in counts)
        target = 1.4 * t["adagrad_us"] + LAUNCH_FLOOR_US
        emit({"what": "optimizer", "ids": variant, "tables": list(rows), "n_ids": batch, "dim": dim, "distinct": distinct,
              "segments": len(counts), "n_slabs": n_slabs, **{k2: round(v2, 3) for k2, v2 in t.items()},
              "adam_to_adagrad": round(t["adam_us"] / t["adagrad_us"], 3), "target_us": round(target, 3),
              "target_with_spread_us": round(1.1 * target, 3), "meets_target": bool(t["adam_us"] <= 1.1 * target),
              "adam_bytes": nbytes(2), "adagrad_bytes": nbytes(1), "sgd_bytes": nbytes(0),
              "adam_frac_hbm": round(nbytes(2) / (t["adam_us"] * 1e-6) / PEAK_HBM, 4),
              "adagrad_frac_hbm": round(nbytes(1) / (t["adagrad_us"] * 1e-6) / PEAK_HBM, 4),
              "sgd_frac_hbm": round(nbytes(0) / (t["sgd_us"] * 1e-6) / PEAK_HBM, 4)})


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    opts = ("sgd", "adagrad", "adam")
    trainers = {}
    for opt in opts:
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer=opt, batch_size=CFG3["batch"])
        trainers[opt] = TwoTowerTrainer(cfg, dev, seed=1001)
    for variant in ("U", "Z"):
        batches = [trainers["sgd"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {opt: [] for opt in opts}
        for rnd in range(args.rounds + 1):                                # round 0 warms all three up
            for opt in opts:
                tr = trainers[opt]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    tr.step(*batches[s % len(batches)])
                torch.cuda.synchronize()
                if rnd:
                    times[opt].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for tr in trainers.values():
            tr.check_ids()
        med = {opt: statistics.median(times[opt]) for opt in opts}
        emit({"what": "step", "ids": variant, "batch": CFG3["batch"], "dim": CFG3["dim"], "tower_dims": CFG3["towers"],
              "tables": [args.users, args.items], "steps": args.steps, "rounds": args.rounds,
              **{f"step_ms_{opt}": round(med[opt], 4) for opt in opts},
              "adam_to_adagrad": round(med["adam"] / med["adagrad"], 4), "adam_to_sgd": round(med["adam"] / med["sgd"], 4),
              **{f"rounds_ms_{opt}": [round(v, 4) for v in times[opt]] for opt in opts}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--users", type=int, default=CFG3["n_users"], help="rows of the first table (cfg3: 5,000,000)")
    ap.add_argument("--items", type=int, default=CFG3["n_items"], help="rows of the second table (cfg3: 10,000,000)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adam.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    optimizer_phase(args, emit)
    torch.cuda.empty_cache()
    steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

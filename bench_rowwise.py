"""Row-wise Adagrad (tt_rowwise_adagrad_step_f32: two launches) against Adagrad (tt_sparse_adagrad_f32) and lazy Adam
(tt_adam_step_f32) over the same sort plan, and the cfg3 train step with rowwise_adagrad against adagrad.  JSON lines, printed and
appended to --out:

    python bench_rowwise.py [--iters 200] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/rowwise.jsonl]

Sparse lines ("what": "sparse"): ONE table of 10M rows x dim 128, lists of 8192 and 1M ids, uniform ("U") and power-law ("Z");
the sort plan runs once, outside:
  rowwise_us / adagrad_us / adam_us   per call, from replays of a HIP graph of back-to-back calls (no host time between them; the
                         1M lists use iters / 10 calls); rowwise_us_again: the first figure repeated, the spread of the method
  rowwise_sparse_kernel_us, rowwise_finish_kernel_us   the dispatches' own begin-to-end times (the library's built-in timing)
  *_frac_hbm             the byte model per DISTINCT row - rowwise 12*dim + 20, Adagrad 20*dim + 12, Adam 28*dim + 12 - over the
                         call time, as a fraction of 8.0e12 B/s;  *_frac_hbm_occ: the same with the gradient row, sorted id and
                         position counted per OCCURRENCE (what a list with duplicates really reads)
Step lines ("what": "step"): trainer.step at cfg3 for adagrad and rowwise_adagrad, alternating for `rounds` rounds of `steps`
steps in one process (host clock around steps that end in a synchronise); the median round of each, and the optimizer-state
bytes of both.
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

from bench_adam import CFG3, PEAK_HBM, _graph_us, _kernel_us  # noqa: E402


def sparse_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, rows = CFG3["dim"], args.rows
    table = torch.empty(rows, dim, device=dev).uniform_(-0.05, 0.05)
    row_accum = torch.full((rows,), 0.1, device=dev)
    accum = torch.full_like(table, 0.1)
    mom, var = torch.zeros_like(table), torch.zeros_like(table)
    g = torch.Generator(device=dev).manual_seed(7)
    hyper = ops.AdamHyper(lr=0.001, step=100)
    for n in args.ids:
        grads = torch.randn(n, dim, device=dev, generator=g) * 0.01
        plan = ops.SparsePlan(n, dev)
        iters = args.iters if n <= 65536 else max(args.iters // 10, 5)
        for variant in ("U", "Z"):
            ids = torch.empty(n, dtype=torch.int64, device=dev)
            ops.fill_ids_(ids, 1001, 3, rows, variant)
            plan.run(ids, rows)
            distinct = int(torch.unique(ids).numel())

            def rowwise():
                ops.rowwise_adagrad_step_([(table, row_accum, grads, plan)], [], 0.001, 1e-7)

            def adagrad():
                ops.sparse_adagrad_(table, accum, grads, plan, 0.001, 1e-7)

            def adam():
                ops.adam_step_([(table, mom, var, grads, plan)], [], hyper)
            t = {"rowwise_us": _graph_us(rowwise, iters, args.warmup)}
            t["adagrad_us"] = _graph_us(adagrad, iters, args.warmup)
            t["adam_us"] = _graph_us(adam, iters, args.warmup)
            t["rowwise_us_again"] = _graph_us(rowwise, iters, args.warmup)
            k = _kernel_us(["rowwise_sparse", "rowwise_finish"], rowwise, iters)
            t["rowwise_sparse_kernel_us"], t["rowwise_finish_kernel_us"] = k["rowwise_sparse"], k["rowwise_finish"]
            per_row = {"rowwise": 12 * dim + 20, "adagrad": 20 * dim + 12, "adam": 28 * dim + 12}
            per_occ = {"rowwise": n * (4 * dim + 12) + distinct * (8 * dim + 8), "adagrad": n * (4 * dim + 12) + distinct * 16 * dim,
                       "adam": n * (4 * dim + 12) + distinct * 24 * dim}
            emit({"what": "sparse", "ids": variant, "rows": rows, "n_ids": n, "dim": dim, "distinct": distinct, "calls_per_graph": iters,
                  **{k2: round(v2, 3) for k2, v2 in t.items()},
                  "rowwise_to_adagrad": round(t["rowwise_us"] / t["adagrad_us"], 3), "rowwise_to_adam": round(t["rowwise_us"] / t["adam_us"], 3),
                  "byte_model_rowwise_to_adagrad": round(per_row["rowwise"] / per_row["adagrad"], 3),
                  **{f"{o}_bytes": distinct * per_row[o] for o in per_row},
                  **{f"{o}_frac_hbm": round(distinct * per_row[o] / (t[f"{o}_us"] * 1e-6) / PEAK_HBM, 4) for o in per_row},
                  **{f"{o}_frac_hbm_occ": round(per_occ[o] / (t[f"{o}_us"] * 1e-6) / PEAK_HBM, 4) for o in per_row}})


def _state_bytes(tr) -> int:
    state = [x for t in tr.tables.values() for x in (t.accum, t.m, t.v, t.row_accum)] + [tr.dense_accum, tr.dense_m, tr.dense_v]
    return sum(x.numel() * x.element_size() for x in state if x is not None)


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    opts = ("adagrad", "rowwise_adagrad")
    trainers = {}
    for opt in opts:
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer=opt, batch_size=CFG3["batch"])
        trainers[opt] = TwoTowerTrainer(cfg, dev, seed=1001)
    for variant in ("U", "Z"):
        batches = [trainers["adagrad"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {opt: [] for opt in opts}
        for rnd in range(args.rounds + 1):                                # round 0 warms both up
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
              "rowwise_to_adagrad": round(med["rowwise_adagrad"] / med["adagrad"], 4),
              **{f"state_bytes_{opt}": _state_bytes(trainers[opt]) for opt in opts},
              **{f"rounds_ms_{opt}": [round(v, 4) for v in times[opt]] for opt in opts}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows of the sparse phase's table")
    ap.add_argument("--ids", type=int, nargs="+", default=[8192, 1 << 20], help="id-list lengths of the sparse phase")
    ap.add_argument("--users", type=int, default=CFG3["n_users"], help="rows of the step phase's user table (cfg3: 5,000,000)")
    ap.add_argument("--items", type=int, default=CFG3["n_items"], help="rows of the step phase's item table (cfg3: 10,000,000)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rowwise.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowwise.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    sparse_phase(args, emit)
    torch.cuda.empty_cache()
    steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The time-of-interaction context features: the forward launch (tt_time_context_fwd_f32, the user row as its base) and the
backward launch (tt_time_context_bwd_f32) beside their torch eager equivalents on the same device, and the cfg3 train step with and
without the feature.  JSON lines, printed and appended to --out:

    python bench_time.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/time_context.jsonl]

Kernel lines ("what": "time_kernels"): 8192 pairs x dim 128, all four fields, N in {64, 1000, 4096} period buckets, on "uniform"
timestamps (uniform over a five-year range) and on "one_hour" (every pair inside one hour: every adder of the hour, day-of-week
and month fields on ONE row each, and on one or two period rows - the backward launch's worst case).
  fwd_us / bwd_us / torch_fwd_us / torch_bwd_us   per call, from replays of a HIP graph of `iters` back-to-back calls (no host time
                                between them; the best of five replays); *_again: the same measurement repeated - the spread of
                                the method
  fwd_kernel_us / bwd_kernel_us the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_fwd is users.index_select(0, ids) + table[rows].sum(1) with the row numbers [n, F] GIVEN (the launch derives them from the
  timestamps itself); torch_bwd is grad.zero_() + one index_add_ per field (float atomics).
  launch_floor_us: the empty-kernel floor the README records, for scale.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) without the feature and with it (all fields, --buckets
periods), in the same process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a
synchronise); the median round of each and every round's time, on uniform ("U") and power-law ("Z") ids.  The base of the ratio is
the step WITHOUT the feature (which keeps the fused lookup and the one-call step; the feature materialises the tower inputs).
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

from bench_adam import CFG3, LAUNCH_FLOOR_US, _graph_us, _kernel_us  # noqa: E402

ALL = ("hour", "day_of_week", "month", "period")
T_MIN = 1_000_000_000
T_MAX = T_MIN + 5 * 365 * 86400


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, n = CFG3["dim"], CFG3["batch"]
    g = torch.Generator(device=dev).manual_seed(7)
    users = torch.randn(args.users, dim, device=dev, generator=g) * 0.05
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    ops.fill_ids_(ids, 1001, 3, args.users, "Z")
    dy = torch.randn(n, dim, device=dev, generator=g) * 0.01
    stamps = {"uniform": torch.randint(T_MIN, T_MAX + 1, (n,), device=dev, generator=g),
              "one_hour": torch.randint(T_MIN + 86400 * 700, T_MIN + 86400 * 700 + 3600, (n,), device=dev, generator=g)}
    for buckets in (64, 1000, 4096):
        offs, R = ops.time_field_layout(ALL, buckets)
        table = torch.randn(R, dim, device=dev, generator=g) * 0.05
        for data, ts in stamps.items():
            out, idx = torch.empty(n, dim, device=dev), torch.empty(n, 4, dtype=torch.int32, device=dev)
            grad, tgrad = torch.empty(R, dim, device=dev), torch.empty(R, dim, device=dev)

            def fwd():
                ops.time_context(ts, table, ALL, buckets, T_MIN, T_MAX, out=out, base=(users, ids), idx_out=idx)

            def bwd():
                ops.time_context_bwd(idx, dy, ALL, buckets, grad=grad)
            fwd()
            rows = idx.long() + torch.tensor([offs[f] for f in ALL], device=dev)

            def torch_fwd():
                return users.index_select(0, ids) + table[rows].sum(1)

            def torch_bwd():
                tgrad.zero_()
                for k in range(4):
                    tgrad.index_add_(0, rows[:, k], dy)
            err = ((out - torch_fwd()).abs().max() / out.abs().max()).item()
            bwd()
            torch_bwd()
            gerr = ((grad - tgrad).abs().max() / tgrad.abs().max()).item()
            if not (err <= 1e-5 and gerr <= 1e-4):
                raise SystemExit(f"bench_time.py: the launches and the torch forms disagree (relative errors {err:.2e}, {gerr:.2e})")
            t = {}
            for again in ("", "_again"):
                for name, fn in (("fwd_us", fwd), ("bwd_us", bwd), ("torch_fwd_us", torch_fwd), ("torch_bwd_us", torch_bwd)):
                    t[name + again] = _graph_us(fn, args.iters, args.warmup)
            t["fwd_kernel_us"] = _kernel_us(["time_context_fwd"], fwd, args.iters)["time_context_fwd"]
            t["bwd_kernel_us"] = _kernel_us(["time_context_bwd"], bwd, args.iters)["time_context_bwd"]
            hot = int(torch.bincount(rows.view(-1), minlength=R).max().item())
            emit({"what": "time_kernels", "timestamps": data, "rows": n, "dim": dim, "fields": list(ALL), "buckets": buckets, "table_rows": R,
                  "adders_on_hottest_row": hot, **{k: round(v, 3) for k, v in t.items()}, "launch_floor_us": LAUNCH_FLOOR_US,
                  "torch_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3),
                  "fwd_vs_torch_rel_err": float(f"{err:.3e}"), "bwd_vs_torch_rel_err": float(f"{gerr:.3e}")})


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name, kw in (("plain", {}), ("time", dict(time_fields=ALL, time_buckets=args.buckets, time_min=T_MIN, time_max=T_MAX))):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], **kw)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    stamps = [trainers["time"].synthetic_timestamps(1001, s) for s in range(16)]
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms both up
            for name, t in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    k = s % len(batches)
                    if name == "time":
                        t.step(*batches[k], timestamps=stamps[k])
                    else:
                        t.step(*batches[k])
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for t in trainers.values():
            t.check_ids()
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"what": "step", "ids": variant, "optimizer": "adagrad", "batch": CFG3["batch"], "dim": CFG3["dim"],
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "fields": list(ALL), "buckets": args.buckets,
              "steps": args.steps, "rounds": args.rounds, "step_ms_plain": round(med["plain"], 4),
              "step_ms_time": round(med["time"], 4), "time_to_plain": round(med["time"] / med["plain"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buckets", type=int, default=1000, help="period buckets of the step lines")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_context.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_time.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    kernel_phase(args, emit)
    torch.cuda.empty_cache()
    if not args.skip_steps:
        steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The pooled item-title feature: the bag forward kernel (tt_embedding_bag_fwd_f32) beside torch.nn.functional.embedding_bag on
the same device, and the cfg3 train step with and without the feature.  JSON lines, printed and appended to --out:

    python bench_title.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/title.jsonl]

Forward lines ("what": "bag_fwd"): n_bags 8192 and 1M (identity bags) x L 16 x dim 128 over a --buckets-row table, mean pooling,
uniform ("U") and power-law ("Z") tokens, a quarter of the slots padding:
  bag_us / torch_us     per call, from replays of a HIP graph of `iters` back-to-back calls (no host time between them)
  bag_kernel_us         the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  bytes = 4 * dim * (sum(cnt) + 2 * n_bags) - every valid token's row read, one row per bag written and (when accumulating) read -
  and bytes / call time as a fraction of 8.0e12 B/s.  Nothing here is a target: the yardstick is the gather's fraction
  (DESIGN.md section 4, K1).
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad) without the feature and with it (--buckets rows, L 16, mean),
alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median round of each.
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


def _eager_us(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def forward_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, L = CFG3["dim"], args.max_tokens
    table = torch.empty(args.buckets, dim, device=dev).uniform_(-0.05, 0.05)
    g = torch.Generator(device=dev).manual_seed(7)
    for n_bags in (8192, 1 << 20):
        iters = args.iters if n_bags <= 8192 else max(args.iters // 10, 5)
        out = torch.zeros(n_bags, dim, device=dev)
        for variant in ("U", "Z"):
            tok64 = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
            ops.fill_ids_(tok64, 1001, 8, args.buckets, variant)
            pad = torch.rand(n_bags * L, device=dev, generator=g) < 0.25
            tokens = torch.where(pad, -1, tok64).to(torch.int32).view(n_bags, L).contiguous()
            cnt = int((tokens >= 0).sum().item())
            # torch: the padding id is an extra row behind the table
            tpad = torch.cat([table, torch.zeros(1, dim, device=dev)])
            idx = torch.where(tokens < 0, args.buckets, tokens.to(torch.int64))

            def bag():
                ops.embedding_bag(table, tokens, pooling="mean", out=out, accumulate=True)

            def ref():
                torch.nn.functional.embedding_bag(idx, tpad, mode="mean", padding_idx=args.buckets)
            t = {"bag_us": _graph_us(bag, iters, args.warmup)}
            try:
                t["torch_us"], torch_timing = _graph_us(ref, iters, args.warmup), "graph"
            except RuntimeError:                # an op that cannot be captured: device events around eager calls (host time included)
                torch.cuda.synchronize()
                t["torch_us"], torch_timing = _eager_us(ref, iters, args.warmup), "eager"
            t["bag_us_again"] = _graph_us(bag, iters, args.warmup)             # the spread of the method
            t["bag_kernel_us"] = _kernel_us(["bag_fwd"], bag, iters)["bag_fwd"]
            nbytes = 4 * dim * (cnt + 2 * n_bags)
            emit({"what": "bag_fwd", "tokens": variant, "n_bags": n_bags, "L": L, "dim": dim, "buckets": args.buckets,
                  "pooling": "mean", "accumulate": True, "torch_timing": torch_timing, "valid_slots": cnt, "distinct": int(torch.unique(tokens).numel()) - 1,
                  **{k: round(v, 3) for k, v in t.items()}, "bytes": nbytes,
                  "bag_frac_hbm": round(nbytes / (t["bag_us"] * 1e-6) / PEAK_HBM, 4),
                  "bag_kernel_frac_hbm": round(nbytes / (t["bag_kernel_us"] * 1e-6) / PEAK_HBM, 4),
                  "torch_frac_hbm": round(nbytes / (t["torch_us"] * 1e-6) / PEAK_HBM, 4),
                  "torch_to_bag": round(t["torch_us"] / t["bag_us"], 3)})
            del tok64, pad, tokens, tpad, idx
        del out
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name, buckets in (("plain", 0), ("title", args.buckets)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], n_title_buckets=buckets, title_max_tokens=args.max_tokens)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    trainers["title"].set_item_titles(trainers["title"].synthetic_item_titles(1001))
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms both up
            for name, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    tr.step(*batches[s % len(batches)])
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for tr in trainers.values():
            tr.check_ids()
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"what": "step", "ids": variant, "optimizer": "adagrad", "batch": CFG3["batch"], "dim": CFG3["dim"],
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "title_buckets": args.buckets, "L": args.max_tokens,
              "steps": args.steps, "rounds": args.rounds, "step_ms_plain": round(med["plain"], 4),
              "step_ms_title": round(med["title"], 4), "title_to_plain": round(med["title"] / med["plain"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--buckets", type=int, default=1_000_000, help="rows of the title table")
    ap.add_argument("--max-tokens", type=int, default=16)
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the forward lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "title.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_title.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    forward_phase(args, emit)
    torch.cuda.empty_cache()
    if not args.skip_steps:
        steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

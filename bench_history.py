"""The pooled user-history feature: the one-launch tower input (tt_history_bag_fwd_f32 with exclude and base) beside the
two-launch form (embedding_gather, then the accumulating tt_embedding_bag_fwd_f32) and torch.nn.functional.embedding_bag on the
same device, and the cfg3 train step with and without the feature.  JSON lines, printed and appended to --out:

    python bench_history.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/history.jsonl]

Kernel lines ("what": "history_fwd"): 8192 bags x dim 128 x L in {8, 20, 64} over a --items-row history table and a
--users-row base table; power-law ("Z") users and items, every user's history holds 1..L items (left-aligned), half of the
pairs' positives stand in their user's history (and are left out).  All three forms pool the SAME slots: the two-launch form and
torch run on the pre-masked per-bag token matrix.
  one_us / two_us / torch_us    per call, from replays of a HIP graph of `iters` back-to-back calls (no host time between them; the
                                best of five replays); *_again: the same measurement repeated - the spread of the method
  one_kernel_us                 the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  two_kernel_us                 the same for the gather and the bag dispatch, summed
  torch_us is the pooling alone (no base row is added): embedding_bag(mode="mean", padding_idx)
  bytes = 4 * dim * (sum(cnt) + 2 * n_bags) - every pooled slot's row read, one base row read and one row written per bag (the
  two-launch form moves 2 * n_bags more rows: the gathered rows written and read back) - and bytes / call time, also as a
  fraction of 8.0e12 B/s.  Nothing here is a target.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) without the feature and with it (L 20, mean), in the same
process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median round
of each and every round's time.  The base of the ratio is the step WITHOUT the feature.
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


def synthetic_histories(n_users: int, n_items: int, L: int, dev, seed: int = 1001) -> torch.Tensor:
    """int32 [n_users, L]: power-law items, 1..L of them per user, left-aligned, the rest padding."""
    from two_tower_amazon_recommender_amd import ops
    tok = torch.empty(n_users * L, dtype=torch.int64, device=dev)
    length = torch.empty(n_users, dtype=torch.int64, device=dev)
    ops.fill_ids_(tok, seed, 12, n_items, "Z")
    ops.fill_ids_(length, seed, 13, L, "U")
    slot = torch.arange(L, device=dev)
    return torch.where(slot[None, :] <= length[:, None], tok.view(n_users, L), -1).to(torch.int32).contiguous()


def forward_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, n_bags = CFG3["dim"], CFG3["batch"]
    table = torch.empty(args.items, dim, device=dev).uniform_(-0.05, 0.05)
    base_table = torch.empty(args.users, dim, device=dev).uniform_(-0.05, 0.05)
    tpad = torch.cat([table, torch.zeros(1, dim, device=dev)])       # torch: the padding id is an extra row behind the table
    users = torch.empty(n_bags, dtype=torch.int64, device=dev)
    ops.fill_ids_(users, 1001, 3, args.users, "Z")
    out = torch.zeros(n_bags, dim, device=dev)
    for L in (8, 20, 64):
        hist = synthetic_histories(args.users, args.items, L, dev)
        items = torch.empty(n_bags, dtype=torch.int64, device=dev)
        ops.fill_ids_(items, 1001, 4, args.items, "Z")
        own = hist[users, 0].to(torch.int64)                          # (slot 0 is always valid)
        items = torch.where(torch.arange(n_bags, device=dev) % 2 == 0, own, items)
        per = hist[users]
        per = torch.where(per.to(torch.int64) == items[:, None], -1, per).contiguous()       # the pre-masked per-bag matrix
        cnt = int((per >= 0).sum().item())
        excluded = int(((hist[users] >= 0) & (per < 0)).sum().item())
        idx = torch.where(per < 0, args.items, per.to(torch.int64))

        def one():
            ops.history_bag(table, hist, bag_rows=users, exclude=items, base=(base_table, users), pooling="mean", out=out)

        def two():
            ops.embedding_gather(base_table, users, out=out)
            ops.embedding_bag(table, per, pooling="mean", out=out, accumulate=True)

        def ref():
            torch.nn.functional.embedding_bag(idx, tpad, mode="mean", padding_idx=args.items)
        one()
        a = out.clone()
        two()
        if not torch.equal(a, out):
            raise SystemExit("bench_history.py: the one-launch and the two-launch form disagree")
        t = {"one_us": _graph_us(one, args.iters, args.warmup), "two_us": _graph_us(two, args.iters, args.warmup)}
        try:
            t["torch_us"], torch_timing = _graph_us(ref, args.iters, args.warmup), "graph"
        except RuntimeError:                    # an op that cannot be captured: device events around eager calls (host time included)
            torch.cuda.synchronize()
            from bench_title import _eager_us
            t["torch_us"], torch_timing = _eager_us(ref, args.iters, args.warmup), "eager"
        t["one_us_again"], t["two_us_again"] = _graph_us(one, args.iters, args.warmup), _graph_us(two, args.iters, args.warmup)
        t["one_kernel_us"] = _kernel_us(["bag_fwd"], one, args.iters)["bag_fwd"]
        t["two_kernel_us"] = sum(_kernel_us(["gather", "bag_fwd"], two, args.iters).values())
        nbytes = 4 * dim * (cnt + 2 * n_bags)
        emit({"what": "history_fwd", "tokens": "Z", "n_bags": n_bags, "L": L, "dim": dim, "table_rows": args.items,
              "base_rows": args.users, "pooling": "mean", "torch_timing": torch_timing, "pooled_slots": cnt, "excluded_slots": excluded,
              **{k: round(v, 3) for k, v in t.items()}, "bytes": nbytes,
              **{f"{k}_bytes_per_s": round(nbytes / (t[f"{k}_us"] * 1e-6), 0) for k in ("one", "two", "torch")},
              **{f"{k}_frac_hbm": round(nbytes / (t[f"{k}_us"] * 1e-6) / PEAK_HBM, 4) for k in ("one", "two", "torch", "one_kernel")},
              "two_to_one": round(t["two_us"] / t["one_us"], 3), "torch_to_one": round(t["torch_us"] / t["one_us"], 3)})
        del hist, per, idx, items, own
    del table, base_table, tpad, out
    torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    L = args.history_len
    trainers = {}
    for name, hl in (("plain", 0), ("history", L)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], user_history_len=hl)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    trainers["history"].set_user_histories(synthetic_histories(args.users, args.items, L, dev))
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        # half of the pairs' positives stand in their user's history, as after training on those pairs
        hist = trainers["history"].user_history
        batches = [(u, torch.where(torch.arange(u.numel(), device=dev) % 2 == 0, hist[u, 0].to(torch.int64), i)) for u, i in batches]
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
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "L": L, "pooling": "mean",
              "steps": args.steps, "rounds": args.rounds, "step_ms_plain": round(med["plain"], 4),
              "step_ms_history": round(med["history"], 4), "history_to_plain": round(med["history"] / med["plain"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--history-len", type=int, default=20, help="L of the step lines")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_history.py needs a GPU: nothing here is measured on the CPU")
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

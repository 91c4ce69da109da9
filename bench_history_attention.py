"""Attention pooling of the user history: the forward and the backward launch (tt_history_attention_fwd_f32 /
tt_history_attention_bwd_f32) beside the mean-pooling history_bag launch at the same shape and a torch eager equivalent on the
same device, and the cfg3 train step with mean and with attention pooling.  JSON lines, printed and appended to --out:

    python bench_history_attention.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/history_attention.jsonl]

Kernel lines ("what": "history_attention"): 8192 bags x dim 128 x L in {8, 20, 64} over a --items-row history table and a
--users-row base table - bench_history.py's problem: power-law ("Z") users and items, every user's history holds 1..L items, half
of the pairs' positives stand in their user's history (and are left out).  attn = [a ~ N(0, 20^2) | p ~ N(0, 1)]: logits of
order 1 on rows in U(-0.05, 0.05).
  fwd_us / mean_us / bwd_us     per call, from replays of a HIP graph of `iters` back-to-back calls (the best of five replays),
                                measured alternating, twice (*_again: the spread of the method); mean_us is the history_bag launch
  fwd_kernel_us / bwd_kernel_us the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_fwd_us / torch_bwd_us   the eager equivalent on the pre-masked per-bag token matrix (index_select -> matmul -> masked
                                softmax -> bmm, + the base rows) and its autograd backward w.r.t. the table (dense) and attn:
                                device events around eager calls, host time included
  fwd_bytes = 4 dim (sum(cnt) + 3 n_bags), bwd_bytes = 4 dim (2 sum(cnt) + 2 n_bags), and bytes / call time as a fraction of
  8.0e12 B/s.  Nothing here is a target.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192, L 20) with mean pooling - the step as it was - and with
attention pooling, in the same process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a
synchronise), on uniform and on power-law ids; the median round of each and every round's time.
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
from bench_history import synthetic_histories  # noqa: E402
from bench_rating import _eager_us  # noqa: E402


def _attn(dim: int, L: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(11)
    return torch.cat([20.0 * torch.randn(dim, device=dev, generator=g), torch.randn(L, device=dev, generator=g)])


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, n_bags = CFG3["dim"], CFG3["batch"]
    table = torch.empty(args.items, dim, device=dev).uniform_(-0.05, 0.05)
    base_table = torch.empty(args.users, dim, device=dev).uniform_(-0.05, 0.05)
    users = torch.empty(n_bags, dtype=torch.int64, device=dev)
    ops.fill_ids_(users, 1001, 3, args.users, "Z")
    out, out_mean = torch.zeros(n_bags, dim, device=dev), torch.zeros(n_bags, dim, device=dev)
    dy = torch.randn(n_bags, dim, device=dev) * 0.01
    for L in (8, 20, 64):
        hist = synthetic_histories(args.users, args.items, L, dev)
        items = torch.empty(n_bags, dtype=torch.int64, device=dev)
        ops.fill_ids_(items, 1001, 4, args.items, "Z")
        own = hist[users, 0].to(torch.int64)                          # (slot 0 is always valid)
        items = torch.where(torch.arange(n_bags, device=dev) % 2 == 0, own, items)
        per = hist[users]
        per = torch.where(per.to(torch.int64) == items[:, None], -1, per).contiguous()       # the pre-masked per-bag matrix
        cnt = int((per >= 0).sum().item())
        attn = _attn(dim, L, dev)
        ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
        weights, pooled = torch.empty(n_bags, L, device=dev), torch.empty(n_bags, dim, device=dev)
        slot_grads = torch.zeros(n_bags * L, dim, device=dev)
        slabs = torch.empty(ops.history_attention_num_slabs(n_bags), dim + L, device=dev)

        def fwd():
            ops.history_attention(table, hist, attn, bag_rows=users, exclude=items, base=(base_table, users), out=out, batch_ids=ids,
                                  weights=weights, pooled=pooled)

        def mean():
            ops.history_bag(table, hist, bag_rows=users, exclude=items, base=(base_table, users), pooling="mean", out=out_mean)

        def bwd():
            ops.history_attention_bwd(table, ids, weights, pooled, dy, attn, L, slot_grads=slot_grads, dattn_slabs=slabs)

        # the torch eager equivalent, on the gathered rows of the table (the table's gradient is left sparse: the rows' gradient)
        valid = per >= 0
        idx = per.clamp(min=0).to(torch.int64).reshape(-1)
        rank = (valid.flip(1).cumsum(1).flip(1) - valid.to(torch.int64)).clamp(0, L - 1)
        a_t = attn.clone().requires_grad_(True)
        state = {}

        def torch_fwd():
            rows = table.index_select(0, idx).view(n_bags, L, dim).requires_grad_(True)
            e = torch.matmul(rows, a_t[:dim]) * (dim ** -0.5) + a_t[dim:][rank]
            w = torch.softmax(e.masked_fill(~valid, float("-inf")), dim=1).nan_to_num(0.0)
            state["rows"], state["out"] = rows, base_table.index_select(0, users) + torch.bmm(w.unsqueeze(1), rows).squeeze(1)

        def torch_bwd():
            torch.autograd.grad(state["out"], (state["rows"], a_t), dy, retain_graph=True)

        fwd(); torch_fwd()
        err = (out - state["out"]).abs().max().item() / state["out"].abs().max().item()
        if not err <= 1e-4:
            raise SystemExit(f"bench_history_attention.py: the launch and the torch equivalent disagree ({err:.2e})")
        t = {}
        for again in ("", "_again"):
            for k, fn in (("fwd", fwd), ("mean", mean), ("bwd", bwd)):
                t[f"{k}_us{again}"] = _graph_us(fn, args.iters, args.warmup)
        t["fwd_kernel_us"] = _kernel_us(["history_attn_fwd"], fwd, args.iters)["history_attn_fwd"]
        t["bwd_kernel_us"] = _kernel_us(["history_attn_bwd"], bwd, args.iters)["history_attn_bwd"]
        t["mean_kernel_us"] = _kernel_us(["bag_fwd"], mean, args.iters)["bag_fwd"]
        eager_iters = max(args.iters // 5, 5)
        t["torch_fwd_us"] = _eager_us(torch_fwd, eager_iters, 3)
        t["torch_bwd_us"] = _eager_us(torch_bwd, eager_iters, 3)
        fb, bb, mb = 4 * dim * (cnt + 3 * n_bags), 4 * dim * (2 * cnt + 2 * n_bags), 4 * dim * (cnt + 2 * n_bags)
        emit({"what": "history_attention", "tokens": "Z", "n_bags": n_bags, "L": L, "dim": dim, "table_rows": args.items,
              "base_rows": args.users, "pooled_slots": cnt, "n_slabs": slabs.shape[0], "torch_timing": "eager",
              **{k: round(v, 3) for k, v in t.items()}, "fwd_bytes": fb, "bwd_bytes": bb, "mean_bytes": mb,
              "fwd_frac_hbm": round(fb / (t["fwd_us"] * 1e-6) / PEAK_HBM, 4), "bwd_frac_hbm": round(bb / (t["bwd_us"] * 1e-6) / PEAK_HBM, 4),
              "mean_frac_hbm": round(mb / (t["mean_us"] * 1e-6) / PEAK_HBM, 4),
              "fwd_kernel_frac_hbm": round(fb / (t["fwd_kernel_us"] * 1e-6) / PEAK_HBM, 4),
              "bwd_kernel_frac_hbm": round(bb / (t["bwd_kernel_us"] * 1e-6) / PEAK_HBM, 4),
              "fwd_to_mean": round(t["fwd_us"] / t["mean_us"], 3), "torch_fwd_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3),
              "torch_bwd_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3)})
        state.clear()
        del hist, per, idx, items, own, valid, rank, slot_grads
    del table, base_table, out, out_mean
    torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    L = args.history_len
    trainers = {}
    for name in ("mean", "attention"):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], user_history_len=L, history_pooling=name)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
        trainers[name].set_user_histories(synthetic_histories(args.users, args.items, L, dev))
    trainers["attention"].history_attn.copy_(_attn(CFG3["dim"], L, dev))
    for variant in ("U", "Z"):
        batches = [trainers["mean"].synthetic_batch(1001, s, variant) for s in range(16)]
        # half of the pairs' positives stand in their user's history, as after training on those pairs
        hist = trainers["mean"].user_history
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
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "L": L,
              "steps": args.steps, "rounds": args.rounds, "step_ms_mean": round(med["mean"], 4),
              "step_ms_attention": round(med["attention"], 4), "attention_to_mean": round(med["attention"] / med["mean"], 4),
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_attention.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_history_attention.py needs a GPU: nothing here is measured on the CPU")
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

"""The multi-head self-attention encoder of the user history: the forward family (resolve, T GEMM, pool forward, O GEMM, combine)
and the backward family ((dP, dWvo) GEMM, pool backward, (dxn, dWqk) GEMM, query gradient) launch by launch, beside a torch eager
equivalent, the attention pool and the GRU on the same problem, and the cfg3 train step with mean pooling, the attention pool, the
GRU and self-attention.  JSON lines, printed and appended to --out:

    python bench_history_self_attention.py [--iters 10] [--warmup 2] [--steps 100] [--rounds 3] [--out profiles/history_self_attention.jsonl]

Kernel lines ("what": "history_self_attention"): 8192 bags x dim 128 x L in {8, 20, 64} x heads in {1, 4, 8} over a --items-row
history table and a --users-row base table - bench_history.py's problem: power-law ("Z") users and items, every user's history
holds 1..L items, half of the pairs' positives stand in their user's history (and are left out).  Wqk, Wvo Glorot-uniform, p = 0.
  fwd_us / bwd_us               per call of ops.history_self_attention(keep=buffers) / ops.history_self_attention_bwd, from replays
                                of a HIP graph of `iters` back-to-back calls (the best of five replays), measured alternating, twice
  *_kernel_us                   every launch's own begin-to-end time (the library's built-in timing, eager launches): resolve, gemm_t,
                                pool_fwd, gemm_o, combine; gemm_dp (a list: the dx and dW launches), pool_bwd, gemm_dxn, query_grad
  torch_fwd_us / torch_bwd_us   the eager equivalent on the pre-masked per-bag token matrix - a gather, two matmuls, a masked
                                softmax over einsum logits - and autograd's backward w.r.t. the gathered rows, Wqk, Wvo and p:
                                device events around eager calls, host time included
  attn_fwd_us / attn_bwd_us     ops.history_attention / history_attention_bwd on the same bags (graph replays), once per L
  gru_fwd_us / gru_bwd_us       ops.history_gru / history_gru_bwd on the same bags (graph replays), once per L
  gather_bytes, pool_fwd_gbps   4 D sum(cnt) bytes of rows the pool forward gathers (+ T and P), over its own time
  owner                         which of launch floor (launches * ~2.5 us inside a graph), gather (the two pool launches and the
                                resolve) or GEMM (the four GEMM launches) holds most of fwd + bwd, from the per-launch times
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192, L 20, 4 heads) with mean, attention, gru and
self_attention, in the same process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a
synchronise), on uniform and on power-law ids; the median round of each and every round's time.  Nothing here is a target.
"""
import argparse
import json
import math
import pathlib
import statistics
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from bench_adam import CFG3, _graph_us  # noqa: E402
from bench_history import synthetic_histories  # noqa: E402
from bench_rating import _eager_us  # noqa: E402

TAGS = ["history_selfattn_resolve", "dense_fwd", "history_selfattn_pool_fwd", "history_selfattn_combine", "dense_bwd", "dense_bwd_dx",
        "dense_bwd_dw", "history_selfattn_pool_bwd", "history_selfattn_query_grad"]


def _params(dim: int, L: int, heads: int, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    u = lambda shape, fan: (torch.rand(*shape, device=dev, generator=g) * 2 - 1) * math.sqrt(6.0 / fan)
    return u((dim, heads * dim), 2 * dim), u((heads * dim, dim), heads * dim + dim), torch.zeros(heads, L, device=dev)


def _launch_us(fn, iters: int) -> dict:
    """Median begin-to-end time of every tagged launch ``fn`` makes, in launch order per tag: {tag: [us of its 1st, 2nd .. launch]}."""
    from two_tower_amazon_recommender_amd import _lib
    _lib.profile_enable(",".join(TAGS), 4 * iters)
    for _ in range(iters):
        fn()
    out = {}
    for t in TAGS:
        ms, n = _lib.profile_read(t, 4 * iters)
        per = n // iters if iters else 0
        if per:
            out[t] = [statistics.median(ms[k::per]) * 1e3 for k in range(per)]
    _lib.profile_enable("")
    return out


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, n_bags = CFG3["dim"], CFG3["batch"]
    table = torch.empty(args.items, dim, device=dev).uniform_(-0.05, 0.05)
    base_table = torch.empty(args.users, dim, device=dev).uniform_(-0.05, 0.05)
    users = torch.empty(n_bags, dtype=torch.int64, device=dev)
    ops.fill_ids_(users, 1001, 3, args.users, "Z")
    out = torch.zeros(n_bags, dim, device=dev)
    dy = torch.randn(n_bags, dim, device=dev) * 0.01
    for L in (8, 20, 64):
        hist = synthetic_histories(args.users, args.items, L, dev)
        items = torch.empty(n_bags, dtype=torch.int64, device=dev)
        ops.fill_ids_(items, 1001, 4, args.items, "Z")
        own = hist[users, 0].to(torch.int64)                          # (slot 0 is always valid)
        items = torch.where(torch.arange(n_bags, device=dev) % 2 == 0, own, items)
        per = hist[users]
        per = torch.where(per.to(torch.int64) == items[:, None], -1, per).contiguous()       # the pre-masked per-bag matrix
        valid = per >= 0
        cnt = int(valid.sum().item())
        idx = per.clamp(min=0).to(torch.int64).reshape(-1)
        slot_grads = torch.zeros(n_bags * L, dim, device=dev)
        base = (base_table, users)
        # the neighbours on the same bags: the attention pool and the GRU
        attn = torch.zeros(dim + L, device=dev)
        ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
        wts, pooled = torch.empty(n_bags, L, device=dev), torch.empty(n_bags, dim, device=dev)
        ha_slabs = torch.empty(ops.history_attention_num_slabs(n_bags), dim + L, device=dev)
        near = {}
        a_fwd = lambda: ops.history_attention(table, hist, attn, bag_rows=users, exclude=items, base=base, out=out, batch_ids=ids,
                                              weights=wts, pooled=pooled)
        a_bwd = lambda: ops.history_attention_bwd(table, ids, wts, pooled, dy, attn, L, slot_grads=slot_grads, dattn_slabs=ha_slabs)
        near["attn_fwd_us"], near["attn_bwd_us"] = _graph_us(a_fwd, args.iters, args.warmup), _graph_us(a_bwd, args.iters, args.warmup)
        lim = math.sqrt(6.0 / (4 * dim))
        gW, gU = ((torch.rand(dim, 3 * dim, device=dev) * 2 - 1) * lim for _ in range(2))
        gb = torch.zeros(2, 3 * dim, device=dev)
        gbufs = ops.GruBuffers(n_bags, L, dim, dev)
        g_fwd = lambda: ops.history_gru(table, hist, gW, gU, gb, bag_rows=users, exclude=items, base=base, out=out, keep=gbufs)
        g_bwd = lambda: ops.history_gru_bwd(gbufs, dy, gW, gU, slot_grads=slot_grads)
        near["gru_fwd_us"], near["gru_bwd_us"] = _graph_us(g_fwd, args.iters, args.warmup), _graph_us(g_bwd, args.iters, args.warmup)
        del gbufs, gW, gU, gb
        torch.cuda.empty_cache()
        for heads in (1, 4, 8):
            Wqk, Wvo, p = _params(dim, L, heads, dev)
            bufs = ops.SelfAttnBuffers(n_bags, L, dim, heads, dev)
            ns, nsp = ops.dense_bwd_num_slabs(n_bags), ops.history_self_attention_num_slabs(n_bags)
            dwqk, dwvo = torch.empty(ns, dim, heads * dim, device=dev), torch.empty(ns, heads * dim, dim, device=dev)
            dp = torch.empty(nsp, heads * L, device=dev)

            def fwd():
                ops.history_self_attention(table, hist, Wqk, Wvo, p, bag_rows=users, exclude=items, base=base, out=out, keep=bufs)

            def bwd():
                ops.history_self_attention_bwd(bufs, dy, Wqk, Wvo, slot_grads=slot_grads, dwqk_slabs=dwqk, dwvo_slabs=dwvo, dp_slabs=dp)

            # the torch eager equivalent, on the gathered rows of the table (the table's gradient is left sparse: the rows' gradient)
            Wq, Wv, pt = (t.clone().requires_grad_(True) for t in (Wqk, Wvo, p))
            v64 = valid.to(torch.int64)
            rank = (v64.flip(1).cumsum(1).flip(1) - v64).clamp(0, L - 1)
            some = valid.any(1)
            newest = (L - 1 - torch.argmax(v64.flip(1), dim=1)).clamp(0, L - 1)
            state = {}

            def torch_fwd():
                rows = (table.index_select(0, idx) * valid.reshape(-1, 1)).requires_grad_(True)
                x = rows.view(n_bags, L, dim)
                xn = x[torch.arange(n_bags, device=dev), newest] * some[:, None]
                Tq = (xn @ Wq).view(n_bags, heads, dim)
                e = torch.einsum("bld,bhd->bhl", x, Tq) / math.sqrt(dim) + pt[:, rank].permute(1, 0, 2)
                w = torch.softmax(e.masked_fill(~valid[:, None, :], -1e30), dim=2) * valid[:, None, :]
                P = torch.einsum("bhl,bld->bhd", w, x).reshape(n_bags, heads * dim)
                state["rows"], state["out"] = rows, base_table.index_select(0, users) + P @ Wv

            def torch_bwd():
                torch.autograd.grad(state["out"], (state["rows"], Wq, Wv, pt), dy, retain_graph=True)

            fwd(); torch_fwd()
            err = (out - state["out"]).abs().max().item() / state["out"].abs().max().item()
            if not err <= 1e-4:
                raise SystemExit(f"bench_history_self_attention.py: the launches and the torch equivalent disagree ({err:.2e})")
            slot_grads.zero_()
            bwd()
            ref = torch.autograd.grad(state["out"], (state["rows"], Wq, Wv), dy, retain_graph=True)
            for name, got, want in (("slot_grads", slot_grads * valid.reshape(-1, 1), ref[0]), ("dWqk", dwqk.sum(0), ref[1]),
                                    ("dWvo", dwvo.sum(0), ref[2])):
                e = (got - want).abs().max().item() / want.abs().max().item()
                if not e <= 1e-3:
                    raise SystemExit(f"bench_history_self_attention.py: {name} and torch autograd disagree ({e:.2e})")
            t = {}
            for again in ("", "_again"):
                for k, fn in (("fwd", fwd), ("bwd", bwd)):
                    t[f"{k}_us{again}"] = _graph_us(fn, args.iters, args.warmup)
            kf, kb = _launch_us(fwd, args.iters), _launch_us(bwd, args.iters)
            gemm_b = [v for tag in ("dense_bwd", "dense_bwd_dx", "dense_bwd_dw") for v in kb.get(tag, [])]
            kern = {"resolve_kernel_us": kf["history_selfattn_resolve"][0], "gemm_t_kernel_us": kf["dense_fwd"][0],
                    "pool_fwd_kernel_us": kf["history_selfattn_pool_fwd"][0], "gemm_o_kernel_us": kf["dense_fwd"][1],
                    "combine_kernel_us": kf["history_selfattn_combine"][0], "pool_bwd_kernel_us": kb["history_selfattn_pool_bwd"][0],
                    "query_grad_kernel_us": kb["history_selfattn_query_grad"][0], "gemm_bwd_kernel_us": [round(v, 3) for v in gemm_b]}
            eager_iters = max(args.iters // 3, 2)
            t["torch_fwd_us"] = _eager_us(torch_fwd, eager_iters, 1)
            t["torch_bwd_us"] = _eager_us(torch_bwd, eager_iters, 1)
            gather = kern["resolve_kernel_us"] + kern["pool_fwd_kernel_us"] + kern["pool_bwd_kernel_us"]
            gemm = kern["gemm_t_kernel_us"] + kern["gemm_o_kernel_us"] + sum(gemm_b)
            n_launch = 5 + 2 + len(gemm_b)
            floor = 2.5 * n_launch
            small = kern["combine_kernel_us"] + kern["query_grad_kernel_us"]
            owner = max((("gather", gather), ("gemm", gemm), ("launch_floor", floor + small)), key=lambda kv: kv[1])[0]
            gather_bytes = 4 * dim * cnt
            fwd_bytes = gather_bytes + 2 * 4 * n_bags * heads * dim
            emit({"what": "history_self_attention", "tokens": "Z", "n_bags": n_bags, "L": L, "dim": dim, "heads": heads,
                  "table_rows": args.items, "base_rows": args.users, "kept_slots": cnt, "n_slabs": [ns, nsp], "torch_timing": "eager",
                  **{k: round(v, 3) for k, v in t.items()}, **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in kern.items()},
                  **{k: round(v, 3) for k, v in near.items()},
                  "gather_bytes": gather_bytes, "pool_fwd_gbps": round(fwd_bytes / (kern["pool_fwd_kernel_us"] * 1e-6) / 1e9, 1),
                  "pool_fwd_valu_gflops": round(4.0 * cnt * heads * dim / (kern["pool_fwd_kernel_us"] * 1e-6) / 1e9, 1),
                  "gemm_flops": 2 * 2 * n_bags * dim * heads * dim,
                  "gather_us": round(gather, 3), "gemm_us": round(gemm, 3), "launches": n_launch, "owner": owner,
                  "torch_fwd_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_bwd_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3),
                  "fwd_to_attn": round(t["fwd_us"] / near["attn_fwd_us"], 3), "bwd_to_attn": round(t["bwd_us"] / near["attn_bwd_us"], 3),
                  "fwd_to_gru": round(t["fwd_us"] / near["gru_fwd_us"], 3), "bwd_to_gru": round(t["bwd_us"] / near["gru_bwd_us"], 3)})
            state.clear()
            del bufs, dwqk, dwvo, dp, ref, Wq, Wv, pt
            torch.cuda.empty_cache()
        del hist, per, idx, items, own, valid, slot_grads
        torch.cuda.empty_cache()
    del table, base_table, out
    torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    L = args.history_len
    trainers = {}
    for name in ("mean", "attention", "gru", "self_attention"):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], user_history_len=L, history_pooling=name, history_heads=args.heads)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
        trainers[name].set_user_histories(synthetic_histories(args.users, args.items, L, dev))
    for variant in ("U", "Z"):
        batches = [trainers["mean"].synthetic_batch(1001, s, variant) for s in range(16)]
        # half of the pairs' positives stand in their user's history, as after training on those pairs
        hist = trainers["mean"].user_history
        batches = [(u, torch.where(torch.arange(u.numel(), device=dev) % 2 == 0, hist[u, 0].to(torch.int64), i)) for u, i in batches]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms all up
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
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "L": L, "heads": args.heads,
              "steps": args.steps, "rounds": args.rounds, **{f"step_ms_{k}": round(v, 4) for k, v in med.items()},
              **{f"{k}_to_mean": round(med[k] / med["mean"], 4) for k in med if k != "mean"},
              "self_attention_to_attention": round(med["self_attention"] / med["attention"], 4),
              "self_attention_to_gru": round(med["self_attention"] / med["gru"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--history-len", type=int, default=20, help="L of the step lines")
    ap.add_argument("--heads", type=int, default=4, help="heads of the step lines")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--skip-kernels", action="store_true", help="the step lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_self_attention.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_history_self_attention.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    if not args.skip_kernels:
        kernel_phase(args, emit)
        torch.cuda.empty_cache()
    if not args.skip_steps:
        steps(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

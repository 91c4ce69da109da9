"""The GRU encoder of the user history: the forward family (slot resolve, input projection, recurrent forward) and the backward
family (recurrent backward, the two gradient GEMM launches) launch by launch, beside a torch eager equivalent on the same device,
and the cfg3 train step with mean pooling and with the GRU.  JSON lines, printed and appended to --out:

    python bench_history_gru.py [--iters 10] [--warmup 2] [--steps 100] [--rounds 3] [--out profiles/history_gru.jsonl]

Kernel lines ("what": "history_gru"): 8192 bags x dim 128 x L in {8, 20, 64} over a --items-row history table and a --users-row
base table - bench_history.py's problem: power-law ("Z") users and items, every user's history holds 1..L items, half of the pairs'
positives stand in their user's history (and are left out).  W, U Glorot-uniform (fan D + 3D), b = 0: a fresh model.
  fwd_us / bwd_us               per call of ops.history_gru(keep=buffers) / ops.history_gru_bwd, from replays of a HIP graph of
                                `iters` back-to-back calls (the best of five replays), measured alternating, twice (*_again)
  *_kernel_us                   every launch's own begin-to-end time (the library's built-in timing, eager launches): resolve,
                                proj (the input projection GEMM), rec_fwd, rec_bwd, grad_w (dx + dW + db_i), grad_u (dU + db_r)
  torch_fwd_us / torch_bwd_us   the eager equivalent on the pre-masked per-bag token matrix - a gather, addmm and a Python loop of
                                the GRU-cell math with torch.where for the mask - and autograd's backward of that loop w.r.t. the
                                gathered rows, W, U and b: device events around eager calls, host time included
  rec_fwd_frac_mfma / rec_bwd_frac_mfma   2 B L D 3D (forward) and 4 B L D 3D (backward) FLOPs over the recurrent launch's own
                                time, as a fraction of the 157.3 TF f32 MFMA peak - every slot counted, kept or not
  kept_bytes                    what the step keeps for the backward (x, gates, gn, hprev, da, dg: 48 B L D bytes)
  fwd_tile_rows                 32: the product's recurrent forward (32-row tiles, v_mfma_f32_32x32x2_f32); 16: the A/B build
                                (`make BUILD=build_t16 LIB=../../scratch/variants/gru_tile16.so EXTRA=-DTT_GRU_TILE16` in csrc,
                                run with TT_LIB_PATH=scratch/variants/gru_tile16.so --fwd-tile-rows 16 --skip-steps): 16-row
                                tiles on v_mfma_f32_16x16x4_f32, twice the workgroups; the backward is the same in both
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192, L 20) with mean pooling and with the GRU, in the same
process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise), on uniform and on
power-law ids; the median round of each and every round's time.  Nothing here is a target.
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

PEAK_F32_MFMA = 157.3e12


def _params(dim: int, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    lim = math.sqrt(6.0 / (4 * dim))
    W = (torch.rand(dim, 3 * dim, device=dev, generator=g) * 2 - 1) * lim
    U = (torch.rand(dim, 3 * dim, device=dev, generator=g) * 2 - 1) * lim
    return W, U, torch.zeros(2, 3 * dim, device=dev)


def _launch_us(fn, iters: int) -> dict:
    """Median begin-to-end time of every tagged launch ``fn`` makes, in launch order per tag: {tag: [us of its 1st, 2nd .. launch]}."""
    from two_tower_amazon_recommender_amd import _lib
    tags = ["history_gru_resolve", "dense_fwd", "history_gru_fwd", "history_gru_bwd", "dense_bwd", "dense_bwd_dx", "dense_bwd_dw"]
    _lib.profile_enable(",".join(tags), 4 * iters)
    for _ in range(iters):
        fn()
    out = {}
    for t in tags:
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
    W, U, b = _params(dim, dev)
    for L in (8, 20, 64):
        hist = synthetic_histories(args.users, args.items, L, dev)
        items = torch.empty(n_bags, dtype=torch.int64, device=dev)
        ops.fill_ids_(items, 1001, 4, args.items, "Z")
        own = hist[users, 0].to(torch.int64)                          # (slot 0 is always valid)
        items = torch.where(torch.arange(n_bags, device=dev) % 2 == 0, own, items)
        per = hist[users]
        per = torch.where(per.to(torch.int64) == items[:, None], -1, per).contiguous()       # the pre-masked per-bag matrix
        cnt = int((per >= 0).sum().item())
        bufs = ops.GruBuffers(n_bags, L, dim, dev)
        ns = ops.dense_bwd_num_slabs(n_bags * L)
        slot_grads = torch.zeros(n_bags * L, dim, device=dev)
        dw, du, db = (torch.empty(ns, dim, 3 * dim, device=dev), torch.empty(ns, dim, 3 * dim, device=dev),
                      torch.empty(2, ns, 3 * dim, device=dev))

        def fwd():
            ops.history_gru(table, hist, W, U, b, bag_rows=users, exclude=items, base=(base_table, users), out=out, keep=bufs)

        def bwd():
            ops.history_gru_bwd(bufs, dy, W, U, slot_grads=slot_grads, dw_slabs=dw, du_slabs=du, db_slabs=db)

        # the torch eager equivalent, on the gathered rows of the table (the table's gradient is left sparse: the rows' gradient)
        valid = per >= 0
        idx = per.clamp(min=0).to(torch.int64).reshape(-1)
        Wt, Ut, bt = (t.clone().requires_grad_(True) for t in (W, U, b))
        state = {}

        def torch_fwd():
            rows = (table.index_select(0, idx) * valid.reshape(-1, 1)).requires_grad_(True)
            a = torch.addmm(bt[0], rows, Wt).view(n_bags, L, 3 * dim)
            h = torch.zeros(n_bags, dim, device=dev)
            for t in range(L):
                g = torch.addmm(bt[1], h, Ut)
                z = torch.sigmoid(a[:, t, :dim] + g[:, :dim])
                r = torch.sigmoid(a[:, t, dim:2 * dim] + g[:, dim:2 * dim])
                n = torch.tanh(a[:, t, 2 * dim:] + r * g[:, 2 * dim:])
                h = torch.where(valid[:, t, None], z * h + (1 - z) * n, h)
            state["rows"], state["out"] = rows, base_table.index_select(0, users) + h

        def torch_bwd():
            torch.autograd.grad(state["out"], (state["rows"], Wt, Ut, bt), dy, retain_graph=True)

        fwd(); torch_fwd()
        err = (out - state["out"]).abs().max().item() / state["out"].abs().max().item()
        if not err <= 1e-4:
            raise SystemExit(f"bench_history_gru.py: the launches and the torch equivalent disagree ({err:.2e})")
        bwd()
        ref = torch.autograd.grad(state["out"], (state["rows"], Wt, Ut), dy, retain_graph=True)
        for name, got, want in (("slot_grads", slot_grads, ref[0]), ("dW", dw.sum(0), ref[1]), ("dU", du.sum(0), ref[2])):
            e = (got - want).abs().max().item() / want.abs().max().item()
            if not e <= 1e-3:
                raise SystemExit(f"bench_history_gru.py: {name} and torch autograd disagree ({e:.2e})")
        t = {}
        for again in ("", "_again"):
            for k, fn in (("fwd", fwd), ("bwd", bwd)):
                t[f"{k}_us{again}"] = _graph_us(fn, args.iters, args.warmup)
        kf, kb = _launch_us(fwd, args.iters), _launch_us(bwd, args.iters)
        kern = {"resolve_kernel_us": kf["history_gru_resolve"][0], "proj_kernel_us": kf["dense_fwd"][0],
                "rec_fwd_kernel_us": kf["history_gru_fwd"][0], "rec_bwd_kernel_us": kb["history_gru_bwd"][0]}
        grads = [v for tag in ("dense_bwd", "dense_bwd_dx", "dense_bwd_dw") for v in kb.get(tag, [])]
        kern["grad_gemm_kernel_us"] = [round(v, 3) for v in grads]
        eager_iters = max(args.iters // 3, 2)
        t["torch_fwd_us"] = _eager_us(torch_fwd, eager_iters, 1)
        t["torch_bwd_us"] = _eager_us(torch_bwd, eager_iters, 1)
        flops = 2.0 * n_bags * L * dim * 3 * dim
        emit({"what": "history_gru", "tokens": "Z", "n_bags": n_bags, "L": L, "dim": dim, "table_rows": args.items,
              "base_rows": args.users, "kept_slots": cnt, "n_slabs": ns, "torch_timing": "eager", "fwd_tile_rows": args.fwd_tile_rows,
              **{k: round(v, 3) for k, v in t.items()}, **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in kern.items()},
              "rec_fwd_frac_mfma": round(flops / (kern["rec_fwd_kernel_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "rec_bwd_frac_mfma": round(2 * flops / (kern["rec_bwd_kernel_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "kept_bytes": 48 * n_bags * L * dim,
              "torch_fwd_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_bwd_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3)})
        state.clear()
        del hist, per, idx, items, own, valid, slot_grads, bufs, dw, du, db, ref
        torch.cuda.empty_cache()
    del table, base_table, out
    torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    L = args.history_len
    trainers = {}
    for name in ("mean", "gru"):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], user_history_len=L, history_pooling=name)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
        trainers[name].set_user_histories(synthetic_histories(args.users, args.items, L, dev))
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
              "step_ms_gru": round(med["gru"], 4), "gru_to_mean": round(med["gru"] / med["mean"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--history-len", type=int, default=20, help="L of the step lines")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--fwd-tile-rows", type=int, default=32, choices=(32, 16),
                    help="label of the records: the recurrent forward's tile height of the library in use - 32 (the product) or 16 "
                         "(a build with -DTT_GRU_TILE16, loaded through TT_LIB_PATH: the tile A/B)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_gru.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_history_gru.py needs a GPU: nothing here is measured on the CPU")
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

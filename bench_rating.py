"""The rating-prediction head: the forward launch (tt_rating_head_fwd_f32) and the backward launch (tt_rating_head_bwd_f32) beside
the same math as a torch sequence on the same device (cat -> addmm -> relu -> mv, autograd for the backward), and the cfg3 train
step with the head on and off.  JSON lines, printed and appended to --out:

    python bench_rating.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/rating.jsonl]

Kernel lines ("what": "rating_kernels"): n = 8192 pairs, D = 128, H in {64, 128, 256}; a tenth of the ratings missing, sample
weights given; the backward launch accumulates into dq / dc and writes tt_rating_head_num_slabs(8192) = 64 slabs, as the
train step does.
  fwd_us / bwd_us            per call, from replays of a HIP graph of `iters` back-to-back calls (the best of five replays);
                             *_again: the same measurement repeated - the spread of the method
  fwd_kernel_us / bwd_kernel_us   the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_fwd_us               cat + addmm + relu + mv + add, the same way
  torch_fwd_bwd_us           that forward, the masked MSE on its predictions and autograd's backward for all six inputs;
                             torch_bwd_us = the difference ("torch_timing": "graph", or "eager" - events around back-to-back
                             eager calls - where the backward could not be captured)
  fwd_frac_mfma / bwd_frac_mfma   2 n 2D H / fwd time and 4 n 2D H / bwd time as fractions of the f32 MFMA peak (157.3e12)
Nothing here is a target: nobody had measured any of it before this file.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) with the head off and on (H = 128, rating_weight 0.5),
in the same process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the
median round of each and every round's time, on uniform ("U") and power-law ("Z") ids.  The base of the ratio is the step
WITHOUT the head.
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

from bench_adam import CFG3, _graph_us, _kernel_us  # noqa: E402

PEAK_F32_MFMA = 157.3e12
WEIGHT = 0.5


def _eager_us(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    n, d = CFG3["batch"], 128
    g = torch.Generator(device=dev).manual_seed(7)
    q = torch.randn(n, d, device=dev, generator=g) * 0.3
    c = torch.randn(n, d, device=dev, generator=g) * 0.3
    rating = torch.randint(1, 6, (n,), device=dev, generator=g).to(torch.float32)
    rating[torch.rand(n, device=dev, generator=g) < 0.1] = float("nan")
    sw = torch.rand(n, device=dev, generator=g) * 2.0
    valid, rating0 = torch.isfinite(rating), torch.nan_to_num(rating)
    ns = ops.rating_head_num_slabs(n)
    scale = 2.0 * WEIGHT / n
    for h in (64, 128, 256):
        lim = (6.0 / (2 * d + h)) ** 0.5
        w1 = (torch.rand(2 * d, h, device=dev, generator=g) * 2 - 1) * lim
        b1 = torch.randn(h, device=dev, generator=g) * 0.1
        w2 = torch.randn(h, device=dev, generator=g) * 0.2
        b2 = torch.full((1,), 3.0, device=dev)
        pred, hid = torch.empty(n, device=dev), torch.empty(n, h, device=dev)
        dq, dc = torch.zeros(n, d, device=dev), torch.zeros(n, d, device=dev)
        ks, bs, se = torch.empty(ns, 2 * d * h + h, device=dev), torch.empty(ns, h + 1, device=dev), torch.empty(ns, device=dev)
        leaves = [t.clone().requires_grad_(True) for t in (q, c, w1, b1, w2, b2)]

        def fwd():
            ops.rating_head(q, c, w1, b1, w2, b2, pred=pred, h=hid)

        def bwd():
            ops.rating_head_bwd(q, c, hid, pred, rating, w1, w2, scale, dq, dc, ks, bs, se, sample_weight=sw, accumulate=True)

        def ref_fwd(t=(q, c, w1, b1, w2, b2)):
            return torch.mv(torch.relu(torch.addmm(t[3], torch.cat([t[0], t[1]], dim=1), t[2])), t[4]) + t[5]

        def ref_fwd_bwd():
            p = ref_fwd(leaves)
            e = torch.where(valid, p - rating0, torch.zeros_like(p))
            return torch.autograd.grad(WEIGHT * (sw * e * e).sum() / n, leaves)

        fwd()
        err = ((pred - ref_fwd()).abs().max() / ref_fwd().abs().max()).item()
        if not err <= 1e-5:
            raise SystemExit(f"bench_rating.py: the forward launch and the torch form disagree (relative error {err:.2e})")
        dq.zero_(); dc.zero_()
        bwd()
        grads = ref_fwd_bwd()
        werr = max(((dq - grads[0]).abs().max() / grads[0].abs().max()).item(),
                   ((ks.sum(0)[:2 * d * h].view(2 * d, h) - grads[2]).abs().max() / grads[2].abs().max()).item())
        if not werr <= 1e-4:
            raise SystemExit(f"bench_rating.py: the backward launch and autograd disagree (relative error {werr:.2e})")
        t = {"fwd_us": _graph_us(fwd, args.iters, args.warmup), "bwd_us": _graph_us(bwd, args.iters, args.warmup),
             "torch_fwd_us": _graph_us(ref_fwd, args.iters, args.warmup)}
        how = "graph"
        try:
            t["torch_fwd_bwd_us"] = _graph_us(ref_fwd_bwd, args.iters, args.warmup)
        except Exception as exc:                             # autograd's backward refused the capture: time it eagerly
            print(f"bench_rating.py: torch fwd+bwd not captured ({type(exc).__name__}); timing it eagerly", file=sys.stderr)
            torch.cuda.synchronize()
            how = "eager"
            t["torch_fwd_us"] = _eager_us(ref_fwd, args.iters, args.warmup)
            t["torch_fwd_bwd_us"] = _eager_us(ref_fwd_bwd, args.iters, args.warmup)
        t["torch_bwd_us"] = t["torch_fwd_bwd_us"] - t["torch_fwd_us"]
        t["fwd_us_again"], t["bwd_us_again"] = _graph_us(fwd, args.iters, args.warmup), _graph_us(bwd, args.iters, args.warmup)
        t["fwd_kernel_us"] = _kernel_us(["rating_fwd"], fwd, args.iters)["rating_fwd"]
        t["bwd_kernel_us"] = _kernel_us(["rating_bwd"], bwd, args.iters)["rating_bwd"]
        flops = 2.0 * n * 2 * d * h
        emit({"what": "rating_kernels", "rows": n, "D": d, "H": h, "n_slabs": ns, "torch_timing": how,
              **{k: round(v, 3) for k, v in t.items()},
              "fwd_frac_mfma": round(flops / (t["fwd_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "bwd_frac_mfma": round(2 * flops / (t["bwd_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "torch_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3),
              "fwd_vs_torch_rel_err": float(f"{err:.3e}")})
        del leaves, grads, ks
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name, w in (("plain", 0.0), ("head", WEIGHT)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], rating_weight=w, rating_hidden=args.hidden)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    trainers["head"].init_rating_bias(3.0)
    g = torch.Generator(device=dev).manual_seed(7)
    ratings = [torch.randint(1, 6, (CFG3["batch"],), device=dev, generator=g).to(torch.float32) for _ in range(16)]
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms both up
            for name, t in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    kw = {"ratings": ratings[s % 16]} if name == "head" else {}
                    t.step(*batches[s % len(batches)], **kw)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for t in trainers.values():
            t.check_ids()
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"what": "step", "ids": variant, "optimizer": "adagrad", "batch": CFG3["batch"], "dim": CFG3["dim"],
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "H": args.hidden, "rating_weight": WEIGHT,
              "steps": args.steps, "rounds": args.rounds, "step_ms_plain": round(med["plain"], 4),
              "step_ms_head": round(med["head"], 4), "head_to_plain": round(med["head"] / med["plain"], 4),
              "rating_loss": round(trainers["head"].rating_loss.item(), 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=128, help="H of the step lines")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rating.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rating.py needs a GPU: nothing here is measured on the CPU")
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

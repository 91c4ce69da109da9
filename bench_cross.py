"""The DCN-v2 cross layer: the forward launch (tt_cross_fwd_f32) and the backward launch (tt_cross_bwd_f32), both towers per
launch, beside the same math as a torch sequence on the same device (x0 * addmm(b, x, w) + x, autograd for the backward), and
the cfg3 train step with 0 / 1 / 2 cross layers.  JSON lines, printed and appended to --out:

    python bench_cross.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/cross.jsonl]

Kernel lines ("what": "cross_kernels"): two problems (both towers) of n = 8192 rows each, D in {64, 128, 256}; the forward launch
keeps u, the backward launch runs in its upper-layer form (dx, dx0 written) with tt_cross_num_slabs(8192) = 64 slabs, as the
train step's does.
  fwd_us / bwd_us            per launch (BOTH towers), from replays of a HIP graph of `iters` back-to-back calls (the best of five
                             replays); *_again: the same measurement repeated - the spread of the method
  fwd_kernel_us / bwd_kernel_us   the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_fwd_us               x0 * addmm(b, x, w) + x for both towers, the same way
  torch_fwd_bwd_us           that forward and autograd's backward for all four inputs of both towers; torch_bwd_us = the
                             difference ("torch_timing": "graph", or "eager" where the backward could not be captured)
  fwd_frac_mfma / bwd_frac_mfma   2 * 2 n D D / fwd time and 2 * 4 n D D / bwd time as fractions of the f32 MFMA peak (157.3e12)
  fwd_gbs / bwd_gbs          the bytes the launch must move (fwd: x0, x in, u, y out; bwd: x0, x, u, g in, dx, dx0 out) per second
Nothing here is a target: nobody had measured any of it before this file.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) with cross_layers 0, 1 and 2 in the same process,
alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median round of each
and every round's time, on uniform ("U") and power-law ("Z") ids.  Two bases: the step without the layers as bench.py runs it
(fused lookup, one C call), and the same step on materialised tower inputs through the Python sequence of launches
("plain_materialised") - the path every feature takes, and the one the layers are added to.
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
from bench_rating import _eager_us  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    n = CFG3["batch"]
    g = torch.Generator(device=dev).manual_seed(7)
    ns = ops.cross_num_slabs(n)
    for d in (64, 128, 256):
        lim = (6.0 / (2 * d)) ** 0.5
        sides = []
        for _ in range(2):
            x0 = torch.rand(n, d, device=dev, generator=g) * 2 - 1
            x = torch.rand(n, d, device=dev, generator=g) * 2 - 1
            w = (torch.rand(d, d, device=dev, generator=g) * 2 - 1) * lim
            b = torch.rand(d, device=dev, generator=g) * 0.4 - 0.2
            go = torch.randn(n, d, device=dev, generator=g)
            sides.append(dict(x0=x0, x=x, w=w, b=b, g=go, u=torch.empty(n, d, device=dev), y=torch.empty(n, d, device=dev),
                              dx=torch.empty(n, d, device=dev), dx0=torch.empty(n, d, device=dev)))
        stride = 2 * (d * d + d)
        slabs = torch.empty(ns * stride, device=dev)
        leaves = [[s[k].clone().requires_grad_(True) for k in ("x0", "x", "w", "b")] for s in sides]

        def fwd():
            ops.cross_layer(*[(s["x0"], s["x"], s["w"], s["b"], s["y"]) for s in sides], u=tuple(s["u"] for s in sides))

        def bwd():
            ops.cross_layer_bwd(*[(s["x0"], s["x"], s["u"], s["w"], s["g"], s["dx"], s["dx0"], slabs[k * d * d:],
                                   slabs[2 * d * d + k * d:]) for k, s in enumerate(sides)], n_slabs=ns, slab_stride=stride)

        def ref_fwd(ts=None):
            ts = [(s["x0"], s["x"], s["w"], s["b"]) for s in sides] if ts is None else ts
            return [t[0] * torch.addmm(t[3], t[1], t[2]) + t[1] for t in ts]

        def ref_fwd_bwd():
            ys = ref_fwd(leaves)
            return torch.autograd.grad(ys, [t for l in leaves for t in l], [s["g"] for s in sides])

        fwd()
        want = ref_fwd()
        err = max(((s["y"] - y).abs().max() / y.abs().max()).item() for s, y in zip(sides, want))
        if not err <= 1e-5:
            raise SystemExit(f"bench_cross.py: the forward launch and the torch form disagree (relative error {err:.2e})")
        bwd()
        grads = ref_fwd_bwd()
        dw = torch.as_strided(slabs, (ns, d, d), (stride, d, 1)).sum(0)
        werr = max(((sides[0]["dx"] - grads[1]).abs().max() / grads[1].abs().max()).item(),
                   ((sides[0]["dx0"] - grads[0]).abs().max() / grads[0].abs().max()).item(),
                   ((dw - grads[2]).abs().max() / grads[2].abs().max()).item())
        if not werr <= 1e-4:
            raise SystemExit(f"bench_cross.py: the backward launch and autograd disagree (relative error {werr:.2e})")
        t = {"fwd_us": _graph_us(fwd, args.iters, args.warmup), "bwd_us": _graph_us(bwd, args.iters, args.warmup),
             "torch_fwd_us": _graph_us(ref_fwd, args.iters, args.warmup)}
        how = "graph"
        try:
            t["torch_fwd_bwd_us"] = _graph_us(ref_fwd_bwd, args.iters, args.warmup)
        except Exception as exc:                             # autograd's backward refused the capture: time it eagerly
            print(f"bench_cross.py: torch fwd+bwd not captured ({type(exc).__name__}); timing it eagerly", file=sys.stderr)
            torch.cuda.synchronize()
            how = "eager"
            t["torch_fwd_us"] = _eager_us(ref_fwd, args.iters, args.warmup)
            t["torch_fwd_bwd_us"] = _eager_us(ref_fwd_bwd, args.iters, args.warmup)
        t["torch_bwd_us"] = t["torch_fwd_bwd_us"] - t["torch_fwd_us"]
        t["fwd_us_again"], t["bwd_us_again"] = _graph_us(fwd, args.iters, args.warmup), _graph_us(bwd, args.iters, args.warmup)
        t["fwd_kernel_us"] = _kernel_us(["cross_fwd"], fwd, args.iters)["cross_fwd"]
        t["bwd_kernel_us"] = _kernel_us(["cross_bwd"], bwd, args.iters)["cross_bwd"]
        flops = 2 * 2.0 * n * d * d                                                  # both towers
        fwd_bytes, bwd_bytes = 2 * 4 * n * d * 4, 2 * 6 * n * d * 4
        emit({"what": "cross_kernels", "rows_per_side": n, "sides": 2, "D": d, "n_slabs": ns, "torch_timing": how,
              **{k: round(v, 3) for k, v in t.items()},
              "fwd_frac_mfma": round(flops / (t["fwd_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "bwd_frac_mfma": round(2 * flops / (t["bwd_us"] * 1e-6) / PEAK_F32_MFMA, 4),
              "fwd_gbs": round(fwd_bytes / (t["fwd_us"] * 1e-6) / 1e9, 1), "bwd_gbs": round(bwd_bytes / (t["bwd_us"] * 1e-6) / 1e9, 1),
              "torch_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3),
              "fwd_vs_torch_rel_err": float(f"{err:.3e}")})
        del leaves, grads, slabs, sides
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name, layers in (("plain", 0), ("plain_materialised", 0), ("cross1", 1), ("cross2", 2)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], cross_layers=layers)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    trainers["plain_materialised"].fuse_lookup = False
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms all of them up
            for name, t in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    t.step(*batches[s % len(batches)])
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for t in trainers.values():
            t.check_ids()
        med = {k: statistics.median(v) for k, v in times.items()}
        emit({"what": "step", "ids": variant, "optimizer": "adagrad", "batch": CFG3["batch"], "dim": CFG3["dim"],
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "steps": args.steps, "rounds": args.rounds,
              **{f"step_ms_{k}": round(v, 4) for k, v in med.items()},
              "cross1_to_plain": round(med["cross1"] / med["plain"], 4), "cross2_to_plain": round(med["cross2"] / med["plain"], 4),
              "cross1_to_materialised": round(med["cross1"] / med["plain_materialised"], 4),
              "cross2_to_materialised": round(med["cross2"] / med["plain_materialised"], 4),
              "loss_cross2": round(trainers["cross2"].loss.item(), 3),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cross.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross.py needs a GPU: nothing here is measured on the CPU")
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

"""Layer normalisation of the tower hidden layers: the forward launch (tt_layer_norm_fwd_f32, LayerNorm + ReLU + sign bits) and
the backward launch (tt_layer_norm_bwd_f32), both towers per launch, beside torch eager's relu(F.layer_norm(z, ...)) and its
autograd backward on the same device, and the cfg3 train step with and without layer_norm.  JSON lines, printed and appended
to --out:

    python bench_layernorm.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/layernorm.jsonl]

Kernel lines ("what": "layernorm_kernels"): two problems (both towers) of 8192 rows each, hidden width in {128, 256, 512}; the
backward launch runs in place (dz on dn) with tt_layer_norm_num_slabs(8192) = 256 slabs, as the train step's does.
  fwd_us / bwd_us            per launch (BOTH towers), from replays of a HIP graph of `iters` back-to-back calls (the best of five
                             replays); *_again: the same measurement repeated - the spread of the method
  fwd_kernel_us / bwd_kernel_us   the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_fwd_us               relu(F.layer_norm(z, (dim,), gamma, beta, eps)) for both towers, the same way
  torch_fwd_bwd_us           that forward and autograd's backward for z, gamma and beta of both towers; torch_bwd_us = the
                             difference ("torch_timing": "graph", or "eager" where the backward could not be captured)
  fwd_gbs / bwd_gbs          8 * rows * dim (z in, y out) and 12 * rows * dim (z, dn in, dz out) bytes per tower per second
  fwd_frac_hbm / bwd_frac_hbm     those as fractions of 8.0e12 B/s
Nothing here is a target: nobody had measured any of it before this file.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) without and with layer_norm in the same process,
alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median round of each
and every round's time, on uniform ("U") and power-law ("Z") ids.  Two bases: the step without the option as bench.py runs it
(one C call), and the same step through the Python sequence of launches ("plain_sequence": TT_COMPOSITE_STEP=0's path, which
keeps the fused two-layer forward) - the path the normalisation launches are added to, at the price of that fused forward.
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

PEAK_HBM = 8.0e12
EPS = 1e-3


def kernel_phase(args, emit):
    import torch.nn.functional as F
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    n = CFG3["batch"]
    g = torch.Generator(device=dev).manual_seed(7)
    ns = ops.layer_norm_num_slabs(n)
    for d in (128, 256, 512):
        sides = []
        for _ in range(2):
            z = 0.5 + 1.5 * torch.randn(n, d, device=dev, generator=g)
            sides.append(dict(z=z, gamma=torch.rand(d, device=dev, generator=g) + 0.5, beta=torch.rand(d, device=dev, generator=g) * 0.4 - 0.2,
                              g=torch.randn(n, d, device=dev, generator=g), y=torch.empty(n, d, device=dev),
                              bits=ops.relu_bits_like(n, d, dev), dn=torch.empty(n, d, device=dev)))
        stride = 4 * d
        slabs = torch.empty(ns * stride, device=dev)
        leaves = [[s[k].clone().requires_grad_(True) for k in ("z", "gamma", "beta")] for s in sides]

        def fwd():
            ops.layer_norm2(*[(s["z"], s["gamma"], s["beta"], s["y"], s["bits"]) for s in sides], eps=EPS, relu=True)

        def bwd():
            ops.layer_norm_bwd2(*[(s["z"], s["gamma"], s["dn"], s["dn"], slabs[k * d:], slabs[2 * d + k * d:]) for k, s in enumerate(sides)],
                                eps=EPS, n_slabs=ns, slab_stride=stride)

        def ref_fwd(ts=None):
            ts = [(s["z"], s["gamma"], s["beta"]) for s in sides] if ts is None else ts
            return [torch.relu(F.layer_norm(t[0], (d,), t[1], t[2], EPS)) for t in ts]

        def ref_fwd_bwd():
            ys = ref_fwd(leaves)
            return torch.autograd.grad(ys, [t for l in leaves for t in l], [s["g"] for s in sides])

        fwd()
        want = ref_fwd()
        err = max(((s["y"] - y).abs().max() / y.abs().max()).item() for s, y in zip(sides, want))
        if not err <= 1e-5:
            raise SystemExit(f"bench_layernorm.py: the forward launch and the torch form disagree (relative error {err:.2e})")
        for s in sides:                                      # dn: the upstream gradient behind the ReLU mask, as the dx epilogue leaves it
            s["dn"].copy_(s["g"] * (s["y"] > 0))
        bwd()
        grads = ref_fwd_bwd()
        dg = torch.as_strided(slabs, (ns, d), (stride, 1)).sum(0)
        werr = max(((sides[0]["dn"] - grads[0]).abs().max() / grads[0].abs().max()).item(),
                   ((dg - grads[1]).abs().max() / grads[1].abs().max()).item())
        if not werr <= 1e-4:
            raise SystemExit(f"bench_layernorm.py: the backward launch and autograd disagree (relative error {werr:.2e})")
        t = {"fwd_us": _graph_us(fwd, args.iters, args.warmup), "bwd_us": _graph_us(bwd, args.iters, args.warmup),
             "torch_fwd_us": _graph_us(ref_fwd, args.iters, args.warmup)}
        how = "graph"
        try:
            t["torch_fwd_bwd_us"] = _graph_us(ref_fwd_bwd, args.iters, args.warmup)
        except Exception as exc:                             # autograd's backward refused the capture: time it eagerly
            print(f"bench_layernorm.py: torch fwd+bwd not captured ({type(exc).__name__}); timing it eagerly", file=sys.stderr)
            torch.cuda.synchronize()
            how = "eager"
            t["torch_fwd_us"] = _eager_us(ref_fwd, args.iters, args.warmup)
            t["torch_fwd_bwd_us"] = _eager_us(ref_fwd_bwd, args.iters, args.warmup)
        t["torch_bwd_us"] = t["torch_fwd_bwd_us"] - t["torch_fwd_us"]
        t["fwd_us_again"], t["bwd_us_again"] = _graph_us(fwd, args.iters, args.warmup), _graph_us(bwd, args.iters, args.warmup)
        t["fwd_kernel_us"] = _kernel_us(["layer_norm_fwd"], fwd, args.iters)["layer_norm_fwd"]
        t["bwd_kernel_us"] = _kernel_us(["layer_norm_bwd"], bwd, args.iters)["layer_norm_bwd"]
        fwd_bytes, bwd_bytes = 2 * 8 * n * d, 2 * 12 * n * d                          # both towers
        fwd_bs, bwd_bs = fwd_bytes / (t["fwd_us"] * 1e-6), bwd_bytes / (t["bwd_us"] * 1e-6)
        emit({"what": "layernorm_kernels", "rows_per_side": n, "sides": 2, "dim": d, "n_slabs": ns, "torch_timing": how,
              **{k: round(v, 3) for k, v in t.items()},
              "fwd_gbs": round(fwd_bs / 1e9, 1), "bwd_gbs": round(bwd_bs / 1e9, 1),
              "fwd_frac_hbm": round(fwd_bs / PEAK_HBM, 4), "bwd_frac_hbm": round(bwd_bs / PEAK_HBM, 4),
              "torch_to_fwd": round(t["torch_fwd_us"] / t["fwd_us"], 3), "torch_to_bwd": round(t["torch_bwd_us"] / t["bwd_us"], 3),
              "fwd_vs_torch_rel_err": float(f"{err:.3e}")})
        del leaves, grads, slabs, sides
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name, on in (("plain", False), ("plain_sequence", False), ("layer_norm", True)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], layer_norm=on)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    trainers["plain_sequence"].use_composite = False
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
              "layer_norm_to_plain": round(med["layer_norm"] / med["plain"], 4),
              "layer_norm_to_sequence": round(med["layer_norm"] / med["plain_sequence"], 4),
              "loss_layer_norm": round(trainers["layer_norm"].loss.item(), 3),
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "layernorm.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_layernorm.py needs a GPU: nothing here is measured on the CPU")
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

"""The dense numeric side features: the forward launch (tt_dense_features_fwd_f32) and the backward launch
(tt_dense_features_bwd_f32) beside the torch equivalent of the forward (index_select, normalise, addmm) on the same device, and
the cfg3 train step with and without the feature.  JSON lines, printed and appended to --out:

    python bench_features.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/features.jsonl]

Kernel lines ("what": "features_kernels"): both towers in ONE launch - 8192 rows x dim 128 on each side, F in {5, 16, 32}, a
--users-row and an --items-row feature matrix, power-law ("Z") ids - accumulating into materialised tower-input rows and keeping
the normalised rows, as the train step does; the backward launch reduces both sides' rows into
tt_dense_features_num_slabs(8192) = 64 slabs each.
  fwd_us / bwd_us / torch_us    per call, from replays of a HIP graph of `iters` back-to-back calls (no host time between them; the
                                best of five replays); *_again: the same measurement repeated - the spread of the method
  fwd_kernel_us / bwd_kernel_us the dispatch's own begin-to-end time (the library's built-in timing, eager launches)
  torch_us is, per side, index_select + (x - mean) * inv_std + clamp + addmm into the rows (eight or so launches for both sides)
  fwd_bytes = per side n * (8 + 4 F) read (ids, feature rows) + n * (8 dim + 4 F) moved (rows read and written, z written)
  + 4 F dim (the kernel, once); bwd_bytes = per side n * 4 (F + dim) read + slabs * 4 F dim written; bytes / call time, also as
  a fraction of 8.0e12 B/s.  Nothing here is a target: at these sizes the launches sit near the launch floor.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) without the feature and with it (F on both sides), in the
same process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median
round of each and every round's time, on uniform ("U") and power-law ("Z") ids.  The base of the ratio is the step WITHOUT the
feature.
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

CLIP = 3.0


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    dim, n = CFG3["dim"], CFG3["batch"]
    ids = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
    ops.fill_ids_(ids[0], 1001, 3, args.users, "Z")
    ops.fill_ids_(ids[1], 1001, 4, args.items, "Z")
    g = torch.Generator(device=dev).manual_seed(7)
    rows0 = [torch.randn(n, dim, device=dev, generator=g) * 0.05 for _ in range(2)]
    dys = [torch.randn(n, dim, device=dev, generator=g) * 0.01 for _ in range(2)]
    ns = ops.dense_features_num_slabs(n)
    for F in (5, 16, 32):
        feats = [torch.rand(r, F, device=dev, generator=g) * 5.0 for r in (args.users, args.items)]
        means = [f.mean(0) for f in feats]
        inv_stds = [1.0 / f.std(0, unbiased=False).clamp_min(1e-7) for f in feats]
        projs = [torch.randn(F, dim, device=dev, generator=g) * 0.1 for _ in range(2)]
        outs = [r.clone() for r in rows0]
        zs = [torch.empty(n, F, device=dev) for _ in range(2)]
        slabs = [torch.empty(ns, F, dim, device=dev) for _ in range(2)]
        touts = [r.clone() for r in rows0]

        def fwd():
            ops.dense_features(*[(feats[i], ids[i], means[i], inv_stds[i], projs[i], outs[i], True, zs[i]) for i in range(2)], clip=CLIP)

        def bwd():
            ops.dense_features_bwd(*[(zs[i], dys[i], slabs[i]) for i in range(2)])

        def ref():
            for i in range(2):
                z = ((feats[i].index_select(0, ids[i]) - means[i]) * inv_stds[i]).clamp_(-CLIP, CLIP)
                touts[i].addmm_(z, projs[i])
        fwd()
        ref()
        err = max(((outs[i] - touts[i]).abs().max() / touts[i].abs().max()).item() for i in range(2))
        if not err <= 1e-5:
            raise SystemExit(f"bench_features.py: the launch and the torch form disagree (relative error {err:.2e})")
        bwd()
        werr = max(((slabs[i].sum(0) - zs[i].t() @ dys[i]).abs().max() / (zs[i].t() @ dys[i]).abs().max()).item() for i in range(2))
        if not werr <= 1e-4:
            raise SystemExit(f"bench_features.py: the slab sum and the torch product disagree (relative error {werr:.2e})")
        t = {"fwd_us": _graph_us(fwd, args.iters, args.warmup), "bwd_us": _graph_us(bwd, args.iters, args.warmup),
             "torch_us": _graph_us(ref, args.iters, args.warmup)}
        t["fwd_us_again"], t["bwd_us_again"] = _graph_us(fwd, args.iters, args.warmup), _graph_us(bwd, args.iters, args.warmup)
        t["torch_us_again"] = _graph_us(ref, args.iters, args.warmup)
        t["fwd_kernel_us"] = _kernel_us(["features_fwd"], fwd, args.iters)["features_fwd"]
        t["bwd_kernel_us"] = _kernel_us(["features_bwd"], bwd, args.iters)["features_bwd"]
        fwd_bytes = 2 * (n * (8 + 4 * F) + n * (8 * dim + 4 * F) + 4 * F * dim)
        bwd_bytes = 2 * (n * 4 * (F + dim) + ns * 4 * F * dim)
        emit({"what": "features_kernels", "ids": "Z", "rows": n, "dim": dim, "F": F, "sides": 2, "feature_rows": [args.users, args.items],
              "clip": CLIP, "n_slabs": ns, **{k: round(v, 3) for k, v in t.items()},
              "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
              "fwd_frac_hbm": round(fwd_bytes / (t["fwd_us"] * 1e-6) / PEAK_HBM, 4),
              "bwd_frac_hbm": round(bwd_bytes / (t["bwd_us"] * 1e-6) / PEAK_HBM, 4),
              "torch_to_fwd": round(t["torch_us"] / t["fwd_us"], 3), "fwd_vs_torch_rel_err": float(f"{err:.3e}")})
        del feats, outs, zs, slabs, touts
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    F = args.features
    trainers = {}
    for name, f in (("plain", 0), ("features", F)):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], n_user_features=f, n_item_features=f, feature_clip=CLIP if f else 0.0)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    tr = trainers["features"]
    g = torch.Generator(device=dev).manual_seed(7)
    for side, rows in (("user", args.users), ("item", args.items)):          # U(0, 5) columns with their exact statistics
        x = torch.rand(rows, F, device=dev, generator=g) * 5.0
        getattr(tr, f"{side}_features").copy_(x)
        getattr(tr, f"{side}_feature_mean").copy_(x.mean(0))
        getattr(tr, f"{side}_feature_inv_std").copy_(1.0 / x.std(0, unbiased=False).clamp_min(1e-7))
        del x
    for variant in ("U", "Z"):
        batches = [trainers["plain"].synthetic_batch(1001, s, variant) for s in range(16)]
        times = {k: [] for k in trainers}
        for rnd in range(args.rounds + 1):                                # round 0 warms both up
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
              "tower_dims": CFG3["towers"], "tables": [args.users, args.items], "F": [F, F], "clip": CLIP,
              "steps": args.steps, "rounds": args.rounds, "step_ms_plain": round(med["plain"], 4),
              "step_ms_features": round(med["features"], 4), "features_to_plain": round(med["features"] / med["plain"], 4),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--features", type=int, default=5, help="F of the step lines, on both sides (rating_stats has 5 columns)")
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "features.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_features.py needs a GPU: nothing here is measured on the CPU")
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

"""Global-norm gradient clipping: the two launches of tt_clip_global_norm_f32 over the cfg3 train step's gradient buffers, and
the cfg3 train step with clipping off and on.  JSON lines, printed and appended to --out:

    python bench_clip.py [--iters 100] [--warmup 10] [--steps 200] [--rounds 3] [--out profiles/clip.jsonl]

Kernel line ("what": "clip_kernels"): the buffer list of a cfg3 trainer (Adagrad, batch 8192: the two [8192, 128] tower-input
gradients and the 8 dense segments' 32 slabs each) behind one forward_backward, timed from replays of a HIP graph of `iters`
back-to-back calls (the best of five replays).
  pass_us            trainer.clip_gradients() where nothing is clipped (c = 1e30): launch 1 reads every gradient byte once,
                     launch 2 only the partials
  clip_us            where the gradient IS clipped: launch 2 also reads and writes every byte.  A clipped gradient has the norm c,
                     so the next call would clip nothing: every call is preceded by copies that restore the buffers, and
                     restore_us (the copies alone, the same way) is subtracted
  sumsq_kernel_us / scale_kernel_us   the dispatches' own begin-to-end times (the library's built-in timing, eager launches, the
                     pass case)
  grad_bytes         bytes of all the buffers;  pass_frac_hbm = grad_bytes / pass_us and clip_frac_hbm = 3 * grad_bytes / clip_us
                     as fractions of 8.0e12 B/s
Step lines ("what": "step"): trainer.step at cfg3 in the same process, alternating for `rounds` rounds of `steps` steps (host
clock around steps that end in a synchronise), the median round of each and every round's time, on uniform ("U") and power-law
("Z") ids: "default" (clipping off, the one C call bench.py times), "sequence" (off, use_composite = False: the Python sequence
the clip launches are added to) and "clip" (global_clipnorm = 1: every step of this workload is clipped).
Nothing here is a target: nobody had measured any of it before this file.
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

PEAK_HBM = 8.0e12


def _trainer(args, dev, **kw):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"], temperature=0.1,
                         l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad", batch_size=CFG3["batch"], **kw)
    return TwoTowerTrainer(cfg, dev, seed=1001)


def kernel_phase(args, emit):
    dev = torch.device("cuda:0")
    tr = _trainer(args, dev, global_clipnorm=1e30)
    tr.forward_backward(*tr.synthetic_batch(1001, 0, "U"))
    tr.check_ids()
    bufs = [tr.user_tower.demb, tr.item_tower.demb]
    for tw in (tr.user_tower, tr.item_tower):
        bufs += list(tw.dw_slabs) + list(tw.db_slabs)
    saved = [b.clone() for b in bufs]
    grad_bytes = sum(b.numel() * 4 for b in bufs)
    tr.clip_gradients()
    norm = tr.grad_norm.item()

    def restore():
        for b, s in zip(bufs, saved):
            b.copy_(s)

    def restore_and_clip():
        restore()
        tr.clip_gradients()

    t = {"pass_us": _graph_us(tr.clip_gradients, args.iters, args.warmup)}
    t.update({f"{k}_kernel_us": v for k, v in zip(("sumsq", "scale"), _kernel_us(["clip_sumsq", "clip_scale"], tr.clip_gradients, args.iters).values())})
    t["pass_us_again"] = _graph_us(tr.clip_gradients, args.iters, args.warmup)
    tr.cfg.global_clipnorm = norm / 4
    t["restore_us"] = _graph_us(restore, args.iters, args.warmup)
    t["restore_and_clip_us"] = _graph_us(restore_and_clip, args.iters, args.warmup)
    t["clip_us"] = t["restore_and_clip_us"] - t["restore_us"]
    if tr.clip_scale.item() != 0.25 or tr.grad_norm.item() != norm:
        raise SystemExit(f"bench_clip.py: the restored gradient was not clipped to a quarter (scale {tr.clip_scale.item()})")
    emit({"what": "clip_kernels", "batch": CFG3["batch"], "dim": CFG3["dim"], "tower_dims": CFG3["towers"], "buffers": tr._clip.n,
          "grad_bytes": grad_bytes, "grad_norm": norm, **{k: round(v, 3) for k, v in t.items()},
          "pass_frac_hbm": round(grad_bytes / (t["pass_us"] * 1e-6) / PEAK_HBM, 4),
          "clip_frac_hbm": round(3 * grad_bytes / (t["clip_us"] * 1e-6) / PEAK_HBM, 4)})


def steps(args, emit):
    dev = torch.device("cuda:0")
    trainers = {"default": _trainer(args, dev), "sequence": _trainer(args, dev), "clip": _trainer(args, dev, global_clipnorm=1.0)}
    trainers["sequence"].use_composite = False
    for variant in ("U", "Z"):
        batches = [trainers["default"].synthetic_batch(1001, s, variant) for s in range(16)]
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
              "clip_to_default": round(med["clip"] / med["default"], 4), "clip_to_sequence": round(med["clip"] / med["sequence"], 4),
              "sequence_to_default": round(med["sequence"] / med["default"], 4),
              "grad_norm_clip": round(trainers["clip"].grad_norm.item(), 3), "clip_scale": trainers["clip"].clip_scale.item(),
              **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel line only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clip.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs a GPU: nothing here is measured on the CPU")
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

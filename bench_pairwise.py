"""The pairwise retrieval losses (csrc/pairwise.hip): the training entry beside the softmax scorer's at the same shape and beside
the same math as a torch sequence with its autograd backward, and the cfg3 train step under each retrieval loss.  JSON lines,
printed and appended to --out:

    python bench_pairwise.py [--iters 20] [--warmup 3] [--steps 100] [--rounds 3] [--out profiles/pairwise.jsonl]

Kernel lines ("what": "pairwise_kernels"): 8192 x 8192, dim in {64, 128, 256}, kind logistic (BPR) / hinge, cand_ids off / on
(accidental-hit removal; about a tenth of the ids duplicated), temperature 0.1, reduction mean.
  fwd_bwd_us                 tt_retrieval_pairwise_fwd_bwd_f32 per call, from replays of a HIP graph of `iters` back-to-back
                             calls (the best of five replays); fwd_bwd_us_again: the same measurement repeated - the spread
  pass_q_us / pass_c_us / aux_us   the dispatches' own begin-to-end times (the library's built-in timing, eager launches;
                             aux_us: the median of the call's small launches - row terms, combine, loss sum, dc reduction)
  softmax_fwd_bwd_us         ops.retrieval_fwd_bwd (the softmax scorer's training entry) at the same shape, the same way
  torch_fwd_bwd_us           matmul, the loss on the [8192, 8192] matrix and autograd's backward for q and c, eager calls
                             between events (dim 128 only: it does not depend on the dim to speak of)
  frac_mfma                  the 8 nq nc D executed FLOPs over fwd_bwd_us as a fraction of the f32 MFMA peak (157.3e12)
  softmax_frac_mfma          the scorer's 6 nq nc D over its time, likewise
Nothing here is a target: nobody had measured any of it before this file.
Step lines ("what": "step"): trainer.step at cfg3 (Adagrad, batch 8192) with retrieval_loss softmax / bpr / hinge in the same
process, alternating for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise); the median round
of each and every round's time.  The base of the ratios is the softmax step.
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
INV_T, MARGIN = 10.0, 0.5


def _torch_loss(q, c, kind, ids):
    s = q @ c.t() * INV_T
    x = s.diagonal()[:, None] - s
    phi = torch.nn.functional.softplus(-x) if kind == "logistic" else torch.clamp(MARGIN - x, min=0.0)
    valid = ~torch.eye(q.shape[0], dtype=torch.bool, device=q.device)
    if ids is not None:
        valid &= ids[None, :] != ids[:, None]
    n = valid.sum(1).clamp(min=1).to(torch.float32)
    return (torch.where(valid, phi, torch.zeros_like(phi)).sum(1) / n).sum()


def kernel_phase(args, emit):
    from two_tower_amazon_recommender_amd import ops
    dev = torch.device("cuda:0")
    n = CFG3["batch"]
    g = torch.Generator(device=dev).manual_seed(7)
    ids_all = torch.arange(n, device=dev, dtype=torch.int64)
    dup = torch.rand(n, device=dev, generator=g) < 0.1
    ids_all[dup] = torch.randint(0, n, (int(dup.sum()),), device=dev, generator=g)
    for d in (64, 128, 256):
        q = (torch.rand(n, d, device=dev, generator=g) * 2 - 1) / d ** 0.5
        c = (torch.rand(n, d, device=dev, generator=g) * 2 - 1) / d ** 0.5
        ws = torch.empty(ops.retrieval_pairwise_workspace_bytes(n, n, d), dtype=torch.uint8, device=dev)
        ws_s = torch.empty(ops.retrieval_workspace_bytes(n, n, d), dtype=torch.uint8, device=dev)
        per_row, loss, lse = torch.empty(n, device=dev), torch.empty(1, device=dev), torch.empty(n, device=dev)
        dq, dc = torch.empty_like(q), torch.empty_like(c)
        for ids in (None, ids_all):
            def softmax():
                ops.retrieval_fwd_bwd(q, c, INV_T, ws_s, lse, per_row, loss, dq, dc, cand_ids=ids)
            softmax_us = _graph_us(softmax, args.iters, args.warmup)
            for kind in ("logistic", "hinge"):
                def call():
                    ops.retrieval_pairwise_fwd_bwd(q, c, INV_T, ws, per_row, loss, dq, dc, kind=kind, margin=MARGIN, cand_ids=ids)
                rec = {"what": "pairwise_kernels", "nq": n, "nc": n, "dim": d, "kind": kind, "cand_ids": ids is not None,
                       "workspace_bytes": ws.numel(), "softmax_workspace_bytes": ws_s.numel()}
                if d == 128:                                 # the torch form: also the check that both compute the same thing
                    leaves = [q.clone().requires_grad_(True), c.clone().requires_grad_(True)]
                    def ref():
                        return torch.autograd.grad(_torch_loss(leaves[0], leaves[1], kind, ids), leaves)
                    call()
                    want = ref()
                    err = max(((dq - want[0]).abs().max() / want[0].abs().max()).item(),
                              ((dc - want[1]).abs().max() / want[1].abs().max()).item())
                    if not err <= 1e-2:                      # (the torch side is f32 eager; hinge pairs on the kink may differ)
                        raise SystemExit(f"bench_pairwise.py: the entry and the torch form disagree (relative error {err:.2e})")
                    rec["torch_fwd_bwd_us"] = round(_eager_us(ref, max(args.iters // 4, 3), 2), 3)
                    rec["vs_torch_rel_err"] = float(f"{err:.3e}")
                    del leaves, want
                    torch.cuda.empty_cache()
                t = _graph_us(call, args.iters, args.warmup)
                again = _graph_us(call, args.iters, args.warmup)
                parts = _kernel_us(["pairwise_q", "pairwise_c", "pairwise_aux"], call, args.iters)
                rec.update(fwd_bwd_us=round(t, 3), fwd_bwd_us_again=round(again, 3), pass_q_us=round(parts["pairwise_q"], 3),
                           pass_c_us=round(parts["pairwise_c"], 3), aux_us=round(parts["pairwise_aux"], 3),
                           softmax_fwd_bwd_us=round(softmax_us, 3), pairwise_to_softmax=round(t / softmax_us, 4),
                           frac_mfma=round(8.0 * n * n * d / (t * 1e-6) / PEAK_F32_MFMA, 4),
                           softmax_frac_mfma=round(6.0 * n * n * d / (softmax_us * 1e-6) / PEAK_F32_MFMA, 4))
                if "torch_fwd_bwd_us" in rec:
                    rec["torch_to_pairwise"] = round(rec["torch_fwd_bwd_us"] / t, 3)
                emit(rec)
        del ws, ws_s
        torch.cuda.empty_cache()


def steps(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    trainers = {}
    for name in ("softmax", "bpr", "hinge"):
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad",
                             batch_size=CFG3["batch"], retrieval_loss=name, pairwise_margin=MARGIN)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    batches = [trainers["softmax"].synthetic_batch(1001, s, "U") for s in range(16)]
    times = {k: [] for k in trainers}
    for rnd in range(args.rounds + 1):                                    # round 0 warms all three up
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
    emit({"what": "step", "ids": "U", "optimizer": "adagrad", "batch": CFG3["batch"], "dim": CFG3["dim"], "tower_dims": CFG3["towers"],
          "tables": [args.users, args.items], "steps": args.steps, "rounds": args.rounds,
          **{f"step_ms_{k}": round(v, 4) for k, v in med.items()},
          "bpr_to_softmax": round(med["bpr"] / med["softmax"], 4), "hinge_to_softmax": round(med["hinge"] / med["softmax"], 4),
          **{f"loss_{k}": round(t.loss.item(), 4) for k, t in trainers.items()},
          **{f"rounds_ms_{k}": [round(v, 4) for v in times[k]] for k in times}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--users", type=int, default=CFG3["n_users"])
    ap.add_argument("--items", type=int, default=CFG3["n_items"])
    ap.add_argument("--skip-steps", action="store_true", help="the kernel lines only")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pairwise.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairwise.py needs a GPU: nothing here is measured on the CPU")
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

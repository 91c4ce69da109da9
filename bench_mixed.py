"""Mixed negative sampling against the in-batch train step at cfg3, and the sampler launch alone.  JSON lines, printed and
appended to --out:

    python bench_mixed.py [--steps 200] [--rounds 3] [--iters 200] [--optimizers sgd,adagrad,adam] [--out profiles/mixed.jsonl]

Step lines ("what": "step"), one per optimizer and id distribution (uniform "U", power-law "Z"): trainer.step of three trainers
on the same batches - in-batch (the step the flagship benchmark measures), mixed with N = B/4 and mixed with N = B sampled
negatives - ALTERNATING for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise; round 0 warms
every trainer up); the median round of each and the ratios to the in-batch step.
Sampler lines ("what": "sampler"): tt_sample_candidates_i64 at B = 8192 for N = B/4 and N = B, uniform and alias sampler, with and
without the probabilities: the dispatch's own begin-to-end time (the library's built-in timing, tag "sample") and the bytes the
launch moves.
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

CFG3 = dict(n_users=5_000_000, n_items=10_000_000, dim=128, towers=[256, 128], batch=8192)


def _item_freq(n_items: int, dev) -> torch.Tensor:
    """A power-law frequency vector (item rank r: ~ 1 / (r + 1)), as a vocabulary in order of frequency has."""
    f = 1.0 / torch.arange(1, n_items + 1, device=dev, dtype=torch.float64)
    return (f / f.sum()).to(torch.float32)


def sampler_phase(args, emit):
    from two_tower_amazon_recommender_amd import _lib, ops
    dev = torch.device("cuda:0")
    b, n_items = CFG3["batch"], args.items
    pos = torch.empty(b, dtype=torch.int64, device=dev)
    ops.fill_ids_(pos, 1001, 4, n_items, "Z")
    freq = _item_freq(n_items, dev)
    w = freq.double() ** 0.75
    sp = (w / w.sum()).to(torch.float32)
    thr, idx = (torch.from_numpy(a).to(dev) for a in ops.build_alias_table(w.cpu().numpy()))
    for n_neg in (b // 4, b):
        ids = torch.empty(b + n_neg, dtype=torch.int64, device=dev)
        prob = torch.empty(b + n_neg, device=dev)
        for sampler in ("uniform", "alias"):
            for with_prob in (False, True):
                kw = dict(sampler=sampler, alias=(thr, idx) if sampler == "alias" else None, item_freq=freq if with_prob else None,
                          sampler_prob=sp if (with_prob and sampler == "alias") else None, seed=1001, tensor_id=10)
                for s in range(args.warmup):
                    ops.sample_candidates(pos, n_items, n_neg, ids, prob, start=s * n_neg, **kw)
                _lib.profile_enable("sample", args.iters)
                for s in range(args.iters):
                    ops.sample_candidates(pos, n_items, n_neg, ids, prob, start=s * n_neg, **kw)
                ms = _lib.profile_read("sample", args.iters)[0]
                _lib.profile_enable("")
                n = b + n_neg
                # ids in and out, the probabilities out, and per candidate the random 4-byte reads (alias: 2 per draw; 1-2 per probability)
                nbytes = 8 * b + 8 * n + (4 * n * (1 + 1 + (sampler == "alias")) if with_prob else 0) + (8 * n_neg if sampler == "alias" else 0)
                emit({"what": "sampler", "batch": b, "n_neg": n_neg, "n_items": n_items, "sampler": sampler, "probabilities": with_prob,
                      "kernel_us": round(statistics.median(ms) * 1e3, 3), "kernel_us_min": round(min(ms) * 1e3, 3), "bytes": nbytes,
                      "launches": len(ms)})


def step_phase(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    b = CFG3["batch"]
    freq = _item_freq(args.items, dev) if args.correct_sampling_bias else None
    for opt in args.optimizers.split(","):
        variants = {"in_batch": 0, "mixed_quarter": b // 4, "mixed_full": b}
        trainers = {}
        for name, n_neg in variants.items():
            mixed = dict(candidate_sampling="mixed", n_sampled_negatives=n_neg) if n_neg else {}
            cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                                 temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer=opt, batch_size=b, **mixed)
            trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
            if n_neg and freq is not None:
                trainers[name].set_item_frequencies(freq)
        for ids_variant in ("U", "Z"):
            batches = [trainers["in_batch"].synthetic_batch(1001, s, ids_variant) for s in range(16)]
            times = {name: [] for name in variants}
            for rnd in range(args.rounds + 1):                            # round 0 warms every trainer up
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
            med = {name: statistics.median(times[name]) for name in variants}
            emit({"what": "step", "optimizer": opt, "ids": ids_variant, "batch": b, "dim": CFG3["dim"], "tower_dims": CFG3["towers"],
                  "tables": [args.users, args.items], "steps": args.steps, "rounds": args.rounds,
                  "correction": bool(args.correct_sampling_bias), "n_neg": variants,
                  **{f"step_ms_{name}": round(med[name], 4) for name in variants},
                  "mixed_quarter_to_in_batch": round(med["mixed_quarter"] / med["in_batch"], 4),
                  "mixed_full_to_in_batch": round(med["mixed_full"] / med["in_batch"], 4),
                  **{f"rounds_ms_{name}": [round(v, 4) for v in times[name]] for name in variants}})
        del trainers
        torch.cuda.empty_cache()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="sampler launches timed per shape")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--optimizers", default="sgd,adagrad,adam")
    ap.add_argument("--correct-sampling-bias", action="store_true", help="mixed trainers also write and apply the mixture probabilities")
    ap.add_argument("--users", type=int, default=CFG3["n_users"], help="rows of the user table (cfg3: 5,000,000)")
    ap.add_argument("--items", type=int, default=CFG3["n_items"], help="rows of the item table (cfg3: 10,000,000)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixed.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    sampler_phase(args, emit)
    torch.cuda.empty_cache()
    step_phase(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The streaming frequency estimator: the call alone beside the gather it replaces, and the cfg3 train step with the estimator
off and on.  JSON lines, printed and appended to --out:

    python bench_freq.py [--steps 200] [--rounds 3] [--iters 200] [--out profiles/freq.jsonl]

Call lines ("what": "call"): tt_frequency_estimate_i64 at n = 8192 with n_update = n (the in-batch step's call: one launch) and at
n = 8192 + 8192 with n_update = 8192 and the mixture formula (the mixed step's call: two launches), 2 hash rows of 2^25 slots,
10M items, power-law ids, the step counted on from call to call: each dispatch's own begin-to-end time (the library's built-in
timing, tags "freq_update" / "freq_estimate"), the stream time per call between two events around `iters` calls, and - between
the same events - the `item_prob[ids]` gather of the offline correction at the same n.
Step lines ("what": "step"): trainer.step at cfg3 with the Adagrad optimizer on the same batches - without a correction ("off"),
with the offline correction (`item_prob[ids]` gathered per step and passed as candidate_sampling_probability) and with the
estimator on (in-batch) - ALTERNATING for `rounds` rounds of `steps` steps (host clock around steps that end in a synchronise;
round 0 warms every trainer up); the median round of each and the ratios.
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
HASHES, SLOTS, ALPHA, TID = 2, 1 << 25, 0.01, 56


def _stream_us(fn, iters: int) -> float:
    """Stream time per call of ``fn(i)`` in microseconds: two events around ``iters`` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(i)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def call_phase(args, emit):
    from two_tower_amazon_recommender_amd import _lib, ops
    dev = torch.device("cuda:0")
    b, n_items = CFG3["batch"], args.items
    item_prob = torch.full((n_items,), 1.0 / n_items, device=dev)
    for name, n, n_update, mix in (("in_batch", b, b, False), ("mixed", 2 * b, b, True)):
        ids = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(16)]           # 16 batches, taken in turn
        for s, t in enumerate(ids):
            ops.fill_ids_(t, 1001, 4, n_items, "Z", start=s * n)
        sketch = ops.new_frequency_sketch(HASHES, SLOTS, dev)
        prob = torch.empty(n, device=dev)
        step = [0]

        def call(i):
            step[0] += 1
            ops.frequency_estimate_(sketch, ids[i % len(ids)], n_update, step[0], ALPHA, n_items, prob, seed=1001, tensor_id=TID, mix=mix)

        def gather(i):
            torch.index_select(item_prob, 0, ids[i % len(ids)], out=prob)
        for i in range(args.warmup):
            call(i); gather(i)
        tags = ("freq_update", "freq_estimate") if mix else ("freq_update",)
        _lib.profile_enable(",".join(tags), args.iters)
        for i in range(args.iters):
            call(i)
        kernel_us = {tag: [v * 1e3 for v in _lib.profile_read(tag, args.iters)[0]] for tag in tags}
        _lib.profile_enable("")
        call_us, gather_us = _stream_us(call, args.iters), _stream_us(gather, args.iters)
        # per id: 8 bytes of id in, 4 of probability out, HASHES random 8-byte slot reads and (updating ids) as many writes
        nbytes = 12 * n + 8 * HASHES * (n + n_update)
        emit({"what": "call", "shape": name, "n": n, "n_update": n_update, "mix": mix, "hashes": HASHES, "slots": SLOTS, "n_items": n_items,
              **{f"kernel_us_{tag}": round(statistics.median(v), 3) for tag, v in kernel_us.items()},
              **{f"kernel_us_min_{tag}": round(min(v), 3) for tag, v in kernel_us.items()},
              "call_stream_us": round(call_us, 3), "gather_stream_us": round(gather_us, 3), "bytes": nbytes, "iters": args.iters})
        del sketch
        torch.cuda.empty_cache()


def step_phase(args, emit):
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    dev = torch.device("cuda:0")
    b = CFG3["batch"]
    # "offline": the correction as train.py --correct-sampling-bias applies it - a gather from a counted [n_items] vector per step,
    # passed as candidate_sampling_probability - so that the estimator's cost is seen beside the correction's own
    variants = {"off": {}, "offline": {}, "streaming": dict(sampling_bias_estimator="streaming", freq_alpha=ALPHA, freq_hashes=HASHES)}
    item_prob = torch.full((args.items,), 1.0 / args.items, device=dev)
    trainers = {}
    for name, kw in variants.items():
        cfg = TwoTowerConfig(n_users=args.users, n_items=args.items, embedding_dim=CFG3["dim"], tower_dims=CFG3["towers"],
                             temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer="adagrad", batch_size=b, **kw)
        trainers[name] = TwoTowerTrainer(cfg, dev, seed=1001)
    for ids_variant in ("U", "Z"):
        batches = [trainers["off"].synthetic_batch(1001, s, ids_variant) for s in range(16)]
        times = {name: [] for name in variants}
        for rnd in range(args.rounds + 1):                                # round 0 warms both trainers up
            for name, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in range(args.steps):
                    u, i = batches[s % len(batches)]
                    if name == "offline":
                        tr.step(u, i, candidate_sampling_probability=item_prob[i])
                    else:
                        tr.step(u, i)
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
        for tr in trainers.values():
            tr.check_ids()
        med = {name: statistics.median(times[name]) for name in variants}
        emit({"what": "step", "optimizer": "adagrad", "ids": ids_variant, "batch": b, "dim": CFG3["dim"], "tower_dims": CFG3["towers"],
              "tables": [args.users, args.items], "steps": args.steps, "rounds": args.rounds, "hashes": HASHES,
              "slots": trainers["streaming"].cfg.freq_slot_count,
              **{f"step_ms_{name}": round(med[name], 4) for name in variants},
              "streaming_to_off": round(med["streaming"] / med["off"], 4),
              "streaming_to_offline": round(med["streaming"] / med["offline"], 4),
              **{f"rounds_ms_{name}": [round(v, 4) for v in times[name]] for name in variants}})


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="estimator calls timed per shape")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--users", type=int, default=CFG3["n_users"], help="rows of the user table (cfg3: 5,000,000)")
    ap.add_argument("--items", type=int, default=CFG3["n_items"], help="rows of the item table (cfg3: 10,000,000)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "freq.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_freq.py needs a GPU: nothing here is measured on the CPU")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    call_phase(args, emit)
    torch.cuda.empty_cache()
    step_phase(args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())

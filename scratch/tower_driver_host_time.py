"""Host time of the tower drivers alone: forward + backward of both towers with every launcher replaced by a no-op and the
towers built on CPU tensors.  This is Python overhead per train step and nothing else - no kernel runs, no GPU is needed.
Per row: the median over 5 repeats of 2000 iterations, in microseconds per forward + backward."""
import os
import statistics
import sys
import time

import pytest

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
import test_tower_drivers_cpu as T  # noqa: E402
from two_tower_amazon_recommender_amd import ops, trainer  # noqa: E402

ROWS = {"symmetric [64, 32, 32], dropout": dict(user=[64, 32, 32], dropout=0.1),
        "[64, 32] / [64, 64, 32]": dict(user=[64, 32], item=[64, 64, 32]),
        "[64, 32] / [64, 64, 32], layer norm": dict(user=[64, 32], item=[64, 64, 32], ln=True),
        "symmetric [64, 32, 32], layer norm, 2 cross layers": dict(user=[64, 32, 32], ln=True, cross=2)}


def step_fn(case):
    cfg, ut, it = T.build_towers(case)

    def step(s):
        drops = tuple((cfg.dropout_rate, T.SEED, i, s * T.BATCH) for i in range(2))
        trainer.towers_forward((ut, it), dropouts=drops)
        trainer.towers_backward((ut, it), cfg.dropout_rate)
    return step


def main(iters=2000, repeats=5):
    mp = pytest.MonkeyPatch()
    T.Recorder(mp)                                   # the shape queries' fixed answers
    count = [0]
    for name in T.LAUNCHERS:
        mp.setattr(ops, name, lambda *a, **k: count.__setitem__(0, count[0] + 1))
    for name, case in ROWS.items():
        step = step_fn(case)
        count[0] = 0
        step(0)
        launches, times = count[0], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for s in range(iters):
                step(s)
            times.append((time.perf_counter() - t0) / iters * 1e6)
        print(f"{name:52s} {launches:3d} launches  {statistics.median(times):7.1f} us", flush=True)
    mp.undo()


if __name__ == "__main__":
    main()

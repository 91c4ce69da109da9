"""The shared run / piece decode of the sparse optimizers (csrc/sparse_runs.h): ONE hand-built id list, whose sorted slot positions
are known because it is built from run lengths, through every entry point that decodes runs with the shared helpers -
sparse_sgd_, sparse_adagrad_, optimizer_step_ (SGD and Adagrad, with one small dense segment: the body without rows requested
ahead), adam_step_ and rowwise_adagrad_step_ - each against its existing NumPy restatement BIT FOR BIT, and each twice on the same
plan and workspace (the second call shows that the arrival tickets of the one-launch kernels were left at zero).

Out-of-range ids become the plan's sentinel and sort behind every valid id, so a list that holds them cannot also END in a valid
run.  The list therefore comes in two forms built from the same runs: "padded" (the valid runs + 128 out-of-range ids: the
skipped slots cross two block boundaries and end in a piece of one slot) and "valid" (the valid runs alone: the last run
continues into a last piece of one slot at the very end of the list).  Both hold n % 64 == 1 ids."""
import functools

import numpy as np
import pytest
import torch

import adam_check as ac
import rowwise_check as rc
from oracle import two_tower as tt
from two_tower_amazon_recommender_amd import ops

ROWS = 40
LR, EPS = 0.01, 1e-7
PIECE = tt.PIECE
# (id, run length) in sorted order; the comments give the run's sorted slots [start, end)
RUNS = [
    (0, 64),     # [0, 64)      exactly one block from slot 0: ends on a boundary, and the next run starts on one
    (1, 3),      # [64, 67)     a short run that starts exactly on a boundary
    (2, 61),     # [67, 128)    starts mid-block, ends exactly on a boundary, no continuation
    (3, 2),      # [128, 130)   2, 5, 6 (and the 3 above) inside a block: the walk's tail alone, its unrolled part alone, + tail
    (4, 5),      # [130, 135)
    (5, 6),      # [135, 141)
    (6, 1),      # [141, 142)   singletons
    (7, 1),      # [142, 143)
    (8, 70),     # [143, 213)   crosses one boundary (192)
    (9, 3),      # [213, 216)
    (10, 250),   # [216, 466)   5 blocks: the head piece + 4 boundary pieces (the four-in-flight add without a tail)
    (11, 1),     # [466, 467)
    (12, 320),   # [467, 787)   6 blocks: the head piece + 5 boundary pieces (... with its tail)
    (13, 2),     # [787, 789)
] + [(14 + i, n) for i, n in enumerate([1, 2, 3, 5, 6, 9, 1, 4] * 3)] + [   # [789, 882)  ids 14..37
    (38, 463),   # [882, 1345)  the last valid run: ends in a piece of ONE slot (slot 1344 = 21 * 64); id 39 is never touched
]
N_PAD = 128      # out-of-range ids of the padded form


@functools.lru_cache(maxsize=None)
def id_list(form):
    """The batch's ids (int64, in a fixed shuffled order).  Asserts, from np.sort and the run starts, that every corner the
    decode has is really in the list - a later edit of RUNS cannot drop one unnoticed."""
    rng = np.random.default_rng(7)
    ids = np.concatenate([np.full(n, i, dtype=np.int64) for i, n in RUNS])
    if form == "padded":
        bad = np.where(np.arange(N_PAD) % 2 == 0, ROWS, -1 - np.arange(N_PAD) % 5).astype(np.int64)   # id == rows, negative padding
        ids = np.concatenate([ids, bad])
    ids = ids[rng.permutation(len(ids))]
    n = len(ids)
    ok = (ids >= 0) & (ids < ROWS)
    sid = np.sort(ids[ok])                                   # the valid part of the plan's sorted list (the sentinel sorts last)
    start = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    end = np.r_[start[1:], len(sid)]
    length, blocks = end - start, (end - 1) // PIECE - start // PIECE + 1
    assert 1300 <= n <= 1700 and n % PIECE == 1, n                                        # about 1,500 ids: 1,473 padded, 1,345 valid
    assert start[0] == 0 and length[0] == PIECE and start[1] == PIECE                    # one whole block at slot 0, then a head on a boundary
    assert ((start % PIECE == 0) & (length <= 4)).any()                                   # a short run starting on a boundary
    assert ((start % PIECE != 0) & (end % PIECE == 0) & (blocks == 1)).any()              # mid-block to a boundary, no continuation
    assert ((start % PIECE != 0) & (blocks == 2)).any()                                   # crosses one boundary
    assert ((start % PIECE != 0) & (blocks == 5)).any() and ((start % PIECE != 0) & (blocks == 6)).any()
    for want in (1, 2, 3, 5, 6):
        assert ((length == want) & (blocks == 1) & (start % PIECE != 0)).any(), want      # inside a block
    assert length[-1] > 1 and end[-1] % PIECE == 1                                        # the last valid run ends in a piece of one slot
    assert len(np.setdiff1d(np.arange(ROWS), sid))                                        # a row that no id touches
    if form == "padded":
        assert (~ok).sum() >= 70 and (ids == ROWS).any() and (ids < 0).any()
        assert len(sid) // PIECE < (n - 1) // PIECE                                       # the skipped slots cross a boundary
    else:
        assert ok.all() and end[-1] == n                                                  # ... at the very end of the list
    return ids


@functools.lru_cache(maxsize=None)
def problem(form, dim):
    """(ids, grads [n, dim], w [ROWS, dim], second state array [ROWS, dim], third [ROWS, dim], row accumulators [ROWS])."""
    ids = id_list(form)
    rng = np.random.default_rng(1000 + dim)
    grads = (rng.standard_normal((len(ids), dim)) * 0.01).astype(np.float32)
    w = rng.uniform(-0.05, 0.05, (ROWS, dim)).astype(np.float32)
    s1 = rng.uniform(0.1, 0.3, (ROWS, dim)).astype(np.float32)
    s2 = rng.uniform(1e-5, 1e-3, (ROWS, dim)).astype(np.float32)
    return ids, grads, w, s1, s2, s1[:, 0].copy()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _valid(ids, grads):
    ok = (ids >= 0) & (ids < ROWS)
    return ids[ok], grads[ok]


DENSE = 200      # elements of optimizer_step_'s dense segment (two gradient slabs)


def _dense(dim):
    rng = np.random.default_rng(5000 + dim)
    return (rng.uniform(-0.1, 0.1, DENSE).astype(np.float32), rng.uniform(0.1, 0.3, DENSE).astype(np.float32),
            (rng.standard_normal((2, DENSE)) * 0.01).astype(np.float32))


@functools.lru_cache(maxsize=None)
def expected(entry, form, dim):
    """The restatement's result for ``entry``: a tuple of arrays in the order of ``initial``.  Computed once, never written."""
    ids, grads, w, s1, s2, ra = problem(form, dim)
    vi, vg = _valid(ids, grads)
    w = w.copy()
    if entry in ("sgd", "step_sgd"):
        out = (tt.sparse_sgd(w, vi, vg, LR),)
    elif entry in ("adagrad", "step_adagrad"):
        acc = s1.copy()
        tt.sparse_adagrad(w, acc, vi, vg, LR, EPS)
        out = (w, acc)
    elif entry == "adam":
        m, v = s2.copy(), s2.copy() * 0.5
        ac.sparse_adam(w, m, v, ids, grads, LR, 3)
        out = (w, m, v)
    else:
        a = ra.copy()
        rc.sparse_rowwise_adagrad(w, a, ids, grads, LR, EPS)
        out = (w, a)
    if entry.startswith("step_"):
        dw, dacc, slabs = _dense(dim)
        dw, dacc = dw.copy(), dacc.copy()
        if entry == "step_sgd":
            dw = dw - np.float32(LR) * (slabs[0] + slabs[1])
        else:
            rc.dense_adagrad(dw, dacc, slabs, 0.0, LR, EPS)
        out = out + (dw,)
    for a in out:
        a.setflags(write=False)
    return out


def initial(entry, form, dim):
    ids, grads, w, s1, s2, ra = problem(form, dim)
    state = {"sgd": (w,), "step_sgd": (w,), "adagrad": (w, s1), "step_adagrad": (w, s1), "adam": (w, s2, s2 * 0.5),
             "rowwise": (w, ra)}[entry]
    return state + ((_dense(dim)[0],) if entry.startswith("step_") else ())


def test_the_id_list_holds_every_corner_of_the_decode():
    for form in ("padded", "valid"):
        id_list(form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["padded", "valid"])
@pytest.mark.parametrize("dim", [4, 12, 128, 200, 260])
@pytest.mark.parametrize("entry", ["sgd", "adagrad", "step_sgd", "step_adagrad", "adam", "rowwise"])
def test_every_entry_point_decodes_the_list_alike_bit_for_bit_and_twice(dev, entry, dim, form):
    """dim 4: one lane per row; 12: three chunks on four lanes (the clamped lane); 128; 200: two chunks per lane in row-wise;
    260: 65 chunks - the chunk loop of SGD / Adagrad / Adam runs more than once with a partial last pass, row-wise takes its
    four-chunk instantiation with idle chunks (one piece sum in flight)."""
    ids, grads = problem(form, dim)[:2]
    want = expected(entry, form, dim)
    init = initial(entry, form, dim)
    d = [T(a, dev) for a in init]
    g = T(grads, dev)
    plan = ops.SparsePlan(len(ids), dev).run(T(ids, dev), ROWS)
    dacc, slabs = (T(a, dev) for a in _dense(dim)[1:])
    for call in (1, 2):                                      # the same plan, the same workspaces
        for t, a in zip(d, init):
            t.copy_(T(a, dev))
        if entry == "sgd":
            ops.sparse_sgd_(d[0], g, plan, LR)
        elif entry == "adagrad":
            ops.sparse_adagrad_(d[0], d[1], g, plan, LR, EPS)
        elif entry == "step_sgd":
            ops.optimizer_step_("sgd", [(d[0], None, g, plan)], [ops.make_dense_seg(d[1], None, slabs, 2, 0.0)], LR, EPS)
        elif entry == "step_adagrad":
            dacc.copy_(T(_dense(dim)[1], dev))
            ops.optimizer_step_("adagrad", [(d[0], d[1], g, plan)], [ops.make_dense_seg(d[2], dacc, slabs, 2, 0.0)], LR, EPS)
        elif entry == "adam":
            ops.adam_step_([(d[0], d[1], d[2], g, plan)], [], ops.AdamHyper(lr=LR, step=3))
        else:
            ops.rowwise_adagrad_step_([(d[0], d[1], g, plan)], [], LR, EPS)
        for i, (t, w) in enumerate(zip(d, want)):
            bad = rc.bits(t.cpu().numpy()) != rc.bits(w)
            assert not bad.any(), (entry, form, dim, f"call {call}", f"array {i}", int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (rc.bits(want[0]) != rc.bits(init[0])).any() and (rc.bits(want[0][39]) == rc.bits(init[0][39])).all()

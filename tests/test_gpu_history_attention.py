"""Attention pooling of the user history on the GPU (tt_history_attention_fwd_f32 / tt_history_attention_bwd_f32,
csrc/history_attn.hip): the forward launch against the f64 restatement of tests/attention_check.py within the project's bars
(relative <= 1e-4, max-abs <= 1e-4 * max|ref|: DESIGN section 2 - the device takes the exponential in hardware, so only the
listed properties are bit for bit), the flags, the backward launch, the history table's update, then the trainer - parity with
the f64 autograd restatement, training, checkpoints, the inference paths - the custom ops, the CLIs and the refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import attention_check as atc
import bag_check as bc
import history_check as hc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001
BAR = 1e-4


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _bad(got, want):
    b = bc.bits(got) != bc.bits(want)
    return int(b.sum()), np.argwhere(b)[:4].tolist()


_errs = atc.errs                                  # (max-abs error / max|ref|, relative error in the 2-norm) against an f64 reference
_problem = atc.problem                            # the special bags


def _within(got, want, what, worst=None, zero_scale=None):
    """Asserts the bars; ``worst`` collects the largest error per result name (the last entry of ``what``).  ``zero_scale``: the
    size of the terms of a reference that may be zero in every entry (``attention_check.uncancelled_scales``)."""
    e = _errs(got, want, zero_scale)
    if worst is not None:
        worst[what[-1]] = max(worst.get(what[-1], 0.0), *e)
    assert e[0] <= BAR and e[1] <= BAR, (what, e)
    return e


def _device_forward(dev, table_t, tok, bag_rows, exclude, base_t, attn_t):
    n_bags = len(tok) if bag_rows is None else len(bag_rows)
    L, dim = tok.shape[1], table_t.shape[1]
    out = torch.full((n_bags, dim), 7.0, device=dev)
    ids = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
    w = torch.full((n_bags, L), -7.0, device=dev)
    pooled = torch.full((n_bags, dim), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), T(exclude, dev), base_t, out=out, batch_ids=ids,
                          weights=w, pooled=pooled, oob_flag=flag)
    return N(out), N(w), N(pooled), N(ids), int(flag.item())


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("dim", [4, 36, 128, 256, 516, 1024])
def test_forward_matches_the_restatement_and_keeps_its_bitwise_properties(dev, dim):
    """dim (every lane-group width, a partly filled group, NV 1..4) x {37, 300} bags x L {1, 7, 37, 64} x {no base, base} x
    identity / indirect bag rows (50 token rows), always with ``exclude``; rows, a and p ~ N(0, 1)."""
    rng = np.random.default_rng(dim)
    rows, n_rows = 97, 50
    table = rng.standard_normal((rows, dim)).astype(np.float32)
    base_table = rng.standard_normal((40, dim)).astype(np.float32)
    base_table[2] = -0.0
    table_t, base_table_t = T(table, dev), T(base_table, dev)
    worst = {}
    for L in (1, 7, 37, 64):
        attn = rng.standard_normal(dim + L).astype(np.float32)
        attn_t = T(attn, dev)
        for n_bags in (37, 300):
            for indirect in (False, True):
                tok, bag_rows, exclude = _problem(rng, n_rows if indirect else n_bags, n_bags, L, rows, indirect)
                base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
                base_ids[1] = 2                                      # the emptied bag's base row is the -0.0 row: written as it is
                base_ids_t = T(base_ids, dev)
                for with_base in (False, True):
                    what = (dim, L, n_bags, indirect, with_base)
                    base = (base_table, base_ids) if with_base else None
                    base_t = (base_table_t, base_ids_t) if with_base else None
                    want = atc.attention_forward(table, tok, attn, bag_rows, exclude, base)
                    got = _device_forward(dev, table_t, tok, bag_rows, exclude, base_t, attn_t)
                    # the ids and the flag: the bag launch's, as integers
                    ids2 = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
                    flag2 = torch.zeros(1, dtype=torch.int32, device=dev)
                    ops.history_bag(table_t, T(tok, dev), T(bag_rows, dev), T(exclude, dev), base_t, "mean", batch_ids=ids2, oob_flag=flag2)
                    assert np.array_equal(got[3], N(ids2)) and np.array_equal(got[3], want[3]), what
                    assert got[4] == int(flag2.item()) == want[4] == 0, what
                    for k, name in enumerate(("out", "weights", "pooled")):
                        _within(got[k], want[k], what + (name,), worst)
                    w, ids = got[1], got[3].reshape(n_bags, L)
                    valid = ids >= 0
                    cnt = valid.sum(1)
                    assert (w[~valid] == 0).all() and not np.signbit(w[~valid]).any(), what       # skipped slots: exactly +0
                    # emptied bags: the base row's bits, or +0; their pooled row is +0
                    base_rows = base_table[base_ids] if with_base else np.zeros((n_bags, dim), np.float32)
                    assert cnt[1] == 0 and (cnt == 0).sum() >= 1, what
                    assert not _bad(got[0][cnt == 0], base_rows[cnt == 0])[0], what
                    assert not _bad(got[2][cnt == 0], np.zeros_like(got[2][cnt == 0]))[0], what
                    # one valid slot: weight exactly 1, pooled = that row, out = base + that row (one add)
                    one = np.flatnonzero(cnt == 1)
                    assert L > 1 or len(one) > 0, what
                    for b in one:
                        j = int(np.argmax(valid[b]))
                        row = table[ids[b, j]]
                        assert w[b, j] == 1.0 and not _bad(got[2][b], row)[0], (what, b)
                        assert not _bad(got[0][b], (base_rows[b] + row) if with_base else row)[0], (what, b)
                    # a second run gives the same bits
                    again = _device_forward(dev, table_t, tok, bag_rows, exclude, base_t, attn_t)
                    assert all(not _bad(a, g)[0] for a, g in zip(again[:3], got[:3])), what
                    if n_bags == 300:                                # the first 37 bags, launched alone: the same bits
                        head = _device_forward(dev, table_t, tok if indirect else tok[:37], None if bag_rows is None else bag_rows[:37],
                                               exclude[:37], (base_table_t, T(base_ids[:37], dev)) if with_base else None, attn_t)
                        assert all(not _bad(h, g[:37])[0] for h, g in zip(head[:3], got[:3])), what
                        assert np.array_equal(head[3], got[3][:37 * L]), what
    print(f"dim {dim}: worst errors {({k: f'{v:.2e}' for k, v in worst.items()})}")


def _extreme_problem(dim):
    """(table [8, dim], attn, tokens [3, 5], base_table, base_ids, the generator): rows 0 and 1 are u and -u, a is u scaled so
    that their logits are +200 and -200, the other rows' are small."""
    rng = np.random.default_rng(1000 + dim)
    table = (0.1 * rng.standard_normal((8, dim))).astype(np.float32)
    u = rng.standard_normal(dim).astype(np.float32)
    table[0], table[1] = u, -u
    L = 5
    attn = np.concatenate([u * np.float32(200.0 * np.sqrt(dim) / float((u.astype(np.float64) ** 2).sum())),
                           rng.standard_normal(L).astype(np.float32)]).astype(np.float32)
    tok = np.array([[1, 2, 0, 3, 1], [0, 1, 4, 5, 6], [2, -1, 1, 0, -1]], dtype=np.int32)
    base_table = rng.standard_normal((3, dim)).astype(np.float32)
    base_ids = np.arange(3, dtype=np.int64)
    return table, attn, tok, base_table, base_ids, rng


@pytest.mark.parametrize("dim", [4, 36, 128, 516])
def test_forward_extreme_logits_and_zero_attention(dev, dim):
    """A bag whose logits reach -200 and +200 (a scaled query; the running max moves up AND stays: slots -200, small, +200,
    small, -200): finite, the one-hot pool of the restatement.  With attn = 0 the weights are 1 / cnt and out is the mean bag's."""
    table, attn, tok, base_table, base_ids, _ = _extreme_problem(dim)
    want = atc.attention_forward(table, tok, attn, None, None, (base_table, base_ids))
    e = table[tok[0]].astype(np.float64) @ attn[:dim].astype(np.float64) / np.sqrt(dim)
    assert e.max() > 195 and e.min() < -195 and want[1].max(1).min() >= 1 - 1e-12          # the restatement is one-hot
    got = _device_forward(dev, T(table, dev), tok, None, None, (T(base_table, dev), T(base_ids, dev)), T(attn, dev))
    for k, name in enumerate(("out", "weights", "pooled")):
        print(dim, name, _within(got[k], want[k], (dim, "extreme", name)))
    assert got[1][0, 2] == 1.0 and got[1][1, 0] == 1.0 and got[1][2, 3] == 1.0
    # attn = 0: mean pooling
    rng = np.random.default_rng(2000 + dim)
    rows, n_rows, n_bags, L = 97, 50, 300, 7
    table = rng.standard_normal((rows, dim)).astype(np.float32)
    base_table = rng.standard_normal((40, dim)).astype(np.float32)
    tok, bag_rows, exclude = _problem(rng, n_rows, n_bags, L, rows, True)
    base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
    base_t = (T(base_table, dev), T(base_ids, dev))
    got = _device_forward(dev, T(table, dev), tok, bag_rows, exclude, base_t, torch.zeros(dim + L, device=dev))
    inv = torch.empty(n_bags, device=dev)
    mean = ops.history_bag(T(table, dev), T(tok, dev), T(bag_rows, dev), T(exclude, dev), base_t, "mean", inv=inv)
    valid = got[3].reshape(n_bags, L) >= 0
    assert np.array_equal(got[1], np.where(valid, N(inv)[:, None], np.float32(0)))          # exp(0) = 1: the weights are 1 / cnt
    print(dim, "mean", _within(got[0], N(mean).astype(np.float64), (dim, "attn = 0", "out")))


# ------------------------------------------------------------------------------------------ 2. flags
def test_flags_and_argument_checks(dev):
    rng = np.random.default_rng(9)
    rows, dim, L, n_rows, n_bags = 60, 128, 7, 50, 37
    table = rng.standard_normal((rows, dim)).astype(np.float32)
    base_table = rng.standard_normal((40, dim)).astype(np.float32)
    attn = rng.standard_normal(dim + L).astype(np.float32)
    table_t, base_table_t, attn_t = T(table, dev), T(base_table, dev), T(attn, dev)
    tok, bag_rows, exclude = _problem(rng, n_rows, n_bags, L, rows, True)
    base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
    for kind in ("token_high", "token_low", "row_high", "row_low", "base_high", "base_low", "base_minus_one", "clean"):
        tk, br, bi = tok.copy(), bag_rows.copy(), base_ids.copy()
        if kind == "token_high":
            tk[6, 2] = rows
        elif kind == "token_low":
            tk[6, 0] = -2
        elif kind == "row_high":
            br[9] = n_rows
        elif kind == "row_low":
            br[9] = -3
        elif kind == "base_high":
            bi[4] = 40
        elif kind == "base_low":
            bi[4] = -2
        elif kind == "base_minus_one":
            bi[4] = -1
        want = atc.attention_forward(table, tk, attn, br, exclude, (base_table, bi))
        got = _device_forward(dev, table_t, tk, br, exclude, (base_table_t, T(bi, dev)), attn_t)
        assert got[4] == want[4] == (0 if kind in ("clean", "base_minus_one") else 1), kind
        assert np.array_equal(got[3], want[3]), kind
        for k, name in enumerate(("out", "weights", "pooled")):
            _within(got[k], want[k], (kind, name))
        if kind.startswith("base_"):            # a zero base row: the row is 0 + the pooled term
            assert not _bad(got[0][4], np.float32(0) + got[2][4])[0], kind
        if kind.startswith("row_"):             # an empty bag: the base row itself
            assert not _bad(got[0][9], base_table[bi[9]])[0] and (got[1][9] == 0).all(), kind
    # no optional output, fresh results
    out, w, pooled = ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), T(exclude, dev), (base_table_t, T(base_ids, dev)))
    want = atc.attention_forward(table, tok, attn, bag_rows, exclude, (base_table, base_ids))
    _within(N(out), want[0], "fresh out"); _within(N(w), want[1], "fresh weights"); _within(N(pooled), want[2], "fresh pooled")
    with pytest.raises(RuntimeError, match="attn"):
        ops.history_attention(table_t, T(tok, dev), attn_t[:-1], T(bag_rows, dev))
    with pytest.raises(RuntimeError, match="exclude"):
        ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), T(exclude[:-1], dev))
    with pytest.raises(RuntimeError, match="base"):
        ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), base=(base_table_t, T(base_ids[:-1], dev)))
    with pytest.raises(RuntimeError, match="weights"):
        ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), weights=torch.empty(n_bags, L + 1, device=dev))
    with pytest.raises(ValueError, match="pooling"):
        ops.history_bag(table_t, T(tok, dev), pooling="attention")
    with pytest.raises(ValueError, match="pooling"):
        ops.embedding_bag(table_t, T(tok, dev), pooling="attention")


# ------------------------------------------------------------------------------------------ 3. backward
def _update_problem(n_bags, dim, seed=77):
    """The update problem of tests/test_gpu_history.py: L 16, 60 rows (rows 50..59 stand in no bag).  Item 49 stands only in
    bags that exclude it: its row gets no gradient.  Item 7 fills a fixed slot of bags 100..299 (when there are that many)."""
    rng = np.random.default_rng(seed)
    L, rows = 16, 60
    tok = rng.integers(0, 50, (n_bags, L)).astype(np.int32)
    tok[rng.random((n_bags, L)) < 0.3] = -1
    tok[100:300, 4] = 7
    own = tok[np.arange(n_bags), rng.integers(0, L, n_bags)].astype(np.int64)
    exclude = np.where(rng.random(n_bags) < 0.5, own, rng.integers(0, 50, n_bags))
    exclude[(tok == 49).any(1)] = 49
    table = rng.uniform(-0.05, 0.05, (rows, dim)).astype(np.float32)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    attn = np.concatenate([20.0 * rng.standard_normal(dim), rng.standard_normal(L)]).astype(np.float32)
    return table, tok, exclude.astype(np.int64), dy, attn


@pytest.fixture(scope="module")
def update_problem():
    return _update_problem(512, 128)


NAN_BITS = 0x7FC00000


def _device_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs):
    n_bags, dim = dy_t.shape
    sg = torch.full((n_bags * L, dim), float("nan"), device=dev)
    slabs = torch.full((n_slabs, dim + L), float("nan"), device=dev)
    ops.history_attention_bwd(table_t, ids, w, pooled, dy_t, attn_t, L, slot_grads=sg, dattn_slabs=slabs)
    return sg, slabs


@pytest.mark.parametrize("n_bags,dim", [(512, 128), (64, 36), (64, 516)])
def test_backward_matches_the_closed_form(dev, n_bags, dim):
    table, tok, exclude, dy, attn = _update_problem(n_bags, dim)
    L = tok.shape[1]
    table_t, dy_t, attn_t = T(table, dev), T(dy, dev), T(attn, dev)
    ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
    _, w, pooled = ops.history_attention(table_t, T(tok, dev), attn_t, exclude=T(exclude, dev), batch_ids=ids)
    f = atc.attention_forward(table, tok, attn, None, exclude, None)
    assert np.array_equal(N(ids), f[3])
    want_sg, want_da, want_dp, _ = atc.attention_backward(table, f[3], f[1], f[2], dy, attn, L)
    valid = f[3] >= 0
    assert (~valid).sum() > L and valid.sum() > n_bags
    sums = {}
    for n_slabs in (1, 3, ops.history_attention_num_slabs(n_bags)):
        sg, slabs = _device_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
        sg2, slabs2 = _device_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
        assert torch.equal(sg.view(torch.int32), sg2.view(torch.int32)) and torch.equal(slabs, slabs2), n_slabs   # bit-reproducible
        g = N(sg)
        assert (bc.bits(g[~valid]) == NAN_BITS).all(), n_slabs                       # skipped slots' rows are untouched
        e_sg = _within(g[valid], want_sg[valid], (n_bags, dim, n_slabs, "slot_grads"))
        total = N(slabs).astype(np.float64).sum(0)
        e_da = _within(total[:dim], want_da, (n_bags, dim, n_slabs, "da"))
        e_dp = _within(total[dim:], want_dp, (n_bags, dim, n_slabs, "dp"))
        zero = abs(total[dim:].sum()) / np.abs(want_dp).max()
        print(f"bags {n_bags} dim {dim} slabs {n_slabs}: slot_grads {e_sg[0]:.2e} da {e_da[0]:.2e} dp {e_dp[0]:.2e} sum(dp) {zero:.2e} of max|dp|")
        assert zero <= BAR, (n_slabs, zero)
        sums[n_slabs] = total
    assert ops.history_attention_num_slabs(n_bags) == n_bags // 8


def _forward_tensors(dev, table_t, tok, bag_rows, exclude, base_t, attn_t):
    """The device forward into pre-filled buffers, kept on the device: (batch_ids, weights, pooled)."""
    n_bags = len(tok) if bag_rows is None else len(bag_rows)
    L, dim = tok.shape[1], table_t.shape[1]
    ids = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
    w = torch.full((n_bags, L), -7.0, device=dev)
    pooled = torch.full((n_bags, dim), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.history_attention(table_t, T(tok, dev), attn_t, T(bag_rows, dev), T(exclude, dev), base_t, batch_ids=ids, weights=w,
                          pooled=pooled, oob_flag=flag)
    assert flag.item() == 0
    return ids, w, pooled


def _guarded_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs):
    """The backward launch into NaN-filled buffers with one row more than the launch is given: (slot_grads [n_bags * L + 1, dim],
    slabs [n_slabs + 1, dim + L]) - the last row of each is the guard behind what the launch may write."""
    n_bags, dim = dy_t.shape
    sg = torch.full((n_bags * L + 1, dim), float("nan"), device=dev)
    slabs = torch.full((n_slabs + 1, dim + L), float("nan"), device=dev)
    ops.history_attention_bwd(table_t, ids, w, pooled, dy_t, attn_t, L, slot_grads=sg[:-1], dattn_slabs=slabs[:-1])
    return sg, slabs


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _is_nan_fill(t):
    return bool((t.view(torch.int32) == NAN_BITS).all().item())


def _zero_floor(ref, zero_scale):
    """max|ref|, or - where the reference is zero but for its own rounding - the size of its terms."""
    m = np.abs(ref).max()
    return zero_scale if m <= 1e-9 * zero_scale else m


def _backward_sweep(dev, dim, shapes):
    """Every check of the backward sweep for one dim over ``shapes`` = ((L, n_bags), ...); returns the worst error per result."""
    rng = np.random.default_rng(dim)
    base_table_t = T(rng.standard_normal((40, dim)).astype(np.float32), dev)
    worst = {}
    for L, n_bags in shapes:
        what = (dim, L, n_bags)
        p = atc.backward_problem(dim, L, n_bags)
        table_t, dy_t, attn_t = T(p["table"], dev), T(p["dy"], dev), T(p["attn"], dev)
        base_t = (base_table_t, T(rng.integers(0, 40, n_bags).astype(np.int64), dev))
        ids, w, pooled = _forward_tensors(dev, table_t, p["tokens"], p["bag_rows"], p["exclude"], base_t, attn_t)
        f = atc.attention_forward(p["table"], p["tokens"], p["attn"], p["bag_rows"], p["exclude"], None)
        assert np.array_equal(N(ids), f[3]), what
        ref = (p["table"], f[3], f[1], f[2], p["dy"], p["attn"], L)
        want_sg, want_da, want_dp, _ = atc.attention_backward(*ref)
        bag_da, bag_dp = atc.attention_dattn_per_bag(*ref)
        za, zp = atc.uncancelled_scales(*ref[:5], L)
        full_a, full_p = _zero_floor(want_da, za), _zero_floor(want_dp, zp)
        sum_a = np.concatenate([np.zeros((1, dim)), np.cumsum(bag_da, 0)])
        sum_p = np.concatenate([np.zeros((1, L)), np.cumsum(bag_dp, 0)])
        valid = f[3] >= 0
        assert valid.any() and (L < 3 or valid.reshape(n_bags, L).all(1).any()), what
        first = None
        for n_slabs in (1, 3, ops.history_attention_num_slabs(n_bags), n_bags + 2):
            sg, slabs = _guarded_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
            sg2, slabs2 = _guarded_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
            assert _same_bits(sg, sg2) and _same_bits(slabs, slabs2), (what, n_slabs)                   # a second launch: the same bits
            assert _is_nan_fill(sg[-1]) and _is_nan_fill(slabs[-1]), (what, n_slabs)                    # the guards
            if first is None:
                first = sg
                g = N(sg[:-1])
                assert (bc.bits(g[~valid]) == NAN_BITS).all(), what                                     # skipped slots' rows are untouched
                _within(g[valid], want_sg[valid], what + ("slot_grads",), worst)
            else:
                assert _same_bits(sg, first), (what, n_slabs)                                           # the slot rows do not depend on n_slabs
            sl = N(slabs[:-1])
            assert np.isfinite(sl).all(), (what, n_slabs)
            total = sl.astype(np.float64).sum(0)
            _within(total[:dim], want_da, what + (n_slabs, "da"), worst, za)
            _within(total[dim:], want_dp, what + (n_slabs, "dp"), worst, zp)
            zero = abs(total[dim:].sum()) / full_p
            worst["sum(dp)"] = max(worst.get("sum(dp)", 0.0), zero)
            assert zero <= BAR, (what, n_slabs, zero)
            # slab s holds the sums over ITS bags; a slab without bags is +0 in every entry
            per = -(-n_bags // n_slabs)
            lo = np.minimum(np.arange(n_slabs) * per, n_bags)
            hi = np.minimum(lo + per, n_bags)
            empty = lo == hi
            assert empty.any() == (n_slabs > n_bags) and (n_slabs != n_bags + 2 or empty.sum() >= 2), (what, n_slabs)
            assert not bc.bits(sl[empty]).any(), (what, n_slabs)
            for part, cum, full, name in ((sl[:, :dim], sum_a, full_a, "slab da"), (sl[:, dim:], sum_p, full_p, "slab dp")):
                want = cum[hi] - cum[lo]
                bound = BAR * np.maximum(np.abs(want).max(1), full)
                err = np.abs(part - want).max(1)
                worst[name] = max(worst.get(name, 0.0), float((err / np.maximum(np.abs(want).max(1), full)).max()))
                assert (err <= bound).all(), (what, n_slabs, name, int(np.argmax(err / bound)), float((err / bound).max()))
        if n_bags == 300:          # a bag's gradient rows depend on that bag only: the first 37 bags, launched alone
            sg37, _ = _guarded_backward(dev, table_t, ids[:37 * L], w[:37], pooled[:37], dy_t[:37], attn_t, L, 5)
            assert _same_bits(sg37[:-1], first[:37 * L]) and _is_nan_fill(sg37[-1]), what
    return worst


@pytest.mark.parametrize("dim", atc.SWEEP_DIMS)
def test_backward_sweep_matches_the_closed_form_slab_by_slab_and_touches_nothing_else(dev, dim):
    """The forward's sweep for the backward: dim (every lane-group width 1 .. 64, a partly filled group, NV 1 .. 4, KF 4 and 2)
    x L {1, 7, 37, 64} (up to 64 chunks of the slot loop at dim 4, 3 and 4 at dim 36, 2 at dim 128; the halved workgroup at
    dim 4, L 64 and the last full one at L 37) x {1, 37, 300} bags x n_slabs {1, 3, the default, n_bags + 2}, on the problems of
    ``attention_check.backward_problem`` (tests/test_history_attention_cpu.py: the closed form in float32 meets a tenth of the
    bar on every one of them).  The device forward - exclude, indirect bag rows, a base row - feeds the device backward.

    Where da and dp are zero in every entry (L = 1: one slot per bag) they are held to the bar of the size of their terms."""
    worst = _backward_sweep(dev, dim, [(L, n_bags) for L in atc.SWEEP_LS for n_bags in atc.SWEEP_BAGS])
    print(f"dim {dim}: worst errors {({k: f'{v:.2e}' for k, v in worst.items()})}")


@pytest.mark.parametrize("dim,L,n_bags", atc.NV2_SHAPES)
def test_backward_with_two_float4_per_lane(dev, dim, L, n_bags):
    """The sweep's dims leave out NV = 2 (dim 260 .. 512): one float4 of the second round at dim 260, both rounds full at 512."""
    assert atc.backward_launch_shape(dim, L) == (64, 2, 4, 256, 1)
    worst = _backward_sweep(dev, dim, [(L, n_bags)])
    print(f"dim {dim}: worst errors {({k: f'{v:.2e}' for k, v in worst.items()})}")


@pytest.mark.parametrize("dim", [4, 36, 128, 516])
def test_backward_extreme_logits_zero_attention_and_skipped_ids(dev, dim):
    """One-hot weights (the forward's extreme-logit bags: logits of -200 and +200), attn = 0 (the mean bag) and batch ids the
    launch promises to skip without reading their weights.

    With one-hot weights pooled IS the one kept row, so t = G and da, dp are zero in every entry: they are held to the bar of
    the size of their terms (``attention_check.uncancelled_scales``)."""
    # 1. one-hot weights from the device forward
    table, attn, tok, base_table, base_ids, rng = _extreme_problem(dim)
    n_bags, L = tok.shape
    dy = rng.standard_normal((n_bags, dim)).astype(np.float32)
    table_t, attn_t, dy_t = T(table, dev), T(attn, dev), T(dy, dev)
    ids, w, pooled = _forward_tensors(dev, table_t, tok, None, None, (T(base_table, dev), T(base_ids, dev)), attn_t)
    wn, idn = N(w), N(ids).reshape(n_bags, L)
    valid = idn >= 0
    assert np.array_equal(np.argmax(wn, 1), [2, 0, 3]) and (wn.max(1) == 1.0).all() and (wn.sum(1) == 1.0).all()
    none = valid & (wn == 0)
    assert none.sum() == 4 + 4 + 2 and (~valid).sum() == 2
    ref = atc.attention_backward(table, idn, wn, N(pooled), dy, attn, L)                  # the closed form fed the SAME weights
    za, zp = atc.uncancelled_scales(table, idn, wn, N(pooled), dy, L)
    for n_slabs in (1, 3):
        sg, slabs = _guarded_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
        g, sl = N(sg[:-1]).reshape(n_bags, L, dim), N(slabs[:-1])
        assert np.isfinite(g[valid]).all() and np.isfinite(sl).all() and (bc.bits(g[~valid]) == NAN_BITS).all()
        assert _is_nan_fill(sg[-1]) and _is_nan_fill(slabs[-1])
        assert (g[none] == 0).all()                                                        # weight exactly 0: a row that compares equal to 0
        for b, j in enumerate(np.argmax(wn, 1)):
            print(dim, "one-hot row", b, _within(g[b, j], dy[b], (dim, "one-hot", n_slabs, b, "slot_grads")))
        total = sl.astype(np.float64).sum(0)
        print(dim, "one-hot da, dp", _within(total[:dim], ref[1], (dim, "one-hot", n_slabs, "da"), zero_scale=za),
              _within(total[dim:], ref[2], (dim, "one-hot", n_slabs, "dp"), zero_scale=zp))
    # 2. attn = 0: weights 1 / cnt, rows g / cnt
    L, n_bags = 7, 37
    p = atc.backward_problem(dim, L, n_bags, seed=1)
    table_t, dy_t, zero_t = T(p["table"], dev), T(p["dy"], dev), torch.zeros(dim + L, device=dev)
    ids, w, pooled = _forward_tensors(dev, table_t, p["tokens"], p["bag_rows"], p["exclude"], None, zero_t)
    f = atc.attention_forward(p["table"], p["tokens"], np.zeros(dim + L, np.float32), p["bag_rows"], p["exclude"], None)
    valid = f[3].reshape(n_bags, L) >= 0
    cnt = valid.sum(1)
    assert np.array_equal(N(ids), f[3]) and np.array_equal(N(w), np.where(valid, np.float32(1) / np.maximum(cnt, 1).astype(np.float32)[:, None], 0))
    ref = atc.attention_backward(p["table"], f[3], f[1], f[2], p["dy"], np.zeros(dim + L), L)
    sg, slabs = _guarded_backward(dev, table_t, ids, w, pooled, dy_t, zero_t, L, 5)
    g = N(sg[:-1]).reshape(n_bags, L, dim)
    rows = np.broadcast_to((p["dy"].astype(np.float64) / np.maximum(cnt, 1)[:, None])[:, None, :], g.shape)
    total = N(slabs[:-1]).astype(np.float64).sum(0)
    print(dim, "attn = 0", _within(g[valid], rows[valid], (dim, "attn = 0", "slot_grads")), _within(total[:dim], ref[1], (dim, "attn = 0", "da")),
          _within(total[dim:], ref[2], (dim, "attn = 0", "dp")))
    assert (bc.bits(g[~valid]) == NAN_BITS).all() and _is_nan_fill(sg[-1]) and _is_nan_fill(slabs[-1])
    # 3. ids >= table_rows and ids < -1: skipped like -1, their weights never read
    L, n_bags = 37, 37
    p = atc.backward_problem(dim, L, n_bags, seed=2)
    table_t, dy_t, attn_t = T(p["table"], dev), T(p["dy"], dev), T(p["attn"], dev)
    ids, w, pooled = _forward_tensors(dev, table_t, p["tokens"], p["bag_rows"], p["exclude"], None, attn_t)
    idn, wn = N(ids), N(w).reshape(-1)
    kept = np.flatnonzero(idn >= 0)
    assert (idn[8 * L:9 * L] >= 0).all()                                                   # bag 8 is full: a skipped id in each part of it
    at = np.unique(np.concatenate([kept[[0, 1, len(kept) // 2, -1]], 8 * L + np.array([0, 3, L // 2, L - 2, L - 1])]))
    bad_ids, bad_w, clean_ids, clean_w = idn.copy(), wn.copy(), idn.copy(), wn.copy()
    bad_ids[at] = np.resize([atc.ROWS, atc.ROWS + 7, -5], len(at))
    bad_w[at] = np.nan
    clean_ids[at], clean_w[at] = -1, 0.0
    n_slabs = ops.history_attention_num_slabs(n_bags)
    bad = _guarded_backward(dev, table_t, T(bad_ids, dev), T(bad_w.reshape(n_bags, L), dev), pooled, dy_t, attn_t, L, n_slabs)
    clean = _guarded_backward(dev, table_t, T(clean_ids, dev), T(clean_w.reshape(n_bags, L), dev), pooled, dy_t, attn_t, L, n_slabs)
    assert _same_bits(bad[0], clean[0]) and _same_bits(bad[1], clean[1])
    assert _is_nan_fill(bad[0][:-1][T(at, dev)]) and _is_nan_fill(bad[0][-1]) and torch.isfinite(bad[1][:-1]).all().item()
    untouched = _guarded_backward(dev, table_t, ids, w, pooled, dy_t, attn_t, L, n_slabs)
    assert not _same_bits(untouched[1], bad[1]) and torch.isfinite(untouched[0][:-1][T(at, dev)]).all().item()   # the slots DID count before


# ------------------------------------------------------------------------------------------ 4. the update
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_update_from_the_slot_rows_is_bit_exact(dev, update_problem, opt):
    table, tok, exclude, dy, attn = update_problem
    n_bags, L = tok.shape
    rng = np.random.default_rng(5)
    state = [table]
    if opt == "adagrad":
        state = [table, np.full_like(table, 0.1)]
    elif opt == "adam":
        state = [table, (rng.standard_normal(table.shape) * 0.01).astype(np.float32),
                 ((rng.standard_normal(table.shape) * 0.01) ** 2).astype(np.float32)]
    d = [T(a, dev) for a in state]
    attn_t = T(attn, dev)
    ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
    _, w, pooled = ops.history_attention(d[0], T(tok, dev), attn_t, exclude=T(exclude, dev), batch_ids=ids)
    sg, _ = _device_backward(dev, d[0], ids, w, pooled, T(dy, dev), attn_t, L, ops.history_attention_num_slabs(n_bags))
    plan = ops.SparsePlan(n_bags * L, dev)
    assert plan.grad_order is plan.order and plan.grad_rows == n_bags * L
    plan.run(ids, table.shape[0])
    if opt == "sgd":
        ops.sparse_sgd_(d[0], sg, plan, LR)
    elif opt == "adagrad":
        ops.sparse_adagrad_(d[0], d[1], sg, plan, LR)
    else:
        ops.adam_step_([(d[0], d[1], d[2], sg, plan)], [], ops.AdamHyper(lr=LR, step=7))
    want_ids = hc.history_forward(table, tok, None, exclude, None, "mean")[1]
    assert np.array_equal(N(ids), want_ids)
    assert (tok == 49).any() and not (want_ids == 49).any() and (want_ids == 48).any()
    want = [a.copy() for a in state]
    touched = bc.bag_update(opt, want, want_ids, N(sg), 1, LR, step=7)          # one gradient row per slot: "bags" of one slot
    for g, wnt, name in zip(d, want, ("table", "state 1", "state 2")):
        assert np.isfinite(N(g)).all(), (opt, name)
        assert not _bad(N(g), wnt)[0], (opt, name, _bad(N(g), wnt))
    rest = np.setdiff1d(np.arange(len(table)), touched)
    assert 49 in rest and len(rest) == 11
    for g, s0 in zip(d, state):
        assert not _bad(N(g)[rest], s0[rest])[0]                                # row 49 and rows 50..59 keep their bits
        assert (bc.bits(N(g)[touched]) != bc.bits(s0[touched])).any()


# ------------------------------------------------------------------------------------------ 5. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=2000, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **kw)


def _history_trainer(dev, opt="adagrad", seed=1001, pooling="attention", L=5, batches=2, **kw):
    """Histories from the pairs of the first synthetic batches (``data.user_histories``, file order): the steps' positives are
    in them."""
    tr = TwoTowerTrainer(_cfg(opt, user_history_len=L, history_pooling=pooling, **kw), dev, seed=seed)
    pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(batches)]
    u = torch.cat([p[0] for p in pairs]).cpu().numpy()
    i = torch.cat([p[1] for p in pairs]).cpu().numpy()
    tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, L), dev))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _set_attn(tr, seed):
    rng = np.random.default_rng(seed)
    d, L = tr.cfg.embedding_dim, tr.cfg.user_history_len
    tr.history_attn.copy_(T(np.concatenate([60.0 * rng.standard_normal(d), rng.standard_normal(L)]).astype(np.float32), tr.dev))


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


@pytest.mark.parametrize("L", [5, 20])
def test_trainer_matches_the_f64_restatement_and_trains(dev, L):
    """L = 5 (one chunk of the backward's slot loop at dim 32, where a lane group is 8 lanes) and L = 20 (three chunks: some users'
    histories fill more than 8 slots): loss and every gradient - the history table's (the scatter-add of the slot rows), da and dp included - within the
    bars of the f64 autograd restatement given the device's ReLU masks, with attn set to random values first (at zero the second
    term of the slot rows vanishes); then 20 Adam steps from the zero initialisation lower the loss and move attn off zero.  The
    item tower's last bias gradient is identically zero under the in-batch softmax and is held to 1e-4 of max|dc|, as in the
    history feature's test."""
    seed, batch = 1001, 256
    tr = _history_trainer(dev, "sgd", seed, L=L)
    assert not tr.fuse_lookup and tr.history_attn.storage_offset() % 4 == 0 and not tr.history_attn.any()
    assert len(tr._segs) == len(_history_trainer(dev, "sgd", seed, pooling="mean", L=L)._segs) + 1 == tr.cfg.dense_segment_count()
    _set_attn(tr, 5)
    hist = tr.user_history.cpu().numpy()
    assert hist.shape == (300, L) and atc.backward_launch_shape(32, L)[:2] == (8, 1)
    if L == 20:                                                                    # histories that reach into a second and a third chunk
        assert ((hist >= 0).sum(1) > 8).sum() >= 3 and ((hist >= 0).sum(1) > 16).any()
    d = tr.cfg.embedding_dim
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        un, inn = u.cpu().numpy(), i.cpu().numpy()
        valid = hist[un] >= 0
        match = valid & (hist[un] == inn[:, None])
        assert L == 5 or ((valid & ~match).sum(1) > 8).sum() >= 8                   # ... in this batch, after the leave-one-out
        assert match.any() and (valid.any(1) & (match.sum(1) == valid.sum(1))).any() and (valid & ~match).any()
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table", "history_table")}
        attn = tr.history_attn.cpu().numpy().astype(np.float64)
        towers = _towers64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
        r = atc.step_f64(before["user_table"], before["item_table"], before["history_table"], attn, towers, un, inn, hist, 0.1, masks)
        print(f"step {step}: loss {loss} (f64 {r['loss']})")
        assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
        # the leave-one-out rule reached the device's slots
        ids = tr.history_ids.cpu().numpy()
        assert np.array_equal(ids.reshape(batch, L), np.where(valid & ~match, hist[un], -1))
        w = tr.history_weights.cpu().numpy()
        assert w.max() > 0.9 and ((w > 0.05) & (w < 0.5)).any()                    # the attention is neither uniform nor one-hot everywhere
        sg = tr.history_slot_grads.cpu().numpy().astype(np.float64)
        g_hist = np.zeros_like(before["history_table"])
        np.add.at(g_hist, ids[ids >= 0], sg[ids >= 0])
        g_user = np.zeros_like(before["user_table"])
        np.add.at(g_user, un, tr.user_tower.demb.cpu().numpy().astype(np.float64))
        dattn = tr._ha_slabs.cpu().numpy().astype(np.float64).sum(0)
        checks = [("due", tr.user_tower.demb.cpu().numpy(), r["due"]), ("die", tr.item_tower.demb.cpu().numpy(), r["die"]),
                  ("history_table", g_hist, r["history_table"]), ("user_table", g_user, r["user_table"]),
                  ("da", dattn[:d], r["da"]), ("dp", dattn[d:], r["dp"])]
        for t, tw in enumerate((tr.user_tower, tr.item_tower)):
            for l in range(tw.n_layers):
                checks += [(f"dw[{t}][{l}]", tw.dw_slabs[l].cpu().numpy().astype(np.float64).sum(0), r["dw"][t][l]),
                           (f"db[{t}][{l}]", tw.db_slabs[l].cpu().numpy().astype(np.float64).sum(0), r["db"][t][l])]
        last = f"db[1][{tr.item_tower.n_layers - 1}]"
        for what, got, want in checks:
            err = np.abs(got - want).max()
            scale = np.abs(want).max()
            if what == last:
                assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
                scale = np.abs(r["dc"]).max()
            print(f"step {step}: {what} error {err / scale:.2e} of max |g|")
            assert scale > 0 and err <= 1e-4 * scale, (step, what, err)
        a0 = tr.history_attn.clone()
        tr.apply_gradients(step_ids=[u, i])
        assert not torch.equal(a0, tr.history_attn)                                # the dense segment trains the vector
    tr2 = _history_trainer(dev, "adam", seed, L=L)
    batch0 = tr2.synthetic_batch(seed, 0, "Z")
    t0 = tr2.history_table.clone()
    losses = [tr2.step(*batch0).item() for _ in range(20)]
    tr2.check_ids()
    print(f"20 steps: {losses[0]:.3f} -> {losses[-1]:.3f}; |attn| max {tr2.history_attn.abs().max().item():.3e}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(t0, tr2.history_table)
    assert tr2.history_attn[:d].any() and tr2.history_attn[d:].any() and torch.isfinite(tr2.history_attn).all()


def _names(tr):
    opt = tr.cfg.optimizer
    names = ["user_table", "item_table", "dense_flat", "history_table", "user_history", "title_table", "item_titles", "loss", "history_attn"]
    if opt == "adagrad":
        names += ["user_accum", "item_accum", "dense_accum", "history_accum", "title_accum"]
    if opt == "adam":
        names += ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "history_m", "history_v", "title_m", "title_v"]
    return names


# ------------------------------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17
    kw = dict(dropout_rate=0.1, n_title_buckets=300, title_max_tokens=5)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _history_trainer(dev, opt, seed, **kw)
    run(a, range(4))
    b = _history_trainer(dev, opt, seed, **kw)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["user_history_len"] == 5 and sd["config"]["history_pooling"] == "attention"
    mean = _history_trainer(dev, opt, seed, pooling="mean", **kw)
    assert set(sd) == set(mean.state_dict()) and sd["dense"].numel() == mean.dense_flat.numel() + 32 + 5
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values, no histories set
    c.load_state_dict(sd)
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    for k in _names(a):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert a.history_attn.any() and not torch.equal(a.history_attn, b.history_attn)
    with pytest.raises(ValueError, match="history_pooling"):
        mean.load_state_dict(sd)
    with pytest.raises(ValueError, match="history_pooling"):
        c.load_state_dict(mean.state_dict())


# ------------------------------------------------------------------------------------------ 7. inference
def test_inference_paths_attend_over_the_full_history(dev):
    """``evaluate``, ``user_embeddings`` (700 ids at batch 256: three chunks, the last ragged) and ``evaluate_topk`` feed the user
    tower user row + the attention pool of the FULL history - nothing left out - within the bars of the restatement, and not
    what the train step fed, where the positive was left out."""
    from two_tower_amazon_recommender_amd.metrics import FactorizedTopK
    seed = 23
    tr = _history_trainer(dev, "sgd", seed, batches=3)
    _set_attn(tr, 6)
    for s in range(3):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    u, i = tr.synthetic_batch(seed, 1, "Z")
    table, hist, users = N(tr.history_table), N(tr.user_history), N(tr.user_table)
    attn = N(tr.history_attn)
    un = N(u)
    assert (hist[un] == N(i)[:, None]).any()                                  # the positives are there - and stay in
    want = atc.attention_forward(table, hist, attn, un, None, (users, un))[0]
    train_in = atc.attention_forward(table, hist, attn, un, N(i), (users, un))[0]
    assert np.abs(want - train_in).max() > 1e-2 * np.abs(want).max()
    tr.evaluate(u, i)
    print("evaluate", _within(N(tr.user_tower.acts[0]), want, "evaluate"))
    q_eval = tr.user_tower.acts[-1].clone()
    tr.user_tower.acts[0].zero_()
    tr.evaluate_topk(u, i, FactorizedTopK(ks=(5,), temperature=0.1))
    print("evaluate_topk", _within(N(tr.user_tower.acts[0]), want, "evaluate_topk"))
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 300, 700)).to(dev)
    emb = tr.user_embeddings(ids)
    tr.check_ids()
    idn = N(ids)
    last = atc.attention_forward(table, hist, attn, idn[512:], None, (users, idn[512:]))[0]
    print("user_embeddings", _within(N(tr.user_tower.acts[0][:188]), last, "user_embeddings"))
    assert emb.shape == (700, 32)
    err = (tr.user_embeddings(u) - q_eval).abs().max().item()
    assert err <= 1e-4 * q_eval.abs().max().item(), err


# ------------------------------------------------------------------------------------------ 8. custom ops, CLIs
def test_custom_ops_pass_opcheck_equal_the_ops_calls_and_differentiate_attn(dev):
    """(dim 64, L 6) and (dim 32, L 20): a lane group of 8 walks 20 slots in 3 chunks.  The gradient of attn through the op is held
    to the closed form and to f64 autograd of ``attention_forward_torch`` on the op's own batch ids."""
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(3)
    for dim, L in ((64, 6), (32, 20)):
        assert atc.backward_launch_shape(dim, L)[4] == (1 if L == 6 else 3)
        table_np = rng.standard_normal((80, dim)).astype(np.float32)
        table = T(table_np, dev)
        base_np = rng.standard_normal((30, dim)).astype(np.float32)
        base_table = T(base_np, dev)
        tok, bag_rows, exclude = _problem(rng, 33, 50, L, 80, True)
        tok_t, rows, ex = T(tok, dev), T(bag_rows, dev), T(exclude, dev)
        base_ids_np = rng.integers(0, 30, 50).astype(np.int64)
        base_ids = T(base_ids_np, dev)
        attn_np = rng.standard_normal(dim + L).astype(np.float32)
        tok33 = tok_t[:33]
        for args in ((table, tok33, None, None, None, None), (table, tok_t, rows, ex, None, None), (table, tok_t, rows, ex, base_table, base_ids)):
            attn = T(attn_np, dev).requires_grad_(True)
            torch.library.opcheck(torch.ops.twotower.history_attention, args + (attn,))
            out, w, pooled, ids = torch.ops.twotower.history_attention(*args, attn)
            base = None if args[4] is None else (args[4], args[5])
            ids2 = torch.empty_like(ids)
            want = ops.history_attention(table, args[1], attn.detach(), args[2], args[3], base, batch_ids=ids2)
            assert torch.equal(out, want[0]) and torch.equal(w, want[1]) and torch.equal(pooled, want[2]) and torch.equal(ids, ids2)
            n_bags = out.shape[0]
            dy = T(rng.uniform(-1, 1, (n_bags, dim)).astype(np.float32), dev)
            out.backward(dy)
            sg, dattn = torch.ops.twotower.history_attention_bwd(table, ids, w.detach(), pooled.detach(), dy, attn.detach())
            assert torch.equal(attn.grad, dattn)
            ref = atc.attention_backward(table_np, N(ids), N(w), N(pooled), N(dy), attn_np, L)
            print("dattn", _within(N(attn.grad), np.concatenate([ref[1], ref[2]]), "autograd dattn"))
            print("slot rows", _within(N(sg), ref[0], "custom-op slot rows"))          # (the op zero-fills the skipped slots' rows)
            # f64 autograd through the forward restatement, from the op's ids
            kept = ids.cpu().view(n_bags, L)
            assert (kept >= 0).sum(1).max().item() > 8 or L == 6                       # bags that reach into a second chunk
            a64 = torch.tensor(attn_np.astype(np.float64), requires_grad=True)
            t64 = torch.tensor(table_np.astype(np.float64), requires_grad=True)
            base_rows = None if base is None else torch.from_numpy(base_np.astype(np.float64))[torch.from_numpy(base_ids_np)]
            o64 = atc.attention_forward_torch(t64, kept, a64, base_rows)[0]
            (o64 * dy.cpu().double()).sum().backward()
            print("dattn (f64 autograd)", _within(N(attn.grad), a64.grad.numpy(), (dim, L, "autograd dattn against f64 autograd")))
            g_table = np.zeros((80, dim))
            np.add.at(g_table, N(ids)[N(ids) >= 0], N(sg).astype(np.float64)[N(ids) >= 0])
            print("table (f64 autograd)", _within(g_table, t64.grad.numpy(), (dim, L, "scattered slot rows against f64 autograd")))
            torch.library.opcheck(torch.ops.twotower.history_attention_bwd, (table, ids, w.detach(), pooled.detach(), dy, attn.detach()))
    with pytest.raises(ValueError, match="go together"):
        torch.ops.twotower.history_attention(table, tok_t, rows, ex, base_table, None, T(attn_np, dev))


def test_train_cli_runs_with_attention_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  features:\n    history:\n      max_items: 9\n      pooling: sqrtn\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    ck, recs = tmp_path / "a.pt", tmp_path / "a.parquet"
    with contextlib.redirect_stdout(io.StringIO()):                        # 600 pairs, 10 % held out: 2 training steps
        assert train.main(["--config", str(cfgp), "--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--optimizer", "adam", "--history-len", "4", "--history-pooling", "attention", "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 2 and sd["adam_step"] == 3
    assert (sd["config"]["user_history_len"], sd["config"]["history_pooling"]) == (4, "attention")   # the CLI's pooling over the YAML's
    assert tuple(sd["history_table"].shape) == (200, 32) and tuple(sd["user_history"].shape) == (300, 4)
    assert sd["dense"][-36:].any().item() and sd["dense_m"][-36:].any().item()      # the attention vector trained, with its moments
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
    got = pq.read_table(recs).to_pydict()
    assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all()


# ------------------------------------------------------------------------------------------ 9. combinations and refusals
def test_combinations_and_refusals(dev):
    seed = 31
    kw = dict(cross_layers=1, rating_weight=0.5, rating_hidden=32, n_user_features=3, n_item_features=2, normalize_embeddings=True)
    for opt in ("adagrad", "adam"):
        tr = _history_trainer(dev, opt, seed, **kw)
        assert len(tr._segs) == tr.cfg.dense_segment_count() == 8 + 2 + 2 + 2 + 1
        tr.set_user_features(tr.synthetic_user_features(seed)); tr.set_item_features(tr.synthetic_item_features(seed))
        u, i = tr.synthetic_batch(seed, 0, "Z")
        ratings = torch.rand(256, device=dev) * 4 + 1
        losses = [tr.step(u, i, ratings=ratings).item() for _ in range(6)]
        tr.check_ids()
        assert np.isfinite(losses).all(), losses
        assert tr.history_attn.any() and torch.isfinite(tr.dense_flat).all() and torch.isfinite(tr.history_table).all()
    with pytest.raises(NotImplementedError, match="attention"):
        TwoTowerTrainer(_cfg("sgd", tower_dims=(128, 64, 32), user_history_len=4, history_pooling="attention", rating_weight=0.5,
                             n_user_features=3, n_item_features=2), dev, seed=1)
    tr = _history_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="history"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises((NotImplementedError, ValueError), match="history"):
        ShardedTwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="attention"), dev, seed=1)
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="attention", candidate_sampling="mixed",
                             n_sampled_negatives=64), dev, seed=1)

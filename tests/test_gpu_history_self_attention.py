"""The multi-head self-attention encoder of the user history on the GPU (tt_history_self_attention_*_f32,
csrc/history_selfattn.hip, and the GEMM launches around them): forward and backward against the f64 restatement of
tests/selfattn_check.py within the project's bars (relative <= 1e-4 in the 2-norm, max-abs <= 1e-4 * max|ref|: DESIGN section 2),
the ids, the newest slots and the flag exactly, the written outputs (weights exactly 0 / exactly 1, sentinels, guard bands), the
bitwise properties (padding is invisible, a bag's bits are its own, runs repeat, emptied bags give the base row), the agreement
with the attention pool, the history table's update, then the trainer - parity with the f64 autograd restatement, training,
checkpoints, the inference paths, clipping - the custom ops, the CLIs, combinations and refusals."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import bag_check as bc
import selfattn_check as sc
from two_tower_amazon_recommender_amd import _lib, data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001
BAR = sc.BAR
KEPT = ("batch_ids", "newest", "xn", "T", "P", "weights", "dP", "dT", "dxn")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(bc.bits(np.asarray(a, dtype=np.float32)), bc.bits(np.asarray(b, dtype=np.float32)))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded_buffers(n_bags, L, dim, heads, dev):
    """``ops.SelfAttnBuffers`` whose tensors are the leading part of longer ones filled with a sentinel: the guard bands."""
    big = ops.SelfAttnBuffers(n_bags + 1, L, dim, heads, dev)
    big.long = {k: getattr(big, k) for k in KEPT}
    for k, t in big.long.items():
        t.fill_(-7)
        setattr(big, k, t[:n_bags * L] if k == "batch_ids" else t[:n_bags])
    big.n_bags = n_bags
    return big


def _bands_intact(bufs):
    n, L = bufs.n_bags, bufs.L
    return all(bool((t[n * L if k == "batch_ids" else n:] == -7).all().item()) for k, t in bufs.long.items())


def _device_forward(dev, p, keep=True):
    """One forward on the device from a ``selfattn_check.forward_problem``: (out, flag, buffers or None, guard bands intact)."""
    tok, bag_rows = p["tokens"], p["bag_rows"]
    n_bags = len(tok) if bag_rows is None else len(bag_rows)
    L, dim, heads = tok.shape[1], p["table"].shape[1], p["p"].shape[0]
    out = torch.full((n_bags + 1, dim), 7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    base = None if p["base"] is None else (T(p["base"][0], dev), T(p["base"][1], dev))
    bufs = _guarded_buffers(n_bags, L, dim, heads, dev) if keep else False
    ops.history_self_attention(T(p["table"], dev), T(tok, dev), T(p["Wqk"], dev), T(p["Wvo"], dev), T(p["p"], dev), T(bag_rows, dev),
                               T(p["exclude"], dev), base, out=out[:n_bags], oob_flag=flag, keep=bufs)
    intact = bool((out[n_bags:] == 7).all().item()) and (not keep or _bands_intact(bufs))
    return N(out[:n_bags]), int(flag.item()), (bufs if keep else None), intact


def _device_backward(dev, bufs, p):
    """The backward on the device into sentinel-filled outputs: (dict of results - the GEMM slabs summed in f64, the dp slabs as
    they are -, checks ok)."""
    n_bags, L, dim, h = bufs.n_bags, bufs.L, bufs.dim, bufs.heads
    m, ns, nsp = n_bags * L, ops.dense_bwd_num_slabs(n_bags), ops.history_self_attention_num_slabs(n_bags)
    nan = float("nan")
    sg = torch.full((m + 1, dim), nan, device=dev)
    dwqk, dwvo = torch.full((ns + 1, dim, h * dim), nan, device=dev), torch.full((ns + 1, h * dim, dim), nan, device=dev)
    dp = torch.full((nsp + 1, h * L), nan, device=dev)
    for t in (bufs.dP, bufs.dT, bufs.dxn):
        t.fill_(nan)                                                                # (views: the guard bands behind them stay)
    ops.history_self_attention_bwd(bufs, T(p["dy"], dev), T(p["Wqk"], dev), T(p["Wvo"], dev), slot_grads=sg[:m], dwqk_slabs=dwqk[:ns],
                                   dwvo_slabs=dwvo[:ns], dp_slabs=dp[:nsp])
    ids = N(bufs.batch_ids)
    sgn = N(sg[:m])
    ok = all(bool(torch.isfinite(t).all().item()) for t in (dwqk[:ns], dwvo[:ns], dp[:nsp], bufs.dP, bufs.dT, bufs.dxn))   # written in full
    ok = ok and all(bool(torch.isnan(t).all().item()) for t in (sg[m:], dwqk[ns:], dwvo[ns:], dp[nsp:]))                  # not beyond
    ok = ok and np.isnan(sgn[ids < 0]).all() and np.isfinite(sgn[ids >= 0]).all()        # a skipped slot's row keeps the sentinel
    ok = ok and _bands_intact(bufs)
    sgn = np.where((ids >= 0)[:, None], sgn, 0.0)
    return dict(slot_grads=sgn, dWqk=N(dwqk[:ns]).astype(np.float64).sum(0), dWvo=N(dwvo[:ns]).astype(np.float64).sum(0),
                dp_slabs=N(dp[:nsp]), dT=N(bufs.dT), dP=N(bufs.dP)), bool(ok)


def _reference(p):
    out, ids, flag, saved = sc.forward(p["table"], p["tokens"], p["Wqk"], p["Wvo"], p["p"], p["bag_rows"], p["exclude"], p["base"])
    return out, ids, flag, saved


def _forward_and_backward_within_bars(dev, p, what, worst):
    want_out, want_ids, want_flag, saved = _reference(p)
    valid, newest = saved["valid"], saved["newest"]
    n_bags, L = valid.shape
    h, dim = p["p"].shape[0], p["table"].shape[1]
    out, flag, bufs, intact = _device_forward(dev, p)
    assert np.array_equal(N(bufs.batch_ids), want_ids) and flag == want_flag and intact, what
    assert np.array_equal(N(bufs.newest), newest), what
    assert _same_bits(N(bufs.xn), saved["xn"].astype(np.float32)), what                  # the newest kept rows, +0 where none
    w = N(bufs.weights)
    assert not w[~np.broadcast_to(valid[:, None, :], w.shape)].any(), what                # exactly 0 in a skipped slot
    one = valid.sum(1) == 1
    assert one.any() and np.array_equal(w[one].sum(2), np.ones((one.sum(), h), dtype=np.float32)), what   # exactly 1 for one kept slot
    assert set(np.unique(w[one])) <= {0.0, 1.0}
    assert not N(bufs.P)[newest < 0].any() and not N(bufs.T)[newest < 0].any(), what
    res = {"out": (out, want_out, None), "weights": (w, saved["w"], None), "P": (N(bufs.P).reshape(n_bags, h, dim), saved["P"], None)}
    # the inference form (nothing kept) gives the same bits
    out2, flag2, _, intact2 = _device_forward(dev, p, keep=False)
    assert _same_bits(out, out2) and flag2 == flag and intact2, what
    got, ok = _device_backward(dev, bufs, p)
    assert ok, what
    want = sc.backward(saved, p["dy"], p["Wqk"], p["Wvo"])
    zs = sc.uncancelled_scales(saved, p["dy"], p["Wqk"], p["Wvo"])
    dp_bag, _ = sc.per_bag_terms(saved, p["dy"], p["Wvo"])
    nsp = got["dp_slabs"].shape[0]
    per = -(-n_bags // nsp)
    want_slabs = np.stack([dp_bag[s * per:(s + 1) * per].sum(0).reshape(-1) for s in range(nsp)])    # contiguous bags, a ragged last one
    for k in ("slot_grads", "dWqk", "dWvo", "dT", "dP"):
        res[k] = (got[k], want[k], zs.get(k))
    res["dp_slabs"] = (got["dp_slabs"], want_slabs, zs["dp"])
    res["dp"] = (got["dp_slabs"].astype(np.float64).sum(0).reshape(h, L), want["dp"], zs["dp"])
    for k, (g, wnt, z) in res.items():
        worst[k] = max(worst.get(k, 0.0), max(sc.within_bars(g, wnt, (k,) + what, z)))
    return saved, out, bufs


# ------------------------------------------------------------------------------------------ 1. forward and backward, the sweep
@pytest.mark.parametrize("L", sc.LS)
@pytest.mark.parametrize("dim", sc.DIMS)
def test_forward_and_backward_match_the_restatement(dev, dim, L):
    """Every combination of dim {32, 96, 128, 256} (lane groups of 8, 32 with idle lanes, 32 and 64) x L {1, 3, 7, 64} x heads
    {1, 2, 4, 8} x bags {33, 300} (a ragged last lane group, a ragged last slab), at both logit scales of
    ``selfattn_check.SCALES``, with ``attention_check.problem``'s special bags, indirect bag rows, ``exclude`` and a base with a
    -1 id: out, weights, P, slot_grads, dT, dP, the summed slabs of dWqk and dWvo and every dp slab within the bars of the f64
    restatement; batch_ids, newest, xn and the flag exactly; weights exactly 0 in skipped slots and exactly 1 for a single kept
    slot; untouched slot_grads rows keep the sentinel; every output written in full and the guard bands behind them intact."""
    worst = {}
    for nb in sc.BAGS:
        for heads in sc.HEADS:
            for scale in sc.SCALES:
                p = sc.forward_problem(dim, nb, L, heads, scale)
                _forward_and_backward_within_bars(dev, p, (dim, nb, L, heads, scale), worst)
    print(dim, L, {k: f"{v:.2e}" for k, v in worst.items()})


def _flag_problem(what):
    """``forward_problem(32, 33, 7, 2)`` (flag 0: its bag rows, tokens and base ids are valid or -1) with ONE kind of
    out-of-range entry, or all of them: bags 16 / 17 / 18 pool token rows 20 / 21 / 22, which nothing else touches."""
    p = sc.forward_problem(32, 33, 7, 2)
    tok, rows, base_ids, exclude = p["tokens"].copy(), p["bag_rows"].copy(), p["base"][1].copy(), p["exclude"].copy()
    tok[20:23] = np.arange(21).reshape(3, 7) + 30
    exclude[13:21] = sc.ROWS - 1                                                      # (matches nothing)
    rows[16:19] = [20, 21, 22]
    rows[13:16] = [3, 4, 5]
    rows[19:21] = [6, 6]
    base_ids[13:21] = [1, 2, 3, 4, 5, 6, 7, 8]
    if what in ("token >= rows", "all"):
        tok[20, 1], tok[21, 6] = sc.ROWS, sc.ROWS + 1000                              # (21, 6): the newest slot falls away
    if what in ("token < -1", "all"):
        tok[22, 0], tok[22, 3] = -5, -2
    if what in ("bag row >= rows", "all"):
        rows[13] = sc.TOKEN_ROWS
    if what in ("bag row < -1", "all"):
        rows[14] = -3
    if what in ("base id >= rows", "all"):
        base_ids[19] = 40
    if what in ("base id < -1", "all"):
        base_ids[20] = -4
    if what == "-1 only":
        tok[20, 1], tok[22, 0], rows[13], rows[14], base_ids[19], base_ids[20] = -1, -1, -1, -1, -1, -1
    p.update(tokens=tok, bag_rows=rows, exclude=exclude, base=(p["base"][0], base_ids))
    return p


@pytest.mark.parametrize("what", ["none", "-1 only", "token >= rows", "token < -1", "bag row >= rows", "bag row < -1", "base id >= rows",
                                  "base id < -1", "all"])
def test_out_of_range_entries_set_the_flag_and_count_as_skipped(dev, what):
    """Every path that raises the flag, one at a time and together: a token >= table_rows, a negative token other than -1, a bag
    row >= n_token_rows or < -1, a base id >= base_rows or < -1 (all in the resolve launch).  The flag equals the restatement's -
    1 with any of them, 0 with none and with -1 alone -, the slot ids are -1 there, the newest slot is the newest KEPT one, a bad
    base id gives a zero base row, and ``out`` meets the bars; the inference form raises the same flag."""
    p = _flag_problem(what)
    want_out, want_ids, want_flag, saved = _reference(p)
    assert want_flag == (0 if what in ("none", "-1 only") else 1)
    out, flag, bufs, intact = _device_forward(dev, p)
    ids = N(bufs.batch_ids)
    assert flag == want_flag and np.array_equal(ids, want_ids) and intact and np.array_equal(N(bufs.newest), saved["newest"])
    sc.within_bars(out, want_out, what)
    out2, flag2, _, _ = _device_forward(dev, p, keep=False)
    assert flag2 == want_flag and _same_bits(out, out2)
    ids7, newest = ids.reshape(33, 7), N(bufs.newest)
    if what in ("token >= rows", "all"):
        assert ids7[16, 1] == -1 and ids7[17, 6] == -1 and newest[17] == 5
    if what in ("token < -1", "all"):
        assert ids7[18, 0] == -1 and ids7[18, 3] == -1
    if what in ("bag row >= rows", "all"):
        assert (ids7[13] == -1).all() and newest[13] == -1 and _same_bits(out[13], p["base"][0][1])     # an emptied bag: the base row
    if what in ("bag row < -1", "all"):
        assert (ids7[14] == -1).all() and _same_bits(out[14], p["base"][0][2])
    if what in ("base id >= rows", "base id < -1", "all"):
        k = 19 if what != "base id < -1" else 20
        no_base = dict(p, base=None)
        assert _same_bits(out[k], _device_forward(dev, no_base, keep=False)[0][k])          # a zero base row: O alone


# ------------------------------------------------------------------------------------------ 2. bitwise properties
@pytest.mark.parametrize("dim,L,heads,scale", [(32, 7, 2, 1.0), (128, 64, 4, 4.0), (256, 3, 8, 4.0), (96, 64, 1, 1.0)])
def test_padding_is_invisible_and_emptied_bags_give_the_base_row(dev, dim, L, heads, scale):
    """A bag's two kept items in slots (0, 2), (0, 1) or (L-2, L-1) give the same out, P and kept weights bit for bit, with the
    second item kept by position or uncovered by ``exclude``; an all-padding bag, and a bag of one token excluded in every slot,
    give the base row itself (also a base row of -0.0s: the bits, not the value); two runs are identical, forward and backward,
    the dp slabs included."""
    rng = np.random.default_rng([dim, L])
    p = sc.forward_problem(dim, 33, L, heads, scale, indirect=False)
    tok = np.full((33, L), -1, dtype=np.int32)
    tok[0, 0], tok[0, 2] = 3, 9
    tok[1, 0], tok[1, 1] = 3, 9
    tok[2, L - 2], tok[2, L - 1] = 3, 9
    tok[3] = [3, 44, 9] + [44] * (L - 3)                                        # 44 is excluded: the same two items remain
    tok[5] = 11                                                                 # emptied by the exclusion
    tok[6:] = rng.integers(0, sc.ROWS - 1, (27, L))
    exclude = np.full(33, sc.ROWS - 1, dtype=np.int64)
    exclude[3], exclude[5] = 44, 11
    base_table, base_ids = p["base"][0].copy(), p["base"][1].copy()
    base_table[7, ::2] = -0.0
    base_ids[:6] = 7
    p.update(tokens=tok, exclude=exclude, base=(base_table, base_ids))
    out, flag, bufs, intact = _device_forward(dev, p)
    ids = N(bufs.batch_ids)
    assert flag == 0 and (ids.reshape(33, L)[:4] >= 0).sum(1).tolist() == [2, 2, 2, 2] and intact and np.isfinite(out).all()
    assert N(bufs.newest)[:6].tolist() == [2, 1, L - 1, 2, -1, -1]
    Pn, wn = N(bufs.P), N(bufs.weights)
    for k in (1, 2, 3):
        assert _same_bits(out[0], out[k]) and _same_bits(Pn[0], Pn[k]), k
        assert _same_bits(wn[0][:, ids.reshape(33, L)[0] >= 0], wn[k][:, ids.reshape(33, L)[k] >= 0]), k
    assert not _same_bits(out[0], base_table[7])
    assert _same_bits(out[4], base_table[7]) and _same_bits(out[5], base_table[7])
    back, ok = _device_backward(dev, bufs, p)
    assert ok
    out_b, _, bufs2, _ = _device_forward(dev, p)
    assert _same_bits(out, out_b) and all(_same_bits(N(getattr(bufs, k)), N(getattr(bufs2, k))) for k in ("xn", "T", "P", "weights"))
    back2, ok2 = _device_backward(dev, bufs2, p)
    assert ok2 and all(_same_bits(back[k], back2[k]) for k in ("slot_grads", "dp_slabs", "dT", "dP"))
    assert all(np.array_equal(back[k], back2[k]) for k in ("dWqk", "dWvo"))
    # with one dy for all, the two kept slots of bags 0..3 get the same gradient rows and the bags the same dT, wherever they sit
    dy_same = dict(p, dy=np.repeat(p["dy"][:1], 33, 0))
    back3 = _device_backward(dev, _device_forward(dev, dy_same)[2], dy_same)[0]
    kept3 = [back3["slot_grads"].reshape(33, L, dim)[k][ids.reshape(33, L)[k] >= 0] for k in range(4)]
    assert all(_same_bits(kept3[0], kept3[k]) and _same_bits(back3["dT"][0], back3["dT"][k]) for k in (1, 2, 3))


def _pool_fwd(dev, table, ids, Tm, p, n_bags, L, heads):
    d = table.shape[1]
    P = torch.full((n_bags + 1, heads * d), -7.0, device=dev)
    w = torch.full((n_bags + 1, heads, L), -7.0, device=dev)
    _lib.check(_lib.load().tt_history_self_attention_pool_fwd_f32(_ptr(table), table.shape[0], d, L, heads, _ptr(ids), n_bags, _ptr(Tm),
                                                                  _ptr(p), _ptr(P), _ptr(w), _stream()), "pool_fwd")
    assert bool((P[n_bags:] == -7).all().item()) and bool((w[n_bags:] == -7).all().item())
    return P[:n_bags], w[:n_bags]


def _pool_bwd(dev, table, ids, w, P, dP, Tm, n_bags, L, heads, n_slabs):
    d = table.shape[1]
    sg = torch.zeros(n_bags * L, d, device=dev)
    dT = torch.full((n_bags + 1, heads * d), -7.0, device=dev)
    slabs = torch.full((n_slabs + 1, heads * L), -7.0, device=dev)
    _lib.check(_lib.load().tt_history_self_attention_pool_bwd_f32(_ptr(table), table.shape[0], d, L, heads, _ptr(ids), _ptr(w), _ptr(P),
                                                                  _ptr(dP), _ptr(Tm), n_bags, _ptr(sg), _ptr(dT), _ptr(slabs), n_slabs,
                                                                  _stream()), "pool_bwd")
    assert bool((dT[n_bags:] == -7).all().item()) and bool((slabs[n_slabs:] == -7).all().item())
    return sg, dT[:n_bags], slabs[:n_slabs]


def test_a_bag_alone_equals_the_same_bag_inside_a_300_bag_launch(dev):
    """The pool launches given the same T (forward: P and weights; backward: the slot rows and dT, and the bag's dp line as a
    one-bag slab against the f64 per-bag term), and ``ops.history_self_attention`` end to end, bit for bit."""
    for dim, L, heads, scale in ((32, 7, 2, 1.0), (96, 64, 4, 4.0), (256, 3, 8, 1.0), (128, 64, 1, 4.0)):
        p = sc.forward_problem(dim, 300, L, heads, scale)
        out, _, bufs, _ = _device_forward(dev, p)
        back, ok = _device_backward(dev, bufs, p)
        assert ok and np.isfinite(out).all()
        table = T(p["table"], dev)
        saved = _reference(p)[3]
        dp_bag, _ = sc.per_bag_terms(saved, p["dy"], p["Wvo"])
        zs = sc.uncancelled_scales(saved, p["dy"], p["Wqk"], p["Wvo"])["dp"]
        sg300 = back["slot_grads"].reshape(300, L, dim)
        for k in (0, 2, 8, 11, 12, 31, 32, 150, 299):
            one = dict(p, bag_rows=p["bag_rows"][k:k + 1], exclude=p["exclude"][k:k + 1], base=(p["base"][0], p["base"][1][k:k + 1]))
            o1, _, b1, _ = _device_forward(dev, one)
            assert _same_bits(o1[0], out[k]) and np.array_equal(N(b1.batch_ids), N(bufs.batch_ids)[k * L:(k + 1) * L]), (dim, L, k)
            # the pool launches alone, from the 300-bag launch's own T / dP rows
            ids1 = bufs.batch_ids[k * L:(k + 1) * L].clone()
            P1, w1 = _pool_fwd(dev, table, ids1, bufs.T[k:k + 1].clone(), T(p["p"], dev), 1, L, heads)
            assert _same_bits(N(P1[0]), N(bufs.P[k])) and _same_bits(N(w1[0]), N(bufs.weights[k])), (dim, L, k)
            sg1, dT1, slab1 = _pool_bwd(dev, table, ids1, w1.contiguous(), P1.contiguous(), bufs.dP[k:k + 1].clone(),
                                        bufs.T[k:k + 1].clone(), 1, L, heads, 1)
            keep = N(ids1) >= 0
            # (the 300-bag launch's newest row also carries += dxn: compare the rows before it, i.e. all but the newest)
            nw = int(N(bufs.newest)[k])
            rows = keep.copy()
            if nw >= 0:
                rows[nw] = False
            assert _same_bits(N(sg1)[rows], sg300[k][rows]) and _same_bits(N(dT1[0]), back["dT"][k]), (dim, L, k)
            sc.within_bars(N(slab1[0]), dp_bag[k].reshape(-1), ("dp line", dim, L, k), zs)


def test_agreement_with_the_attention_pool(dev):
    """The pool forward with one head and every bag's T row equal to a vector a IS the attention pool with attn = [a | p]: its
    weights and pooled rows agree with tt_history_attention_fwd_f32's within the bars - and bit for bit: the kernel keeps the
    attention pool's operation order (the fmaf chain inside the lane, the xor butterfly, the online softmax's updates, the
    normalisation), so the stronger statement is asserted too."""
    for dim, L in ((32, 7), (96, 64), (128, 20), (256, 3)):
        p = sc.forward_problem(dim, 300, L, 1, 1.0)
        rng = np.random.default_rng([dim, L])
        a = (4.0 * np.sqrt(dim) * rng.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
        attn = T(np.concatenate([a, p["p"][0]]), dev)
        table, tok = T(p["table"], dev), T(p["tokens"], dev)
        ids = torch.empty(300 * L, dtype=torch.int64, device=dev)
        _, w_att, pooled_att = ops.history_attention(table, tok, attn, T(p["bag_rows"], dev), T(p["exclude"], dev), batch_ids=ids)
        Tm = T(np.repeat(a[None, :], 300, 0), dev)
        P, w = _pool_fwd(dev, table, ids, Tm, T(p["p"], dev), 300, L, 1)
        print(dim, L, "weights", sc.within_bars(N(w[:, 0]), N(w_att).astype(np.float64), "weights"),
              "pooled", sc.within_bars(N(P), N(pooled_att).astype(np.float64), "pooled"))
        assert _same_bits(N(w[:, 0]), N(w_att)) and _same_bits(N(P), N(pooled_att)), (dim, L)


def test_ops_argument_checks(dev):
    p = sc.forward_problem(32, 33, 7, 2)
    a = [T(p[k], dev) for k in ("table", "tokens", "Wqk", "Wvo", "p")]
    rows, ex = T(p["bag_rows"], dev), T(p["exclude"], dev)
    with pytest.raises(RuntimeError, match=r"Wqk must be \[32, H \* 32\]"):
        ops.history_self_attention(a[0], a[1], a[2][:, :-1].contiguous(), a[3], a[4], rows)
    with pytest.raises(RuntimeError, match="heads in"):
        ops.history_self_attention(a[0], a[1], torch.zeros(32, 96, device=dev), torch.zeros(96, 32, device=dev),
                                   torch.zeros(3, 7, device=dev), rows)
    with pytest.raises(RuntimeError, match="Wqk must be"):
        ops.history_self_attention(a[0], a[1], a[2], a[3], a[4][:, :-1].contiguous(), rows)
    with pytest.raises(RuntimeError, match="exclude must hold"):
        ops.history_self_attention(*a, rows, ex[:-1])
    with pytest.raises(RuntimeError, match="base must be"):
        ops.history_self_attention(*a, rows, base=(T(p["base"][0], dev), T(p["base"][1][:-1], dev)))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.history_self_attention(torch.zeros(10, 36, device=dev), a[1], torch.zeros(36, 36, device=dev),
                                   torch.zeros(36, 36, device=dev), torch.zeros(1, 7, device=dev), rows)
    with pytest.raises(RuntimeError, match="SelfAttnBuffers"):
        ops.history_self_attention(*a, rows, keep=ops.SelfAttnBuffers(5, 7, 32, 2, dev))
    with pytest.raises(RuntimeError, match="scratch must be"):
        ops.history_self_attention(*a, rows, scratch=ops.SelfAttnBuffers(5, 7, 32, 2, dev, backward=False))
    out, bufs = ops.history_self_attention(*a, rows, ex, keep=True)
    with pytest.raises(RuntimeError, match="dy must be"):
        ops.history_self_attention_bwd(bufs, torch.zeros(32, 32, device=dev), a[2], a[3])
    with pytest.raises(RuntimeError, match="dwqk_slabs must be"):
        ops.history_self_attention_bwd(bufs, torch.zeros(33, 32, device=dev), a[2], a[3], dwqk_slabs=torch.zeros(1, 32, 32, device=dev))
    with pytest.raises(RuntimeError, match="dp_slabs must be"):
        ops.history_self_attention_bwd(bufs, torch.zeros(33, 32, device=dev), a[2], a[3], dp_slabs=torch.zeros(5, 13, device=dev))
    with pytest.raises(RuntimeError, match="with backward buffers"):
        ops.history_self_attention_bwd(ops.SelfAttnBuffers(33, 7, 32, 2, dev, backward=False), torch.zeros(33, 32, device=dev), a[2], a[3])
    # a scratch for more bags serves a shorter call and gives the same bits as fresh allocations
    scratch = ops.SelfAttnBuffers(40, 7, 32, 2, dev, backward=False)
    assert torch.equal(ops.history_self_attention(*a, rows, ex, scratch=scratch), ops.history_self_attention(*a, rows, ex))
    assert torch.equal(ops.history_self_attention(*a, rows, ex), out)


# ------------------------------------------------------------------------------------------ 3. the update
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_update_from_the_slot_rows_is_bit_exact(dev, opt):
    """slot_grads through a plain SparsePlan(n_bags * L) into SGD, Adagrad and lazy Adam: the table and its state equal the
    restatement's update of the same rows bit for bit; rows no kept slot names keep their bits.  Bag 1 holds token 7 in its first
    AND its newest slot: the += dxn lands on one of two equal ids (the rows differ, the update sums them), and the slot rows
    themselves meet the bars of the f64 closed form."""
    rng = np.random.default_rng(5)
    n_bags, L, dim, heads = 64, 7, 32, 2
    table = rng.uniform(-0.05, 0.05, (60, dim)).astype(np.float32)
    tok = rng.integers(0, 50, (n_bags, L)).astype(np.int32)
    tok[rng.random((n_bags, L)) < 0.25] = -1
    tok[tok == 49] = 48
    tok[:, 0] = np.where(np.arange(n_bags) % 2 == 0, 49, tok[:, 0])               # token 49 only where it is excluded
    tok[1, 0] = tok[1, L - 1] = 7
    exclude = np.where(np.arange(n_bags) % 2 == 0, 49, 55).astype(np.int64)
    Wqk, Wvo, p = sc.params(rng, dim, L, heads, 4.0)
    Wqk *= 20.0                                                                   # (rows of size 0.05, not 1: logits of order 1 again)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    state = [table]
    if opt == "adagrad":
        state = [table, np.full_like(table, 0.1)]
    elif opt == "adam":
        state = [table, (rng.standard_normal(table.shape) * 0.01).astype(np.float32),
                 ((rng.standard_normal(table.shape) * 0.01) ** 2).astype(np.float32)]
    d = [T(a, dev) for a in state]
    out, bufs = ops.history_self_attention(d[0], T(tok, dev), T(Wqk, dev), T(Wvo, dev), T(p, dev), exclude=T(exclude, dev), keep=True)
    sg = ops.history_self_attention_bwd(bufs, T(dy, dev), T(Wqk, dev), T(Wvo, dev), slot_grads=torch.zeros(n_bags * L, dim, device=dev))[0]
    ids = bufs.batch_ids
    _, want_ids, _, saved = sc.forward(table, tok, Wqk, Wvo, p, None, exclude)
    want_sg = sc.backward(saved, dy, Wqk, Wvo)
    print("slot rows", sc.within_bars(N(sg), want_sg["slot_grads"], "slot rows"))
    assert saved["newest"][1] == L - 1 and want_ids.reshape(n_bags, L)[1, 0] == 7 == want_ids.reshape(n_bags, L)[1, L - 1]
    assert np.abs(want_sg["dxn"][1]).max() > 0 and not _same_bits(N(sg)[L], N(sg)[2 * L - 1])
    plan = ops.SparsePlan(n_bags * L, dev)
    plan.run(ids, table.shape[0])
    if opt == "sgd":
        ops.sparse_sgd_(d[0], sg, plan, LR)
    elif opt == "adagrad":
        ops.sparse_adagrad_(d[0], d[1], sg, plan, LR)
    else:
        ops.adam_step_([(d[0], d[1], d[2], sg, plan)], [], ops.AdamHyper(lr=LR, step=7))
    assert np.array_equal(N(ids), want_ids) and (tok == 49).any() and not (want_ids == 49).any() and (want_ids == 48).any()
    want = [a.copy() for a in state]
    touched = bc.bag_update(opt, want, want_ids, N(sg), 1, LR, step=7)          # one gradient row per slot: "bags" of one slot
    for g, wnt, name in zip(d, want, ("table", "state 1", "state 2")):
        assert np.isfinite(N(g)).all() and _same_bits(N(g), wnt), (opt, name)
    rest = np.setdiff1d(np.arange(len(table)), touched)
    assert 49 in rest and 7 in touched
    for g, s0 in zip(d, state):
        assert _same_bits(N(g)[rest], s0[rest]) and not _same_bits(N(g)[touched], s0[touched])


# ------------------------------------------------------------------------------------------ 4. trainer
def _cfg(opt, batch=64, dim=32, tower_dims=(64, 32), n_users=100, n_items=400, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **kw)


def _sa_trainer(dev, opt="adagrad", seed=1001, pooling="self_attention", L=7, heads=2, batches=3, **kw):
    """Histories from the pairs of the first synthetic batches (``data.user_histories``, file order): the steps' positives are in
    them."""
    tr = TwoTowerTrainer(_cfg(opt, user_history_len=L, history_pooling=pooling, history_heads=heads, **kw), dev, seed=seed)
    pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(batches)]
    u = torch.cat([p[0] for p in pairs]).cpu().numpy()
    i = torch.cat([p[1] for p in pairs]).cpu().numpy()
    tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, L), dev))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _set_p(tr, seed):
    """A random recency bias (it starts at zero), distinct per head and rank, and rows large enough for logits of order 1 - so
    that dp, and a slot counted at a wrong rank, show from the first step on."""
    tr.sa_p.copy_(T((np.random.default_rng(seed).standard_normal(tuple(tr.sa_p.shape)) * 0.5).astype(np.float32), tr.dev))


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def _step_against_f64(tr, seed, step):
    """One forward_backward against ``selfattn_check.step_f64``: (the restatement's results, the loss, the step's ids, the checks as
    (name, got, want, zero_scale) with the device's gradients summed over their slabs in f64)."""
    cfg = tr.cfg
    L = cfg.user_history_len
    hist = N(tr.user_history)
    u, i = tr.synthetic_batch(seed, step, "Z")
    un, inn = N(u), N(i)
    before = {k: N(getattr(tr, k)).astype(np.float64) for k in ("user_table", "item_table", "history_table", "sa_Wqk", "sa_Wvo", "sa_p")}
    towers = _towers64(tr)
    loss = tr.forward_backward(u, i).item()
    tr.check_ids()
    masks = tuple([N(t.acts[l + 1] > 0) for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    r = sc.step_f64(before["user_table"], before["item_table"], before["history_table"], before["sa_Wqk"], before["sa_Wvo"],
                    before["sa_p"], towers, un, inn, hist, 0.1, masks)
    valid = hist[un] >= 0
    match = valid & (hist[un] == inn[:, None])
    ids = N(tr.history_ids)
    assert np.array_equal(ids.reshape(cfg.batch_size, L), np.where(valid & ~match, hist[un], -1))      # the leave-one-out rule
    sg = N(tr.history_slot_grads).astype(np.float64)
    g_hist = np.zeros_like(before["history_table"])
    np.add.at(g_hist, ids[ids >= 0], sg[ids >= 0])
    saved = sc.forward(before["history_table"].astype(np.float32), hist, before["sa_Wqk"], before["sa_Wvo"], before["sa_p"], un, inn)[3]
    zs = sc.uncancelled_scales(saved, r["due"], before["sa_Wqk"], before["sa_Wvo"])
    dwqk, dwvo, dp = (N(x).astype(np.float64) for x in tr._sa_slabs)
    checks = [("due", N(tr.user_tower.demb), r["due"], None), ("die", N(tr.item_tower.demb), r["die"], None),
              ("history_table", g_hist, r["history_table"], None), ("dWqk", dwqk.sum(0), r["dWqk"], zs["dWqk"]),
              ("dWvo", dwvo.sum(0), r["dWvo"], None), ("dp", dp.sum(0).reshape(r["dp"].shape), r["dp"], zs["dp"])]
    return r, loss, (u, i, un, inn, ids, sg, match, valid), checks, before, saved


@pytest.mark.parametrize("L", [1, 7])
def test_trainer_step_matches_the_f64_restatement(dev, L):
    """One step (and a second, from updated parameters) at batch 64, dim 32, towers [64, 32], two heads, p randomised first: the
    loss, due, the history table's gradient (the scatter-add of the slot rows), dWqk, dWvo and dp within the bars of f64 torch
    autograd given the device's ReLU masks (L = 1: dWqk and dp are pure cancellation, held to the bar of their terms' size)."""
    seed = 1001
    tr = _sa_trainer(dev, "sgd", seed, L=L)
    lay = tr.layout
    assert not tr.fuse_lookup and tr.sa_Wqk.storage_offset() % 4 == 0 and not tr.sa_p.any() and tr.sa_Wqk.any() and tr.sa_Wvo.any()
    assert list(lay.blocks)[-3:] == ["history_sa.Wqk", "history_sa.Wvo", "history_sa.p"]
    assert len(tr._segs) == tr.cfg.dense_segment_count() == 8 + 3
    for w, fan in ((tr.sa_Wqk, 32 + 32), (tr.sa_Wvo, 64 + 32)):                        # Glorot-uniform
        lim = np.sqrt(6.0 / fan)
        assert 0.9 * lim < w.abs().max().item() <= lim
    _set_p(tr, 5)
    tr.history_table.mul_(10.0)                                                        # rows of size 0.5: logits that matter
    for step in range(2):
        r, loss, (u, i, un, inn, ids, sg, match, valid), checks, _, _ = _step_against_f64(tr, seed, step)
        print(f"L {L} step {step}: loss {loss} (f64 {r['loss']})")
        assert abs(loss - r["loss"]) <= BAR * abs(r["loss"]), (loss, r["loss"])
        assert match.any() and (valid & ~match).any()
        for what, got, want, z in checks:
            print(f"L {L} step {step}: {what}", sc.within_bars(got, want, (L, step, what), z))
        if L > 1:
            assert np.abs(r["dp"]).max() > 0 and np.abs(r["dWqk"]).max() > 0
        q0, v0, p0 = tr.sa_Wqk.clone(), tr.sa_Wvo.clone(), tr.sa_p.clone()
        tr.apply_gradients(step_ids=[u, i])
        assert not torch.equal(v0, tr.sa_Wvo) and (L == 1 or (not torch.equal(q0, tr.sa_Wqk) and not torch.equal(p0, tr.sa_p)))


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam", "rowwise_adagrad"])
def test_thirty_steps_lower_the_loss(dev, opt):
    seed = 7
    tr = _sa_trainer(dev, opt, seed)
    batch0 = tr.synthetic_batch(seed, 0, "Z")
    t0, q0, v0 = tr.history_table.clone(), tr.sa_Wqk.clone(), tr.sa_Wvo.clone()
    losses = [tr.step(*batch0).item() for _ in range(30)]
    tr.check_ids()
    print(opt, f"{losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(t0, tr.history_table) and not torch.equal(q0, tr.sa_Wqk) and not torch.equal(v0, tr.sa_Wvo)
    assert tr.sa_p.any() and torch.isfinite(tr.dense_flat).all()


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17
    kw = dict(dropout_rate=0.1)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _sa_trainer(dev, opt, seed, **kw)
    run(a, range(4))
    b = _sa_trainer(dev, opt, seed, **kw)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["user_history_len"] == 7 and sd["config"]["history_pooling"] == "self_attention" and sd["config"]["history_heads"] == 2
    mean = _sa_trainer(dev, opt, seed, pooling="mean", **kw)
    assert set(sd) == set(mean.state_dict()) and sd["dense"].numel() == mean.dense_flat.numel() + 2 * 32 * 64 + 2 * 7
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values, no histories set
    c.load_state_dict(sd)
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "history_table", "user_history", "loss", "sa_Wqk", "sa_Wvo", "sa_p"]
    if opt == "adam":
        names += ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "history_m", "history_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.sa_Wqk, b.sa_Wqk)
    with pytest.raises(ValueError, match="history_pooling"):
        mean.load_state_dict(sd)
    with pytest.raises(ValueError, match="history_pooling"):
        c.load_state_dict(mean.state_dict())
    with pytest.raises(ValueError, match="history_heads"):
        _sa_trainer(dev, opt, seed, heads=4, **kw).load_state_dict(sd)


def test_inference_paths_encode_the_full_history(dev):
    """``evaluate``, ``user_embeddings`` (150 ids at batch 64: three chunks, the last ragged), ``evaluate_topk`` and the indexes'
    ``index_from_trainer`` feed the user tower user row + the encoder's output over the FULL history - nothing left out - within
    the bars of the restatement, and not what the train step fed, where the positive was left out; the encoder's own chunks
    (64 bags at a time against all at once) give the same bits; an inference pass between a step's backward and its update
    changes nothing the update reads."""
    from two_tower_amazon_recommender_amd.metrics import FactorizedTopK
    seed = 23
    tr = _sa_trainer(dev, "sgd", seed)
    _set_p(tr, 6)
    tr.history_table.mul_(10.0)
    for s in range(2):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    u, i = tr.synthetic_batch(seed, 1, "Z")
    table, hist, users = N(tr.history_table), N(tr.user_history), N(tr.user_table)
    Wqk, Wvo, p = N(tr.sa_Wqk), N(tr.sa_Wvo), N(tr.sa_p)
    un = N(u)
    assert (hist[un] == N(i)[:, None]).any()                                  # the positives are there - and stay in
    want = sc.forward(table, hist, Wqk, Wvo, p, un, None, (users, un))[0]
    train_in = sc.forward(table, hist, Wqk, Wvo, p, un, N(i), (users, un))[0]
    assert np.abs(want - train_in).max() > 1e-2 * np.abs(want).max()
    tr.evaluate(u, i)
    print("evaluate", sc.within_bars(N(tr.user_tower.acts[0]), want, "evaluate"))
    q_eval = tr.user_tower.acts[-1].clone()
    tr.user_tower.acts[0].zero_()
    tr.evaluate_topk(u, i, FactorizedTopK(ks=(5,), temperature=0.1))
    print("evaluate_topk", sc.within_bars(N(tr.user_tower.acts[0]), want, "evaluate_topk"))
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 100, 150)).to(dev)
    emb = tr.user_embeddings(ids)
    tr.check_ids()
    idn = N(ids)
    last = sc.forward(table, hist, Wqk, Wvo, p, idn[128:], None, (users, idn[128:]))[0]
    print("user_embeddings", sc.within_bars(N(tr.user_tower.acts[0][:22]), last, "user_embeddings"))
    assert emb.shape == (150, 32)
    err = (tr.user_embeddings(u) - q_eval).abs().max().item()
    assert err <= BAR * q_eval.abs().max().item(), err
    # the encoder's own chunking: 150 bags 64 at a time (the last chunk ragged, the scratch reused) against all at once
    whole, parts = torch.empty(150, 32, device=dev), torch.full((151, 32), 7.0, device=dev)
    tr._history_self_attention((ids, whole), None, False)
    assert tr._sa_scratch.n_bags == 150
    tr._sa_scratch = None
    tr._history_self_attention((ids, parts[:150]), None, False, chunk=64)
    assert tr._sa_scratch.n_bags == 64 and torch.equal(whole, parts[:150]) and bool((parts[150] == 7).all().item())
    print("chunks", sc.within_bars(N(whole), sc.forward(table, hist, Wqk, Wvo, p, idn, None, (users, idn))[0], "chunks"))
    from two_tower_amazon_recommender_amd import serving
    q5 = tr.user_embeddings(u[:5]).clone()
    want_scores = (q5 @ tr.item_corpus_embeddings().t()).topk(3, dim=1)[0]
    for index in (serving.BruteForce(k=3), serving.Int8BruteForce(k=3), serving.IVF(k=3, nlist=4, nprobe=4),
                  serving.Int8IVF(k=3, nlist=4, nprobe=4)):                     # queries are user ids run through the user tower
        scores, items = index.index_from_trainer(tr)(u[:5])
        assert tuple(items.shape) == (5, 3) and torch.isfinite(scores).all()
        assert (scores - want_scores).abs().max().item() <= BAR * want_scores.abs().max().item(), type(index).__name__
    # predict_ratings: the head's pairs go through the same full-history user input
    trr = _sa_trainer(dev, "sgd", seed, rating_weight=0.5, rating_hidden=32)
    pred = trr.predict_ratings(u, i)
    want_r = sc.forward(N(trr.history_table), N(trr.user_history), N(trr.sa_Wqk), N(trr.sa_Wvo), N(trr.sa_p), un, None,
                        (N(trr.user_table), un))[0]
    print("predict_ratings", sc.within_bars(N(trr.user_tower.acts[0]), want_r, "predict_ratings"))
    assert tuple(pred.shape) == (64,) and torch.isfinite(pred).all()
    # an inference pass between forward_backward and apply_gradients leaves the step's kept buffers alone
    tr2, tr3 = _sa_trainer(dev, "sgd", seed), _sa_trainer(dev, "sgd", seed)
    for t, peek in ((tr2, False), (tr3, True)):
        t.forward_backward(u, i)
        if peek:
            t.user_embeddings(ids)
        t.apply_gradients(step_ids=[u, i])
    assert torch.equal(tr2.history_table, tr3.history_table) and torch.equal(tr2.dense_flat, tr3.dense_flat)


def test_global_clipnorm_counts_a_kept_slot_once(dev):
    """grad_norm of a clipped step within the bars of the restatement's: the user and item rows per occurrence, ONE row per kept
    slot of the history (the slot rows of the closed form from the restatement's due), every dense gradient summed first."""
    seed = 29
    tr = _sa_trainer(dev, "sgd", seed, global_clipnorm=0.05)
    _set_p(tr, 3)
    tr.history_table.mul_(10.0)
    r, loss, (u, i, un, inn, ids, sg, match, valid), checks, before, saved = _step_against_f64(tr, seed, 0)
    slot = sc.backward(saved, r["due"], before["sa_Wqk"], before["sa_Wvo"])["slot_grads"]
    sq = (r["due"] ** 2).sum() + (r["die"] ** 2).sum() + (slot ** 2).sum() + sum((r[k] ** 2).sum() for k in ("dWqk", "dWvo", "dp"))
    sq += sum((g ** 2).sum() for t in range(2) for g in r["dw"][t] + r["db"][t])
    tr.clip_gradients()
    got, want = tr.grad_norm.item(), float(np.sqrt(sq))
    print("grad_norm", got, want, "scale", tr.clip_scale.item())
    assert abs(got - want) <= BAR * want and want > 0.05
    assert abs(tr.clip_scale.item() - 0.05 / want) <= BAR * 0.05 / want
    clipped = np.where((ids >= 0)[:, None], N(tr.history_slot_grads).astype(np.float64), 0.0)
    print("clipped slot rows", sc.within_bars(clipped, slot * (0.05 / want), "clipped slot rows"))
    tr.apply_gradients(step_ids=[u, i])
    assert torch.isfinite(tr.dense_flat).all()


# ------------------------------------------------------------------------------------------ 5. custom ops, CLIs
def test_custom_ops_pass_opcheck_equal_the_ops_calls_and_differentiate_the_parameters(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    for dim, L, heads, ind, base in ((32, 7, 2, True, True), (64, 3, 4, False, False)):
        p = sc.forward_problem(dim, 33, L, heads, 4.0, indirect=ind, with_base=base)
        table, tok = T(p["table"], dev), T(p["tokens"], dev)
        rows, ex = T(p["bag_rows"], dev), T(p["exclude"], dev)
        bt, bi = (None, None) if p["base"] is None else (T(p["base"][0], dev), T(p["base"][1], dev))
        Wqk, Wvo, pp = (T(p[k], dev).requires_grad_(True) for k in ("Wqk", "Wvo", "p"))
        args = (table, tok, rows, ex, bt, bi, Wqk, Wvo, pp)
        torch.library.opcheck(torch.ops.twotower.history_self_attention, args)
        out, ids, newest, xn, Tm, P, w = torch.ops.twotower.history_self_attention(*args)
        want, bufs = ops.history_self_attention(table, tok, Wqk.detach(), Wvo.detach(), pp.detach(), rows, ex,
                                                None if bt is None else (bt, bi), keep=True)
        assert torch.equal(out, want) and torch.equal(ids, bufs.batch_ids) and torch.equal(newest, bufs.newest)
        assert torch.equal(P, bufs.P) and torch.equal(w, bufs.weights) and torch.equal(Tm, bufs.T) and torch.equal(xn, bufs.xn)
        dy = T(p["dy"], dev)
        out.backward(dy)
        det = tuple(t.detach() for t in (table, ids, newest, xn, Tm, P, w))
        sg, dWqk, dWvo, dp = torch.ops.twotower.history_self_attention_bwd(*det, dy, Wqk.detach(), Wvo.detach())
        assert torch.equal(Wqk.grad, dWqk) and torch.equal(Wvo.grad, dWvo) and torch.equal(pp.grad, dp)
        sg2, q2, v2, p2 = ops.history_self_attention_bwd(bufs, dy, Wqk.detach(), Wvo.detach(),
                                                         slot_grads=torch.zeros(33 * L, dim, device=dev))
        assert torch.equal(sg, sg2) and torch.equal(dWqk, q2.sum(0)) and torch.equal(dWvo, v2.sum(0))
        assert torch.equal(dp, p2.sum(0).view(heads, L))
        saved = _reference(p)[3]
        ref = sc.backward(saved, p["dy"], p["Wqk"], p["Wvo"])
        assert not N(sg)[N(ids) < 0].any()                                             # the op's rows of skipped slots are zero
        for name, g in (("slot_grads", sg), ("dWqk", Wqk.grad), ("dWvo", Wvo.grad), ("dp", pp.grad)):
            print(dim, L, name, sc.within_bars(N(g), ref[name], name))
        torch.library.opcheck(torch.ops.twotower.history_self_attention_bwd, det + (dy, Wqk.detach(), Wvo.detach()))
    with pytest.raises(ValueError, match="go together"):
        torch.ops.twotower.history_self_attention(table, tok, rows, ex, T(p["table"], dev), None, Wqk, Wvo, pp)


def test_train_cli_runs_with_self_attention_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  features:\n    history:\n      max_items: 9\n      pooling: sqrtn\n      heads: 2\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    ck, recs = tmp_path / "a.pt", tmp_path / "a.parquet"
    with contextlib.redirect_stdout(io.StringIO()):                        # 600 pairs, 10 % held out: 2 training steps
        assert train.main(["--config", str(cfgp), "--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--optimizer", "adam", "--history-len", "4", "--history-pooling", "self_attention", "--history-heads", "4",
                           "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 2 and sd["adam_step"] == 3
    cf = sd["config"]
    assert (cf["user_history_len"], cf["history_pooling"], cf["history_heads"]) == (4, "self_attention", 4)   # the CLI over the YAML
    assert tuple(sd["history_table"].shape) == (200, 32) and tuple(sd["user_history"].shape) == (300, 4)
    n = 2 * 32 * 128 + 4 * 4
    assert sd["dense"][-n:].any().item() and sd["dense_m"][-n:].any().item() and sd["dense"][-16:].any().item()   # p trained
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
    got = pq.read_table(recs).to_pydict()
    assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all()
    # recommend scored the users' FULL stored histories: its scores are user_embeddings' (held to the restatement in the
    # inference test) against the corpus
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=1)
    tr.load_state_dict(sd)
    q = tr.user_embeddings(torch.arange(7, device=dev)).clone()
    top = (q @ tr.item_corpus_embeddings().t()).topk(5, dim=1)[0].cpu().numpy()
    order = np.lexsort((got["rank"], got["user_idx"]))
    assert np.abs(np.asarray(got["score"])[order].reshape(7, 5) - top).max() <= BAR * np.abs(top).max()
    # the YAML's own pooling and heads
    cfgp.write_text(cfgp.read_text().replace("pooling: sqrtn", "pooling: self_attention"))
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(["--config", str(cfgp), "--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--save", str(ck)]) == 0
    cf = torch.load(ck, weights_only=True)["config"]
    assert (cf["user_history_len"], cf["history_pooling"], cf["history_heads"]) == (9, "self_attention", 2)


# ------------------------------------------------------------------------------------------ 6. combinations and refusals
def test_combinations_and_refusals(dev):
    """The encoder beside the category, title, numeric and time features, cross layers, layer norm and the rating head (in two
    groups: the dense optimizer launches take 16 segments), under every optimizer; then the refusals."""
    seed = 31
    groups = (dict(n_category_buckets=7, n_title_buckets=50, title_max_tokens=4, n_user_features=3, n_item_features=2, layer_norm=True,
                   time_fields=("hour", "period"), time_buckets=4, time_min=0, time_max=10_000, normalize_embeddings=True),
              dict(cross_layers=1, rating_weight=0.5, rating_hidden=32, heads=8))
    for kw, segs in zip(groups, (8 + 3 + 2 + 1 + 1, 8 + 3 + 2 + 2)):
        for opt in ("sgd", "adagrad", "adam", "rowwise_adagrad"):
            tr = _sa_trainer(dev, opt, seed, **kw)
            assert len(tr._segs) == tr.cfg.dense_segment_count() == segs
            extra = {}
            if tr.sides:
                tr.set_user_features(tr.synthetic_user_features(seed)); tr.set_item_features(tr.synthetic_item_features(seed))
            u, i = tr.synthetic_batch(seed, 0, "Z")
            if tr.cat_table is not None:
                extra["category_ids"] = torch.arange(64, device=dev) % 7
            if tr.time_on:
                extra["timestamps"] = (torch.arange(64, device=dev, dtype=torch.int64) * 151) % 10_000
            if tr.rating_on:
                extra["ratings"] = torch.rand(64, device=dev) * 4 + 1
            q0 = tr.sa_Wqk.clone()
            losses = [tr.step(u, i, **extra).item() for _ in range(4)]
            tr.check_ids()
            assert np.isfinite(losses).all(), (opt, losses)
            assert not torch.equal(q0, tr.sa_Wqk) and torch.isfinite(tr.dense_flat).all() and torch.isfinite(tr.history_table).all()
    with pytest.raises(NotImplementedError, match="self-attention"):
        TwoTowerTrainer(_cfg("sgd", tower_dims=(128, 64, 32), user_history_len=4, history_pooling="self_attention", n_user_features=3,
                             n_item_features=3), dev, seed=1)
    with pytest.raises(ValueError, match="multiple of 32"):
        TwoTowerTrainer(_cfg("sgd", dim=48, user_history_len=4, history_pooling="self_attention"), dev, seed=1)
    with pytest.raises(ValueError, match="history_heads"):
        TwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="self_attention", history_heads=3), dev, seed=1)
    tr = _sa_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="history"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises((NotImplementedError, ValueError), match="history"):
        ShardedTwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="self_attention"), dev, seed=1)
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="self_attention", candidate_sampling="mixed",
                             n_sampled_negatives=64), dev, seed=1)

"""The GRU encoder of the user history on the GPU (tt_history_gru_resolve_f32 / tt_history_gru_fwd_f32 / tt_history_gru_bwd_f32,
csrc/history_gru.hip, and the GEMM launches around them): the forward against the f64 restatement of tests/gru_check.py within
the project's bars (relative <= 1e-4 in the 2-norm, max-abs <= 1e-4 * max|ref|: DESIGN section 2), the ids and the flag exactly,
the bitwise properties (padding is invisible, a bag's bits are its own, runs repeat, emptied bags and zero parameters give the
base row), the backward, the history table's update, then the trainer - parity with the f64 autograd restatement, training,
checkpoints, the inference paths, clipping - the custom ops, the CLIs, combinations and refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import bag_check as bc
import gru_check as gc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001
BAR = gc.BAR


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(bc.bits(np.asarray(a, dtype=np.float32)), bc.bits(np.asarray(b, dtype=np.float32)))


def _guarded_buffers(n_bags, L, dim, dev):
    """``ops.GruBuffers`` whose tensors are the leading part of longer ones filled with a sentinel: (buffers, the long tensors)."""
    big = ops.GruBuffers(n_bags + 1, L, dim, dev)
    m = n_bags * L
    long = {k: getattr(big, k) for k in ("batch_ids", "x", "gates", "gn", "hprev", "da", "dg")}
    for k, t in long.items():
        t.fill_(-7)
        setattr(big, k, t[:m])
    big.n_bags = n_bags
    big.long = long
    return big, long


def _tails_keep_the_sentinel(long, m):
    return all(bool((t[m:] == -7).all().item()) for t in long.values())


def _device_forward(dev, p, keep=True):
    """One forward on the device from a ``gru_check.forward_problem``: (out, ids, flag, buffers or None, tails intact)."""
    tok, bag_rows = p["tokens"], p["bag_rows"]
    n_bags = len(tok) if bag_rows is None else len(bag_rows)
    L, dim = tok.shape[1], p["table"].shape[1]
    out = torch.full((n_bags + 1, dim), 7.0, device=dev)
    ids = torch.full((n_bags * L + 3,), -7, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    base = None if p["base"] is None else (T(p["base"][0], dev), T(p["base"][1], dev))
    bufs, long = _guarded_buffers(n_bags, L, dim, dev) if keep else (False, {})
    res = ops.history_gru(T(p["table"], dev), T(tok, dev), T(p["W"], dev), T(p["U"], dev), T(p["b"], dev), T(bag_rows, dev),
                          T(p["exclude"], dev), base, out=out[:n_bags], batch_ids=ids[:n_bags * L], oob_flag=flag, keep=bufs)
    intact = bool((out[n_bags:] == 7).all().item()) and bool((ids[n_bags * L:] == -7).all().item())
    if keep:
        long.pop("batch_ids")                                                   # (the caller's ids took their place)
        intact = intact and _tails_keep_the_sentinel(long, n_bags * L)
    return N(out[:n_bags]), N(ids[:n_bags * L]), int(flag.item()), (res[1] if keep else None), intact


def _device_backward(dev, bufs, p):
    """The backward on the device into sentinel-filled outputs: (slot_grads, dW, dU, db - the slabs summed in f64 -, checks ok)."""
    n_bags, L, dim = bufs.n_bags, bufs.L, bufs.dim
    m, ns = n_bags * L, ops.dense_bwd_num_slabs(n_bags * L)
    nan = float("nan")
    sg = torch.full((m + 1, dim), nan, device=dev)
    dw, du = torch.full((ns + 1, dim, 3 * dim), nan, device=dev), torch.full((ns + 1, dim, 3 * dim), nan, device=dev)
    db = torch.full((2, ns, 3 * dim), nan, device=dev)
    bufs.da.fill_(nan), bufs.dg.fill_(nan)                                      # (views: the sentinel tails behind them stay)
    ops.history_gru_bwd(bufs, T(p["dy"], dev), T(p["W"], dev), T(p["U"], dev), slot_grads=sg[:m], dw_slabs=dw[:ns], du_slabs=du[:ns],
                        db_slabs=db)
    ok = all(bool(torch.isfinite(t).all().item()) for t in (sg[:m], dw[:ns], du[:ns], db, bufs.da, bufs.dg))      # written in full
    ok = ok and all(bool(torch.isnan(t).all().item()) for t in (sg[m:], dw[ns:], du[ns:]))                          # and not beyond
    ok = ok and _tails_keep_the_sentinel({k: bufs.long[k] for k in ("x", "gates", "gn", "hprev", "da", "dg")}, m)
    return N(sg[:m]), N(dw[:ns]).astype(np.float64).sum(0), N(du[:ns]).astype(np.float64).sum(0), N(db).astype(np.float64).sum(1), ok


def _forward_and_backward_within_bars(dev, shape, scale, worst):
    dim, nb, L, ind, base = shape
    p = gc.forward_problem(dim, nb, L, ind, base, scale)
    want_out, want_ids, want_flag, saved = gc.gru_forward(p["table"], p["tokens"], p["W"], p["U"], p["b"], p["bag_rows"], p["exclude"],
                                                          p["base"])
    out, ids, flag, bufs, intact = _device_forward(dev, p)
    assert np.array_equal(ids, want_ids) and flag == want_flag and intact, shape
    res = {"out": (out, want_out)}
    # the inference form (nothing kept) gives the same bits
    out2, ids2, flag2, _, intact2 = _device_forward(dev, p, keep=False)
    assert _same_bits(out, out2) and np.array_equal(ids, ids2) and flag2 == flag and intact2, shape
    sg, dW, dU, db, ok = _device_backward(dev, bufs, p)
    assert ok, shape
    assert not sg[want_ids < 0].any(), shape                                    # the rows of skipped slots are zero
    want = gc.gru_backward(saved, p["dy"], p["W"], p["U"])
    res.update(zip(("slot_grads", "dW", "dU", "db"), zip((sg, dW, dU, db), want)))
    for k, (g, w) in res.items():
        worst[k] = max(worst.get(k, 0.0), max(gc.within_bars(g, w, (k,) + shape + (scale,))))
    return p, saved, out


# ------------------------------------------------------------------------------------------ 1. forward and backward, the sweep
@pytest.mark.parametrize("dim", [32, 96, 128, 256])
def test_forward_and_backward_match_the_restatement(dev, dim):
    """Every shape of ``gru_check.SHAPES`` at this width - bags {1, 33, 300} x L {1, 2, 7, 64}, identity and indirect bag rows, with
    and without a base row, always with ``exclude`` - with rows, W and U ~ N(0, 1) / sqrt(dim), and the shapes with L <= 2 again
    with the parameters scaled by 20 (``gru_check.SATURATED_SHAPES`` says why not beyond): out, slot_grads and the summed slabs of
    dW, dU and db within the bars of the f64 restatement; batch_ids and the flag exactly; the rows of skipped slots zero; every
    output written in full and nothing past its end; the special bags (every slot valid, kept slots only in the oldest 8, only in
    the newest 8, a single kept slot, emptied bags) are bags 8..11, 1 and 7 of the 33- and 300-bag problems."""
    worst = {}
    for scale, shapes in ((1.0, gc.SHAPES), (gc.SATURATED_SCALE, gc.SATURATED_SHAPES)):
        for shape in shapes:
            if shape[0] == dim:
                _forward_and_backward_within_bars(dev, shape, scale, worst)
    print(dim, {k: f"{v:.2e}" for k, v in worst.items()})


def test_saturated_gates_are_saturated(dev):
    """The second set does what it is for: on the device as in the f64 restatement a share of the z and r of the scaled problem
    sits within 1e-3 of 0 or 1 - a pre-activation beyond +-6.9, which the plain problem (|pre-activation| of order 1) never has."""
    sat = lambda g: float(((g < 1e-3) | (g > 1 - 1e-3)).mean())
    share = {}
    for scale in (1.0, gc.SATURATED_SCALE):
        p = gc.forward_problem(32, 300, 2, True, True, scale)
        saved = gc.gru_forward(p["table"], p["tokens"], p["W"], p["U"], p["b"], p["bag_rows"], p["exclude"], p["base"])[3]
        _, ids, _, bufs, _ = _device_forward(dev, p)
        want = sat(np.concatenate([saved["z"][saved["valid"]], saved["r"][saved["valid"]]], 1))
        share[scale] = (sat(N(bufs.gates)[ids >= 0][:, :64]), want)
    print(share)
    assert share[1.0] == (0.0, 0.0)
    got, want = share[gc.SATURATED_SCALE]
    assert want > 0.1 and abs(got - want) <= 1e-3


def _flag_problem(what):
    """``forward_problem(32, 33, 7, indirect, base)`` (flag 0: its bag rows, tokens and base ids are valid or -1) with ONE kind of
    out-of-range entry, or all of them: bags 16 / 17 / 18 pool token rows 20 / 21 / 22, which nothing else touches."""
    p = gc.forward_problem(32, 33, 7, True, True)
    tok, rows, base_ids = p["tokens"].copy(), p["bag_rows"].copy(), p["base"][1].copy()
    tok[20:23] = np.arange(21).reshape(3, 7) + 30
    rows[16:19] = [20, 21, 22]
    rows[12:16] = [3, 4, 5, 6]
    base_ids[12:19] = [1, 2, 3, 4, 5, 6, 7]
    if what in ("token >= rows", "all"):
        tok[20, 1], tok[21, 6] = gc.ROWS, gc.ROWS + 1000
    if what in ("token < -1", "all"):
        tok[22, 0], tok[22, 3] = -5, -2
    if what in ("bag row >= rows", "all"):
        rows[12] = gc.TOKEN_ROWS
    if what in ("bag row < -1", "all"):
        rows[13] = -3
    if what in ("base id >= rows", "all"):
        base_ids[14] = 40
    if what in ("base id < -1", "all"):
        base_ids[15] = -4
    if what == "-1 only":
        tok[20, 1], tok[22, 0], rows[12], rows[13], base_ids[14], base_ids[15] = -1, -1, -1, -1, -1, -1
    p.update(tokens=tok, bag_rows=rows, base=(p["base"][0], base_ids))
    return p


@pytest.mark.parametrize("what", ["none", "-1 only", "token >= rows", "token < -1", "bag row >= rows", "bag row < -1", "base id >= rows",
                                  "base id < -1", "all"])
def test_out_of_range_entries_set_the_flag_and_count_as_skipped(dev, what):
    """Every path that raises the flag, one at a time and together: a token >= table_rows, a negative token other than -1 (the
    resolve launch), a bag row >= n_token_rows or < -1 (the resolve launch), a base id >= base_rows or < -1 (the recurrent
    launch).  The flag equals the restatement's - 1 with any of them, 0 with none and with -1 alone -, the slot ids are -1 there,
    the slot rows are zero rows, a bad base id gives a zero base row, and ``out`` meets the bars; the inference form (which takes
    its own template instantiation) raises the same flag."""
    p = _flag_problem(what)
    want_out, want_ids, want_flag, saved = gc.gru_forward(p["table"], p["tokens"], p["W"], p["U"], p["b"], p["bag_rows"], p["exclude"],
                                                          p["base"])
    assert want_flag == (0 if what in ("none", "-1 only") else 1)
    out, ids, flag, bufs, intact = _device_forward(dev, p)
    assert flag == want_flag and np.array_equal(ids, want_ids) and intact
    assert _same_bits(N(bufs.x), saved["x"].reshape(-1, 32).astype(np.float32))            # the table's rows, zeros where skipped
    gc.within_bars(out, want_out, what)
    out2, ids2, flag2, _, _ = _device_forward(dev, p, keep=False)
    assert flag2 == want_flag and np.array_equal(ids2, want_ids) and _same_bits(out, out2)
    ids7 = ids.reshape(33, 7)
    if what in ("token >= rows", "all"):
        assert ids7[16, 1] == -1 and ids7[17, 6] == -1 and not N(bufs.x).reshape(33, 7, 32)[16, 1].any()
    if what in ("token < -1", "all"):
        assert ids7[18, 0] == -1 and ids7[18, 3] == -1
    if what in ("bag row >= rows", "all"):
        assert (ids7[12] == -1).all() and _same_bits(out[12], p["base"][0][1])              # an emptied bag: the base row
    if what in ("bag row < -1", "all"):
        assert (ids7[13] == -1).all() and _same_bits(out[13], p["base"][0][2])
    if what in ("base id >= rows", "base id < -1", "all"):
        k = 14 if what != "base id < -1" else 15
        no_base = dict(p, base=None)
        assert _same_bits(out[k], _device_forward(dev, no_base, keep=False)[0][k])          # a zero base row: h alone


# ------------------------------------------------------------------------------------------ 2. bitwise properties
@pytest.mark.parametrize("dim,L,scale", [(32, 7, 1.0), (128, 64, 1.0), (256, 3, 1.0), (32, 7, gc.SATURATED_SCALE),
                                         (128, 64, gc.SATURATED_SCALE)])
def test_padding_is_invisible_and_emptied_bags_give_the_base_row(dev, dim, L, scale):
    """A bag's two kept items in slots (0, 2), (0, 1) or (L-2, L-1) give the same out bit for bit, with the second item kept by
    position or uncovered by ``exclude``; an all-padding bag, and a bag of one token excluded in every slot, give the base row
    itself; W = U = 0, b = 0 gives the base row for every bag; two runs are identical.  Also with the parameters scaled by 20 at
    L = 7 and 64 - saturated gates in a long recurrence, where no f64 bar can be held (``gru_check.SATURATED_SHAPES``) but every
    bitwise property can, with finite results forward and backward."""
    rng = np.random.default_rng([dim, L])
    p = gc.forward_problem(dim, 33, L, False, True, scale)
    tok = np.full((33, L), -1, dtype=np.int32)
    tok[0, 0], tok[0, 2] = 3, 9
    tok[1, 0], tok[1, 1] = 3, 9
    tok[2, L - 2], tok[2, L - 1] = 3, 9
    tok[3] = [3, 44, 9] + [44] * (L - 3)                                        # 44 is excluded: the same two items remain
    tok[5] = 11                                                                 # emptied by the exclusion
    tok[6:] = rng.integers(0, gc.ROWS - 1, (27, L))
    exclude = np.full(33, gc.ROWS - 1, dtype=np.int64)
    exclude[3], exclude[5] = 44, 11
    base_ids = p["base"][1].copy()
    base_ids[:6] = 7
    p.update(tokens=tok, exclude=exclude, base=(p["base"][0], base_ids))
    out, ids, flag, bufs, intact = _device_forward(dev, p)
    assert flag == 0 and (ids.reshape(33, L)[:4] >= 0).sum(1).tolist() == [2, 2, 2, 2]
    assert np.isfinite(out).all() and intact and np.abs(out[6:]).max() > 0.1
    back = _device_backward(dev, bufs, p)
    if scale == 1.0 or L <= 7:                                                  # (64 chaotic steps: the gradient itself overflows f32)
        assert back[4] and all(np.isfinite(x).all() for x in back[:4]) and not back[0][ids < 0].any()
    bufs2 = _device_forward(dev, p)[3]
    assert all(_same_bits(a, b) for a, b in zip(back[:4], _device_backward(dev, bufs2, p)[:4]))          # the backward repeats too
    for k in (1, 2, 3):
        assert _same_bits(out[0], out[k]), k
    assert not _same_bits(out[0], p["base"][0][7])
    assert _same_bits(out[4], p["base"][0][7]) and _same_bits(out[5], p["base"][0][7])
    again = _device_forward(dev, p)[0]
    assert _same_bits(out, again)
    zero = dict(p, W=np.zeros_like(p["W"]), U=np.zeros_like(p["U"]), b=np.zeros_like(p["b"]))
    out0 = _device_forward(dev, zero)[0]
    assert _same_bits(out0, p["base"][0][base_ids])


def test_a_bag_alone_equals_the_same_bag_inside_a_300_bag_launch(dev):
    """Plain parameters, and scaled by 20 at L = 7 and 64 (saturated gates in a long recurrence: bitwise properties only)."""
    S = gc.SATURATED_SCALE
    for dim, L, scale in ((32, 7, 1.0), (96, 64, 1.0), (256, 2, 1.0), (32, 7, S), (128, 64, S)):
        p = gc.forward_problem(dim, 300, L, True, True, scale)
        out, ids, _, _, _ = _device_forward(dev, p, keep=False)
        assert np.isfinite(out).all()
        for k in (0, 2, 8, 31, 32, 150, 299):
            one = dict(p, bag_rows=p["bag_rows"][k:k + 1], exclude=p["exclude"][k:k + 1], base=(p["base"][0], p["base"][1][k:k + 1]))
            o1, i1, _, _, _ = _device_forward(dev, one, keep=False)
            assert _same_bits(o1[0], out[k]) and np.array_equal(i1, ids[k * L:(k + 1) * L]), (dim, L, k)


def test_ops_argument_checks(dev):
    p = gc.forward_problem(32, 33, 7, True, True)
    a = [T(p[k], dev) for k in ("table", "tokens", "W", "U", "b")]
    rows, ex = T(p["bag_rows"], dev), T(p["exclude"], dev)
    with pytest.raises(RuntimeError, match="W and U must be"):
        ops.history_gru(a[0], a[1], a[2][:, :-1].contiguous(), a[3], a[4], rows)
    with pytest.raises(RuntimeError, match="exclude must hold"):
        ops.history_gru(*a, rows, ex[:-1])
    with pytest.raises(RuntimeError, match="base must be"):
        ops.history_gru(*a, rows, base=(T(p["base"][0], dev), T(p["base"][1][:-1], dev)))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.history_gru(torch.zeros(10, 36, device=dev), a[1], torch.zeros(36, 108, device=dev), torch.zeros(36, 108, device=dev),
                        torch.zeros(2, 108, device=dev), rows)
    with pytest.raises(RuntimeError, match="GruBuffers"):
        ops.history_gru(*a, rows, keep=ops.GruBuffers(5, 7, 32, dev))
    out, bufs = ops.history_gru(*a, rows, ex, keep=True)
    with pytest.raises(RuntimeError, match="dy must be"):
        ops.history_gru_bwd(bufs, torch.zeros(32, 32, device=dev), a[2], a[3])
    with pytest.raises(RuntimeError, match="dw_slabs must be"):
        ops.history_gru_bwd(bufs, torch.zeros(33, 32, device=dev), a[2], a[3], dw_slabs=torch.zeros(1, 32, 96, device=dev))


# ------------------------------------------------------------------------------------------ 3. the update
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_update_from_the_slot_rows_is_bit_exact(dev, opt):
    """slot_grads through a plain SparsePlan(n_bags * L) into SGD, Adagrad and lazy Adam: the table and its state equal the
    restatement's update of the same rows bit for bit; rows no kept slot names keep their bits."""
    rng = np.random.default_rng(5)
    n_bags, L, dim = 64, 7, 32
    table = rng.uniform(-0.05, 0.05, (60, dim)).astype(np.float32)
    tok = rng.integers(0, 50, (n_bags, L)).astype(np.int32)
    tok[rng.random((n_bags, L)) < 0.25] = -1
    tok[tok == 49] = 48
    tok[:, 0] = np.where(np.arange(n_bags) % 2 == 0, 49, tok[:, 0])               # token 49 only where it is excluded
    exclude = np.where(np.arange(n_bags) % 2 == 0, 49, 55).astype(np.int64)
    W, U, b = gc.params(rng, dim)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    state = [table]
    if opt == "adagrad":
        state = [table, np.full_like(table, 0.1)]
    elif opt == "adam":
        state = [table, (rng.standard_normal(table.shape) * 0.01).astype(np.float32),
                 ((rng.standard_normal(table.shape) * 0.01) ** 2).astype(np.float32)]
    d = [T(a, dev) for a in state]
    out, bufs = ops.history_gru(d[0], T(tok, dev), T(W, dev), T(U, dev), T(b, dev), exclude=T(exclude, dev), keep=True)
    sg = ops.history_gru_bwd(bufs, T(dy, dev), T(W, dev), T(U, dev))[0]
    ids = bufs.batch_ids
    plan = ops.SparsePlan(n_bags * L, dev)
    plan.run(ids, table.shape[0])
    if opt == "sgd":
        ops.sparse_sgd_(d[0], sg, plan, LR)
    elif opt == "adagrad":
        ops.sparse_adagrad_(d[0], d[1], sg, plan, LR)
    else:
        ops.adam_step_([(d[0], d[1], d[2], sg, plan)], [], ops.AdamHyper(lr=LR, step=7))
    want_ids = gc.gru_forward(table, tok, W, U, b, None, exclude)[1]
    assert np.array_equal(N(ids), want_ids) and (tok == 49).any() and not (want_ids == 49).any() and (want_ids == 48).any()
    want = [a.copy() for a in state]
    touched = bc.bag_update(opt, want, want_ids, N(sg), 1, LR, step=7)          # one gradient row per slot: "bags" of one slot
    for g, wnt, name in zip(d, want, ("table", "state 1", "state 2")):
        assert np.isfinite(N(g)).all() and _same_bits(N(g), wnt), (opt, name)
    rest = np.setdiff1d(np.arange(len(table)), touched)
    assert 49 in rest and len(rest) == 11
    for g, s0 in zip(d, state):
        assert _same_bits(N(g)[rest], s0[rest]) and not _same_bits(N(g)[touched], s0[touched])


# ------------------------------------------------------------------------------------------ 4. trainer
def _cfg(opt, batch=64, dim=32, tower_dims=(64, 32), n_users=100, n_items=400, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **kw)


def _gru_trainer(dev, opt="adagrad", seed=1001, pooling="gru", L=7, batches=3, **kw):
    """Histories from the pairs of the first synthetic batches (``data.user_histories``, file order): the steps' positives are in
    them."""
    tr = TwoTowerTrainer(_cfg(opt, user_history_len=L, history_pooling=pooling, **kw), dev, seed=seed)
    pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(batches)]
    u = torch.cat([p[0] for p in pairs]).cpu().numpy()
    i = torch.cat([p[1] for p in pairs]).cpu().numpy()
    tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, L), dev))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _set_bias(tr, seed):
    """Random biases (they start at zero) so that db_i and db_r are told apart from the first step on."""
    tr.gru_b.copy_(T((np.random.default_rng(seed).standard_normal(tuple(tr.gru_b.shape)) * 0.1).astype(np.float32), tr.dev))


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def _step_against_f64(tr, seed, step):
    """One forward_backward against ``gru_check.step_f64``: (the restatement's results, the step's ids, the checks as (name, got,
    want) with the device's gradients summed over their slabs in f64)."""
    cfg = tr.cfg
    L = cfg.user_history_len
    hist = N(tr.user_history)
    u, i = tr.synthetic_batch(seed, step, "Z")
    un, inn = N(u), N(i)
    before = {k: N(getattr(tr, k)).astype(np.float64) for k in ("user_table", "item_table", "history_table", "gru_W", "gru_U", "gru_b")}
    towers = _towers64(tr)
    loss = tr.forward_backward(u, i).item()
    tr.check_ids()
    masks = tuple([N(t.acts[l + 1] > 0) for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    r = gc.step_f64(before["user_table"], before["item_table"], before["history_table"], before["gru_W"], before["gru_U"],
                    before["gru_b"], towers, un, inn, hist, 0.1, masks)
    valid = hist[un] >= 0
    match = valid & (hist[un] == inn[:, None])
    ids = N(tr.history_ids)
    assert np.array_equal(ids.reshape(cfg.batch_size, L), np.where(valid & ~match, hist[un], -1))      # the leave-one-out rule
    sg = N(tr.history_slot_grads).astype(np.float64)
    assert not sg[ids < 0].any()
    g_hist = np.zeros_like(before["history_table"])
    np.add.at(g_hist, ids[ids >= 0], sg[ids >= 0])
    dw, du, db = (N(x).astype(np.float64) for x in tr._gru_slabs)
    checks = [("due", N(tr.user_tower.demb), r["due"]), ("die", N(tr.item_tower.demb), r["die"]), ("history_table", g_hist, r["history_table"]),
              ("dW", dw.sum(0), r["dW"]), ("dU", du.sum(0), r["dU"]), ("db", db.sum(1), r["db"])]
    return r, loss, (u, i, un, inn, ids, sg, match, valid), checks, before


@pytest.mark.parametrize("L", [1, 7])
def test_trainer_step_matches_the_f64_restatement(dev, L):
    """One step (and a second, from updated parameters) at batch 64, dim 32: the loss, due, the history table's gradient (the
    scatter-add of the slot rows), dW, dU and db within the bars of f64 torch autograd given the device's ReLU masks."""
    seed = 1001
    tr = _gru_trainer(dev, "sgd", seed, L=L)
    lay = tr.layout
    assert not tr.fuse_lookup and tr.gru_W.storage_offset() % 4 == 0 and not tr.gru_b.any() and tr.gru_W.any() and tr.gru_U.any()
    assert list(lay.blocks)[-3:] == ["history_gru.W", "history_gru.U", "history_gru.b"]
    assert len(tr._segs) == tr.cfg.dense_segment_count() == 8 + 4
    lim = np.sqrt(6.0 / (4 * 32))                                                # Glorot-uniform with fan D + 3D, both kernels
    for w in (tr.gru_W, tr.gru_U):
        assert 0.9 * lim < w.abs().max().item() <= lim
    assert not torch.equal(tr.gru_W, tr.gru_U)
    _set_bias(tr, 5)
    for step in range(2):
        r, loss, (u, i, un, inn, ids, sg, match, valid), checks, _ = _step_against_f64(tr, seed, step)
        print(f"L {L} step {step}: loss {loss} (f64 {r['loss']})")
        assert abs(loss - r["loss"]) <= BAR * abs(r["loss"]), (loss, r["loss"])
        assert match.any() and (valid & ~match).any()
        for what, got, want in checks:
            print(f"L {L} step {step}: {what}", gc.within_bars(got, want, (L, step, what)))
        w0, u0, b0 = tr.gru_W.clone(), tr.gru_U.clone(), tr.gru_b.clone()
        tr.apply_gradients(step_ids=[u, i])
        assert not torch.equal(w0, tr.gru_W) and not torch.equal(b0, tr.gru_b) and (L == 1 or not torch.equal(u0, tr.gru_U))


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam", "rowwise_adagrad"])
def test_thirty_steps_lower_the_loss(dev, opt):
    seed = 7
    tr = _gru_trainer(dev, opt, seed)
    batch0 = tr.synthetic_batch(seed, 0, "Z")
    t0, w0, u0 = tr.history_table.clone(), tr.gru_W.clone(), tr.gru_U.clone()
    losses = [tr.step(*batch0).item() for _ in range(30)]
    tr.check_ids()
    print(opt, f"{losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(t0, tr.history_table) and not torch.equal(w0, tr.gru_W) and not torch.equal(u0, tr.gru_U)
    assert tr.gru_b.any() and torch.isfinite(tr.dense_flat).all()


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17
    kw = dict(dropout_rate=0.1)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _gru_trainer(dev, opt, seed, **kw)
    run(a, range(4))
    b = _gru_trainer(dev, opt, seed, **kw)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["user_history_len"] == 7 and sd["config"]["history_pooling"] == "gru"
    mean = _gru_trainer(dev, opt, seed, pooling="mean", **kw)
    assert set(sd) == set(mean.state_dict()) and sd["dense"].numel() == mean.dense_flat.numel() + 2 * 32 * 96 + 2 * 96
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values, no histories set
    c.load_state_dict(sd)
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "history_table", "user_history", "loss", "gru_W", "gru_U", "gru_b"]
    if opt == "adam":
        names += ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "history_m", "history_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.gru_U, b.gru_U)
    with pytest.raises(ValueError, match="history_pooling"):
        mean.load_state_dict(sd)
    with pytest.raises(ValueError, match="history_pooling"):
        c.load_state_dict(mean.state_dict())


def test_inference_paths_encode_the_full_history(dev):
    """``evaluate``, ``user_embeddings`` (150 ids at batch 64: three chunks, the last ragged), ``evaluate_topk`` and the exact
    index's ``index_from_trainer`` + ``recommend`` feed the user tower user row + the GRU state over the FULL history - nothing
    left out - within the bars of the restatement, and not what the train step fed, where the positive was left out; an
    inference pass between a step's backward and its update changes nothing the update reads."""
    from two_tower_amazon_recommender_amd.metrics import FactorizedTopK
    seed = 23
    tr = _gru_trainer(dev, "sgd", seed)
    _set_bias(tr, 6)
    for s in range(2):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    u, i = tr.synthetic_batch(seed, 1, "Z")
    table, hist, users = N(tr.history_table), N(tr.user_history), N(tr.user_table)
    W, U, b = N(tr.gru_W), N(tr.gru_U), N(tr.gru_b)
    un = N(u)
    assert (hist[un] == N(i)[:, None]).any()                                  # the positives are there - and stay in
    want = gc.gru_forward(table, hist, W, U, b, un, None, (users, un))[0]
    train_in = gc.gru_forward(table, hist, W, U, b, un, N(i), (users, un))[0]
    assert np.abs(want - train_in).max() > 1e-2 * np.abs(want).max()
    tr.evaluate(u, i)
    print("evaluate", gc.within_bars(N(tr.user_tower.acts[0]), want, "evaluate"))
    q_eval = tr.user_tower.acts[-1].clone()
    tr.user_tower.acts[0].zero_()
    tr.evaluate_topk(u, i, FactorizedTopK(ks=(5,), temperature=0.1))
    print("evaluate_topk", gc.within_bars(N(tr.user_tower.acts[0]), want, "evaluate_topk"))
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 100, 150)).to(dev)
    emb = tr.user_embeddings(ids)
    tr.check_ids()
    idn = N(ids)
    last = gc.gru_forward(table, hist, W, U, b, idn[128:], None, (users, idn[128:]))[0]
    print("user_embeddings", gc.within_bars(N(tr.user_tower.acts[0][:22]), last, "user_embeddings"))
    assert emb.shape == (150, 32)
    err = (tr.user_embeddings(u) - q_eval).abs().max().item()
    assert err <= BAR * q_eval.abs().max().item(), err
    from two_tower_amazon_recommender_amd import serving
    q5 = tr.user_embeddings(u[:5]).clone()
    want_scores = (q5 @ tr.item_corpus_embeddings().t()).topk(3, dim=1)[0]
    for index in (serving.BruteForce(k=3), serving.Int8BruteForce(k=3), serving.IVF(k=3, nlist=4, nprobe=4),
                  serving.Int8IVF(k=3, nlist=4, nprobe=4)):                     # queries are user ids run through the user tower
        scores, items = index.index_from_trainer(tr)(u[:5])
        assert tuple(items.shape) == (5, 3) and torch.isfinite(scores).all()
        # every list probed, exact re-rank: the full-history queries' own top scores, not the leave-one-out ones'
        assert (scores - want_scores).abs().max().item() <= BAR * want_scores.abs().max().item(), type(index).__name__
    exact = serving.BruteForce(k=3).index(tr.item_corpus_embeddings())(q5)
    assert torch.equal(exact[1], serving.BruteForce(k=3).index_from_trainer(tr)(u[:5])[1])
    # predict_ratings: the head's pairs go through the same full-history user input
    trr = _gru_trainer(dev, "sgd", seed, rating_weight=0.5, rating_hidden=32)
    pred = trr.predict_ratings(u, i)
    want_r = gc.gru_forward(N(trr.history_table), N(trr.user_history), N(trr.gru_W), N(trr.gru_U), N(trr.gru_b), un, None,
                            (N(trr.user_table), un))[0]
    print("predict_ratings", gc.within_bars(N(trr.user_tower.acts[0]), want_r, "predict_ratings"))
    assert tuple(pred.shape) == (64,) and torch.isfinite(pred).all()
    # an inference pass between forward_backward and apply_gradients leaves the step's kept buffers alone
    tr2, tr3 = _gru_trainer(dev, "sgd", seed), _gru_trainer(dev, "sgd", seed)
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
    tr = _gru_trainer(dev, "sgd", seed, global_clipnorm=0.05)
    _set_bias(tr, 3)
    r, loss, (u, i, un, inn, ids, sg, match, valid), checks, before = _step_against_f64(tr, seed, 0)
    saved = gc.gru_forward(before["history_table"].astype(np.float32), N(tr.user_history), before["gru_W"], before["gru_U"],
                           before["gru_b"], un, inn)[3]
    slot = gc.gru_backward(saved, r["due"], before["gru_W"], before["gru_U"])[0]
    sq = (r["due"] ** 2).sum() + (r["die"] ** 2).sum() + (slot ** 2).sum() + sum((r[k] ** 2).sum() for k in ("dW", "dU", "db"))
    sq += sum((g ** 2).sum() for t in range(2) for g in r["dw"][t] + r["db_towers"][t])
    tr.clip_gradients()
    got, want = tr.grad_norm.item(), float(np.sqrt(sq))
    print("grad_norm", got, want, "scale", tr.clip_scale.item())
    assert abs(got - want) <= BAR * want and want > 0.05
    assert abs(tr.clip_scale.item() - 0.05 / want) <= BAR * 0.05 / want
    clipped = N(tr.history_slot_grads).astype(np.float64)
    print("clipped slot rows", gc.within_bars(clipped, slot * (0.05 / want), "clipped slot rows"))
    tr.apply_gradients(step_ids=[u, i])
    assert torch.isfinite(tr.dense_flat).all()


# ------------------------------------------------------------------------------------------ 5. custom ops, CLIs
def test_custom_ops_pass_opcheck_equal_the_ops_calls_and_differentiate_the_parameters(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    for dim, L, ind, base in ((32, 7, True, True), (64, 2, False, False)):
        p = gc.forward_problem(dim, 33, L, ind, base)
        table, tok = T(p["table"], dev), T(p["tokens"], dev)
        rows, ex = T(p["bag_rows"], dev), T(p["exclude"], dev)
        bt, bi = (None, None) if p["base"] is None else (T(p["base"][0], dev), T(p["base"][1], dev))
        W, U, b = (T(p[k], dev).requires_grad_(True) for k in ("W", "U", "b"))
        args = (table, tok, rows, ex, bt, bi, W, U, b)
        torch.library.opcheck(torch.ops.twotower.history_gru, args)
        out, ids, x, gates, gn, hprev = torch.ops.twotower.history_gru(*args)
        want, bufs = ops.history_gru(table, tok, W.detach(), U.detach(), b.detach(), rows, ex, None if bt is None else (bt, bi), keep=True)
        assert torch.equal(out, want) and torch.equal(ids, bufs.batch_ids) and torch.equal(gates, bufs.gates) and torch.equal(hprev, bufs.hprev)
        dy = T(p["dy"], dev)
        out.backward(dy)
        det = tuple(t.detach() for t in (ids, x, gates, gn, hprev))
        sg, dW, dU, db = torch.ops.twotower.history_gru_bwd(*det, dy, W.detach(), U.detach())
        assert torch.equal(W.grad, dW) and torch.equal(U.grad, dU) and torch.equal(b.grad, db)
        saved = gc.gru_forward(p["table"], p["tokens"], p["W"], p["U"], p["b"], p["bag_rows"], p["exclude"], p["base"])[3]
        ref = gc.gru_backward(saved, p["dy"], p["W"], p["U"])
        for name, g, w in zip(("slot rows", "dW", "dU", "db"), (sg, W.grad, U.grad, b.grad), ref):
            print(dim, L, name, gc.within_bars(N(g), w, name))
        torch.library.opcheck(torch.ops.twotower.history_gru_bwd, det + (dy, W.detach(), U.detach()))
    with pytest.raises(ValueError, match="go together"):
        torch.ops.twotower.history_gru(table, tok, rows, ex, T(p["table"], dev), None, W, U, b)


def test_train_cli_runs_with_the_gru_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
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
                           "--optimizer", "adam", "--history-len", "4", "--history-pooling", "gru", "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 2 and sd["adam_step"] == 3
    assert (sd["config"]["user_history_len"], sd["config"]["history_pooling"]) == (4, "gru")   # the CLI's pooling over the YAML's
    assert tuple(sd["history_table"].shape) == (200, 32) and tuple(sd["user_history"].shape) == (300, 4)
    n = 2 * 32 * 96 + 2 * 96
    assert sd["dense"][-n:].any().item() and sd["dense_m"][-n:].any().item() and sd["dense"][-192:].any().item()   # the biases trained
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
    # the YAML's own pooling value
    cfgp.write_text(cfgp.read_text().replace("pooling: sqrtn", "pooling: gru"))
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(["--config", str(cfgp), "--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert (sd["config"]["user_history_len"], sd["config"]["history_pooling"]) == (9, "gru")


# ------------------------------------------------------------------------------------------ 6. combinations and refusals
def test_combinations_and_refusals(dev):
    """The GRU beside the category, title, numeric and time features, cross layers, layer norm and the rating head (in two
    groups: the dense optimizer launches take 16 segments), under every optimizer; then the refusals."""
    seed = 31
    groups = (dict(n_category_buckets=7, n_title_buckets=50, title_max_tokens=4, n_user_features=3, n_item_features=2, layer_norm=True,
                   time_fields=("hour", "period"), time_buckets=4, time_min=0, time_max=10_000, normalize_embeddings=True),
              dict(cross_layers=1, rating_weight=0.5, rating_hidden=32))
    for kw, segs in zip(groups, (8 + 4 + 2 + 1 + 1, 8 + 4 + 2 + 2)):
        for opt in ("sgd", "adagrad", "adam", "rowwise_adagrad"):
            tr = _gru_trainer(dev, opt, seed, **kw)
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
            w0 = tr.gru_W.clone()
            losses = [tr.step(u, i, **extra).item() for _ in range(4)]
            tr.check_ids()
            assert np.isfinite(losses).all(), (opt, losses)
            assert not torch.equal(w0, tr.gru_W) and torch.isfinite(tr.dense_flat).all() and torch.isfinite(tr.history_table).all()
    with pytest.raises(NotImplementedError, match="GRU"):
        TwoTowerTrainer(_cfg("sgd", tower_dims=(128, 64, 32), user_history_len=4, history_pooling="gru", n_user_features=3), dev, seed=1)
    with pytest.raises(ValueError, match="multiple of 32"):
        TwoTowerTrainer(_cfg("sgd", dim=48, user_history_len=4, history_pooling="gru"), dev, seed=1)
    tr = _gru_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="history"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises((NotImplementedError, ValueError), match="history"):
        ShardedTwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="gru"), dev, seed=1)
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerTrainer(_cfg("sgd", user_history_len=4, history_pooling="gru", candidate_sampling="mixed", n_sampled_negatives=64),
                        dev, seed=1)

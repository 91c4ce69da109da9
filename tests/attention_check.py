"""Restatements of the history-attention contract of include/twotower_hip.h (tt_history_attention_fwd_f32 /
tt_history_attention_bwd_f32) and of the train step with history_pooling="attention", shared by
tests/test_history_attention_cpu.py and tests/test_gpu_history_attention.py.

* ``attention_forward`` is the forward in f64 NumPy on the f32 inputs, on top of ``history_check.mask_tokens``: for the valid
  slots j of a bag r_j = valid slots behind j, e_j = <h_j, a> / sqrt(dim) + p[r_j], w = softmax(e), out = base row + sum w_j h_j.
  The device takes the exponential in hardware, so it is compared within the project's bars, not bit for bit.
* ``attention_backward`` is the closed form the backward launch computes; tests/test_history_attention_cpu.py holds it to f64
  torch autograd of ``attention_forward_torch``.
* ``step_f64`` is ``history_check.step_f64`` with the attention pool.
* ``problem`` builds the special bags of a forward problem, ``backward_problem`` a whole backward problem for one shape;
  ``attention_backward_f32`` is the closed form in float32, ``attention_dattn_per_bag`` its da / dp terms bag by bag (what a
  slab of the backward launch sums), ``backward_launch_shape`` the form the launch code picks for a shape and ``errs`` the two
  error measures of the project's bars.
"""
import numpy as np

import history_check as hc

BAR = 1e-4                     # relative error in the 2-norm <= BAR and max-abs error <= BAR * max|ref|


def errs(got, want, zero_scale=None):
    """(max-abs error / max|ref|, relative error in the 2-norm) against an f64 reference.  A reference that is zero in every
    entry but for its own rounding - at most 1e-9 of ``zero_scale``, the size of its terms (``uncancelled_scales``) - has
    neither: both measures are then max|got - want| / zero_scale."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale, norm = np.abs(want).max(), np.sqrt((want ** 2).sum())
    assert np.isfinite(got).all()
    if zero_scale is not None and scale <= 1e-9 * zero_scale:
        assert zero_scale > 0
        return np.abs(got - want).max() / zero_scale, np.abs(got - want).max() / zero_scale
    assert scale > 0
    return np.abs(got - want).max() / scale, np.sqrt(((got - want) ** 2).sum()) / norm


def ranks(valid):
    """r[b, j] = number of valid slots behind slot j of bag b (meaningful where valid)."""
    v = valid.astype(np.int64)
    return v[:, ::-1].cumsum(1)[:, ::-1] - v


def attention_forward(table, tokens, attn, bag_rows=None, exclude=None, base=None):
    """Returns (out [n_bags, dim], weights [n_bags, L], pooled [n_bags, dim], batch_ids int64 [n_bags * L], flag 0/1), all f64
    but the ids.  ``attn`` = [a (dim) | p (L)]; ``base`` = (base_table, base_ids) or None."""
    per_bag, flag = hc.mask_tokens(tokens, bag_rows, exclude)
    table = np.asarray(table)
    rows, dim = table.shape
    L = per_bag.shape[1]
    tok = per_bag.astype(np.int64)
    valid = (tok >= 0) & (tok < rows)
    flag |= int((~valid & (tok != -1)).any())
    batch_ids = np.where(valid, tok, -1)
    a, p = np.asarray(attn, dtype=np.float64)[:dim], np.asarray(attn, dtype=np.float64)[dim:dim + L]
    h = table.astype(np.float64)[np.where(valid, tok, 0)]                          # [n_bags, L, dim]
    e = h @ a / np.sqrt(float(dim)) + p[np.clip(ranks(valid), 0, L - 1)]
    e = np.where(valid, e, -np.inf)
    m = np.where(valid.any(1), e.max(1, initial=-np.inf), 0.0)
    x = np.where(valid, np.exp(np.where(valid, e - m[:, None], 0.0)), 0.0)
    den = x.sum(1)
    w = x / np.where(den > 0, den, 1.0)[:, None]
    pooled = (w[:, :, None] * h).sum(1)
    out = pooled.copy()
    if base is not None:
        base_table, base_ids = base
        base_ids = np.asarray(base_ids, dtype=np.int64)
        ok = (base_ids >= 0) & (base_ids < len(base_table))
        flag |= int((~ok & (base_ids != -1)).any())
        b0 = np.zeros_like(pooled)
        b0[ok] = np.asarray(base_table, dtype=np.float64)[base_ids[ok]]
        out = b0 + pooled
    return out, w, pooled, batch_ids.reshape(-1), int(flag)


def _backward_terms(table, batch_ids, weights, pooled, dy, attn, L, dtype):
    """(valid, h, g, w, a, s, de) of the closed form, every operand and every operation in ``dtype``."""
    table = np.asarray(table, dtype=dtype)
    dim = table.shape[1]
    ids = np.asarray(batch_ids).reshape(-1, L)
    valid = ids >= 0
    h = table[np.where(valid, ids, 0)] * valid[:, :, None]
    g = np.asarray(dy, dtype=dtype)
    w = np.asarray(weights, dtype=dtype) * valid
    a = np.asarray(attn, dtype=dtype)[:dim]
    s = dtype(1.0) / np.sqrt(dtype(dim))
    G = (g * np.asarray(pooled, dtype=dtype)).sum(1)
    t = np.matmul(h, g[:, :, None])[:, :, 0]
    de = w * (t - G[:, None])
    return valid, h, g, w, a, s, de


def _backward(table, batch_ids, weights, pooled, dy, attn, L, dtype):
    valid, h, g, w, a, s, de = _backward_terms(table, batch_ids, weights, pooled, dy, attn, L, dtype)
    dim = h.shape[2]
    dh = w[:, :, None] * g[:, None, :] + de[:, :, None] * (a * s)[None, None, :]
    dh = dh * valid[:, :, None]
    da = (de.reshape(-1) @ h.reshape(-1, dim)) * s
    dp = np.zeros(L, dtype=dtype)
    np.add.at(dp, ranks(valid)[valid], de[valid])
    return dh.reshape(-1, dim), da, dp, de


def attention_backward(table, batch_ids, weights, pooled, dy, attn, L):
    """The closed form: (slot_grads [n_bags * L, dim] - zero rows for the skipped slots -, da [dim], dp [L], de [n_bags, L])."""
    return _backward(table, batch_ids, weights, pooled, dy, attn, L, np.float64)


def attention_backward_f32(table, batch_ids, weights, pooled, dy, attn, L):
    """``attention_backward`` with every operand rounded to float32 and every operation in float32 (NumPy's summation order):
    what the formulas themselves lose at that precision, whatever order a kernel sums in."""
    out = _backward(table, batch_ids, weights, pooled, dy, attn, L, np.float32)
    assert all(x.dtype == np.float32 for x in out)
    return out


def attention_dattn_per_bag(table, batch_ids, weights, pooled, dy, attn, L):
    """(da [n_bags, dim], dp [n_bags, L]) in f64: every bag's own terms of the closed form's da and dp - a slab of the backward
    launch holds their sum over its bags."""
    valid, h, _, _, _, s, de = _backward_terms(table, batch_ids, weights, pooled, dy, attn, L, np.float64)
    da = np.matmul(de[:, None, :], h)[:, 0, :] * s
    dp = np.zeros_like(de)
    b, j = np.nonzero(valid)
    dp[b, ranks(valid)[b, j]] = de[b, j]                                           # (a bag's ranks are distinct)
    return da, dp


def uncancelled_scales(table, batch_ids, weights, pooled, dy, L):
    """(max over the entries of da, max over the ranks of dp) of the sums the closed form would give if nothing cancelled:
    de_j = w_j (t_j - G) with |t_j| + |G| in place of the difference and |h_j| in place of h_j.  A bag with ONE kept slot has
    w = 1 and pooled = h, so t = G and its de is 0: at L = 1, or with one-hot weights, da and dp are zero in every entry, and what
    a float32 evaluation leaves there is rounding of t and of G - it is held to the bar of THIS scale, the size of the terms."""
    table = np.asarray(table, dtype=np.float64)
    dim = table.shape[1]
    ids = np.asarray(batch_ids).reshape(-1, L)
    valid = ids >= 0
    h = np.abs(table[np.where(valid, ids, 0)]) * valid[:, :, None]
    g = np.asarray(dy, dtype=np.float64)
    G = np.abs((g * np.asarray(pooled, dtype=np.float64)).sum(1))
    t = np.abs(np.matmul(table[np.where(valid, ids, 0)], g[:, :, None])[:, :, 0])
    de = np.abs(np.asarray(weights, dtype=np.float64)) * valid * (t + G[:, None])
    dp = np.zeros(L)
    np.add.at(dp, ranks(valid)[valid], de[valid])
    return float(((de.reshape(-1) @ h.reshape(-1, dim)) / np.sqrt(float(dim))).max()), float(dp.max())


def backward_launch_shape(dim, L):
    """(lpr, NV, KF, threads, chunks) of the backward launch for a shape, restated from ``lane_group`` and the launch code of
    csrc/history_attn.hip: a group of lpr lanes (the power of two >= dim / 4, at most 64) owns a bag, NV float4 per lane, KF rows
    in flight, a 256-thread workgroup halved while its groups' LDS lines exceed 48 KiB, the slots walked in chunks of lpr."""
    dim4, lg = dim // 4, 0
    while (1 << lg) < dim4 and lg < 6:
        lg += 1
    lpr = 1 << lg
    nv = -(-dim4 // lpr)
    threads = 256
    while threads > 64 and (threads >> lg) * (dim + L) * 4 > 48 * 1024:
        threads >>= 1
    return lpr, nv, 2 if nv >= 3 else 4, threads, -(-L // lpr)


def attention_forward_torch(table, tok, attn, base_rows=None):
    """The forward on torch tensors (any float dtype, differentiable): ``tok`` [n_bags, L] int64, already masked (-1 = skipped)."""
    import torch
    rows, dim = table.shape
    L = tok.shape[1]
    valid = (tok >= 0) & (tok < rows)
    a, p = attn[:dim], attn[dim:dim + L]
    h = table[tok.clamp(0, rows - 1)]
    v = valid.to(torch.int64)
    r = v.flip(1).cumsum(1).flip(1) - v
    e = h @ a / float(np.sqrt(float(dim))) + p[r.clamp(0, L - 1)]
    e = torch.where(valid, e, torch.full_like(e, -1e300))
    w = torch.softmax(e, dim=1) * valid
    pooled = (w[:, :, None] * h).sum(1)
    return (pooled if base_rows is None else base_rows + pooled), w, pooled


def step_f64(user_table, item_table, history_table, attn, towers, user_ids, item_ids, user_history, temperature, relu_masks):
    """``history_check.step_f64`` with the attention pool: f64 torch-CPU autograd of one step, the positive of every pair left out
    of its bag, the ReLU masks handed in.  Returns the loss and the gradients w.r.t. both towers' inputs and outputs, the tables
    (dense [rows, dim]), attn (``da`` [dim], ``dp`` [L]) and every kernel and bias."""
    import torch
    f = lambda x: torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    ut, it, hb, at = f(user_table), f(item_table), f(history_table), f(attn)
    uid, iid = torch.from_numpy(np.asarray(user_ids)), torch.from_numpy(np.asarray(item_ids))
    tok = torch.from_numpy(np.asarray(user_history).astype(np.int64))[uid]
    tok = torch.where(tok == iid[:, None], torch.full_like(tok, -1), tok)                # leave-one-out
    ue = attention_forward_torch(hb, tok, at, ut[uid])[0]
    ie = it[iid]
    ue.retain_grad(); ie.retain_grad()
    params, outs = [], []
    for x, (ws, bs), masks in ((ue, towers[0], relu_masks[0]), (ie, towers[1], relu_masks[1])):
        ws, bs = [f(w) for w in ws], [f(b) for b in bs]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                x = x * torch.from_numpy(np.asarray(masks[l], dtype=np.float64))
        params.append((ws, bs))
        outs.append(x)
    for o in outs:
        o.retain_grad()
    s = outs[0] @ outs[1].t() / temperature
    loss = (torch.logsumexp(s, dim=1) - s.diagonal()).sum()
    loss.backward()
    g = lambda t: t.grad.numpy()
    dim = np.asarray(history_table).shape[1]
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]), user_table=g(ut), item_table=g(it),
                history_table=g(hb), da=g(at)[:dim], dp=g(at)[dim:],
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b) for b in bs] for _, bs in params])


def problem(rng, n_rows, n_bags, L, rows, indirect):
    """(tokens [n_rows, L], bag_rows or None, exclude [n_bags]) - the special bags of tests/test_gpu_history.py.  Tokens lie in
    [0, rows - 1): token rows - 1 stands in no bag.  Bags 0..7 (bag b pools token row b, bag 7 - indirect only - the row -1):
      0 padding in the middle, an exclude value that is in range and matches nothing     4 as 1, but exclude = -1
      1 one token in every slot, excluded: a repeated match and an emptied bag           5 exclude >= rows (matches nothing, no flag)
      2 the match in the first valid slot (L >= 3: behind a padding slot)                6 random tokens, the in-range no-match value
      3 the match in the last valid slot (L >= 3: in front of a padding slot)
    The other bags exclude a slot of their own row (a padding slot: -1) half of the time, a random item otherwise.  Fewer than
    8 bags: the first of the special ones."""
    tok = rng.integers(0, rows - 1, (n_rows, L)).astype(np.int32)
    tok[rng.random((n_rows, L)) < 0.25] = -1
    tok[8:][rng.random(n_rows - 8) < 0.1] = -1
    tok[0:7] = rng.integers(0, rows - 1, (7, L))
    tok[1], tok[4] = 11, 12
    tok[2, -1] = tok[2, 0]
    tok[2, 1:-1] = np.where(tok[2, 1:-1] == tok[2, 0], tok[2, 0] + 1, tok[2, 1:-1])
    if L >= 3:
        tok[0, 1] = -1
        tok[2, 0], tok[2, 1], tok[2, -1] = -1, 21, 22
        tok[2, 2:-1] = np.where(tok[2, 2:-1] == 21, 23, tok[2, 2:-1])
        tok[3, -1], tok[3, -2] = -1, 31
        tok[3, :-2] = np.where(tok[3, :-2] == 31, 32, tok[3, :-2])
    bag_rows = None
    if indirect:
        bag_rows = rng.integers(0, n_rows, n_bags).astype(np.int64)
        bag_rows[rng.random(n_bags) < 0.08] = -1
        bag_rows[:8] = [0, 1, 2, 3, 4, 5, 6, -1][:n_bags]
    br = np.arange(n_bags) if bag_rows is None else bag_rows
    own = tok[np.maximum(br, 0), rng.integers(0, L, n_bags)].astype(np.int64)
    exclude = np.where(rng.random(n_bags) < 0.5, own, rng.integers(0, rows, n_bags))
    first3 = tok[3][tok[3] >= 0]
    exclude[:7] = [rows - 1, 11, tok[2][tok[2] >= 0][0], first3[-1], -1, rows + 5, rows - 1][:n_bags]
    return tok, bag_rows, exclude.astype(np.int64)


SWEEP_DIMS, SWEEP_LS, SWEEP_BAGS = (4, 36, 128, 256, 516, 1024), (1, 7, 37, 64), (1, 37, 300)
NV2_SHAPES = ((260, 37, 37), (512, 64, 37))         # (dim, L, n_bags) with two float4 per lane, which no dim of the sweep has
ROWS, TOKEN_ROWS = 97, 50


def backward_problem(dim, L, n_bags, seed=0):
    """One deterministic backward problem: dict(table [97, dim], tokens [50, L], bag_rows [n_bags] (indirect, some -1), exclude,
    dy [n_bags, dim], attn = [a | p]) with the values of the update problem of tests/test_gpu_history_attention.py - rows
    uniform(-0.05, 0.05), dy 0.01 N(0, 1), a = 20 N(0, 1) (sharp but finite logits), p ~ N(0, 1): distinct per rank, so a slot
    counted at a wrong rank shows in dp.  The bags are ``problem``'s, and behind its special ones
      bag 8   every slot valid, nothing excluded: the most ranks, every chunk of the backward's slot loop
      bag 9   valid slots in the OLDEST chunk only - the first min(lpr, 8) slots - (the backward meets them in its last chunk, at rank 0)
      bag 10  valid slots in the NEWEST chunk only - the last <= 8 slots, none in front of the chunk's first slot -
    where lpr is the launch's lane group for ``dim`` (``backward_launch_shape``).  Fewer than 11 bags: bag 0 is the full one."""
    rng = np.random.default_rng([seed, dim, L, n_bags])
    tok, bag_rows, exclude = problem(rng, TOKEN_ROWS, n_bags, L, ROWS, True)
    lpr = backward_launch_shape(dim, L)[0]
    last_chunk = (L - 1) // lpr * lpr
    old, new = min(lpr, 8, L), max(last_chunk, L - 8)
    tok[8:11] = rng.integers(0, ROWS - 1, (3, L))
    tok[9, old:] = -1
    tok[10, :new] = -1
    if n_bags >= 11:
        bag_rows[8:11], exclude[8:11] = [8, 9, 10], [ROWS - 1, -1, ROWS + 5]
    else:
        bag_rows[0], exclude[0] = 8, ROWS - 1
    table = rng.uniform(-0.05, 0.05, (ROWS, dim)).astype(np.float32)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    attn = np.concatenate([20.0 * rng.standard_normal(dim), rng.standard_normal(L)]).astype(np.float32)
    assert len(np.unique(attn[dim:])) == L
    # what the issue asks of the bags, on the slots the forward keeps
    kept = hc.mask_tokens(tok, bag_rows, exclude)[0] >= 0
    if L >= 3:
        assert kept.all(1).any()
    if L > 8 and n_bags >= 11:
        assert kept[9, :old].all() and not kept[9, old:].any() and kept[10, new:].all() and not kept[10, :new].any()
        assert old <= lpr and new >= last_chunk
    return dict(table=table, tokens=tok, bag_rows=bag_rows, exclude=exclude, dy=dy, attn=attn)

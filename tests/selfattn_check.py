"""Restatements of the history self-attention contract of include/twotower_hip.h (tt_history_self_attention_*_f32 and the GEMMs
around them) and of the train step with history_pooling="self_attention", shared by tests/test_history_self_attention_cpu.py and
tests/test_gpu_history_self_attention.py.

* ``forward`` is the forward in f64 NumPy on the f32 inputs, on top of ``history_check.mask_tokens`` and
  ``attention_check.ranks``: the newest kept slot n of a bag is the query, T = x_n Wqk, e_hj = <x_j, T_h> / sqrt(dim) + p[h, r_j],
  w_h = softmax_j(e_h), P_h = sum_j w_hj x_j, out = base row + concat_h(P_h) Wvo.
* ``backward`` is the closed form the backward launches compute; tests/test_history_self_attention_cpu.py holds it to f64 torch
  autograd of ``forward_torch``.
* ``forward_f32`` / ``backward_f32`` are the same formulas with every operand and every operation in float32 (NumPy's summation
  order): what the formulas themselves lose at that precision, whatever order a kernel sums in.
* ``per_bag_terms`` gives every bag's own dp and dT terms (a slab of the pool backward holds the dp sum over its bags),
  ``uncancelled_scales`` the size of the sums behind entries that are pure cancellation (one-kept-slot bags, L = 1).
* ``step_f64`` is ``history_check.step_f64`` with this encoder; ``forward_problem`` the problems of the GPU sweep.
"""
import numpy as np

import attention_check as ac
import history_check as hc

BAR = ac.BAR
errs = ac.errs
problem = ac.problem
HEADS = (1, 2, 4, 8)


def resolve(table, tokens, bag_rows=None, exclude=None):
    """(valid [n_bags, L], tok int64 [n_bags, L] - -1 where skipped -, newest [n_bags] - the last kept slot, -1 for none -, flag)."""
    per_bag, flag = hc.mask_tokens(tokens, bag_rows, exclude)
    tok = per_bag.astype(np.int64)
    valid = (tok >= 0) & (tok < len(table))
    flag |= int((~valid & (tok != -1)).any())
    L = valid.shape[1]
    newest = np.where(valid.any(1), L - 1 - np.argmax(valid[:, ::-1], axis=1), -1)
    return valid, np.where(valid, tok, -1), newest, int(flag)


def _forward(table, valid, tok, newest, Wqk, Wvo, p, dtype):
    """(O [n_bags, dim], saved) with every operand and operation in ``dtype``."""
    table, Wqk, Wvo, p = (np.asarray(t, dtype=dtype) for t in (table, Wqk, Wvo, p))
    n_bags, L = valid.shape
    d, H = table.shape[1], p.shape[0]
    some = newest >= 0
    x = np.where(valid[:, :, None], table[np.where(valid, tok, 0)], dtype(0))          # (a skipped slot: +0)
    xn = np.where(some[:, None], x[np.arange(n_bags), np.maximum(newest, 0)], dtype(0))
    T = (xn @ Wqk).reshape(n_bags, H, d)
    s = dtype(1.0) / np.sqrt(dtype(d))
    r = np.clip(ac.ranks(valid), 0, L - 1)
    v3 = valid[:, None, :]
    e = np.einsum("bld,bhd->bhl", x, T) * s + np.transpose(p[:, r], (1, 0, 2))
    e = np.where(v3, e, dtype(-np.inf))
    m = np.where(some[:, None], e.max(2, initial=-np.inf), dtype(0))
    ex = np.where(v3, np.exp(np.where(v3, e - m[:, :, None], dtype(0))), dtype(0))
    den = ex.sum(2)
    w = ex / np.where(den > 0, den, dtype(1))[:, :, None]
    P = np.einsum("bhl,bld->bhd", w, x)
    O = P.reshape(n_bags, H * d) @ Wvo
    saved = dict(x=x, xn=xn, T=T, w=w, P=P)
    assert all(val.dtype == dtype for val in saved.values()) and O.dtype == dtype
    saved.update(valid=valid, newest=newest, ranks=r)
    return O, saved


def _with_base(O, some, base, dtype):
    flag, out = 0, O
    if base is not None:
        base_table, base_ids = base
        base_ids = np.asarray(base_ids, dtype=np.int64)
        ok = (base_ids >= 0) & (base_ids < len(base_table))
        flag = int((~ok & (base_ids != -1)).any())
        rows = np.zeros_like(O)
        rows[ok] = np.asarray(base_table, dtype=dtype)[base_ids[ok]]
        out = np.where(some[:, None], rows + O, rows)                                   # an emptied bag: the base row itself
    return out, flag


def _run_forward(table, tokens, Wqk, Wvo, p, bag_rows, exclude, base, dtype):
    valid, tok, newest, flag = resolve(table, tokens, bag_rows, exclude)
    O, saved = _forward(table, valid, tok, newest, Wqk, Wvo, p, dtype)
    out, f2 = _with_base(O, newest >= 0, base, dtype)
    return out, tok.reshape(-1), int(flag | f2), saved


def forward(table, tokens, Wqk, Wvo, p, bag_rows=None, exclude=None, base=None):
    """Returns (out [n_bags, dim] f64, batch_ids int64 [n_bags * L], flag 0/1, saved) - ``saved`` (x, xn, T [n_bags, H, dim], w
    [n_bags, H, L], P [n_bags, H, dim], valid, newest, ranks) is what ``backward`` takes.  ``Wqk`` [dim, H dim], ``Wvo``
    [H dim, dim], ``p`` [H, L]; ``base`` = (base_table, base_ids)."""
    return _run_forward(table, tokens, Wqk, Wvo, p, bag_rows, exclude, base, np.float64)


def forward_f32(table, tokens, Wqk, Wvo, p, bag_rows=None, exclude=None, base=None):
    return _run_forward(table, tokens, Wqk, Wvo, p, bag_rows, exclude, base, np.float32)


def _backward_terms(saved, dy, Wvo, dtype):
    x, w, P = (np.asarray(saved[k], dtype=dtype) for k in ("x", "w", "P"))
    n_bags, H, d = P.shape
    dy = np.asarray(dy, dtype=dtype)
    dP = (dy @ np.asarray(Wvo, dtype=dtype).T).reshape(n_bags, H, d)
    G = (dP * P).sum(2)
    t = np.einsum("bhd,bld->bhl", dP, x)
    de = w * (t - G[:, :, None])
    return x, w, P, dy, dP, G, t, de


def _backward(saved, dy, Wqk, Wvo, dtype):
    x, w, P, dy, dP, G, t, de = _backward_terms(saved, dy, Wvo, dtype)
    Wqk = np.asarray(Wqk, dtype=dtype)
    xn, T = np.asarray(saved["xn"], dtype=dtype), np.asarray(saved["T"], dtype=dtype)
    valid, newest, r = saved["valid"], saved["newest"], saved["ranks"]
    n_bags, H, d = P.shape
    L = valid.shape[1]
    s = dtype(1.0) / np.sqrt(dtype(d))
    dWvo = P.reshape(n_bags, H * d).T @ dy
    dT = np.einsum("bhl,bld->bhd", de, x) * s
    dxn = dT.reshape(n_bags, H * d) @ Wqk.T
    dWqk = xn.T @ dT.reshape(n_bags, H * d)
    dx = np.einsum("bhl,bhd->bld", w, dP) + np.einsum("bhl,bhd->bld", de, T * s)
    some = newest >= 0
    dx[np.nonzero(some)[0], newest[some]] += dxn[some]
    dx = dx * valid[:, :, None]
    dp = np.zeros((H, L), dtype=dtype)
    b, j = np.nonzero(valid)
    for h in range(H):
        np.add.at(dp[h], r[b, j], de[b, h, j])
    out = dict(slot_grads=dx.reshape(n_bags * L, d), dWqk=dWqk, dWvo=dWvo, dp=dp, dP=dP.reshape(n_bags, H * d),
               dT=dT.reshape(n_bags, H * d), dxn=dxn, de=de)
    assert all(val.dtype == dtype for val in out.values())
    return out


def backward(saved, dy, Wqk, Wvo):
    """The closed form: dict(slot_grads [n_bags * L, dim] - zero rows for the skipped slots -, dWqk [dim, H dim], dWvo
    [H dim, dim], dp [H, L], and the intermediates dP, dT [n_bags, H dim], dxn [n_bags, dim], de [n_bags, H, L])."""
    return _backward(saved, dy, Wqk, Wvo, np.float64)


def backward_f32(saved, dy, Wqk, Wvo):
    return _backward(saved, dy, Wqk, Wvo, np.float32)


def per_bag_terms(saved, dy, Wvo):
    """(dp [n_bags, H, L], dT [n_bags, H dim]) in f64: every bag's own terms - a dp slab of the pool backward launch holds the sum
    of dp over its contiguous bags, dT is written bag by bag."""
    x, w, P, dy, dP, G, t, de = _backward_terms(saved, dy, Wvo, np.float64)
    valid, r = saved["valid"], saved["ranks"]
    n_bags, H, d = P.shape
    dp = np.zeros_like(de)
    b, j = np.nonzero(valid)
    dp[b, :, r[b, j]] = de[b, :, j]                                                     # (a bag's ranks are distinct)
    dT = np.einsum("bhl,bld->bhd", de, x) / np.sqrt(float(d))
    return dp, dT.reshape(n_bags, H * d)


def uncancelled_scales(saved, dy, Wqk, Wvo):
    """dict(dp, dT, dxn, dWqk): the largest entry each would have if nothing cancelled - de_hj = w_hj (t_hj - G_h) with
    |t| + |G| in place of the difference and absolute values in every later product.  A bag with ONE kept slot has w = 1 and
    P = x, so t = G and its de is 0: at L = 1 (or with one kept slot in every bag) dp, dT, dxn and dWqk are zero in every
    entry, and what a float32 evaluation leaves there is rounding of t and of G - it is held to the bar of THIS scale, the size of
    the terms (``attention_check.errs``'s ``zero_scale``)."""
    x, w, P, dy, dP, G, t, _ = _backward_terms(saved, dy, Wvo, np.float64)
    n_bags, H, d = P.shape
    de = np.abs(w) * (np.abs(t) + np.abs(G)[:, :, None])
    dT = (np.einsum("bhl,bld->bhd", de, np.abs(x)) / np.sqrt(float(d))).reshape(n_bags, H * d)
    return dict(dp=float(de.sum((0, 2)).max()), dT=float(dT.max()), dxn=float((dT @ np.abs(np.asarray(Wqk, dtype=np.float64)).T).max()),
                dWqk=float((np.abs(np.asarray(saved["xn"], dtype=np.float64)).T @ dT).max()))


def forward_torch(table, tok, Wqk, Wvo, p, base_rows=None):
    """The forward on torch tensors (any float dtype, differentiable): ``tok`` [n_bags, L] int64, already masked (-1 = skipped)."""
    import torch
    rows, d = table.shape
    n_bags, L = tok.shape
    H = p.shape[0]
    valid = (tok >= 0) & (tok < rows)
    some = valid.any(1)
    x = table[tok.clamp(0, rows - 1)] * valid[:, :, None]
    v = valid.to(torch.int64)
    r = (v.flip(1).cumsum(1).flip(1) - v).clamp(0, L - 1)
    newest = (L - 1 - torch.argmax(v.flip(1), dim=1)).clamp(0, L - 1)
    xn = x[torch.arange(n_bags), newest] * some[:, None]
    T = (xn @ Wqk).reshape(n_bags, H, d)
    e = torch.einsum("bld,bhd->bhl", x, T) / float(np.sqrt(float(d))) + p[:, r].permute(1, 0, 2)
    e = torch.where(valid[:, None, :], e, torch.full_like(e, -1e300))
    w = torch.softmax(e, dim=2) * valid[:, None, :]
    P = torch.einsum("bhl,bld->bhd", w, x)
    O = P.reshape(n_bags, H * d) @ Wvo
    return O if base_rows is None else base_rows + O


def step_f64(user_table, item_table, history_table, Wqk, Wvo, p, towers, user_ids, item_ids, user_history, temperature, relu_masks):
    """``history_check.step_f64`` with the self-attention encoder: f64 torch-CPU autograd of one step, the positive of every pair
    left out of its bag, the ReLU masks handed in.  Returns the loss and the gradients w.r.t. both towers' inputs and outputs, the
    tables (dense [rows, dim]), ``dWqk``, ``dWvo``, ``dp`` and every kernel and bias."""
    import torch
    f = lambda x: torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    ut, it, hb, Wq, Wv, pt = f(user_table), f(item_table), f(history_table), f(Wqk), f(Wvo), f(p)
    uid, iid = torch.from_numpy(np.asarray(user_ids)), torch.from_numpy(np.asarray(item_ids))
    tok = torch.from_numpy(np.asarray(user_history).astype(np.int64))[uid]
    tok = torch.where(tok == iid[:, None], torch.full_like(tok, -1), tok)                # leave-one-out
    ue = forward_torch(hb, tok, Wq, Wv, pt, ut[uid])
    ie = it[iid]
    ue.retain_grad(); ie.retain_grad()
    params, outs = [], []
    for x, (ws, bs), masks in ((ue, towers[0], relu_masks[0]), (ie, towers[1], relu_masks[1])):
        ws, bs = [f(w) for w in ws], [f(v) for v in bs]
        for l, (w, v) in enumerate(zip(ws, bs)):
            x = x @ w + v
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
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]), user_table=g(ut), item_table=g(it),
                history_table=g(hb), dWqk=g(Wq), dWvo=g(Wv), dp=g(pt),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(v) for v in bs] for _, bs in params])


ROWS, TOKEN_ROWS = 97, 50
# the GPU sweep: lane groups of 8, 32 with idle lanes, 32 and 64; one slot, a ragged chunk, an odd length and the longest; every
# head count; a ragged last lane group and a ragged last slab - the full cross product
DIMS, LS, BAGS = (32, 96, 128, 256), (1, 3, 7, 64), (33, 300)
# The logit scales.  Rows are N(0, 1) / sqrt(dim) and Wqk = scale * sqrt(dim) * N(0, 1), so <x_j, T_h> / sqrt(dim) ~ scale * N(0, 1):
# scale 1 is a soft softmax, scale 4 spreads the logits over roughly +-10 (sharp: a few slots carry a head).  float32 NumPy meets
# the bars at both on every problem of the sweep (tests/test_history_self_attention_cpu.py holds that), so none is dropped.
SCALES = (1.0, 4.0)


def params(rng, dim, L, heads, scale=1.0):
    """(Wqk [dim, H dim], Wvo [H dim, dim], p [H, L]): logits of size ``scale``, p ~ N(0, 1) distinct per head and rank - a slot
    counted at a wrong rank, or a head reading another head's line, shows."""
    Wqk = (scale * np.sqrt(dim) * rng.standard_normal((dim, heads * dim))).astype(np.float32)
    Wvo = (rng.standard_normal((heads * dim, dim)) / np.sqrt(heads * dim)).astype(np.float32)
    p = rng.standard_normal((heads, L)).astype(np.float32)
    assert len(np.unique(p)) == heads * L
    return Wqk, Wvo, p


def forward_problem(dim, n_bags, L, heads, scale=1.0, indirect=True, with_base=True, seed=0):
    """One deterministic forward / backward problem: ``attention_check.problem``'s special bags (leave-one-out, emptied bags,
    padding in the middle) over a [97, dim] table with rows N(0, 1) / sqrt(dim), and - where there are bags enough - bag 8 with
    every slot kept, bag 9 with kept slots in the oldest 8 only, bag 10 in the newest 8 only, bag 11 with a single kept slot, bag
    12 with one token in two slots, the NEWEST among them (indirect: those bags pool the token rows 8..12).  The base has a -1 id."""
    rng = np.random.default_rng([seed, dim, n_bags, L, heads, int(scale * 8), int(indirect)])
    n_rows = TOKEN_ROWS if indirect else n_bags
    tok, bag_rows, exclude = problem(rng, max(n_rows, 13), n_bags, L, ROWS, indirect)
    if not indirect:
        tok = tok[:n_bags]
    if n_bags >= 13:
        tok[8:13] = rng.integers(0, ROWS - 1, (5, L))
        tok[9, 8:] = -1
        tok[10, :max(L - 8, 0)] = -1
        tok[11, :] = -1
        tok[11, L // 2] = 5
        tok[12, 0] = tok[12, L - 1]
        exclude[8:13] = [ROWS - 1, -1, ROWS + 5, ROWS - 1, ROWS - 1]
        if indirect:
            bag_rows[8:13] = [8, 9, 10, 11, 12]
    table = (rng.standard_normal((ROWS, dim)) / np.sqrt(dim)).astype(np.float32)
    Wqk, Wvo, p = params(rng, dim, L, heads, scale)
    base = None
    if with_base:
        base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
        if n_bags >= 4:
            base_ids[3] = -1
        base = ((rng.standard_normal((40, dim)) * 0.1).astype(np.float32), base_ids)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    return dict(table=table, tokens=tok, bag_rows=bag_rows, exclude=exclude, Wqk=Wqk, Wvo=Wvo, p=p, base=base, dy=dy)


def within_bars(got, want, what="", zero_scale=None):
    """Holds ``got`` to the project's bars against the f64 ``want`` (``errs``; ``zero_scale``: the size of the terms behind a
    reference that is pure cancellation) and returns the two figures."""
    e = errs(got, want, zero_scale)
    assert e[0] <= BAR and e[1] <= BAR, (what, e)
    return e

"""Restatements of the history-GRU contract of include/twotower_hip.h (tt_history_gru_resolve_f32 / tt_history_gru_fwd_f32 /
tt_history_gru_bwd_f32 and the GEMMs around them) and of the train step with history_pooling="gru", shared by
tests/test_history_gru_cpu.py and tests/test_gpu_history_gru.py.

* ``gru_forward`` is the forward in f64 NumPy on the f32 inputs, on top of ``history_check.mask_tokens``: Keras
  GRU(reset_after=True) with zero initial state over the kept slots in slot order, a skipped slot carrying the state.
* ``gru_backward`` is the closed-form BPTT the backward launches compute; tests/test_history_gru_cpu.py holds it to f64 torch
  autograd of ``gru_forward_torch``.
* ``gru_forward_f32`` / ``gru_backward_f32`` are the same formulas with every operand and every operation in float32: what the
  formulas themselves lose at that precision, whatever order a kernel sums in.
* ``step_f64`` is ``history_check.step_f64`` with the GRU pool; ``problem`` the special bags of ``attention_check.problem``;
  ``errs`` the two error measures of the project's bars, ``within_bars`` the assertion on them.
"""
import numpy as np

import attention_check as ac
import history_check as hc

BAR = ac.BAR
errs = ac.errs
problem = ac.problem


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x)) if x.dtype == np.float64 else (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))).astype(np.float32)


def resolve(table, tokens, bag_rows=None, exclude=None):
    """(valid [n_bags, L], tok int64 [n_bags, L] - -1 where skipped -, flag): the slots a bag keeps."""
    per_bag, flag = hc.mask_tokens(tokens, bag_rows, exclude)
    tok = per_bag.astype(np.int64)
    valid = (tok >= 0) & (tok < len(table))
    flag |= int((~valid & (tok != -1)).any())
    return valid, np.where(valid, tok, -1), int(flag)


def _forward(table, valid, tok, W, U, b, dtype):
    """(h_final [n_bags, dim], saved) with every operand and operation in ``dtype``; saved = dict(x, z, r, n, gn, hprev), each
    [n_bags, L, ...], zeros in the skipped slots but hprev, which is the carried state."""
    table, W, U, b = (np.asarray(t, dtype=dtype) for t in (table, W, U, b))
    n_bags, L = valid.shape
    d = table.shape[1]
    x = np.where(valid[:, :, None], table[np.where(valid, tok, 0)], dtype(0))          # (a skipped slot: +0, as the device writes)
    a = (x.reshape(-1, d) @ W).reshape(n_bags, L, 3 * d) + b[0]
    h = np.zeros((n_bags, d), dtype=dtype)
    keep = {k: np.zeros((n_bags, L, d), dtype=dtype) for k in ("z", "r", "n", "gn", "hprev")}
    one = dtype(1.0)
    for t in range(L):
        g = h @ U + b[1]
        z = _sigmoid(a[:, t, :d] + g[:, :d])
        r = _sigmoid(a[:, t, d:2 * d] + g[:, d:2 * d])
        gn = g[:, 2 * d:]
        n = np.tanh(a[:, t, 2 * d:] + r * gn)
        hn = z * h + (one - z) * n
        v = valid[:, t, None]
        keep["hprev"][:, t] = h
        for k, val in (("z", z), ("r", r), ("n", n), ("gn", gn)):
            keep[k][:, t] = np.where(v, val, 0)
        h = np.where(v, hn, h)
    keep["x"] = x
    assert all(val.dtype == dtype for val in keep.values()) and h.dtype == dtype
    return h, keep


def _with_base(h, valid, base, dtype):
    flag = 0
    out = h
    if base is not None:
        base_table, base_ids = base
        base_ids = np.asarray(base_ids, dtype=np.int64)
        ok = (base_ids >= 0) & (base_ids < len(base_table))
        flag = int((~ok & (base_ids != -1)).any())
        rows = np.zeros_like(h)
        rows[ok] = np.asarray(base_table, dtype=dtype)[base_ids[ok]]
        out = np.where(valid.any(1)[:, None] | ~ok[:, None], rows + h, rows)          # an emptied bag: the base row itself
    return out, flag


def _run_forward(table, tokens, W, U, b, bag_rows, exclude, base, dtype):
    valid, tok, flag = resolve(table, tokens, bag_rows, exclude)
    h, saved = _forward(table, valid, tok, W, U, b, dtype)
    out, f2 = _with_base(h, valid, base, dtype)
    saved["valid"] = valid
    return out, tok.reshape(-1), int(flag | f2), saved


def gru_forward(table, tokens, W, U, b, bag_rows=None, exclude=None, base=None):
    """Returns (out [n_bags, dim] f64, batch_ids int64 [n_bags * L], flag 0/1, saved) - ``saved`` is what ``gru_backward`` takes.
    ``W``, ``U`` [dim, 3 dim] with the gate blocks z | r | n, ``b`` [2, 3 dim] = b_i, b_r; ``base`` = (base_table, base_ids)."""
    return _run_forward(table, tokens, W, U, b, bag_rows, exclude, base, np.float64)


def gru_forward_f32(table, tokens, W, U, b, bag_rows=None, exclude=None, base=None):
    return _run_forward(table, tokens, W, U, b, bag_rows, exclude, base, np.float32)


def _backward(saved, dy, W, U, dtype):
    W, U, dh = np.asarray(W, dtype=dtype), np.asarray(U, dtype=dtype), np.asarray(dy, dtype=dtype).copy()
    valid = saved["valid"]
    n_bags, L = valid.shape
    d = W.shape[0]
    z, r, n, gn, hp, x = (np.asarray(saved[k], dtype=dtype) for k in ("z", "r", "n", "gn", "hprev", "x"))
    dA, dG = np.zeros((n_bags, L, 3 * d), dtype=dtype), np.zeros((n_bags, L, 3 * d), dtype=dtype)
    one = dtype(1.0)
    for t in range(L - 1, -1, -1):
        v = valid[:, t, None]
        dn = dh * (one - z[:, t])
        dz = dh * (hp[:, t] - n[:, t])
        dan = dn * (one - n[:, t] * n[:, t])
        daz = dz * (z[:, t] * (one - z[:, t]))
        dar = (dan * gn[:, t]) * (r[:, t] * (one - r[:, t]))
        a_t = np.where(v, np.concatenate([daz, dar, dan], 1), 0)
        g_t = np.where(v, np.concatenate([daz, dar, dan * r[:, t]], 1), 0)
        dA[:, t], dG[:, t] = a_t, g_t
        dh = np.where(v, z[:, t] * dh + g_t @ U.T, dh)
    dA2, dG2 = dA.reshape(-1, 3 * d), dG.reshape(-1, 3 * d)
    slot_grads = dA2 @ W.T
    dW = x.reshape(-1, d).T @ dA2
    dU = hp.reshape(-1, d).T @ dG2
    db = np.stack([dA2.sum(0), dG2.sum(0)])
    assert slot_grads.dtype == dtype
    return slot_grads, dW, dU, db


def gru_backward(saved, dy, W, U):
    """The closed-form BPTT: (slot_grads [n_bags * L, dim] - zero rows for the skipped slots -, dW, dU [dim, 3 dim], db [2, 3 dim])."""
    return _backward(saved, dy, W, U, np.float64)


def gru_backward_f32(saved, dy, W, U):
    return _backward(saved, dy, W, U, np.float32)


def gru_forward_torch(table, tok, W, U, b, base_rows=None):
    """The forward on torch tensors (any float dtype, differentiable): ``tok`` [n_bags, L] int64, already masked (-1 = skipped)."""
    import torch
    rows, d = table.shape
    valid = (tok >= 0) & (tok < rows)
    x = table[tok.clamp(0, rows - 1)] * valid[:, :, None]
    h = torch.zeros((tok.shape[0], d), dtype=table.dtype)
    for t in range(tok.shape[1]):
        a, g = x[:, t] @ W + b[0], h @ U + b[1]
        z = torch.sigmoid(a[:, :d] + g[:, :d])
        r = torch.sigmoid(a[:, d:2 * d] + g[:, d:2 * d])
        n = torch.tanh(a[:, 2 * d:] + r * g[:, 2 * d:])
        h = torch.where(valid[:, t, None], z * h + (1 - z) * n, h)
    return h if base_rows is None else base_rows + h


def step_f64(user_table, item_table, history_table, W, U, b, towers, user_ids, item_ids, user_history, temperature, relu_masks):
    """``history_check.step_f64`` with the GRU pool: f64 torch-CPU autograd of one step, the positive of every pair left out of
    its bag, the ReLU masks handed in.  Returns the loss and the gradients w.r.t. both towers' inputs and outputs, the tables
    (dense [rows, dim]), ``dW``, ``dU``, ``db`` of the GRU and every kernel and bias."""
    import torch
    f = lambda x: torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    ut, it, hb, Wt, Ut, bt = f(user_table), f(item_table), f(history_table), f(W), f(U), f(b)
    uid, iid = torch.from_numpy(np.asarray(user_ids)), torch.from_numpy(np.asarray(item_ids))
    tok = torch.from_numpy(np.asarray(user_history).astype(np.int64))[uid]
    tok = torch.where(tok == iid[:, None], torch.full_like(tok, -1), tok)                # leave-one-out
    ue = gru_forward_torch(hb, tok, Wt, Ut, bt, ut[uid])
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
                history_table=g(hb), dW=g(Wt), dU=g(Ut), db=g(bt),
                dw=[[g(w) for w in ws] for ws, _ in params], db_towers=[[g(v) for v in bs] for _, bs in params])


ROWS, TOKEN_ROWS = 97, 50
DIMS, BAGS, LS = (32, 96, 128, 256), (1, 33, 300), (1, 2, 7, 64)
# (dim, n_bags, L, indirect bag_rows, base row) of the GPU sweep: every value of every axis of the issue's table, the full cross
# product where it is cheap (dim 32), and each further width at the shortest, an odd and the longest history
SHAPES = [(32, nb, L, ind, base) for nb in BAGS for L in LS for ind, base in ((False, False), (True, True))] + \
         [(d, nb, L, L != 7, L != 64) for d in (96, 128, 256) for nb, L in ((1, 2), (33, 7), (300, 64), (33, 1))]

# The second set - W, U and b scaled by 20, for saturated gates - runs at L = 1 and L = 2 only.  With U scaled by 20 the step map
# h -> h' is no contraction: its Jacobian z + (dz / dg_z, dn / dg_n, ...) U^T carries the factor |U|_2 ~ 20 (1 + sqrt(3)), so a
# float32 rounding of 6e-8 in h grows by one to two orders of magnitude per kept slot (the gates are not saturated in EVERY
# unit) and two float32 evaluations that differ only in summation order part ways: the formulas themselves, in float32 NumPy, miss
# the bars against f64 from L = 7 on (out: up to 2.4e-3 of max|ref| at L = 7, 2.0 - the states' whole range - at L = 64;
# tests/test_history_gru_cpu.py holds both statements).  A bar no float32 evaluation reaches tests nothing, so the saturated set
# keeps the lengths at which the bars ARE reachable: one step (saturated gates from the zero state) and two dependent steps.
SATURATED_SCALE = 20.0
SATURATED_SHAPES = [s for s in SHAPES if s[2] <= 2]


def params(rng, dim, scale=1.0):
    """(W, U, b): N(0, 1) / sqrt(dim) kernels times ``scale`` (20: saturated gates), small random biases times ``scale``."""
    W = (scale * rng.standard_normal((dim, 3 * dim)) / np.sqrt(dim)).astype(np.float32)
    U = (scale * rng.standard_normal((dim, 3 * dim)) / np.sqrt(dim)).astype(np.float32)
    b = (scale * 0.1 * rng.standard_normal((2, 3 * dim))).astype(np.float32)
    return W, U, b


def forward_problem(dim, n_bags, L, indirect, with_base, scale=1.0, seed=0):
    """One deterministic forward / backward problem of the sweep: ``problem``'s special bags over a [97, dim] table with rows
    N(0, 1) / sqrt(dim), and - where there are bags enough - bag 8 with every slot valid, bag 9 with kept slots in the oldest 8
    only, bag 10 in the newest 8 only, bag 11 with a single kept slot (indirect: those bags pool the token rows 8..11)."""
    rng = np.random.default_rng([seed, dim, n_bags, L, int(indirect), int(scale)])
    n_rows = TOKEN_ROWS if indirect else n_bags
    tok, bag_rows, exclude = problem(rng, max(n_rows, 12), n_bags, L, ROWS, indirect)
    if not indirect:
        tok = tok[:n_bags]
    if n_bags >= 12:
        tok[8:12] = rng.integers(0, ROWS - 1, (4, L))
        tok[9, 8:] = -1
        tok[10, :max(L - 8, 0)] = -1
        tok[11, :] = -1
        tok[11, L // 2] = 5
        exclude[8:12] = [ROWS - 1, -1, ROWS + 5, ROWS - 1]
        if indirect:
            bag_rows[8:12] = [8, 9, 10, 11]
    table = (rng.standard_normal((ROWS, dim)) / np.sqrt(dim)).astype(np.float32)
    W, U, b = params(rng, dim, scale)
    base = None
    if with_base:
        base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
        if n_bags >= 4:
            base_ids[3] = -1
        base = ((rng.standard_normal((40, dim)) * 0.1).astype(np.float32), base_ids)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    return dict(table=table, tokens=tok, bag_rows=bag_rows, exclude=exclude, W=W, U=U, b=b, base=base, dy=dy)


def within_bars(got, want, what=""):
    """Holds ``got`` to the project's bars against the f64 ``want`` and returns the two figures.  A reference that is zero in
    every entry has no cancellation behind it here - dU at L = 1 or with one kept slot per bag is a sum of products with the zero
    initial state - so the result must be zero too, exactly."""
    want = np.asarray(want, dtype=np.float64)
    if not want.any():
        assert not np.asarray(got).any(), what
        return 0.0, 0.0
    e = errs(got, want)
    assert e[0] <= BAR and e[1] <= BAR, (what, e)
    return e

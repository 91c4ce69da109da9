"""Restatements of the history-attention contract of include/twotower_hip.h (tt_history_attention_fwd_f32 /
tt_history_attention_bwd_f32) and of the train step with history_pooling="attention", shared by
tests/test_history_attention_cpu.py and tests/test_gpu_history_attention.py.

* ``attention_forward`` is the forward in f64 NumPy on the f32 inputs, on top of ``history_check.mask_tokens``: for the valid
  slots j of a bag r_j = valid slots behind j, e_j = <h_j, a> / sqrt(dim) + p[r_j], w = softmax(e), out = base row + sum w_j h_j.
  The device takes the exponential in hardware, so it is compared within the project's bars, not bit for bit.
* ``attention_backward`` is the closed form the backward launch computes; tests/test_history_attention_cpu.py holds it to f64
  torch autograd of ``attention_forward_torch``.
* ``step_f64`` is ``history_check.step_f64`` with the attention pool.
"""
import numpy as np

import history_check as hc


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


def attention_backward(table, batch_ids, weights, pooled, dy, attn, L):
    """The closed form: (slot_grads [n_bags * L, dim] - zero rows for the skipped slots -, da [dim], dp [L], de [n_bags, L])."""
    table = np.asarray(table, dtype=np.float64)
    dim = table.shape[1]
    ids = np.asarray(batch_ids).reshape(-1, L)
    valid = ids >= 0
    h = table[np.where(valid, ids, 0)] * valid[:, :, None]
    g = np.asarray(dy, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64) * valid
    a = np.asarray(attn, dtype=np.float64)[:dim]
    s = 1.0 / np.sqrt(float(dim))
    G = (g * np.asarray(pooled, dtype=np.float64)).sum(1)
    t = np.einsum("bd,bjd->bj", g, h)
    de = w * (t - G[:, None])
    dh = w[:, :, None] * g[:, None, :] + de[:, :, None] * a[None, None, :] * s
    dh = dh * valid[:, :, None]
    da = np.einsum("bj,bjd->d", de, h) * s
    dp = np.zeros(L)
    np.add.at(dp, ranks(valid)[valid], de[valid])
    return dh.reshape(-1, dim), da, dp, de


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

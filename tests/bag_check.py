"""Restatements of the embedding-bag contract of include/twotower_hip.h (tt_embedding_bag_fwd_f32 / tt_embedding_bag_bwd_f32 and
the bag table's update), shared by tests/test_bag_cpu.py and tests/test_gpu_bag.py.

* ``bag_forward`` mirrors the device arithmetic operation by operation in the table's dtype - NumPy's f32 + * / sqrt are
  correctly rounded, like the device's __fadd_rn / __fmul_rn / __fdiv_rn / sqrtf, and nothing is contracted - so the GPU
  results are compared with it BIT FOR BIT (f32); in f64 it is what torch.nn.functional.embedding_bag computes.

      s = first valid row, + every further valid row in ascending slot order
      sum: inv = 1, pooled = s     mean: inv = 1 / cnt, pooled = s * inv     sqrtn: inv = 1 / sqrt(cnt), pooled = s * inv
      out = out + pooled (accumulate; an empty bag's row is not written)  |  out = pooled (an empty bag: +0);  empty: inv = 0

* ``bag_update`` restates the update of the bag table: gs = dy * inv (dy itself for sum pooling), every valid slot's gradient
  row is its bag's row of gs, equal tokens are summed in the piece order of oracle.two_tower.dedup_sum (what an expansion into
  per-token rows would be summed as), then the optimizer's rows (SGD / Adagrad: oracle.two_tower; Adam: adam_check).
* ``step_f64`` is the whole train step with the feature in f64 torch-CPU autograd: tables -> item input + pooled titles ->
  towers -> in-batch softmax loss (SUM), with the ReLU masks handed in.
"""
import numpy as np

import adam_check as ac
from oracle import two_tower as tt

POOLINGS = ("sum", "mean", "sqrtn")
bits = ac.bits


def bag_forward(table, tokens, bag_rows=None, pooling="mean", accumulate=False, out=None):
    """Returns (out [n_bags, dim], batch_ids int64 [n_bags * L], inv [n_bags], flag 0/1); ``out`` (accumulate) is not changed."""
    assert pooling in POOLINGS
    dt = table.dtype.type
    tokens = np.asarray(tokens)
    n_rows, L = tokens.shape
    table_rows, dim = table.shape
    br = np.arange(n_rows, dtype=np.int64) if bag_rows is None else np.asarray(bag_rows, dtype=np.int64)
    n_bags = len(br)
    row_ok = (br >= 0) & (br < n_rows)
    flag = bool((~row_ok & (br != -1)).any())
    tok = np.full((n_bags, L), -1, dtype=np.int64)
    tok[row_ok] = tokens[br[row_ok]]
    valid = (tok >= 0) & (tok < table_rows)
    flag |= bool((~valid & (tok != -1)).any())
    batch_ids = np.where(valid, tok, -1)
    s = np.zeros((n_bags, dim), dtype=table.dtype)
    cnt = np.zeros(n_bags, dtype=np.int64)
    for k in range(L):
        v = valid[:, k]
        r = table[np.where(v, tok[:, k], 0)]
        first, more = v & (cnt == 0), v & (cnt > 0)
        s = np.where(first[:, None], r, np.where(more[:, None], s + r, s))       # s starts AT the first valid row
        cnt += v
    some = cnt > 0
    c = np.where(some, cnt, 1).astype(table.dtype)
    scale = {"sum": np.ones_like(c), "mean": dt(1) / c, "sqrtn": dt(1) / np.sqrt(c)}[pooling]
    inv = np.where(some, scale, dt(0)).astype(table.dtype)
    pooled = s if pooling == "sum" else s * inv[:, None]
    if accumulate:
        res = np.array(out, dtype=table.dtype, copy=True)
        res[some] = res[some] + pooled[some]
    else:
        res = pooled
    return res, batch_ids.reshape(-1), inv, int(flag)


def bag_gs(dy, inv, pooling):
    """The bags' gradient rows: dy * inv (one rounding), dy itself for sum pooling."""
    return dy if pooling == "sum" else dy * inv[:, None]


def slot_gradients(batch_ids, gs, L):
    """(token, gradient row) of every VALID slot in ascending position: what an expansion into per-token rows would hold."""
    batch_ids = np.asarray(batch_ids)
    pos = np.flatnonzero(batch_ids >= 0)
    return batch_ids[pos], np.ascontiguousarray(gs[pos // L])


def bag_update(opt, state, batch_ids, gs, L, lr, step=1, eps=1e-7):
    """In place on ``state`` = [table] (sgd), [table, accum] (adagrad) or [table, m, v] (adam)."""
    ids, g = slot_gradients(batch_ids, gs, L)
    if opt == "sgd":
        tt.sparse_sgd(state[0], ids, g, lr)
    elif opt == "adagrad":
        tt.sparse_adagrad(state[0], state[1], ids, g, lr, eps)
    else:
        ac.sparse_adam(state[0], state[1], state[2], ids, g, lr, step)
    return np.unique(ids)


def step_f64(user_table, item_table, title_table, towers, user_ids, item_ids, item_titles, pooling, temperature, relu_masks,
             category=None):
    """f64 torch-CPU autograd of one step with the title feature.  ``towers`` = ((user ws, user bs), (item ws, item bs)) NumPy
    arrays; ``relu_masks`` = (user masks, item masks), one boolean [batch, n] per hidden layer (the device's), replacing the ReLU's
    own (discontinuous) derivative; ``category`` = (cat_table, category_ids) or None.  Returns loss (float) and the gradients
    w.r.t. both towers' inputs (due, die) and outputs (dq, dc), the three tables (dense [rows, dim]) and every kernel and bias."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    ut, it, tb = f(user_table), f(item_table), f(title_table)
    uid, iid = torch.from_numpy(np.asarray(user_ids)), torch.from_numpy(np.asarray(item_ids))
    tok = torch.from_numpy(np.asarray(item_titles).astype(np.int64))[iid]                 # [batch, L]
    valid = (tok >= 0) & (tok < tb.shape[0])
    rows = tb[tok.clamp(0, tb.shape[0] - 1)] * valid[..., None]
    cnt = valid.sum(1).to(torch.float64)
    some = cnt > 0
    safe = torch.where(some, cnt, torch.ones_like(cnt))
    inv = {"sum": torch.ones_like(cnt), "mean": 1.0 / safe, "sqrtn": 1.0 / safe.sqrt()}[pooling] * some
    ue = ut[uid]
    ie = it[iid]
    cat_t = None
    if category is not None:
        cat_t = f(category[0])
        ie = ie + cat_t[torch.from_numpy(np.asarray(category[1]))]
    ie = ie + rows.sum(1) * inv[:, None]
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
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]), user_table=g(ut), item_table=g(it), title_table=g(tb),
                cat_table=None if cat_t is None else g(cat_t),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b) for b in bs] for _, bs in params])

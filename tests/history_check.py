"""Restatements of the history-bag contract of include/twotower_hip.h (tt_history_bag_fwd_f32) and of the train step with the
pooled user-history feature, shared by tests/test_history_cpu.py and tests/test_gpu_history.py.

* ``mask_tokens`` is the leave-one-out rule: every slot of bag b whose token equals exclude[b] becomes padding (-1).
* ``history_forward`` is ``bag_check.bag_forward`` on that masked token matrix, accumulating into the gathered base rows (an
  out-of-range base id: a zero row and the flag; -1: a zero row, no flag) - operation by operation the device's arithmetic, so
  the GPU results are compared with it BIT FOR BIT.  With a base, an empty bag's row is the base row itself.
* ``step_f64`` is the whole train step with the feature in f64 torch-CPU autograd: the user tower's input is the user row +
  the pooled history rows WITHOUT the pair's own item, with the ReLU masks handed in.
"""
import numpy as np

import bag_check as bc

POOLINGS = bc.POOLINGS
bits = bc.bits


def mask_tokens(tokens, bag_rows, exclude):
    """(masked token matrix [n_bags, L] - one row per BAG -, identity bag rows with -1 where the bag's row was -1 / out of
    range, flag): the per-bag view ``bag_forward`` is then run on."""
    tokens = np.asarray(tokens)
    n_rows, L = tokens.shape
    br = np.arange(n_rows, dtype=np.int64) if bag_rows is None else np.asarray(bag_rows, dtype=np.int64)
    ok = (br >= 0) & (br < n_rows)
    flag = bool((~ok & (br != -1)).any())
    per_bag = np.full((len(br), L), -1, dtype=tokens.dtype)
    per_bag[ok] = tokens[br[ok]]
    if exclude is not None:
        per_bag = np.where(per_bag.astype(np.int64) == np.asarray(exclude, dtype=np.int64)[:, None], -1, per_bag).astype(tokens.dtype)
    return per_bag, int(flag)


def history_forward(table, tokens, bag_rows=None, exclude=None, base=None, pooling="mean", accumulate=False, out=None):
    """Returns (out [n_bags, dim], batch_ids int64 [n_bags * L], inv [n_bags], flag 0/1).  ``base`` = (base_table, base_ids)."""
    per_bag, flag = mask_tokens(tokens, bag_rows, exclude)
    if base is not None:
        assert not accumulate
        base_table, base_ids = base
        base_ids = np.asarray(base_ids, dtype=np.int64)
        ok = (base_ids >= 0) & (base_ids < len(base_table))
        flag |= int((~ok & (base_ids != -1)).any())
        rows = np.zeros((len(base_ids), table.shape[1]), dtype=table.dtype)
        rows[ok] = base_table[base_ids[ok]]
        accumulate, out = True, rows
    res, batch_ids, inv, f2 = bc.bag_forward(table, per_bag, None, pooling, accumulate, out)
    return res, batch_ids, inv, int(flag | f2)


def step_f64(user_table, item_table, history_table, towers, user_ids, item_ids, user_history, pooling, temperature, relu_masks,
             title=None):
    """f64 torch-CPU autograd of one step with the history feature (``bag_check.step_f64``'s shape, the bag on the user side, the
    positive of every pair excluded).  ``title`` = (title_table, item_titles, pooling) or None.  Returns loss and the gradients
    w.r.t. both towers' inputs and outputs, the tables (dense [rows, dim]) and every kernel and bias."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    ut, it, hb = f(user_table), f(item_table), f(history_table)
    uid, iid = torch.from_numpy(np.asarray(user_ids)), torch.from_numpy(np.asarray(item_ids))

    def pooled(tb, tok, how):
        valid = (tok >= 0) & (tok < tb.shape[0])
        rows = tb[tok.clamp(0, tb.shape[0] - 1)] * valid[..., None]
        cnt = valid.sum(1).to(torch.float64)
        some = cnt > 0
        safe = torch.where(some, cnt, torch.ones_like(cnt))
        inv = {"sum": torch.ones_like(cnt), "mean": 1.0 / safe, "sqrtn": 1.0 / safe.sqrt()}[how] * some
        return rows.sum(1) * inv[:, None]

    tok = torch.from_numpy(np.asarray(user_history).astype(np.int64))[uid]               # [batch, L]
    tok = torch.where(tok == iid[:, None], torch.full_like(tok, -1), tok)                # leave-one-out
    ue = ut[uid] + pooled(hb, tok, pooling)
    ie = it[iid]
    tt_t = None
    if title is not None:
        tt_t = f(title[0])
        ie = ie + pooled(tt_t, torch.from_numpy(np.asarray(title[1]).astype(np.int64))[iid], title[2])
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
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]), user_table=g(ut), item_table=g(it),
                history_table=g(hb), title_table=None if tt_t is None else g(tt_t),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b) for b in bs] for _, bs in params])

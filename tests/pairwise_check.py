"""Restatements of the pairwise-loss contract of include/twotower_hip.h (tt_retrieval_pairwise_fwd_f32 /
tt_retrieval_pairwise_fwd_bwd_f32) and of the train step under a pairwise loss, shared by tests/test_pairwise_cpu.py and
tests/test_gpu_pairwise.py.

* ``pairs``: logits, positives, the valid-pair mask and x = pos - s in f64.
* ``loss`` / ``grads``: the loss (total, per row, n_i) and (dq, dc) in f64 NumPy, written from the header's formulas.
* ``pick_margin``: a hinge margin that keeps every valid pair's x at least 2e-5 away from the kink.  The hinge gradient is
  discontinuous there; an f32 logit on the other side of it is not a kernel error, so the INPUTS keep clear of it (a condition
  on the inputs, not a tolerance).  ``thr_gap``: the same distance between the logits and a row's hard-negative threshold.
* ``thr_natural``: ops.retrieval_hard_negative_thresholds returns log2-domain thresholds (the scorer's domain); the
  restatement compares natural logits.
* ``step_f64``: one train step in f64 torch-CPU autograd, in the shape of tests/rating_check.py's.
"""
import numpy as np

LN2 = float(np.log(2.0))
GAP = 2e-5


def thr_natural(thr):
    """The device's hard-negative thresholds (log2 domain) as natural-logit thresholds."""
    return None if thr is None else np.asarray(thr, dtype=np.float64) * LN2


def pairs(q, c, inv_t, p=None, ids=None, thr=None, off=0):
    """(s [nq, nc], pos [nq], valid [nq, nc] bool, x [nq, nc]) in f64; ``thr``: natural-logit thresholds."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    nq, nc = q.shape[0], c.shape[0]
    s = q @ c.T * inv_t
    if p is not None:
        s = s - np.log(np.clip(np.asarray(p, dtype=np.float64), 1e-6, 1.0))[None, :]
    rows = np.arange(nq)
    pos = s[rows, rows + off]
    valid = np.ones((nq, nc), dtype=bool)
    valid[rows, rows + off] = False
    if ids is not None:
        ids = np.asarray(ids)
        valid &= ids[None, :] != ids[rows + off][:, None]
    if thr is not None:
        valid &= ~(s < np.asarray(thr, dtype=np.float64)[:, None])
    return s, pos, valid, pos[:, None] - s


def _phi(x, kind, margin):
    """(phi, -phi') elementwise."""
    if kind == "logistic":
        return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))), 1.0 / (1.0 + np.exp(x))
    if kind == "hinge":
        return np.maximum(0.0, margin - x), (x < margin).astype(np.float64)
    raise ValueError(kind)


def _row_scale(valid, reduction, w):
    n = valid.sum(1)
    r = 1.0 / np.maximum(n, 1) if reduction == "mean" else np.ones(len(n))
    if reduction not in ("mean", "sum"):
        raise ValueError(reduction)
    return n, r * (np.ones(len(n)) if w is None else np.asarray(w, dtype=np.float64))


def loss(q, c, kind, margin=1.0, reduction="mean", inv_t=1.0, w=None, p=None, ids=None, thr=None, off=0):
    """(loss, per_row [nq], n [nq])."""
    _, _, valid, x = pairs(q, c, inv_t, p, ids, thr, off)
    phi, _ = _phi(x, kind, margin)
    n, wr = _row_scale(valid, reduction, w)
    per_row = wr * np.where(valid, phi, 0.0).sum(1)
    return float(per_row.sum()), per_row, n


def grads(q, c, kind, margin=1.0, reduction="mean", inv_t=1.0, w=None, p=None, ids=None, thr=None, off=0, grad_scale=1.0):
    """(dq [nq, D], dc [nc, D])."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    nq = q.shape[0]
    _, _, valid, x = pairs(q, c, inv_t, p, ids, thr, off)
    _, hp = _phi(x, kind, margin)
    _, wr = _row_scale(valid, reduction, w)
    h = np.where(valid, hp, 0.0) * wr[:, None]
    H = h.sum(1)
    dq = grad_scale * inv_t * (h @ c - H[:, None] * c[off:off + nq])
    dc = h.T @ q
    dc[off:off + nq] -= H[:, None] * q
    return dq, grad_scale * inv_t * dc


def pick_margin(x_ref, valid=None):
    """The first m = 0.500 + 0.001 k, k < 100, that no valid pair's x (``valid``: the pair mask; None: every entry) comes within
    2e-5 of."""
    x = np.asarray(x_ref, dtype=np.float64)
    x = x[valid] if valid is not None else x.reshape(-1)
    for k in range(100):
        m = 0.5 + 0.001 * k
        if x.size == 0 or np.abs(m - x).min() >= GAP:
            return m
    raise AssertionError("pick_margin: no margin in 0.500 .. 0.599 keeps 2e-5 clear of every pair")


def thr_gap(s, thr, candidates):
    """min |s_ij - thr_i| over the pairs ``candidates`` (the mask before the threshold is applied); inf without pairs."""
    d = np.abs(np.asarray(s, dtype=np.float64) - np.asarray(thr, dtype=np.float64)[:, None])[candidates]
    return float(d.min()) if d.size else float("inf")


def step_f64(user_table, item_table, towers, user_ids, item_ids, kind, margin, reduction, temperature, relu_masks,
             normalize_eps=None, sample_weight=None, cand_ids=None, cand_prob=None, head=None, ratings=None, rating_weight=0.0,
             head_mask=None):
    """f64 torch-CPU autograd of one train step under a pairwise retrieval loss.  ``towers`` = ((ws, bs), (ws, bs));
    ``relu_masks`` the towers' hidden masks; ``normalize_eps``: L2-normalised tower outputs; ``cand_ids`` (mixed negative
    sampling): the item side's ids, batch items first, a sampled candidate equal to the row's positive is not a pair;
    ``cand_prob``: the candidates' sampling probabilities; ``head`` = (W1, b1, w2, b2) with ``ratings`` / ``rating_weight`` /
    ``head_mask``: the joint model's rating head.  Returns the retrieval loss, the rating loss and the gradients of the total."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    k = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    ut, it = f(user_table), f(item_table)
    uid = torch.from_numpy(np.asarray(user_ids, dtype=np.int64))
    iid = torch.from_numpy(np.asarray(item_ids if cand_ids is None else cand_ids, dtype=np.int64))
    ue, ie = ut[uid], it[iid]
    ue.retain_grad(); ie.retain_grad()
    params, outs = [], []
    for x, (ws, bs), masks in ((ue, towers[0], relu_masks[0]), (ie, towers[1], relu_masks[1])):
        ws, bs = [f(w) for w in ws], [f(b) for b in bs]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                x = x * k(masks[l])
        params.append((ws, bs))
        if normalize_eps is not None:
            x = x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=normalize_eps))
        outs.append(x)
    for o in outs:
        o.retain_grad()
    b = len(uid)
    s = outs[0] @ outs[1].t() / temperature
    if cand_prob is not None:
        s = s - torch.log(torch.clamp(k(cand_prob), 1e-6, 1.0))[None, :]
    valid = torch.ones(s.shape, dtype=torch.bool)
    valid[torch.arange(b), torch.arange(b)] = False
    if cand_ids is not None:
        pos_ids = torch.from_numpy(np.asarray(item_ids, dtype=np.int64))
        valid &= iid[None, :] != pos_ids[:, None]
    x = s[torch.arange(b), torch.arange(b)][:, None] - s
    phi = torch.nn.functional.softplus(-x) if kind == "logistic" else torch.clamp(margin - x, min=0.0)
    n = valid.sum(1).to(torch.float64)
    r = 1.0 / torch.clamp(n, min=1.0) if reduction == "mean" else torch.ones(b, dtype=torch.float64)
    sw = torch.ones(b, dtype=torch.float64) if sample_weight is None else k(sample_weight)
    retrieval = (sw * r * torch.where(valid, phi, torch.zeros_like(phi)).sum(1)).sum()
    total, l_r, hp = retrieval, None, ()
    if head is not None:
        w1, b1, w2, b2 = hp = tuple(f(t) for t in head)
        d = outs[0].shape[1]
        a = b1 + outs[0] @ w1[:d] + outs[1][:b] @ w1[d:]
        pred = (a * k(head_mask)) @ w2 + b2
        rt = np.asarray(ratings, dtype=np.float64)
        ok = np.isfinite(rt)
        e = (pred - k(np.where(ok, rt, 0.0))) * k(ok.astype(np.float64))
        l_r = (sw * e * e).sum() / b
        total = retrieval + rating_weight * l_r
    total.backward()
    g = lambda t: t.grad.numpy()
    return dict(loss=float(retrieval.detach()), rating_loss=None if l_r is None else float(l_r.detach()), due=g(ue), die=g(ie),
                dq=g(outs[0]), dc=g(outs[1]), x=x.detach().numpy(), valid=valid.numpy(),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b_) for b_ in bs] for _, bs in params],
                dhead=[g(t) for t in hp])

"""Restatements of the rating-head contract of include/twotower_hip.h (tt_rating_head_fwd_f32 / tt_rating_head_bwd_f32) and of
the train step with the head, shared by tests/test_rating_cpu.py and tests/test_gpu_rating.py.

* ``head_forward`` / ``head_backward``: the head and every backward quantity in f64 NumPy.  ``head_backward`` takes h and pred
  as arguments, so a GPU test can hand it the DEVICE's activations and no ReLU mask can disagree.
* ``slab_rows``: the contiguous row blocks of the backward launch.
* ``step_f64``: the whole train step with the head in f64 torch-CPU autograd, the ReLU masks (towers' and head's) handed in.
* the tensor ids of the synthetic initialiser, restated from trainer.py.
"""
import numpy as np

# tensor ids of the counter-based generator (trainer.py): 1..15 tables / ids / features, 16.. the towers' Dense kernels
# (16 + 2 l + tower, at most 8 layers: 16..31), 64.. the dropout streams; the head's two kernels sit between them
TID_RATING_W1, TID_RATING_W2 = 40, 41
TRAINER_TIDS_IN_USE = set(range(1, 16)) | set(range(16, 32)) | set(range(64, 64 + 16))


def head_forward(q, c, w1, b1, w2, b2):
    """(pred [n], h [n, H], a [n, H]) in f64."""
    q, c, w1, b1, w2 = (np.asarray(t, dtype=np.float64) for t in (q, c, w1, b1, w2))
    d = q.shape[1]
    a = b1[None, :] + q @ w1[:d] + c @ w1[d:]
    h = np.maximum(a, 0.0)
    return float(np.asarray(b2, dtype=np.float64).reshape(-1)[0]) + h @ w2, h, a


def rating_loss(pred, rating, sample_weight=None):
    """L_r = (1/n) sum over the finite ratings of w e^2: the divisor is n (Keras MeanSquaredError, SUM_OVER_BATCH_SIZE)."""
    pred, rating = np.asarray(pred, dtype=np.float64), np.asarray(rating, dtype=np.float64)
    w = np.ones_like(pred) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
    valid = np.isfinite(rating)
    e = np.where(valid, pred - np.where(valid, rating, 0.0), 0.0)
    return float((w * e * e).sum() / len(pred)) if len(pred) else 0.0


def head_backward(q, c, h, pred, rating, w1, w2, grad_scale, sample_weight=None):
    """Every backward quantity of the contract in f64, from the given h and pred: dict(g, dq, dc, dw1, db1, dw2, db2, se)."""
    q, c, h, pred, rating, w1, w2 = (np.asarray(t, dtype=np.float64) for t in (q, c, h, pred, rating, w1, w2))
    d = q.shape[1]
    w = np.ones_like(pred) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
    valid = np.isfinite(rating)
    e = np.where(valid, pred - np.where(valid, rating, 0.0), 0.0)
    g = np.where(valid, grad_scale * w * e, 0.0)
    dh = g[:, None] * w2[None, :] * (h > 0)
    x = np.concatenate([q, c], axis=1)
    return dict(g=g, dq=dh @ w1[:d].T, dc=dh @ w1[d:].T, dw1=x.T @ dh, db1=dh.sum(0), dw2=(g[:, None] * h).sum(0),
                db2=float(g.sum()), se=float((w * e * e).sum()))


def slab_rows(n, n_slabs):
    """Slab s holds rows [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs)."""
    r = -(-n // n_slabs) if n else 0
    return [(min(s * r, n), min((s + 1) * r, n)) for s in range(n_slabs)]


def step_f64(user_table, item_table, towers, user_ids, item_ids, head, ratings, rating_weight, temperature, relu_masks,
             head_mask, normalize_eps=None, sample_weight=None, cand_ids=None, category=None, title=None, features=None):
    """f64 torch-CPU autograd of one step of the joint model: total = retrieval + rating_weight * L_r.  ``towers`` =
    ((ws, bs), (ws, bs)); ``head`` = (W1, b1, w2, b2); ``relu_masks`` the towers' hidden masks, ``head_mask`` [B, H] the head's;
    ``normalize_eps``: the towers' outputs are L2-normalised (tf.math.l2_normalize) before both tasks; ``cand_ids`` (mixed
    negative sampling): the item side's ids, batch items first - the head reads the first B candidate rows; ``category`` =
    (table, ids); ``title`` = (table, tokens, pooling); ``features`` = {"user": (feat, mean, inv_std, P, clip) | None, "item": ...}.
    Returns the retrieval loss, L_r and the gradients of the total."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    ut, it = f(user_table), f(item_table)
    uid = torch.from_numpy(np.asarray(user_ids, dtype=np.int64))
    iid = torch.from_numpy(np.asarray(item_ids if cand_ids is None else cand_ids, dtype=np.int64))
    ue, ie = ut[uid], it[iid]
    if category is not None:
        ie = ie + c(category[0])[torch.from_numpy(np.asarray(category[1], dtype=np.int64))]
    if title is not None:
        tb, tok, how = c(title[0]), torch.from_numpy(np.asarray(title[1]).astype(np.int64))[iid], title[2]
        ok = (tok >= 0) & (tok < tb.shape[0])
        rows = tb[tok.clamp(0, tb.shape[0] - 1)] * ok[..., None]
        cnt = ok.sum(1).to(torch.float64)
        some = cnt > 0
        safe = torch.where(some, cnt, torch.ones_like(cnt))
        inv = {"sum": torch.ones_like(cnt), "mean": 1.0 / safe, "sqrtn": 1.0 / safe.sqrt()}[how] * some
        ie = ie + rows.sum(1) * inv[:, None]
    projs = {}
    for side, ids in (("user", uid), ("item", iid)):
        if not features or features.get(side) is None:
            continue
        feat, mean, inv_std, p, clip = features[side]
        z = (c(feat)[ids] - c(mean)) * c(inv_std)
        if clip > 0:
            z = z.clamp(-clip, clip)
        projs[side] = f(p)
        if side == "user":
            ue = ue + z @ projs[side]
        else:
            ie = ie + z @ projs[side]
    ue.retain_grad(); ie.retain_grad()
    params, outs = [], []
    for x, (ws, bs), masks in ((ue, towers[0], relu_masks[0]), (ie, towers[1], relu_masks[1])):
        ws, bs = [f(w) for w in ws], [f(b) for b in bs]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                x = x * c(masks[l])
        params.append((ws, bs))
        if normalize_eps is not None:
            x = x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=normalize_eps))
        outs.append(x)
    for o in outs:
        o.retain_grad()
    b = len(uid)
    s = outs[0] @ outs[1].t() / temperature
    if cand_ids is not None:                             # a sampled candidate that IS the row's positive: a false negative
        pos = torch.from_numpy(np.asarray(item_ids, dtype=np.int64))
        same = iid[None, :] == pos[:, None]
        same[torch.arange(b), torch.arange(b)] = False
        s = s.masked_fill(same, float("-inf"))
    sw = torch.ones(b, dtype=torch.float64) if sample_weight is None else c(sample_weight)
    retrieval = ((torch.logsumexp(s, dim=1) - s[torch.arange(b), torch.arange(b)]) * sw).sum()
    w1, b1, w2, b2 = (f(t) for t in head)
    d = outs[0].shape[1]
    a = b1 + outs[0] @ w1[:d] + outs[1][:b] @ w1[d:]
    pred = (a * c(head_mask)) @ w2 + b2
    r = np.asarray(ratings, dtype=np.float64)
    valid = np.isfinite(r)
    e = (pred - c(np.where(valid, r, 0.0))) * c(valid.astype(np.float64))
    l_r = (sw * e * e).sum() / b
    (retrieval + rating_weight * l_r).backward()
    g = lambda t: t.grad.numpy()
    return dict(loss=float(retrieval.detach()), rating_loss=float(l_r.detach()), pred=pred.detach().numpy(), due=g(ue), die=g(ie),
                dq=g(outs[0]), dc=g(outs[1]), dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b_) for b_ in bs] for _, bs in params],
                dw1=g(w1), db1=g(b1), dw2=g(w2), db2=g(b2), dp={side: g(p) for side, p in projs.items()})

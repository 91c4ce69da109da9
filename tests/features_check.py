"""Restatements of the dense numeric side-feature contract of include/twotower_hip.h (tt_dense_features_fwd_f32 /
tt_dense_features_bwd_f32) and of the train step with the feature, shared by tests/test_features_cpu.py and
tests/test_gpu_features.py.

* ``features_forward`` repeats the device's f32 arithmetic operation by operation - one subtraction, one product, the clamp, then
  the sum over f ascending from +0 of separately rounded products, then (accumulating) one add into the row - so the GPU results
  are compared with it BIT FOR BIT.  An id of -1 gives z = 0 and no flag, any other id outside the matrix z = 0 and the flag.
* ``features_dp`` is the projection kernel's gradient, sum_b z[b, f] * dy[b, d], in f64.
* ``step_f64`` is the whole train step in f64 torch-CPU autograd, the ReLU masks handed in: the tower inputs are the id rows
  (+ category row, + pooled title rows on the item side) + the projected normalised features.
"""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def normalise(feat, ids, mean=None, inv_std=None, clip=0.0):
    """(z [n, F] f32, flag): the normalised (clamped) feature rows of ``ids``, in the device's f32 operations."""
    feat = np.asarray(feat, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < feat.shape[0])
    flag = int((~ok & (ids != -1)).any())
    z = np.zeros((len(ids), feat.shape[1]), dtype=np.float32)
    x = feat[ids[ok]]
    if mean is not None:
        x = ((x - np.asarray(mean, dtype=np.float32)[None, :]).astype(np.float32) * np.asarray(inv_std, dtype=np.float32)[None, :]).astype(np.float32)
    if clip > 0:
        x = np.minimum(np.maximum(x, np.float32(-clip)), np.float32(clip))
    z[ok] = x
    return z, flag


def features_forward(feat, ids, mean, inv_std, proj, clip=0.0, accumulate=False, out=None):
    """Returns (out [n, dim] f32, z [n, F] f32, flag 0/1)."""
    proj = np.asarray(proj, dtype=np.float32)
    z, flag = normalise(feat, ids, mean, inv_std, clip)
    acc = np.zeros((z.shape[0], proj.shape[1]), dtype=np.float32)
    for f in range(proj.shape[0]):                       # ascending f: acc = fadd(acc, fmul(z_f, P[f, :]))
        acc = (acc + (z[:, f:f + 1] * proj[f][None, :]).astype(np.float32)).astype(np.float32)
    if accumulate:
        acc = (np.asarray(out, dtype=np.float32) + acc).astype(np.float32)
    return acc, z, flag


def features_dp(z, dy):
    """dP [F, dim] in f64."""
    return np.asarray(z, dtype=np.float64).T @ np.asarray(dy, dtype=np.float64)


def slab_rows(n, n_slabs):
    """The contiguous row blocks of the backward launch: slab s holds rows [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs)."""
    r = -(-n // n_slabs) if n else 0
    return [(min(s * r, n), min((s + 1) * r, n)) for s in range(n_slabs)]


def step_f64(user_table, item_table, towers, user_ids, item_ids, features, temperature, relu_masks, cand_ids=None,
             category=None, title=None):
    """f64 torch-CPU autograd of one step with the numeric features.  ``features`` = {"user": (feat, mean, inv_std, P, clip) or
    None, "item": ...}; ``cand_ids`` (mixed negative sampling): the item side's ids, batch items first - a sampled candidate equal
    to a row's own positive is masked out of that row, as the scorer does; ``category`` = (table, ids); ``title`` = (table,
    tokens [n_items, L], pooling).  Returns the loss and the gradients w.r.t. the tower inputs, every kernel and bias and the two
    projection kernels."""
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
        valid = (tok >= 0) & (tok < tb.shape[0])
        rows = tb[tok.clamp(0, tb.shape[0] - 1)] * valid[..., None]
        cnt = valid.sum(1).to(torch.float64)
        some = cnt > 0
        safe = torch.where(some, cnt, torch.ones_like(cnt))
        inv = {"sum": torch.ones_like(cnt), "mean": 1.0 / safe, "sqrtn": 1.0 / safe.sqrt()}[how] * some
        ie = ie + rows.sum(1) * inv[:, None]
    projs = {}
    for side, ids, cur in (("user", uid, ue), ("item", iid, ie)):
        if features.get(side) is None:
            continue
        feat, mean, inv_std, p, clip = features[side]
        z = (c(feat)[ids] - c(mean)) * c(inv_std)
        if clip > 0:
            z = z.clamp(-clip, clip)
        projs[side] = f(p)
        if side == "user":
            ue = cur + z @ projs[side]
        else:
            ie = cur + z @ projs[side]
    ue.retain_grad(); ie.retain_grad()
    params, outs = [], []
    for x, (ws, bs), masks in ((ue, towers[0], relu_masks[0]), (ie, towers[1], relu_masks[1])):
        ws, bs = [f(w) for w in ws], [f(b) for b in bs]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                x = x * c(masks[l])
        params.append((ws, bs))
        outs.append(x)
    for o in outs:
        o.retain_grad()
    s = outs[0] @ outs[1].t() / temperature
    b = len(uid)
    if cand_ids is not None:                             # a sampled candidate that IS the row's positive: a false negative
        pos = torch.from_numpy(np.asarray(item_ids, dtype=np.int64))
        same = iid[None, :] == pos[:, None]
        same[torch.arange(b), torch.arange(b)] = False
        s = s.masked_fill(same, float("-inf"))
    loss = (torch.logsumexp(s, dim=1) - s[torch.arange(b), torch.arange(b)]).sum()
    loss.backward()
    g = lambda t: t.grad.numpy()
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b) for b in bs] for _, bs in params],
                dp={side: g(p) for side, p in projs.items()})

"""Restatements of the cross-layer contract of include/twotower_hip.h (tt_cross_fwd_f32 / tt_cross_bwd_f32) and of the train
step with the cross stack, shared by tests/test_cross_cpu.py and tests/test_gpu_cross.py.

* ``layer_forward`` / ``layer_backward``: one DCN-v2 cross layer and every backward quantity in f64 NumPy.  ``layer_backward``
  takes u as an argument, so a GPU test can hand it the DEVICE's u.
* ``stack_forward``: L layers from x_0.
* ``slab_rows``: the contiguous row blocks of the backward launch.
* ``step_f64``: the train step from the towers' summed input rows x_0 on - cross stack, Dense stack, optional L2 normalisation,
  in-batch softmax loss, optional rating head - in f64 torch-CPU autograd, the ReLU masks handed in.  Everything in front of
  x_0 (lookups, bags, projected features) is the business of the features' own tests: the step is handed the device's x_0.
* the tensor ids of the synthetic initialiser, restated from trainer.py.
"""
import numpy as np

TID_CROSS_BASE = 48            # layer l of tower t: 48 + 2 l + t
TRAINER_TIDS_IN_USE = set(range(1, 16)) | set(range(16, 32)) | {40, 41} | set(range(64, 64 + 16))


def layer_forward(x0, x, w, b):
    """(u, y) in f64: u = x W + b, y = x0 * u + x."""
    x0, x, w, b = (np.asarray(t, dtype=np.float64) for t in (x0, x, w, b))
    u = x @ w + b[None, :]
    return u, x0 * u + x


def stack_forward(x0, ws, bs):
    """x_1 .. x_L and u_0 .. u_{L-1} in f64."""
    x0 = np.asarray(x0, dtype=np.float64)
    xs, us, x = [], [], x0
    for w, b in zip(ws, bs):
        u, x = layer_forward(x0, x, w, b)
        us.append(u); xs.append(x)
    return xs, us


def layer_backward(x0, x, u, w, g, x_is_x0=False, dx0_in=None):
    """The contract's backward quantities in f64 from the given u: dict(dx, dx0, dw, db).  Upper form: dx = g + t W^T and
    dx0 = [dx0_in +] g * u.  Layer-0 form (x is x0): dx = g + t W^T + g * u [+ dx0_in], dx0 None."""
    x0, x, u, w, g = (np.asarray(t, dtype=np.float64) for t in (x0, x, u, w, g))
    t = g * x0
    dx = g + t @ w.T
    gu = g * u
    extra = 0.0 if dx0_in is None else np.asarray(dx0_in, dtype=np.float64)
    if x_is_x0:
        return dict(dx=dx + gu + extra, dx0=None, dw=x.T @ t, db=t.sum(0))
    return dict(dx=dx, dx0=gu + extra, dw=x.T @ t, db=t.sum(0))


def slab_rows(n, n_slabs):
    """Slab s holds rows [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs)."""
    r = -(-n // n_slabs) if n else 0
    return [(min(s * r, n), min((s + 1) * r, n)) for s in range(n_slabs)]


def step_f64(x0_user, x0_item, cross, towers, temperature, relu_masks, normalize_eps=None, item_ids=None, cand_ids=None,
             head=None, ratings=None, rating_weight=0.0, head_mask=None):
    """f64 torch-CPU autograd of one step from the summed input rows on.  ``cross`` = ((Ws, bs), (Ws, bs)) per tower, ``towers``
    = ((ws, bs), (ws, bs)), ``relu_masks`` the towers' hidden masks.  Mixed negative sampling: ``x0_item`` holds B + N rows,
    ``item_ids`` [B] / ``cand_ids`` [B + N] mark the sampled candidates that ARE a row's positive (masked).  ``head`` = (W1, b1,
    w2, b2) with ``ratings`` / ``rating_weight`` / ``head_mask``: total = retrieval + rating_weight * L_r.
    Returns the retrieval loss and the gradients of the total: dx0 (per tower), dw / db (towers), dcw / dcb (cross), dq, dc."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    xs0 = [f(x0_user), f(x0_item)]
    cparams, params, outs = [], [], []
    for x0, (cws, cbs), (ws, bs), masks in zip(xs0, cross, towers, relu_masks):
        cws, cbs = [f(w) for w in cws], [f(b) for b in cbs]
        x = x0
        for w, b in zip(cws, cbs):
            x = x0 * (x @ w + b) + x
        ws, bs = [f(w) for w in ws], [f(b) for b in bs]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                x = x * c(masks[l])
        cparams.append((cws, cbs)); params.append((ws, bs))
        if normalize_eps is not None:
            x = x / torch.sqrt(torch.clamp((x * x).sum(1, keepdim=True), min=normalize_eps))
        x.retain_grad()
        outs.append(x)
    b = outs[0].shape[0]
    s = outs[0] @ outs[1].t() / temperature
    if cand_ids is not None:
        pos, cand = torch.from_numpy(np.asarray(item_ids, dtype=np.int64)), torch.from_numpy(np.asarray(cand_ids, dtype=np.int64))
        same = cand[None, :] == pos[:, None]
        same[torch.arange(b), torch.arange(b)] = False
        s = s.masked_fill(same, float("-inf"))
    retrieval = (torch.logsumexp(s, dim=1) - s[torch.arange(b), torch.arange(b)]).sum()
    total = retrieval
    hp = None
    if head is not None:
        hp = [f(t) for t in head]
        w1, b1, w2, b2 = hp
        d = outs[0].shape[1]
        a = b1 + outs[0] @ w1[:d] + outs[1][:b] @ w1[d:]
        pred = (a * c(head_mask)) @ w2 + b2
        r = np.asarray(ratings, dtype=np.float64)
        valid = np.isfinite(r)
        e = (pred - c(np.where(valid, r, 0.0))) * c(valid.astype(np.float64))
        total = retrieval + rating_weight * (e * e).sum() / b
    total.backward()
    g = lambda t: t.grad.numpy()
    return dict(loss=float(retrieval.detach()), dx0=[g(x) for x in xs0], dq=g(outs[0]), dc=g(outs[1]),
                q=outs[0].detach().numpy(), c=outs[1].detach().numpy(),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b_) for b_ in bs] for _, bs in params],
                dcw=[[g(w) for w in ws] for ws, _ in cparams], dcb=[[g(b_) for b_ in bs] for _, bs in cparams])

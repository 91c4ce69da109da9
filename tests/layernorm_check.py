"""Restatements of the layer-normalisation contract of include/twotower_hip.h (tt_layer_norm_fwd_f32 / tt_layer_norm_bwd_f32)
and of the train step with normalised hidden layers, shared by tests/test_layernorm_cpu.py and tests/test_gpu_layernorm.py.

* ``layer_forward`` / ``layer_backward``: one normalisation and every backward quantity in f64 NumPy.
* ``layer_forward_f32`` / ``layer_backward_f32``: the same two-pass arithmetic with every operation rounded to f32 (sums in
  index order): what any f32 kernel can be expected to reach against f64.
* ``slab_rows``: the contiguous row blocks of the backward launch.
* ``problem``: the distributions the bars were worked out for.
* ``step_f64``: the train step from the towers' summed input rows x_0 on - optional cross stack, Dense stack with LayerNorm
  between every hidden layer and its ReLU, optional L2 normalisation, softmax loss, optional rating head - in f64 torch-CPU
  autograd.  The activation masks are handed in as multipliers (the device's (acts > 0) times its dropout scale), so a sign
  that differs between f32 and f64 does not count as an error of the step.
"""
import numpy as np

SHAPES = [(1, 32),          # a single row
          (37, 32),         # several rows per wave, ragged last group
          (130, 96),        # width no power of two
          (77, 160),        # width no power of two
          (257, 256),       # a whole wave per row, one row past a block
          (64, 512),        # 512 columns
          (33, 1024),       # the widest row
          (1000, 128)]      # several slabs
EPSILONS = (1e-3, 1e-5)


def problem(n, d):
    rng = np.random.default_rng(1000 * d + n)
    f = lambda a: a.astype(np.float32)
    return dict(z=f(0.5 + 1.5 * rng.standard_normal((n, d))), gamma=f(rng.uniform(0.5, 1.5, d)), beta=f(rng.uniform(-0.2, 0.2, d)),
                dn=f(rng.standard_normal((n, d))))


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def layer_forward(z, gamma, beta, eps, relu=False):
    """(y, xhat, r) in f64: mu = mean(z), var = mean((z - mu)^2), r = 1 / sqrt(var + eps), y = [relu](xhat * gamma + beta)."""
    z, gamma, beta = (np.asarray(t, dtype=np.float64) for t in (z, gamma, beta))
    mu = z.mean(1, keepdims=True)
    d = z - mu
    r = 1.0 / np.sqrt((d * d).mean(1, keepdims=True) + eps)
    xhat = d * r
    y = xhat * gamma[None, :] + beta[None, :]
    return (np.maximum(y, 0.0) if relu else y), xhat, r


def layer_backward(z, gamma, dn, eps, rows=None):
    """dict(dz, dgamma, dbeta) in f64 for dn = dL/d(xhat * gamma + beta); ``rows`` = (lo, hi): the sums over those rows only."""
    z, gamma, dn = (np.asarray(t, dtype=np.float64) for t in (z, gamma, dn))
    _, xhat, r = layer_forward(z, gamma, np.zeros_like(gamma), eps)
    g = dn * gamma[None, :]
    dz = r * (g - g.mean(1, keepdims=True) - xhat * (g * xhat).mean(1, keepdims=True))
    lo, hi = (0, len(z)) if rows is None else rows
    return dict(dz=dz, dgamma=(dn * xhat)[lo:hi].sum(0), dbeta=dn[lo:hi].sum(0))


def _sum32(a, axis):
    """Sum along ``axis`` in index order, every partial sum rounded to f32."""
    a = np.moveaxis(np.asarray(a, dtype=np.float32), axis, 0)
    s = np.zeros(a.shape[1:], dtype=np.float32)
    for x in a:
        s = (s + x).astype(np.float32)
    return s


def layer_forward_f32(z, gamma, beta, eps, relu=False):
    """``layer_forward`` with every operation rounded to f32 (two-pass; products and sums rounded separately)."""
    f = np.float32
    z, gamma, beta = (np.asarray(t, dtype=f) for t in (z, gamma, beta))
    n = f(z.shape[1])
    mu = (_sum32(z, 1) / n).astype(f)[:, None]
    d = (z - mu).astype(f)
    var = (_sum32((d * d).astype(f), 1) / n).astype(f)[:, None]
    r = (f(1.0) / np.sqrt((var + f(eps)).astype(f)).astype(f)).astype(f)
    xhat = (d * r).astype(f)
    y = ((xhat * gamma[None, :]).astype(f) + beta[None, :]).astype(f)
    return (np.maximum(y, f(0.0)) if relu else y), xhat, r


def layer_backward_f32(z, gamma, dn, eps):
    f = np.float32
    z, gamma, dn = (np.asarray(t, dtype=f) for t in (z, gamma, dn))
    n = f(z.shape[1])
    _, xhat, r = layer_forward_f32(z, gamma, np.zeros_like(gamma), eps)
    g = (dn * gamma[None, :]).astype(f)
    m1 = (_sum32(g, 1) / n).astype(f)[:, None]
    m2 = (_sum32((g * xhat).astype(f), 1) / n).astype(f)[:, None]
    dz = (((g - m1).astype(f) - (xhat * m2).astype(f)).astype(f) * r).astype(f)
    return dict(dz=dz, dgamma=_sum32((dn * xhat).astype(f), 0), dbeta=_sum32(dn, 0))


def slab_rows(n, n_slabs):
    """Slab s holds rows [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs)."""
    r = -(-n // n_slabs) if n else 0
    return [(min(s * r, n), min((s + 1) * r, n)) for s in range(n_slabs)]


def tower_forward(x0, cross, tower, norm, eps, normalize_eps=None):
    """The inference pass of one tower in f64 NumPy: cross stack, Dense -> LayerNorm -> ReLU per hidden layer, linear output."""
    x0 = np.asarray(x0, dtype=np.float64)
    x = x0
    for w, b in zip(*cross):
        x = x0 * (x @ np.asarray(w, dtype=np.float64) + np.asarray(b, dtype=np.float64)) + x
    ws, bs = tower
    for l, (w, b) in enumerate(zip(ws, bs)):
        x = x @ np.asarray(w, dtype=np.float64) + np.asarray(b, dtype=np.float64)
        if l < len(ws) - 1:
            x = layer_forward(x, norm[0][l], norm[1][l], eps, relu=True)[0]
    if normalize_eps is not None:
        x = x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), normalize_eps))
    return x


def step_f64(x0_user, x0_item, cross, towers, norms, eps, temperature, masks, normalize_eps=None, item_ids=None, cand_ids=None,
             head=None, ratings=None, rating_weight=0.0, head_mask=None):
    """f64 torch-CPU autograd of one step from the summed input rows on.  Per tower: ``cross`` = (Ws, bs) (empty lists: no cross
    stack), ``towers`` = (ws, bs), ``norms`` = (gammas, betas) per hidden layer, ``masks`` = per hidden layer the multiplier of
    the normalised value (the device's (acts > 0) times the dropout scale).  Mixed negative sampling: ``x0_item`` holds B + N
    rows, ``item_ids`` [B] / ``cand_ids`` [B + N] mark the sampled candidates that ARE a row's positive (masked).  ``head`` =
    (W1, b1, w2, b2) with ``ratings`` / ``rating_weight`` / ``head_mask``: total = retrieval + rating_weight * L_r.
    Returns the retrieval loss and the gradients of the total: dx0 (per tower), dw / db (towers), dgamma / dbeta (norms),
    dcw / dcb (cross), dq, dc."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    xs0 = [f(x0_user), f(x0_item)]
    cparams, params, nparams, outs = [], [], [], []
    for x0, (cws, cbs), (ws, bs), (gs, betas), ms in zip(xs0, cross, towers, norms, masks):
        cws, cbs = [f(w) for w in cws], [f(b) for b in cbs]
        x = x0
        for w, b in zip(cws, cbs):
            x = x0 * (x @ w + b) + x
        ws, bs, gs, betas = [f(w) for w in ws], [f(b) for b in bs], [f(g) for g in gs], [f(b) for b in betas]
        for l, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w + b
            if l < len(ws) - 1:
                mu = x.mean(1, keepdim=True)
                d = x - mu
                xhat = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
                x = (xhat * gs[l] + betas[l]) * c(ms[l])
        cparams.append((cws, cbs)); params.append((ws, bs)); nparams.append((gs, betas))
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
    if head is not None:
        w1, b1, w2, b2 = (f(t) for t in head)
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
                dgamma=[[g(t) for t in gs] for gs, _ in nparams], dbeta=[[g(t) for t in bs] for _, bs in nparams],
                dcw=[[g(w) for w in ws] for ws, _ in cparams], dcb=[[g(b_) for b_ in bs] for _, bs in cparams])

"""Restatements of the time-of-interaction context contract of include/twotower_hip.h (tt_time_context_fwd_f32 /
tt_time_context_bwd_f32) and of the train step with the feature, shared by tests/test_time_cpu.py and tests/test_gpu_time.py.

* ``time_indices`` is the index arithmetic - integer, floor-divided, civil-from-days for the month - of every enabled field, in
  NumPy int64 (``//`` floors): [n, F] int32, -1 everywhere for ``TIME_MISSING``.
* ``time_forward`` repeats the device's f32 arithmetic operation by operation: s = ((row_0 + row_1) + row_2) + row_3 over the
  enabled fields in order (+0 for a pair without a timestamp), then out = s | out + s | base row + s - compared BIT FOR BIT.
* ``time_backward`` is the table gradient in the kernel's FIXED order: 32 sub-sums, sub-sum g over the matching positions
  g, g + 32, g + 64, ... ascending from +0, then (((s_0 + s_1) + s_2) + ... + s_31) - compared BIT FOR BIT.
  ``time_backward_f64`` is the same sum in f64.
* ``step_f64`` is the whole train step in f64 torch-CPU autograd, the ReLU masks handed in: the user tower's input is the id row
  (+ the pooled history, the pair's own item left out) + the time rows; the item tower's the id row (+ category + pooled titles).
"""
import numpy as np

FIELDS = ("hour", "day_of_week", "month", "period")
ROWS = {"hour": 24, "day_of_week": 7, "month": 12}
TIME_MISSING = -2 ** 63
SUBSUMS = 32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ordered(fields):
    return tuple(f for f in FIELDS if f in fields)


def layout(fields, buckets=0):
    """(offsets {field: first row}, R) in the fixed field order."""
    offsets, r = {}, 0
    for f in ordered(fields):
        offsets[f] = r
        r += buckets if f == "period" else ROWS[f]
    return offsets, r


def calendar(t):
    """(hour, day_of_week [Monday 0], month - 1) of int64 seconds since the epoch; NumPy's // and % floor."""
    t = np.asarray(t, dtype=np.int64)
    days = t // 86400
    hour = (t - 86400 * days) // 3600
    dow = (days + 3) % 7
    z = days + 719468
    era = z // 146097
    doe = z - 146097 * era
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    month = np.where(mp < 10, mp + 3, mp - 9)
    return hour, dow, month - 1


def period(t, buckets, time_min, time_max):
    """floor(clamp(t - time_min, 0, span) * N / (span + 1)) in Python integers (no overflow whatever t is)."""
    span = int(time_max) - int(time_min)
    return np.array([min(max(int(x) - int(time_min), 0), span) * buckets // (span + 1) for x in np.asarray(t).reshape(-1)], dtype=np.int64)


def time_indices(t, fields, buckets=0, time_min=0, time_max=0):
    t = np.asarray(t, dtype=np.int64)
    missing = t == TIME_MISSING
    safe = np.where(missing, 0, t)
    hour, dow, month = calendar(safe)
    cols = {"hour": hour, "day_of_week": dow, "month": month}
    if "period" in fields:
        cols["period"] = period(safe, buckets, time_min, time_max)
    idx = np.stack([cols[f] for f in ordered(fields)], axis=1).astype(np.int32)
    idx[missing] = -1
    return idx


def time_forward(t, table, fields, buckets=0, time_min=0, time_max=0, accumulate=False, out=None, base=None):
    """Returns (out [n, dim] f32, idx [n, F] int32, flag 0/1).  ``base`` = (base_table, base_ids)."""
    table = np.asarray(table, dtype=np.float32)
    idx = time_indices(t, fields, buckets, time_min, time_max)
    offs, _ = layout(fields, buckets)
    s = None
    for k, f in enumerate(ordered(fields)):
        row = np.where((idx[:, k] >= 0)[:, None], table[offs[f] + np.maximum(idx[:, k], 0)], np.float32(0))
        s = row if s is None else (s + row).astype(np.float32)
    flag = 0
    if base is not None:
        bt, ids = np.asarray(base[0], dtype=np.float32), np.asarray(base[1], dtype=np.int64)
        ok = (ids >= 0) & (ids < bt.shape[0])
        flag = int((~ok & (ids != -1)).any())
        b = np.where(ok[:, None], bt[np.where(ok, ids, 0)], np.float32(0))
        s = (b + s).astype(np.float32)
    elif accumulate:
        s = (np.asarray(out, dtype=np.float32) + s).astype(np.float32)
    return s.astype(np.float32), idx, flag


def time_backward(idx, dy, fields, buckets=0):
    """grad [R, dim] f32 in the kernel's order.  Step t adds the (up to) 32 positions 32 t + g, one per sub-sum g, so the fancy-
    indexed add below never meets an accumulator twice: every add is one rounded f32 operation, in ascending t."""
    idx, dy = np.asarray(idx), np.asarray(dy, dtype=np.float32)
    n, dim = dy.shape
    offs, R = layout(fields, buckets)
    sub = np.zeros((SUBSUMS, R, dim), dtype=np.float32)
    for k, f in enumerate(ordered(fields)):
        card = buckets if f == "period" else ROWS[f]
        col = idx[:, k].astype(np.int64)
        for p0 in range(0, n, SUBSUMS):
            p = np.arange(p0, min(p0 + SUBSUMS, n))
            hit = (col[p] >= 0) & (col[p] < card)
            g, r = (p - p0)[hit], offs[f] + col[p][hit]
            sub[g, r] = (sub[g, r] + dy[p[hit]]).astype(np.float32)
    grad = sub[0].copy()
    for g in range(1, SUBSUMS):
        grad = (grad + sub[g]).astype(np.float32)
    return grad


def time_backward_f64(idx, dy, fields, buckets=0):
    idx, dy = np.asarray(idx), np.asarray(dy, dtype=np.float64)
    offs, R = layout(fields, buckets)
    grad = np.zeros((R, dy.shape[1]))
    for k, f in enumerate(ordered(fields)):
        card = buckets if f == "period" else ROWS[f]
        hit = (idx[:, k] >= 0) & (idx[:, k] < card)
        np.add.at(grad, offs[f] + idx[hit, k].astype(np.int64), dy[hit])
    return grad


def step_f64(user_table, item_table, towers, user_ids, item_ids, time, temperature, relu_masks, cand_ids=None, category=None,
             title=None, history=None):
    """f64 torch-CPU autograd of one step with the time feature.  ``time`` = (time_table, idx [n, F] int, fields, buckets);
    ``cand_ids`` (mixed negative sampling): the item side's ids, batch items first - a sampled candidate equal to a row's own
    positive is masked out of that row, as the scorer does; ``category`` = (table, ids); ``title`` = (table, tokens [n_items, L],
    pooling); ``history`` = (table, tokens [n_users, L], pooling), the pair's own item left out.  Returns the loss and the gradients
    w.r.t. the tower inputs and outputs, every kernel and bias and the time table."""
    import torch
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    ut, it = f(user_table), f(item_table)
    uid = torch.from_numpy(np.asarray(user_ids, dtype=np.int64))
    pos = torch.from_numpy(np.asarray(item_ids, dtype=np.int64))
    iid = pos if cand_ids is None else torch.from_numpy(np.asarray(cand_ids, dtype=np.int64))

    def pooled(tb, tok, how):
        valid = (tok >= 0) & (tok < tb.shape[0])
        rows = tb[tok.clamp(0, tb.shape[0] - 1)] * valid[..., None]
        cnt = valid.sum(1).to(torch.float64)
        some = cnt > 0
        safe = torch.where(some, cnt, torch.ones_like(cnt))
        inv = {"sum": torch.ones_like(cnt), "mean": 1.0 / safe, "sqrtn": 1.0 / safe.sqrt()}[how] * some
        return rows.sum(1) * inv[:, None]

    ue, ie = ut[uid], it[iid]
    if history is not None:
        tok = torch.from_numpy(np.asarray(history[1]).astype(np.int64))[uid]
        tok = torch.where(tok == pos[:, None], torch.full_like(tok, -1), tok)
        ue = ue + pooled(c(history[0]), tok, history[2])
    tt_, idx, fields, buckets = f(time[0]), np.asarray(time[1]).astype(np.int64), time[2], time[3]
    offs, _ = layout(fields, buckets)
    for k, fld in enumerate(ordered(fields)):
        col = torch.from_numpy(idx[:, k])
        ue = ue + tt_[offs[fld] + col.clamp(min=0)] * (col >= 0)[:, None]
    if category is not None:
        ie = ie + c(category[0])[torch.from_numpy(np.asarray(category[1], dtype=np.int64))]
    if title is not None:
        ie = ie + pooled(c(title[0]), torch.from_numpy(np.asarray(title[1]).astype(np.int64))[iid], title[2])
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
    if cand_ids is not None:
        same = iid[None, :] == pos[:, None]
        same[torch.arange(b), torch.arange(b)] = False
        s = s.masked_fill(same, float("-inf"))
    loss = (torch.logsumexp(s, dim=1) - s[torch.arange(b), torch.arange(b)]).sum()
    loss.backward()
    g = lambda t: t.grad.numpy()
    return dict(loss=float(loss.detach()), due=g(ue), die=g(ie), dq=g(outs[0]), dc=g(outs[1]), time_table=g(tt_),
                dw=[[g(w) for w in ws] for ws, _ in params], db=[[g(b) for b in bs] for _, bs in params])

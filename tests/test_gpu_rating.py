"""The rating-prediction head on the GPU (tt_rating_head_fwd_f32 / tt_rating_head_bwd_f32, csrc/rating.hip): both launches against
the f64 restatement of tests/rating_check.py and against the same math as torch f32 ops, then the trainer - parity with the f64
autograd restatement for every optimizer, with normalised embeddings, with the input features and under mixed negative sampling,
the head-off path, checkpoints, predict_ratings - the custom op, the CLIs and the refusals.

Bars: a kernel against its f64 restatement rel_err <= 1e-5 (tests/test_gpu_parity.py test_dense_fwd / test_dense_bwd); a trainer
step the bars of tests/test_gpu_features.py::_check_step."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import rating_check as rc
from two_tower_amazon_recommender_amd import _lib, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

SHAPES = [(77, 32, 32), (1000, 128, 96), (256, 256, 256), (33, 64, 160),
          # the other hidden widths: every multiple of 32 in 32..256 is run at the kernels' own bars (tests/test_rating_cpu.py: the
          # same math in f32 stays within them on these problems)
          (65, 32, 64), (130, 64, 224), (40, 128, 192), (33, 256, 128)]


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def _problem(n, d, h):
    """q, c, the four parameters, ratings (about a tenth NaN) and sample weights in [0, 2] (some exactly 0); never modified."""
    rng = np.random.default_rng(7 * n + 3 * d + h)
    q = rng.uniform(-1.0, 1.0, (n, d)).astype(np.float32)
    c = rng.uniform(-1.0, 1.0, (n, d)).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * d + h))
    w1 = rng.uniform(-lim, lim, (2 * d, h)).astype(np.float32)
    b1 = rng.uniform(-0.2, 0.2, h).astype(np.float32)
    w2 = rng.uniform(-0.5, 0.5, h).astype(np.float32)
    b2 = np.array([3.5], dtype=np.float32)
    rating = rng.integers(1, 6, n).astype(np.float32)
    rating[rng.random(n) < 0.1] = np.nan
    rating[0] = np.nan
    sw = rng.uniform(0.0, 2.0, n).astype(np.float32)
    sw[rng.random(n) < 0.1] = 0.0
    sw[1] = 0.0
    return q, c, w1, b1, w2, b2, rating, sw


def _forward(dev, n, d, h):
    q, c, w1, b1, w2, b2, _, _ = _problem(n, d, h)
    pred_buf = torch.full((n + 1,), float("nan"), device=dev)
    h_buf = torch.full((n + 1, h), float("nan"), device=dev)
    ops.rating_head(T(q, dev), T(c, dev), T(w1, dev), T(b1, dev), T(w2, dev), T(b2, dev), pred=pred_buf[:n], h=h_buf[:n])
    return pred_buf, h_buf


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("n,d,h", SHAPES)
def test_forward_matches_f64(dev, n, d, h):
    q, c, w1, b1, w2, b2, _, _ = _problem(n, d, h)
    pred_buf, h_buf = _forward(dev, n, d, h)
    pred, hid = pred_buf.cpu().numpy(), h_buf.cpu().numpy()
    rpred, rh, _ = rc.head_forward(q, c, w1, b1, w2, b2)
    print(f"forward ({n}, {d}, {h}): pred {rel_err(pred[:n], rpred):.2e}  h {rel_err(hid[:n], rh):.2e}")
    assert rel_err(pred[:n], rpred) <= 1e-5
    assert rel_err(hid[:n], rh) <= 1e-5
    assert (hid[:n] >= 0).all()
    assert np.isnan(pred[n]) and np.isnan(hid[n]).all()          # the row behind n is not written


# ------------------------------------------------------------------------------------------ 2. backward
def _backward(dev, n, d, h, n_slabs, accumulate=False, dq0=None, dc0=None, weights=True):
    q, c, w1, b1, w2, b2, rating, sw = _problem(n, d, h)
    pred_buf, h_buf = _forward(dev, n, d, h)
    scale = 2.0 * 0.5 / n
    nan = float("nan")
    dq = torch.full((n + 1, d), nan, device=dev) if dq0 is None else torch.cat([T(dq0, dev), torch.full((1, d), nan, device=dev)])
    dc = torch.full((n + 1, d), nan, device=dev) if dc0 is None else torch.cat([T(dc0, dev), torch.full((1, d), nan, device=dev)])
    ks = torch.full((n_slabs, 2 * d * h + h), nan, device=dev)
    bs = torch.full((n_slabs, h + 1), nan, device=dev)
    se = torch.full((n_slabs,), nan, device=dev)
    ops.rating_head_bwd(T(q, dev), T(c, dev), h_buf[:n], pred_buf[:n], T(rating, dev), T(w1, dev), T(w2, dev), scale, dq[:n], dc[:n],
                        ks, bs, se, sample_weight=T(sw, dev) if weights else None, accumulate=accumulate)
    return dict(dq=dq.cpu().numpy(), dc=dc.cpu().numpy(), ks=ks.cpu().numpy(), bs=bs.cpu().numpy(), se=se.cpu().numpy(),
                pred=pred_buf[:n].cpu().numpy(), h=h_buf[:n].cpu().numpy(), scale=scale)


@pytest.mark.parametrize("n,d,h", SHAPES)
def test_backward_matches_f64(dev, n, d, h):
    q, c, w1, b1, w2, b2, rating, sw = _problem(n, d, h)
    for n_slabs in (1, ops.rating_head_num_slabs(n), n // 32 + 5):
        got = _backward(dev, n, d, h, n_slabs)
        ref = rc.head_backward(q, c, got["h"], got["pred"], rating, w1, w2, got["scale"], sw)     # the DEVICE's h and pred
        for k in ("dq", "dc", "ks", "bs", "se"):
            assert np.isfinite(got[k][:n] if k in ("dq", "dc") else got[k]).all(), (k, n_slabs)
        assert np.isnan(got["dq"][n]).all() and np.isnan(got["dc"][n]).all()
        ks, bs = got["ks"].astype(np.float64).sum(0), got["bs"].astype(np.float64).sum(0)
        errs = dict(dq=rel_err(got["dq"][:n], ref["dq"]), dc=rel_err(got["dc"][:n], ref["dc"]),
                    dw1=rel_err(ks[:2 * d * h].reshape(2 * d, h), ref["dw1"]), dw2=rel_err(ks[2 * d * h:], ref["dw2"]),
                    db1=rel_err(bs[:h], ref["db1"]), db2=rel_err(bs[h:], np.array([ref["db2"]])),
                    se=rel_err(np.array([got["se"].astype(np.float64).sum()]), np.array([ref["se"]])))
        print(f"backward ({n}, {d}, {h}) n_slabs {n_slabs}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert all(v <= 1e-5 for v in errs.values()), errs
        # rows without a label, and rows of weight 0: exactly zero gradient
        dead = ~np.isfinite(rating) | (sw == 0)
        assert dead.sum() >= 2 and not got["dq"][:n][dead].any() and not got["dc"][:n][dead].any()
        for s, (lo, hi) in enumerate(rc.slab_rows(n, n_slabs)):
            if lo == hi:                                         # a slab without rows: exact zeros
                assert not got["ks"][s].any() and not got["bs"][s].any() and got["se"][s] == 0


@pytest.mark.parametrize("n,d,h", SHAPES)
def test_backward_accumulates_bit_for_bit_and_repeats(dev, n, d, h):
    rng = np.random.default_rng(n)
    dq0 = rng.standard_normal((n, d)).astype(np.float32)
    dc0 = rng.standard_normal((n, d)).astype(np.float32)
    ns = ops.rating_head_num_slabs(n)
    over = _backward(dev, n, d, h, ns)
    again = _backward(dev, n, d, h, ns)
    for k in ("dq", "dc", "ks", "bs", "se"):
        assert np.array_equal(over[k].view(np.uint32), again[k].view(np.uint32)), k
    acc = _backward(dev, n, d, h, ns, accumulate=True, dq0=dq0, dc0=dc0)
    for k, base in (("dq", dq0), ("dc", dc0)):
        want = (base + over[k][:n]).astype(np.float32)
        assert np.array_equal(acc[k][:n].view(np.uint32), want.view(np.uint32)), k
    for k in ("ks", "bs", "se"):
        assert np.array_equal(acc[k].view(np.uint32), over[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------ 3. equivalence with torch f32 ops
@pytest.mark.parametrize("n,d,h", SHAPES)
def test_launches_equal_the_torch_sequence(dev, n, d, h):
    q, c, w1, b1, w2, b2, rating, sw = _problem(n, d, h)
    tq, tc, tw1, tb1, tw2, tb2 = (T(a, dev).requires_grad_() for a in (q, c, w1, b1, w2, b2))
    hid = torch.relu(torch.addmm(tb1, torch.cat([tq, tc], dim=1), tw1))
    pred = torch.mv(hid, tw2) + tb2
    valid = torch.isfinite(T(rating, dev))
    e = torch.where(valid, pred - torch.nan_to_num(T(rating, dev)), torch.zeros_like(pred))
    loss = 0.5 * (T(sw, dev) * e * e).sum() / n
    loss.backward()
    got = _backward(dev, n, d, h, ops.rating_head_num_slabs(n))
    ks, bs = got["ks"].astype(np.float64).sum(0), got["bs"].astype(np.float64).sum(0)
    g = lambda t: t.grad.cpu().numpy().astype(np.float64)
    assert rel_err(got["pred"], pred.detach().cpu().numpy().astype(np.float64)) <= 1e-5
    assert rel_err(got["h"], hid.detach().cpu().numpy().astype(np.float64)) <= 1e-5
    errs = dict(dq=rel_err(got["dq"][:n], g(tq)), dc=rel_err(got["dc"][:n], g(tc)),
                dw1=rel_err(ks[:2 * d * h].reshape(2 * d, h), g(tw1)), dw2=rel_err(ks[2 * d * h:], g(tw2)),
                db1=rel_err(bs[:h], g(tb1)), db2=rel_err(bs[h:], g(tb2)),
                loss=rel_err(np.array([0.5 * got["se"].astype(np.float64).sum() / n]), np.array([loss.item()])))
    print(f"torch equivalence ({n}, {d}, {h}): " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-5 for v in errs.values()), errs


# ------------------------------------------------------------------------------------------ 11. refusals of the C entries
def test_c_entries_refuse_bad_arguments(dev):
    lib = _lib.load()
    n, d, h = 64, 32, 32
    q = torch.zeros(n + 1, d, device=dev); c = torch.zeros(n + 1, d, device=dev)
    w1 = torch.zeros(2 * d, h, device=dev); b1 = torch.zeros(h, device=dev); w2 = torch.zeros(h, device=dev); b2 = torch.zeros(1, device=dev)
    pred = torch.zeros(n, device=dev); hid = torch.zeros(n, h, device=dev); rating = torch.zeros(n, device=dev)
    dq = torch.zeros(n, d, device=dev); dc = torch.zeros(n, d, device=dev)
    ks = torch.zeros(2, 2 * d * h + h, device=dev); bs = torch.zeros(2, h + 1, device=dev); se = torch.zeros(2, device=dev)
    p = ops._p

    def fwd(qq=q, dd=d, hh=h, nn=n, w=w1):
        return lib.tt_rating_head_fwd_f32(p(qq) if qq is not None else None, p(c), nn, dd, hh, p(w), p(b1), p(w2), p(b2), p(pred), p(hid), None)

    def bwd(qq=q, dd=d, hh=h, nn=n, slabs=2, dqq=dq):
        return lib.tt_rating_head_bwd_f32(p(qq) if qq is not None else None, p(c), p(hid), p(pred), p(rating), None, 1.0, nn, dd, hh,
                                          p(w1), p(w2), p(dqq), p(dc), 0, p(ks), p(bs), p(se), slabs, None)

    for call, word in ((lambda: fwd(dd=48), b"D must"), (lambda: fwd(hh=40), b"H must"), (lambda: fwd(hh=288), b"H must"),
                       (lambda: fwd(qq=None), b"null"), (lambda: fwd(qq=q.view(-1)[1:]), b"aligned"),
                       (lambda: bwd(dd=16), b"D must"), (lambda: bwd(hh=0), b"H must"), (lambda: bwd(slabs=0), b"n_slabs"),
                       (lambda: bwd(slabs=65536), b"n_slabs"), (lambda: bwd(qq=None), b"null"),
                       (lambda: bwd(dqq=q.view(-1)[1:]), b"aligned")):
        assert call() == _lib.TT_ERR_INVALID_ARG
        assert word in lib.tt_last_error(), lib.tt_last_error()
    assert fwd(nn=0, qq=None) == _lib.TT_OK and bwd(nn=0, qq=None) == _lib.TT_OK
    with pytest.raises(ValueError):
        ops.rating_head(torch.zeros(4, 48, device=dev), torch.zeros(4, 48, device=dev), torch.zeros(96, 32, device=dev), b1, w2, b2)


# ------------------------------------------------------------------------------------------ 4. trainer
LR = 0.001
LR_SGD = 0.0001                      # plain SGD on the SUM loss (tests/test_gpu_features.py: 0.001 diverges with the projected features)
W, HID = 0.5, 32


def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=200, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR_SGD if opt == "sgd" else LR, optimizer=opt, batch_size=batch, **kw)


EXTRAS = dict(n_category_buckets=30, n_title_buckets=100, title_max_tokens=4, n_user_features=5, n_item_features=5, feature_clip=1.5)


def _head_trainer(dev, opt="adagrad", seed=1001, **kw):
    tr = TwoTowerTrainer(_cfg(opt, rating_weight=W, rating_hidden=HID, **kw), dev, seed=seed)
    if tr.user_features is not None:
        tr.set_user_features(tr.synthetic_user_features(seed))
    if tr.item_features is not None:
        tr.set_item_features(tr.synthetic_item_features(seed))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _ratings(dev, seed, step, batch=256):
    """Stars 1..5, about a tenth of them missing."""
    rng = np.random.default_rng(1000 * seed + step)
    r = rng.integers(1, 6, batch).astype(np.float32)
    r[rng.random(batch) < 0.1] = np.nan
    r[3] = np.nan
    return T(r, dev)


def _cut64(tr, t):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    return flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))


def _towers64(tr):
    return tuple(([_cut64(tr, w) for w in tw.w], [_cut64(tr, b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def _head64(tr):
    return tuple(_cut64(tr, t) for t in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating))


def _features64(tr):
    n = lambda t: t.cpu().numpy().astype(np.float64)
    return {side: (n(getattr(tr, f"{side}_features")), n(getattr(tr, f"{side}_feature_mean")), n(getattr(tr, f"{side}_feature_inv_std")),
                   n(getattr(tr, f"P_{side}")), tr.cfg.feature_clip) for side, _, _, _ in tr._feature_sides}


def _reference_step(tr, u, i, ratings, before, towers, head, feats, cand=None, category=None, title=None):
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    return rc.step_f64(before["user_table"], before["item_table"], towers, u.cpu().numpy(), i.cpu().numpy(), head, ratings.cpu().numpy(),
                       tr.cfg.rating_weight, tr.cfg.temperature, masks, (tr._r_h > 0).cpu().numpy(),
                       normalize_eps=tr.cfg.normalize_eps if tr.cfg.normalize_embeddings else None, cand_ids=cand,
                       category=category, title=title, features=feats)


def _check_step(tr, r, loss, step, batch):
    """The bars of tests/test_gpu_features.py::_check_step: loss within 1e-4 relative and 1e-4 per pair, every gradient within
    1e-4 of its max |g| - here for the rating loss and the four head gradients too."""
    d, hd = tr.cfg.tower_dims[-1], tr.cfg.rating_hidden
    lr = tr.rating_loss.item()
    print(f"step {step}: loss {loss} (f64 {r['loss']})  rating loss {lr} (f64 {r['rating_loss']})")
    assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
    assert abs(lr - r["rating_loss"]) <= 1e-4 * abs(r["rating_loss"]) and abs(lr - r["rating_loss"]) <= 1e-4, (lr, r["rating_loss"])
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    ks, bs = n64(tr._r_kslabs).sum(0), n64(tr._r_bslabs).sum(0)
    checks = [("due", n64(tr.user_tower.demb), r["due"]), ("die", n64(tr.item_tower.demb), r["die"]),
              ("dW1", ks[:2 * d * hd].reshape(2 * d, hd), r["dw1"]), ("dw2", ks[2 * d * hd:], r["dw2"]),
              ("db1", bs[:hd], r["db1"]), ("db2", bs[hd:], r["db2"])]
    for side, _, slabs, _ in tr._feature_sides:
        checks.append((f"dP_{side}", n64(slabs).sum(0), r["dp"][side]))
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(tw.n_layers):
            checks += [(f"dw[{t}][{l}]", n64(tw.dw_slabs[l]).sum(0), r["dw"][t][l]), (f"db[{t}][{l}]", n64(tw.db_slabs[l]).sum(0), r["db"][t][l])]
    last = f"db[1][{tr.item_tower.n_layers - 1}]"
    for what, got, want in checks:
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        if what == last and not tr.cfg.normalize_embeddings:
            # _check_step's own rule for the item tower's last bias: it is the column sums of dc, whose retrieval part cancels to
            # ZERO (the bias shifts every logit of a row alike) - what is left here is the head's small share, while the rounding
            # error is that of the rows the device sums: the bar is taken from their scale (max |dc|), as there
            scale = max(scale, np.abs(r["dc"]).max())
        print(f"step {step}: {what} error {err / scale:.2e} of max |g| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (step, what, err, scale)


@pytest.mark.parametrize("opt,variant", [("sgd", "plain"), ("adagrad", "extras"), ("adam", "normalize")])
def test_trainer_matches_the_f64_restatement_and_trains(dev, opt, variant):
    seed, batch = 1001, 256
    extras = variant == "extras"
    kw = dict(EXTRAS) if extras else (dict(normalize_embeddings=True) if variant == "normalize" else {})
    tr = _head_trainer(dev, opt, seed, **kw)
    assert len(tr._segs) == (10 if extras else 8) + 2 and (tr._adam_segs is None or len(tr._adam_segs) == len(tr._segs))
    assert tr.W1_rating.data_ptr() == tr.dense_flat.data_ptr() + 4 * (tr.dense_flat.numel() - (2 * 32 * HID + 2 * HID + 1))
    assert tr.b1_rating.abs().max().item() == 0 and tr.b2_rating.item() == 0 and tr.W1_rating.abs().max().item() > 0
    tr.init_rating_bias(3.0)
    assert tr.b2_rating.item() == 3.0
    for step in range(3):
        u, i = tr.synthetic_batch(seed, step, "Z")
        t = _ratings(dev, seed, step)
        cat = tr.synthetic_categories(seed, step) if extras else None
        ids, rows, plans = [u, i], [300, 200], [tr.user_plan, tr.item_plan]
        if extras:
            ids.append(cat); rows.append(30); plans.append(tr.cat_plan)
        ops.sparse_plan_batched(plans, ids, rows)
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
        towers, head, feats = _towers64(tr), _head64(tr), _features64(tr)
        category = (tr.cat_table.cpu().numpy(), cat.cpu().numpy()) if extras else None
        title = (tr.title_table.cpu().numpy(), tr.item_titles.cpu().numpy(), "mean") if extras else None
        loss = tr.forward_backward(u, i, category_ids=cat, ratings=t).item()
        tr.check_ids()
        r = _reference_step(tr, u, i, t, before, towers, head, feats, category=category, title=title)
        _check_step(tr, r, loss, step, batch)
        tr.apply_gradients()
    p0 = [p.clone() for p in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating)]
    totals = []
    u, i = tr.synthetic_batch(seed, 0, "Z")
    t = _ratings(dev, seed, 0)
    for step in range(6):
        loss = tr.step(u, i, ratings=t, **({"category_ids": tr.synthetic_categories(seed, 0)} if extras else {}))
        totals.append(loss.item() + W * tr.rating_loss.item())
    tr.check_ids()
    print(f"6 steps on one batch: total {totals[0]:.4f} -> {totals[-1]:.4f}")
    assert np.isfinite(totals).all() and totals[-1] < totals[0]
    for was, now in zip(p0, (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating)):
        assert not torch.equal(was, now) and torch.isfinite(now).all()
    assert torch.isfinite(tr.dense_flat).all() and torch.isfinite(tr.user_table).all() and torch.isfinite(tr.item_table).all()
    with pytest.raises(ValueError, match="ratings"):
        tr.step(u, i, **({"category_ids": tr.synthetic_categories(seed, 0)} if extras else {}))


# ------------------------------------------------------------------------------------------ 5. mixed negative sampling
def test_mixed_sampling_step_matches_the_f64_restatement(dev):
    seed, batch, n_neg = 77, 256, 64
    tr = _head_trainer(dev, "sgd", seed, candidate_sampling="mixed", n_sampled_negatives=n_neg)
    u, i = tr.synthetic_batch(seed, 0, "Z")
    t = _ratings(dev, seed, 0)
    before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
    towers, head = _towers64(tr), _head64(tr)
    loss = tr.forward_backward(u, i, ratings=t).item()
    tr.check_ids()
    cand = tr.cand_ids.cpu().numpy()
    assert np.array_equal(cand[:batch], i.cpu().numpy()) and len(cand) == batch + n_neg
    r = _reference_step(tr, u, i, t, before, towers, head, {}, cand=cand)
    _check_step(tr, r, loss, 0, batch)
    # the head's gradient is in the first B candidate rows only: behind them dc is the scorer's, bit for bit
    dq2, dc2 = torch.empty(batch, 32, device=dev), torch.empty(batch + n_neg, 32, device=dev)
    ops.retrieval_fwd_bwd(tr.user_tower.acts[-1], tr.item_tower.acts[-1], 1.0 / tr.cfg.temperature, tr.ws, tr.lse, tr.per_row, tr.loss,
                          dq2, dc2, cand_ids=tr.cand_ids)
    dc = tr.item_tower.dz[-1]
    assert torch.equal(dc[batch:], dc2[batch:]) and not torch.equal(dc[:batch], dc2[:batch])
    tr.apply_gradients(step_ids=[u, i])
    tr.step(*tr.synthetic_batch(seed, 1, "Z"), ratings=_ratings(dev, seed, 1))
    tr.evaluate(*tr.synthetic_batch(seed, 2, "Z"), ratings=_ratings(dev, seed, 2))
    tr.check_ids()
    assert torch.isfinite(tr.dense_flat).all() and np.isfinite(tr.eval_rating_se.item())


# ------------------------------------------------------------------------------------------ 6. head off
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_head_off_is_the_trainer_as_it_was(dev, opt):
    from two_tower_amazon_recommender_amd.trainer import Tower
    seed = 31
    a = TwoTowerTrainer(_cfg(opt, rating_weight=0.0, rating_hidden=64), dev, seed=seed)
    b = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    assert not a.rating_on and a.W1_rating is None and a._r_h is None and a._r_kslabs is None and a.rating_pred is None
    assert a.dense_flat.numel() == b.dense_flat.numel() == 2 * Tower.param_count(a.cfg, [64, 32])
    assert len(a._segs) == len(b._segs) == 8
    for s in range(3):
        a.step(*a.synthetic_batch(seed, s, "Z")); b.step(*b.synthetic_batch(seed, s, "Z"))
    a.check_ids()
    for k in ("user_table", "item_table", "dense_flat", "loss"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    u, i = a.synthetic_batch(seed, 0, "Z")
    for call in (a.step, a.forward_backward, a.evaluate):
        with pytest.raises(ValueError, match="no rating head"):
            call(u, i, ratings=_ratings(dev, seed, 0))
    with pytest.raises(ValueError, match="no rating head"):
        a.predict_ratings(u, i)
    with pytest.raises(ValueError, match="no rating head"):
        a.rating_loss


# ------------------------------------------------------------------------------------------ 7. checkpoints
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"), ratings=_ratings(dev, seed, s))
    a = _head_trainer(dev, opt, seed)
    run(a, range(4))
    b = _head_trainer(dev, opt, seed)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert (sd["config"]["rating_weight"], sd["config"]["rating_hidden"]) == (W, HID)
    assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + 2 * 32 * HID + 2 * HID + 1
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values
    c.load_state_dict(sd)
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "loss", "rating_pred", "_r_se"]
    names += ["user_accum", "item_accum", "dense_accum"] if opt == "adagrad" else ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.W1_rating, b.W1_rating)
    # a head-off checkpoint - one from before the fields existed too - loads into a head-off trainer; a mismatch is refused
    off = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    old = dict(off.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if k not in ("rating_weight", "rating_hidden")}
    off.load_state_dict(old)
    with pytest.raises(ValueError, match="rating head"):
        off.load_state_dict(sd)
    with pytest.raises(ValueError, match="rating head"):
        c.load_state_dict(old)
    wider = TwoTowerTrainer(_cfg(opt, rating_weight=W, rating_hidden=64), dev, seed=seed)
    with pytest.raises(ValueError, match="rating_hidden"):
        wider.load_state_dict(sd)


# ------------------------------------------------------------------------------------------ 8. predict_ratings
def test_predict_ratings_equals_the_restatement_on_the_trainers_embeddings(dev):
    seed = 23
    tr = _head_trainer(dev, "adagrad", seed, normalize_embeddings=True)
    tr.init_rating_bias(3.0)
    for s in range(2):
        tr.step(*tr.synthetic_batch(seed, s, "Z"), ratings=_ratings(dev, seed, s))
    rng = np.random.default_rng(seed)
    u = torch.from_numpy(rng.integers(0, 300, 1000)).to(dev)
    i = torch.from_numpy(rng.integers(0, 200, 1000)).to(dev)
    pred = tr.predict_ratings(u, i)
    tr.check_ids()
    q = tr.user_embeddings(u).cpu().numpy()
    c = tr.item_corpus_embeddings()[i].cpu().numpy()
    want, _, _ = rc.head_forward(q, c, *(t.cpu().numpy() for t in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating)))
    print(f"predict_ratings: rel_err {rel_err(pred.cpu().numpy(), want):.2e}")
    assert pred.shape == (1000,) and rel_err(pred.cpu().numpy(), want) <= 1e-5
    assert tr.predict_ratings(u[:0], i[:0]).shape == (0,)
    with pytest.raises(ValueError, match="one length"):
        tr.predict_ratings(u, i[:5])


# ------------------------------------------------------------------------------------------ 9. custom op
def test_custom_op_passes_opcheck_equals_the_ops_call_and_differentiates_every_input(dev):
    from two_tower_amazon_recommender_amd import tasks, torch_ops  # noqa: F401
    n, d, h = 77, 32, 64
    q, c, w1, b1, w2, b2, rating, sw = _problem(n, d, h)
    args = tuple(T(a, dev).requires_grad_(True) for a in (q, c, w1, b1, w2, b2))
    torch.library.opcheck(torch.ops.twotower.rating_head, args)
    pred = torch.ops.twotower.rating_head(*args)
    want_pred, hid = ops.rating_head(*(a.detach() for a in args))
    assert torch.equal(pred, want_pred)
    go = T(np.random.default_rng(5).uniform(-1, 1, n).astype(np.float32), dev)
    pred.backward(go)
    ref = rc.head_backward(q, c, hid.cpu().numpy(), go.cpu().numpy(), np.zeros(n), w1, w2, 1.0)      # g = the upstream gradient
    for a, k in zip(args, ("dq", "dc", "dw1", "db1", "dw2", "db2")):
        err = rel_err(a.grad.cpu().numpy().astype(np.float64), np.asarray(ref[k], dtype=np.float64).reshape(tuple(a.shape)))
        print(f"custom op: {k} {err:.2e}")
        assert err <= 1e-5, (k, err)
    torch.library.opcheck(torch.ops.twotower.rating_head_bwd, tuple(a.detach() for a in args) + (go,))
    # the TFRS-shaped task on the op's predictions: the contract's loss, gradients through the op
    for a in args:
        a.grad = None
    task = tasks.Ranking(loss=tasks.MeanSquaredError())
    loss = task(T(rating, dev), torch.ops.twotower.rating_head(*args), sample_weight=T(sw, dev))
    assert abs(loss.item() - rc.rating_loss(want_pred.cpu().numpy(), rating, sw)) <= 1e-5 * abs(loss.item())
    loss.backward()
    ref = rc.head_backward(q, c, hid.cpu().numpy(), want_pred.cpu().numpy(), rating, w1, w2, 2.0 / n, sw)
    assert rel_err(args[2].grad.cpu().numpy().astype(np.float64), ref["dw1"]) <= 1e-5
    with pytest.raises(NotImplementedError):
        tasks.Ranking(loss=object())


# ------------------------------------------------------------------------------------------ 10. CLIs
def test_train_cli_logs_a_validation_rmse_and_recommend_ranks_by_rating(dev, tmp_path):
    import json
    import pyarrow.parquet as pq
    from two_tower_amazon_recommender_amd import recommend, train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  ranking:\n    weight: 0.25\n    hidden_dim: 64\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck = tmp_path / "ck.pt"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):            # 1100 pairs, 40 % held out: 2 training steps, 1 validation batch
        assert train.main(["--config", str(cfgp), "--synthetic", "1100", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--val-fraction", "0.4", "--rating-weight", "0.5", "--rating-hidden", "32", "--save", str(ck)]) == 0
    rec = json.loads(out.getvalue().strip().splitlines()[-1])["history"][0]
    print(rec)
    assert np.isfinite(rec["val_rating_rmse"]) and 0 < rec["val_rating_rmse"] < 5 and np.isfinite(rec["val_loss_per_pair"])
    sd = torch.load(ck, weights_only=True)
    assert (sd["config"]["rating_weight"], sd["config"]["rating_hidden"], sd["step_index"]) == (0.5, 32, 2)   # the CLI's flags win
    b2 = sd["dense"][-1].item()
    assert 2.0 < b2 < 4.0                                                    # started from the mean training rating (stars 1..5)
    users = tmp_path / "users.npy"
    np.save(users, np.array([5, 0, 17, 5, 299], dtype=np.int64))             # unsorted, one user twice
    got = {}
    for how in ("score", "rating"):
        recs = tmp_path / f"{how}.parquet"
        extra = ["--predict-ratings"] if how == "score" else ["--rank-by", "rating"]
        assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs), *extra]) == 0
        got[how] = {k: np.asarray(v) for k, v in pq.read_table(recs).to_pydict().items()}
        assert set(got[how]) == {"user_idx", "rank", "item_idx", "score", "predicted_rating"} and len(got[how]["rank"]) == 25
    plain = tmp_path / "plain.parquet"
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(plain)]) == 0
    base = pq.read_table(plain).to_pydict()
    assert set(base) == {"user_idx", "rank", "item_idx", "score"}
    assert np.array_equal(np.asarray(base["item_idx"]), got["score"]["item_idx"])                     # the default output is today's
    cfg = TwoTowerConfig(**sd["config"])
    tr = TwoTowerTrainer(cfg, dev)
    tr.load_state_dict(sd)
    for how in ("score", "rating"):
        g = got[how]
        want = tr.predict_ratings(torch.from_numpy(g["user_idx"]).to(dev), torch.from_numpy(g["item_idx"]).to(dev)).cpu().numpy()
        assert np.array_equal(g["predicted_rating"].astype(np.float32), want)
    s, r = got["score"], got["rating"]
    assert np.array_equal(s["user_idx"], r["user_idx"]) and np.array_equal(r["rank"], np.tile(np.arange(5), 5))
    for k in range(5):                                                       # each request: sorted by the rating, the same item set
        rows = slice(5 * k, 5 * k + 5)
        assert (np.diff(r["predicted_rating"][rows]) <= 0).all()
        assert set(r["item_idx"][rows]) == set(s["item_idx"][rows])
    # a checkpoint without a head refuses both flags
    off = TwoTowerTrainer(_cfg("adagrad"), dev, seed=1)
    torch.save(off.state_dict(), tmp_path / "off.pt")
    for extra in (["--predict-ratings"], ["--rank-by", "rating"]):
        with pytest.raises(SystemExit, match="no rating head"):
            recommend.main(["--checkpoint", str(tmp_path / "off.pt"), "--users-file", str(users), "--out", str(plain), *extra])
    with pytest.raises(NotImplementedError, match="rating head"):
        train.main(["--config", str(cfgp), "--synthetic", "1100", "--distributed"])


# ------------------------------------------------------------------------------------------ 11. refusals
def test_trainer_refusals(dev):
    tr = _head_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="rating head"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="rating head"):
        ShardedTwoTowerTrainer(_cfg("sgd", rating_weight=W), dev, seed=1)
    with pytest.raises(NotImplementedError, match="dense segment"):           # 4-layer towers hold 16 segments already
        TwoTowerTrainer(_cfg("sgd", tower_dims=(64, 64, 64, 32), rating_weight=W), dev, seed=1)
    u, i = tr.synthetic_batch(1, 0, "Z")
    for call in (tr.step, tr.forward_backward, tr.evaluate):
        with pytest.raises(ValueError, match="ratings"):
            call(u, i)
    with pytest.raises(ValueError):
        tr.step(u, i, ratings=_ratings(dev, 1, 0)[:100].contiguous())
    with pytest.raises(ValueError, match="finite"):
        tr.init_rating_bias(float("nan"))

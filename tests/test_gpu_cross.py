"""The DCN-v2 cross layers on the GPU (tt_cross_fwd_f32 / tt_cross_bwd_f32, csrc/cross.hip): both launches against the f64
restatement of tests/cross_check.py, the slab contract, two problems per launch, then the trainer - parity with the f64 autograd
restatement for every optimizer, with every feature on and under mixed negative sampling, the identity at zero parameters, the
inference paths, checkpoints, refusals - the custom op and the CLIs."""
import contextlib
import io

import numpy as np
import pytest
import torch

import cross_check as cc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import Tower, TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

SHAPES = [(77, 32), (33, 64), (1000, 128), (256, 256),     # ragged tiles, one and several column blocks per wave, the largest LDS tile
          # widths that are no power of two: 256 / (D / 4) = 10, 6, 5, 4 rows of t per pass of the dW role (idle threads, a ragged
          # last pass) and 3, 5, 6, 7 column blocks over the four waves (D = 96: wave 3 owns none; D = 224: wave 3 owns one, the
          # others two).  tests/test_cross_cpu.py: the same math in f32 stays within the bars on these problems
          (77, 96), (130, 160), (45, 192), (65, 224)]
LR, LR_SGD = 0.001, 0.0001


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _problem(n, d, seed=0):
    """The distributions the issue's bar was worked out for: uniform(-1, 1) inputs, Glorot-uniform W, uniform(-0.2, 0.2) bias,
    standard-normal g."""
    rng = np.random.default_rng(1000 * d + n + seed)
    lim = np.sqrt(6.0 / (2 * d))
    f = lambda a: a.astype(np.float32)
    return dict(x0=f(rng.uniform(-1, 1, (n, d))), x=f(rng.uniform(-1, 1, (n, d))), w=f(rng.uniform(-lim, lim, (d, d))),
                b=f(rng.uniform(-0.2, 0.2, d)), g=f(rng.standard_normal((n, d))), prev=f(rng.standard_normal((n, d))))


def _guarded(a, dev):
    """[n + 1, D] device buffer, rows 0..n-1 = a, row n NaN; returns (whole, view of the first n rows)."""
    whole = torch.full((a.shape[0] + 1, a.shape[1]), float("nan"), device=dev)
    whole[:-1].copy_(T(a, dev))
    return whole, whole[:-1]


def _nan_rows(n, d, dev):
    whole = torch.full((n + 1, d), float("nan"), device=dev)
    return whole, whole[:-1]


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("n,d", SHAPES)
def test_forward_matches_f64(dev, n, d):
    p = _problem(n, d)
    w, b = T(p["w"], dev), T(p["b"], dev)
    for same in (False, True):
        x0w, x0 = _guarded(p["x0"], dev)
        xw, x = (x0w, x0) if same else _guarded(p["x"], dev)
        uw, u = _nan_rows(n, d, dev)
        yw, y = _nan_rows(n, d, dev)
        (got,) = ops.cross_layer((x0, x, w, b, y), u=(u,))
        assert got is y
        want_u, want_y = cc.layer_forward(p["x0"], p["x0"] if same else p["x"], p["w"], p["b"])
        eu, ey = rel_err(u.cpu().numpy(), want_u), rel_err(y.cpu().numpy(), want_y)
        print(f"n {n} D {d} x is x0 {same}: u {eu:.2e} y {ey:.2e}")
        assert eu <= 1e-5 and ey <= 1e-5
        assert torch.isnan(uw[n]).all().item() and torch.isnan(yw[n]).all().item()           # the row behind n stays NaN
        assert torch.isfinite(u).all().item() and torch.isfinite(y).all().item()
        (y2,) = ops.cross_layer((x0, x, w, b, None))                                          # u_out = NULL: the same y bits
        assert torch.equal(y2.view(torch.int32), y.view(torch.int32))
        # y = x0 * u + x in two rounded f32 operations
        assert torch.equal(y.view(torch.int32), (x0 * u + x).view(torch.int32))


# ------------------------------------------------------------------------------------------ 2. backward
def _run_bwd(dev, p, u, n_slabs, x_is_x0, dx0_in=None, accumulate=False, pad=0):
    n, d = p["x0"].shape
    stride = d * d + d + pad
    x0 = T(p["x0"], dev)
    x = x0 if x_is_x0 else T(p["x"], dev)
    dxw, dx = _nan_rows(n, d, dev)
    if dx0_in is not None:
        d0w, d0 = _guarded(dx0_in, dev)
    elif x_is_x0:
        d0w = d0 = None
    else:
        d0w, d0 = _nan_rows(n, d, dev)
    slabs = torch.full((n_slabs * stride,), float("nan"), device=dev)
    ((gdx, gdx0, dws, dbs),) = ops.cross_layer_bwd((x0, x, T(u, dev), T(p["w"], dev), T(p["g"], dev), dx, d0, slabs, slabs[d * d:]),
                                                  x_is_x0=x_is_x0, accumulate_dx0=accumulate, n_slabs=n_slabs, slab_stride=stride)
    assert gdx is dx and torch.isnan(dxw[n]).all().item() and (d0w is None or torch.isnan(d0w[n]).all().item())
    assert tuple(dws.shape) == (n_slabs, d, d) and tuple(dbs.shape) == (n_slabs, d)
    if pad:
        assert torch.isnan(slabs.view(n_slabs, stride)[:, d * d + d:]).all().item()           # nothing behind a slab is touched
    return dx, d0, dws, dbs


@pytest.mark.parametrize("n,d", SHAPES)
def test_backward_matches_f64(dev, n, d):
    p = _problem(n, d)
    u = cc.layer_forward(p["x0"], p["x"], p["w"], p["b"])[0].astype(np.float32)
    u0 = cc.layer_forward(p["x0"], p["x0"], p["w"], p["b"])[0].astype(np.float32)
    ns_q = ops.cross_num_slabs(n)
    assert ns_q == min(-(-n // 128), 64)
    for n_slabs in (1, ns_q, n // 32 + 5):
        cases = [("upper", False, None, False, u), ("upper+=", False, p["prev"], True, u), ("layer0", True, None, False, u0),
                 ("layer0+dx0", True, p["prev"], False, u0)]
        for name, is0, dx0_in, acc, uu in cases:
            want = cc.layer_backward(p["x0"], p["x0"] if is0 else p["x"], uu, p["w"], p["g"], x_is_x0=is0, dx0_in=dx0_in)
            dx, d0, dws, dbs = _run_bwd(dev, p, uu, n_slabs, is0, dx0_in, acc, pad=8 if n_slabs == 1 else 0)
            errs = dict(dx=rel_err(dx.cpu().numpy(), want["dx"]), dw=rel_err(dws.sum(0).cpu().numpy(), want["dw"]),
                        db=rel_err(dbs.sum(0).cpu().numpy(), want["db"]))
            if not is0:
                errs["dx0"] = rel_err(d0.cpu().numpy(), want["dx0"])
            print(f"n {n} D {d} slabs {n_slabs} {name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert max(errs.values()) <= 1e-5, (name, n_slabs, errs)
            assert torch.isfinite(dws).all().item() and torch.isfinite(dbs).all().item()      # every slab is written in full
            if is0 and dx0_in is not None:                                                    # the incoming dx0 is read only
                assert torch.equal(d0, T(dx0_in, dev))
            if acc:                                                                           # dx0 += g * u, bit for bit
                wantb = T(dx0_in, dev) + T(p["g"], dev) * T(uu, dev)
                assert torch.equal(d0.view(torch.int32), wantb.view(torch.int32))
            if name == "upper":                                                               # slab s holds ITS rows' sums
                for s, (lo, hi) in enumerate(cc.slab_rows(n, n_slabs)):
                    part = cc.layer_backward(p["x0"][lo:hi], p["x"][lo:hi], uu[lo:hi], p["w"], p["g"][lo:hi])
                    assert np.abs(dws[s].cpu().numpy() - part["dw"]).max() <= 1e-5 * max(np.abs(part["dw"]).max(), 1.0), (n_slabs, s)
                    assert np.abs(dbs[s].cpu().numpy() - part["db"]).max() <= 1e-5 * max(np.abs(part["db"]).max(), 1.0), (n_slabs, s)
    # empty slabs are exact zeros: 5 rows in 4 slabs of 2 rows
    p5 = {k: (v[:5] if k in ("x0", "x", "g", "prev") else v) for k, v in p.items()}
    _, _, dws, dbs = _run_bwd(dev, p5, u[:5], 4, False)
    assert not dws[3].any().item() and not dbs[3].any().item() and dws[2].any().item()
    want = cc.layer_backward(p5["x0"], p5["x"], u[:5], p5["w"], p5["g"])
    assert rel_err(dws.sum(0).cpu().numpy(), want["dw"]) <= 1e-5 and rel_err(dbs.sum(0).cpu().numpy(), want["db"]) <= 1e-5


# ------------------------------------------------------------------------------------------ 3. two problems per launch
@pytest.mark.parametrize("d", [32, 96, 128])
def test_two_problems_of_different_n_equal_two_launches_and_repeat(dev, d):
    pa, pb = _problem(256, d, 1), _problem(352, d, 2)
    da, db = ({k: T(v, dev) for k, v in p.items()} for p in (pa, pb))
    new = lambda p: torch.full_like(p["x"], float("nan"))
    ya, ua, yb, ub = new(da), new(da), new(db), new(db)
    ops.cross_layer((da["x0"], da["x"], da["w"], da["b"], ya), (db["x0"], db["x0"], db["w"], db["b"], yb), u=(ua, ub))
    for p, y, u, x in ((da, ya, ua, da["x"]), (db, yb, ub, db["x0"])):
        y1, u1 = new(p), new(p)
        ops.cross_layer((p["x0"], x, p["w"], p["b"], y1), u=(u1,))
        assert torch.equal(y1, y) and torch.equal(u1, u)
    ya2, yb2 = new(da), new(db)
    ops.cross_layer((da["x0"], da["x"], da["w"], da["b"], ya2), (db["x0"], db["x0"], db["w"], db["b"], yb2))
    assert torch.equal(ya2, ya) and torch.equal(yb2, yb)
    # backward: one shared slab array, the two problems' slabs side by side in it (the trainer's layout)
    ns, stride = 3, 2 * (d * d + d)

    def bwd(probs):
        slabs = torch.full((ns * stride,), float("nan"), device=dev)
        outs = []
        args = []
        for k, (p, u, x) in probs:
            dx, dx0 = new(p), new(p)
            args.append((p["x0"], x, u, p["w"], p["g"], dx, dx0, slabs[k * d * d:], slabs[2 * d * d + k * d:]))
            outs += [dx, dx0]
        res = ops.cross_layer_bwd(*args, n_slabs=ns, slab_stride=stride)
        return outs + [t for r in res for t in (r[2].clone(), r[3].clone())]
    both = bwd([(0, (da, ua, da["x"])), (1, (db, ub, db["x"]))])
    again = bwd([(0, (da, ua, da["x"])), (1, (db, ub, db["x"]))])
    one_a, one_b = bwd([(0, (da, ua, da["x"]))]), bwd([(1, (db, ub, db["x"]))])
    for got, want in zip(both, one_a[:2] + one_b[:2] + one_a[2:] + one_b[2:]):
        assert torch.equal(got, want) and torch.isfinite(got).all().item()
    for got, want in zip(both, again):
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------ 4. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=200, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR_SGD if opt == "sgd" else LR, optimizer=opt, batch_size=batch, **kw)


EXTRAS = dict(n_category_buckets=30, n_title_buckets=100, title_max_tokens=4, n_user_features=5, n_item_features=5, feature_clip=1.5,
              user_history_len=5, normalize_embeddings=True, rating_weight=0.5, rating_hidden=64)


def _trainer(dev, opt="adagrad", seed=1001, layers=1, **kw):
    tr = TwoTowerTrainer(_cfg(opt, cross_layers=layers, **kw), dev, seed=seed)
    if tr.user_features is not None:
        tr.set_user_features(tr.synthetic_user_features(seed))
    if tr.item_features is not None:
        tr.set_item_features(tr.synthetic_item_features(seed))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    if tr.user_history is not None:
        pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(2)]
        u, i = (torch.cat([p[k] for p in pairs]).cpu().numpy() for k in (0, 1))
        tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, tr.cfg.user_history_len), dev))
    return tr


def _ratings(dev, seed, step, batch=256):
    rng = np.random.default_rng(1000 * seed + step)
    r = rng.integers(1, 6, batch).astype(np.float32)
    r[rng.random(batch) < 0.1] = np.nan
    return T(r, dev)


def _cut64(tr, t):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    return flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))


def _towers64(tr):
    return tuple(([_cut64(tr, w) for w in tw.w], [_cut64(tr, b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def _cross64(tr):
    return tuple(([_cut64(tr, w) for w in tw.cross_w], [_cut64(tr, b) for b in tw.cross_b]) for tw in (tr.user_tower, tr.item_tower))


def _reference_step(tr, i, params, ratings=None, cand=None):
    """``cross_check.step_f64`` on the device's summed input rows x_0 and ReLU masks, the parameters as they were before the step."""
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    kw = {}
    if tr.rating_on:
        kw = dict(head=params["head"], ratings=ratings.cpu().numpy(), rating_weight=tr.cfg.rating_weight, head_mask=(tr._r_h > 0).cpu().numpy())
    return cc.step_f64(n64(tr.user_tower.acts[0]), n64(tr.item_tower.acts[0]), params["cross"], params["towers"], tr.cfg.temperature, masks,
                       normalize_eps=tr.cfg.normalize_eps if tr.cfg.normalize_embeddings else None,
                       item_ids=None if cand is None else i.cpu().numpy(), cand_ids=cand, **kw)


def _params64(tr):
    p = dict(towers=_towers64(tr), cross=_cross64(tr))
    if tr.rating_on:
        p["head"] = tuple(_cut64(tr, t) for t in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating))
    return p


def _cross_grads(tr):
    """The summed cross slabs as ([dW per layer] per tower, [db per layer] per tower)."""
    L, d = tr.cfg.cross_layers, tr.cfg.embedding_dim
    s = tr._c_slabs.view(tr._c_nslabs, -1).cpu().numpy().astype(np.float64).sum(0)
    nk = 2 * L * d * d
    dw = [[s[(t * L + l) * d * d:(t * L + l + 1) * d * d].reshape(d, d) for l in range(L)] for t in range(2)]
    db = [[s[nk + (t * L + l) * d:nk + (t * L + l + 1) * d] for l in range(L)] for t in range(2)]
    return dw, db


def _check_step(tr, r, loss, step, batch):
    """The bars of tests/test_gpu_features.py::_check_step - loss within 1e-4 relative and 1e-4 per pair, every gradient within
    1e-4 of its max |g| - with its treatment of the item tower's last bias, for the cross gradients too."""
    print(f"step {step}: loss {loss} (f64 {r['loss']})")
    assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    checks = [("due", n64(tr.user_tower.demb), r["dx0"][0]), ("die", n64(tr.item_tower.demb), r["dx0"][1])]
    cdw, cdb = _cross_grads(tr)
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(tw.n_layers):
            checks += [(f"dw[{t}][{l}]", n64(tw.dw_slabs[l]).sum(0), r["dw"][t][l]), (f"db[{t}][{l}]", n64(tw.db_slabs[l]).sum(0), r["db"][t][l])]
        for l in range(tw.n_cross):
            checks += [(f"dcw[{t}][{l}]", cdw[t][l], r["dcw"][t][l]), (f"dcb[{t}][{l}]", cdb[t][l], r["dcb"][t][l])]
    last = f"db[1][{tr.item_tower.n_layers - 1}]"
    for what, got, want in checks:
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        if what == last and not tr.cfg.normalize_embeddings:
            # the item tower's last bias shifts every logit of a row alike: the retrieval part of its gradient, the column sums
            # of dc, is ZERO (the f64 value is rounding noise, plus the head's small share where there is one); the bar is
            # taken from the scale of the rows the device sums
            if not tr.rating_on:
                assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
            scale = max(scale, np.abs(r["dc"]).max())
        print(f"step {step}: {what} error {err / scale:.2e} of max |g| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (step, what, err, scale)


@pytest.mark.parametrize("opt,layers,extras", [("sgd", 1, False), ("adagrad", 2, False), ("adam", 1, False), ("adam", 2, False),
                                                ("sgd", 2, False), ("adagrad", 1, False), ("adagrad", 2, True)])
def test_trainer_matches_the_f64_restatement_and_trains(dev, opt, layers, extras):
    seed, batch = 1001, 256
    tr = _trainer(dev, opt, seed, layers, **(EXTRAS if extras else {}))
    d = 32
    n_cross = 2 * layers * (d * d + d)
    assert not tr.fuse_lookup and len(tr._segs) == (12 if extras else 8) + 2 and (tr._adam_segs is None or len(tr._adam_segs) == len(tr._segs))
    # appended behind everything else: [user W_0.. | item W_0.. | user b_0.. | item b_0..], Glorot kernels, zero biases
    base = tr.dense_flat.data_ptr() + 4 * (tr.dense_flat.numel() - n_cross)
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(layers):
            assert tw.cross_w[l].data_ptr() == base + 4 * (t * layers + l) * d * d
            assert tw.cross_b[l].data_ptr() == base + 4 * (2 * layers * d * d + (t * layers + l) * d)
            lim = np.float32(np.sqrt(6.0 / (2 * d)))
            assert not tw.cross_b[l].any().item() and 0.9 * lim < tw.cross_w[l].abs().max().item() <= lim
    assert not torch.equal(tr.user_tower.cross_w[0], tr.item_tower.cross_w[0])
    plain = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    assert torch.equal(tr.dense_flat[:plain.dense_flat.numel()], plain.dense_flat) and torch.equal(tr.user_table, plain.user_table)
    cat_kw = lambda s: {"category_ids": tr.synthetic_categories(seed, s)} if extras else {}
    for step in range(3):
        u, i = tr.synthetic_batch(seed, step, "Z")
        kw = cat_kw(step)
        if extras:
            kw["ratings"] = _ratings(dev, seed, step)
        ids, rows, plans = [u, i], [300, 200], [tr.user_plan, tr.item_plan]
        if extras:
            ids.append(kw["category_ids"]); rows.append(30); plans.append(tr.cat_plan)
        ops.sparse_plan_batched(plans, ids, rows)
        params = _params64(tr)
        loss = tr.forward_backward(u, i, **kw).item()
        tr.check_ids()
        r = _reference_step(tr, i, params, ratings=kw.get("ratings"))
        _check_step(tr, r, loss, step, batch)
        tr.apply_gradients()
    p0 = tr.dense_flat[-n_cross:].clone()
    reg0 = tr.l2_penalty().item()
    losses = []
    u, i = tr.synthetic_batch(seed, 0, "Z")
    kw = cat_kw(0)
    if extras:
        kw["ratings"] = _ratings(dev, seed, 0)
    for step in range(6):
        loss = tr.step(u, i, **kw)
        losses.append(loss.item() + (tr.cfg.rating_weight * tr.rating_loss.item() if extras else 0.0))
    tr.check_ids()
    print(f"6 steps on one batch: {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    now = tr.dense_flat[-n_cross:]
    nk = 2 * layers * d * d
    for t in range(2 * layers):                                    # every cross kernel and every cross bias has moved
        assert not torch.equal(p0[t * d * d:(t + 1) * d * d], now[t * d * d:(t + 1) * d * d]), t
        assert not torch.equal(p0[nk + t * d:nk + (t + 1) * d], now[nk + t * d:nk + (t + 1) * d]), t
    assert torch.isfinite(tr.dense_flat).all() and torch.isfinite(tr.user_table).all() and torch.isfinite(tr.item_table).all()
    # the cross kernels are counted in the penalty
    want = sum((w.double() ** 2).sum().item() for tw in (tr.user_tower, tr.item_tower) for w in list(tw.w) + list(tw.cross_w))
    if extras:
        want += sum((w.double() ** 2).sum().item() for w in (tr.P_user, tr.P_item, tr.W1_rating, tr.w2_rating))
    assert tr.l2_penalty().item() == pytest.approx(1e-6 * want, rel=1e-9) and tr.l2_penalty().item() != reg0


@pytest.mark.parametrize("layers", [1, 2])
def test_mixed_sampling_step_matches_the_f64_restatement(dev, layers):
    """candidate_sampling='mixed', N = 64: the item tower's cross launches run over B + N rows, the user tower's over B."""
    seed, batch, n_neg = 77, 256, 64
    tr = _trainer(dev, "sgd", seed, layers, candidate_sampling="mixed", n_sampled_negatives=n_neg)
    assert tr.item_tower.xc[0].shape[0] == batch + n_neg and tr.user_tower.xc[0].shape[0] == batch
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        params = _params64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        cand = tr.cand_ids.cpu().numpy()
        assert np.array_equal(cand[:batch], i.cpu().numpy()) and len(cand) == batch + n_neg
        r = _reference_step(tr, i, params, cand=cand)
        _check_step(tr, r, loss, step, batch)
        tr.apply_gradients(step_ids=[u, i])
    w0 = tr.item_tower.cross_w[0].clone()
    tr.step(*tr.synthetic_batch(seed, 2, "Z"))
    # evaluate: the in-batch loss over the first B rows of the longer item tower (a partial-row pass)
    u, i = tr.synthetic_batch(seed, 3, "Z")
    loss = tr.evaluate(u, i).item()
    tr.check_ids()
    assert not torch.equal(w0, tr.item_tower.cross_w[0])
    want = _inference_loss(tr, u, i)
    print(f"mixed evaluate: {loss} (f64 {want})")
    assert abs(loss - want) <= 1e-4 * abs(want) and abs(loss - want) / batch <= 1e-4


# ------------------------------------------------------------------------------------------ 5. identity
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_zero_cross_parameters_are_the_trainer_without_the_layers_bit_for_bit(dev, opt):
    """W = 0, b = 0: x0 * 0 + x == x and dx == g exactly.  The cross parameters are put back to zero in front of every step
    (their gradient x_0^T (G * x_0) is not zero); both trainers run step() on materialised tower inputs."""
    seed = 31
    a = _trainer(dev, opt, seed, 2)
    b = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    b.fuse_lookup = False
    n_cross = 2 * 2 * (32 * 32 + 32)
    for s in range(3):
        a.dense_flat[-n_cross:].zero_()
        u, i = a.synthetic_batch(seed, s, "Z")
        la, lb = a.step(u, i), b.step(u, i)
        assert torch.equal(la, lb), s
        assert torch.equal(a.user_tower.demb, b.user_tower.demb) and torch.equal(a.item_tower.demb, b.item_tower.demb), s
        assert torch.equal(a.user_tower.xc[-1], b.user_tower.acts[0]) and torch.equal(a.item_tower.cg[0], a.item_tower.demb), s
    a.check_ids()
    nb = b.dense_flat.numel()
    assert torch.equal(a.user_table, b.user_table) and torch.equal(a.item_table, b.item_table)
    assert torch.equal(a.dense_flat[:nb], b.dense_flat) and a.dense_flat.numel() == nb + n_cross
    if opt == "adagrad":
        assert torch.equal(a.dense_accum[:nb], b.dense_accum) and torch.equal(a.user_accum, b.user_accum)


# ------------------------------------------------------------------------------------------ 6. inference
def _tower64(tr, tw, x0):
    xs, _ = cc.stack_forward(x0, *[[t.cpu().numpy() for t in ts] for ts in (tw.cross_w, tw.cross_b)])
    x = xs[-1] if xs else np.asarray(x0, dtype=np.float64)
    for l in range(tw.n_layers):
        x = x @ tw.w[l].cpu().numpy().astype(np.float64) + tw.b[l].cpu().numpy().astype(np.float64)
        if l < tw.n_layers - 1:
            x = np.maximum(x, 0.0)
    if tr.cfg.normalize_embeddings:
        x = x / np.sqrt(np.maximum((x * x).sum(1, keepdims=True), tr.cfg.normalize_eps))
    return x


def _inference_loss(tr, u, i):
    q = _tower64(tr, tr.user_tower, tr.user_table[u].cpu().numpy())
    c = _tower64(tr, tr.item_tower, tr.item_table[i].cpu().numpy())
    s = torch.from_numpy(q @ c.T / tr.cfg.temperature)
    return float((torch.logsumexp(s, dim=1) - s.diagonal()).sum())


@pytest.mark.parametrize("layers,normalize", [(1, False), (3, True)])
def test_inference_paths_match_the_f64_restatement(dev, layers, normalize):
    seed, batch = 23, 256
    tr = _trainer(dev, "adagrad", seed, layers, normalize_embeddings=normalize)
    for s in range(2):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 300, 300)).to(dev)        # 256 + a partial chunk of 44
    got = tr.user_embeddings(ids).cpu().numpy()
    eu = rel_err(got, _tower64(tr, tr.user_tower, tr.user_table[ids].cpu().numpy()))
    corpus = tr.item_corpus_embeddings().cpu().numpy()                                        # 200 items: one partial chunk
    ei = rel_err(corpus, _tower64(tr, tr.item_tower, tr.item_table.cpu().numpy()))
    u, i = tr.synthetic_batch(seed, 5, "Z")
    loss, want = tr.evaluate(u, i).item(), _inference_loss(tr, u, i)
    tr.check_ids()
    print(f"L {layers}: user_embeddings {eu:.2e} item_corpus_embeddings {ei:.2e} evaluate {loss} (f64 {want})")
    assert eu <= 1e-5 and ei <= 1e-5 and got.shape == (300, 32) and corpus.shape == (200, 32)
    assert abs(loss - want) <= 1e-4 * abs(want) and abs(loss - want) / batch <= 1e-4
    # evaluate_topk takes the materialised path: the ranks are those of the embeddings above
    from two_tower_amazon_recommender_amd import metrics
    m = metrics.FactorizedTopK(ks=(10,))
    tr.evaluate_topk(u, i, m, corpus=torch.from_numpy(corpus).to(dev))
    tr.check_ids()
    # a partial-row pass of a tower equals the full pass on those rows
    full = tr.user_tower.forward().clone()
    part = tr.user_tower.forward(rows=100).clone()
    assert torch.equal(part, full[:100])


# ------------------------------------------------------------------------------------------ 7. checkpoints and refusals
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _trainer(dev, opt, seed, 2)
    run(a, range(4))
    b = _trainer(dev, opt, seed, 2)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["cross_layers"] == 2
    assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + 4 * (32 * 32 + 32)
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values
    c.load_state_dict(sd)
    assert torch.equal(c.dense_flat, sd["dense"]) and torch.equal(c.user_tower.cross_w[1], b.user_tower.cross_w[1])
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "loss"]
    names += ["user_accum", "item_accum", "dense_accum"] if opt == "adagrad" else ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.user_tower.cross_w[0], b.user_tower.cross_w[0])
    # a checkpoint without the layers - one from before the field existed too - loads into a trainer without them; a mismatch is refused
    off = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    old = dict(off.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if k != "cross_layers"}
    off.load_state_dict(old)
    with pytest.raises(ValueError, match="cross_layers"):
        off.load_state_dict(sd)
    with pytest.raises(ValueError, match="cross_layers"):
        c.load_state_dict(old)
    with pytest.raises(ValueError, match="cross_layers"):
        _trainer(dev, opt, seed, 1).load_state_dict(sd)


def test_trainer_refusals(dev):
    tr = _trainer(dev, "sgd", 1, 1)
    with pytest.raises(NotImplementedError, match="cross layers"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="cross layers"):
        ShardedTwoTowerTrainer(_cfg("sgd", cross_layers=1), dev, seed=1)
    with pytest.raises(ValueError, match="multiple of 32"):
        TwoTowerTrainer(_cfg("sgd", dim=36, cross_layers=1), dev, seed=1)
    TwoTowerTrainer(_cfg("sgd", dim=36), dev, seed=1)                           # without the layers 36 is as fine as before
    with pytest.raises(NotImplementedError, match="dense segment"):            # 4-layer towers hold 16 segments already
        TwoTowerTrainer(_cfg("sgd", tower_dims=(64, 64, 64, 32), cross_layers=1), dev, seed=1)
    u, i = tr.synthetic_batch(1, 0, "Z")
    with pytest.raises(ValueError, match="materialised"):
        tr.user_tower.forward(lookup=ops.make_lookup(tr.user_table, u, oob_flag=tr.oob))
    x = torch.zeros(64, 32, device=dev)
    w, b = torch.zeros(32, 32, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(ValueError, match="alias"):
        ops.cross_layer((x, x, w, b, x))
    with pytest.raises(ValueError, match="alias"):
        g = torch.zeros(64, 32, device=dev)
        ops.cross_layer_bwd((x, x.clone(), x.clone(), w, g, g, None, None, None))
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.cross_layer((x[:, :16].contiguous(),) * 2 + (w[:16, :16].contiguous(), b[:16].contiguous(), None))
    assert ops.cross_layer((x[:0], x[:0], w, b, None))[0].shape == (0, 32)     # no rows: no launch


# ------------------------------------------------------------------------------------------ 8. custom op
def test_custom_op_passes_opcheck_and_differentiates_every_input(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    n, d = 77, 64
    p = _problem(n, d)
    args = tuple(T(p[k], dev).requires_grad_(True) for k in ("x0", "x", "w", "b"))
    torch.library.opcheck(torch.ops.twotower.cross_layer, args)
    y = torch.ops.twotower.cross_layer(*args)
    (want,) = ops.cross_layer(tuple(a.detach() for a in args) + (None,))
    assert torch.equal(y, want)
    want_u, want_y = cc.layer_forward(p["x0"], p["x"], p["w"], p["b"])
    assert rel_err(y.detach().cpu().numpy(), want_y) <= 1e-5
    y.backward(T(p["g"], dev))
    ref = cc.layer_backward(p["x0"], p["x"], want_u, p["w"], p["g"])
    for a, k in zip(args, ("dx0", "dx", "dw", "db")):
        err = rel_err(a.grad.cpu().numpy(), ref[k])
        print(f"custom op: {k} {err:.2e}")
        assert err <= 1e-5, (k, err)
    torch.library.opcheck(torch.ops.twotower.cross_layer_bwd, tuple(a.detach() for a in args) + (T(p["g"], dev),))
    # a two-layer stack through autograd, x0 feeding every layer: the gradient of x0 is the stack's
    x0 = T(p["x0"], dev).requires_grad_(True)
    w2 = T(_problem(n, d, 9)["w"], dev)
    out = torch.ops.twotower.cross_layer(x0, torch.ops.twotower.cross_layer(x0, x0, args[2].detach(), args[3].detach()), w2, args[3].detach())
    out.backward(T(p["g"], dev))
    t0 = torch.tensor(p["x0"].astype(np.float64), requires_grad=True)
    c64 = lambda t: t.detach().cpu().double()
    x1 = t0 * (t0 @ c64(args[2]) + c64(args[3])) + t0
    (t0 * (x1 @ c64(w2) + c64(args[3])) + x1).backward(torch.tensor(p["g"].astype(np.float64)))
    assert rel_err(x0.grad.cpu().numpy(), t0.grad.numpy()) <= 1e-5


# ------------------------------------------------------------------------------------------ 9. CLIs
def test_train_cli_trains_and_saves_and_recommend_needs_only_the_checkpoint(dev, tmp_path):
    import json
    import pyarrow.parquet as pq
    from two_tower_amazon_recommender_amd import recommend, train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  cross:\n    layers: 2\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck = tmp_path / "ck.pt"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):            # 1100 pairs, 40 % held out: 2 training steps, 1 validation batch
        assert train.main(["--config", str(cfgp), "--synthetic", "1100", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--val-fraction", "0.4", "--cross-layers", "1", "--save", str(ck)]) == 0
    rec = json.loads(out.getvalue().strip().splitlines()[-1])["history"][0]
    print(rec)
    assert np.isfinite(rec["val_loss_per_pair"])
    sd = torch.load(ck, weights_only=True)
    assert (sd["config"]["cross_layers"], sd["step_index"]) == (1, 2)                         # the CLI's flag wins over the block
    assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + 2 * (32 * 32 + 32)
    assert sd["dense"][-64:].any().item()                                                     # the cross biases were trained
    users = tmp_path / "users.npy"
    np.save(users, np.array([5, 0, 17, 5, 299], dtype=np.int64))
    recs = tmp_path / "recs.parquet"
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
    got = {k: np.asarray(v) for k, v in pq.read_table(recs).to_pydict().items()}
    assert len(got["item_idx"]) == 25 and np.array_equal(got["rank"], np.tile(np.arange(5), 5))
    # the recommendations are those of the checkpoint's own embeddings
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev)
    tr.load_state_dict(sd)
    q = tr.user_embeddings(torch.tensor([5, 0, 17, 5, 299], device=dev))
    top = (q @ tr.item_corpus_embeddings().t()).topk(5, dim=1).indices.cpu().numpy().reshape(-1)
    assert np.array_equal(got["item_idx"], top)
    with pytest.raises(NotImplementedError, match="cross layers"):
        train.main(["--config", str(cfgp), "--synthetic", "1100", "--distributed"])

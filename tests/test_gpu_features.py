"""The dense numeric side features on the GPU (tt_dense_features_fwd_f32 / tt_dense_features_bwd_f32, csrc/features.hip): the
forward launch against the restatement of tests/features_check.py BIT FOR BIT, the slab reduction against f64, the equivalence with
gather + torch f32 arithmetic, then the trainer - parity with the f64 autograd restatement for every optimizer and under mixed
negative sampling, the feature-off path, checkpoints, the inference paths - the custom op, the CLIs and the refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import features_check as fc
from two_tower_amazon_recommender_amd import ops
from two_tower_amazon_recommender_amd.trainer import Tower, TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001
# plain SGD on the SUM loss: the projected features (|z| up to the clip times a Glorot kernel) are ~20 times the embedding rows'
# U(-0.05, 0.05), and at 0.001 the trajectory diverges within three steps (loss 2.3e3 -> 8.0e3 -> 3.0e5, in f64 alike)
LR_SGD = 0.0001


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bad(got, want):
    b = fc.bits(got) != fc.bits(want)
    return int(b.sum()), np.argwhere(b)[:4].tolist()


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def _problem(rng, n, F, dim, rows=50):
    """A 50-row matrix (ids repeat) with one outlier row, ids with two -1 and ONE out-of-range id, statistics, kernel, rows to accumulate into."""
    feat = (rng.standard_normal((rows, F)) * 3 + 1).astype(np.float32)
    feat[0] += 40.0                                # an outlier row (id 0, always looked up): a clip of 2.5 clamps it, normalised or not
    ids = rng.integers(0, rows, n).astype(np.int64)
    ids[[3, n - 1]] = -1
    ids[5] = 0
    ids[11] = rows
    mean, inv_std = ops.adapt_normalization(feat)
    proj = rng.uniform(-0.2, 0.2, (F, dim)).astype(np.float32)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    return feat, ids, mean, inv_std, proj, base


# ------------------------------------------------------------------------------------------ 1. forward, bit for bit
@pytest.mark.parametrize("dim", [32, 128])
@pytest.mark.parametrize("F", [1, 3, 5, 32])
def test_forward_matches_the_restatement_bit_for_bit(dev, dim, F):
    for n in (77, 256):
        rng = np.random.default_rng(1000 * F + dim + n)
        feat, ids, mean, inv_std, proj, base = _problem(rng, n, F, dim)
        d = [T(a, dev) for a in (feat, ids, mean, inv_std, proj)]
        for accumulate in (False, True):
            for norm in (True, False):
                for clip in (0.0, 2.5):
                    want, want_z, want_flag = fc.features_forward(feat, ids, mean if norm else None, inv_std if norm else None, proj,
                                                                  clip, accumulate, base)
                    out = T(base, dev).clone() if accumulate else torch.full((n, dim), float("nan"), device=dev)
                    z = torch.full((n, F), float("nan"), device=dev)
                    flag = torch.zeros(1, dtype=torch.int32, device=dev)
                    (got,) = ops.dense_features((d[0], d[1], d[2] if norm else None, d[3] if norm else None, d[4], out, accumulate, z),
                                                clip=clip, oob_flag=flag)
                    assert got is out
                    what = (n, accumulate, norm, clip)
                    assert not _bad(out.cpu().numpy(), want)[0], (what, _bad(out.cpu().numpy(), want))
                    assert not _bad(z.cpu().numpy(), want_z)[0], (what, _bad(z.cpu().numpy(), want_z))
                    assert flag.item() == want_flag == 1, what
                    if clip:
                        assert np.abs(want_z).max() == np.float32(clip)                 # the clamp did something
        # without the out-of-range id the flag stays clear; -1 alone never sets it; no z_out, no flag pointer
        ids2 = np.where(ids == 50, -1, ids)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        (got,) = ops.dense_features((d[0], T(ids2, dev), d[2], d[3], d[4], None, False, None), oob_flag=flag)
        assert flag.item() == 0 and not _bad(got.cpu().numpy(), fc.features_forward(feat, ids2, mean, inv_std, proj)[0])[0]
        (got,) = ops.dense_features((d[0], d[1], d[2], d[3], d[4], None, False, None))
        assert not _bad(got.cpu().numpy(), fc.features_forward(feat, ids, mean, inv_std, proj)[0])[0]
        assert not got[[3, 11, n - 1]].any().item()


def test_two_problem_launch_with_different_rows_equals_two_launches(dev):
    """Both towers in ONE launch: different n (mixed sampling's item side is longer), different F, one accumulating."""
    rng = np.random.default_rng(7)
    dim = 32
    pa, pb = _problem(rng, 77, 5, dim), _problem(rng, 256 + 64, 3, dim, rows=200)
    outs, zs, flag = [], [], torch.zeros(1, dtype=torch.int32, device=dev)
    probs = []
    for (feat, ids, mean, inv_std, proj, base), acc in ((pa, True), (pb, False)):
        out = T(base, dev).clone() if acc else torch.full(base.shape, float("nan"), device=dev)
        z = torch.full((len(ids), feat.shape[1]), float("nan"), device=dev)
        probs.append((T(feat, dev), T(ids, dev), T(mean, dev), T(inv_std, dev), T(proj, dev), out, acc, z))
        outs.append(out); zs.append(z)
    ops.dense_features(*probs, clip=2.5, oob_flag=flag)
    for (feat, ids, mean, inv_std, proj, base), acc, out, z in zip((pa, pb), (True, False), outs, zs):
        want, want_z, _ = fc.features_forward(feat, ids, mean, inv_std, proj, 2.5, acc, base)
        assert not _bad(out.cpu().numpy(), want)[0] and not _bad(z.cpu().numpy(), want_z)[0]
    assert flag.item() == 1
    # the other order (the longer problem first) gives the same bits
    probs2 = [tuple(t.clone() if torch.is_tensor(t) and i in (5, 7) else t for i, t in enumerate(p)) for p in probs[::-1]]
    probs2[1][5].copy_(T(pa[5], dev))
    ops.dense_features(*probs2, clip=2.5)
    assert torch.equal(probs2[0][5], outs[1]) and torch.equal(probs2[1][5], outs[0])


# ------------------------------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("dim", [32, 128])
@pytest.mark.parametrize("F", [1, 5, 32])
@pytest.mark.parametrize("n", [77, 1000])
def test_backward_slab_sum_against_f64(dev, n, F, dim):
    rng = np.random.default_rng(n + 10 * F + dim)
    z = rng.standard_normal((n, F)).astype(np.float32)
    dy = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    ns = ops.dense_features_num_slabs(n)
    assert ns == (1 if n == 77 else 8)
    want = fc.features_dp(z, dy)
    for n_slabs in (ns, 3, 11):                   # the query's count; ragged last slab (1000 = 334 + 334 + 332); 11 slabs of 7 rows at n = 77
        slabs = torch.full((n_slabs, F, dim), float("nan"), device=dev)
        (got,) = ops.dense_features_bwd((T(z, dev), T(dy, dev), slabs))
        assert got is slabs and torch.isfinite(slabs).all().item(), n_slabs                  # every slab is written in full
        err = rel_err(slabs.sum(0).cpu().numpy(), want)
        print(f"n {n} F {F} dim {dim} slabs {n_slabs}: rel_err {err:.2e}")
        assert err <= 1e-5
        for s, (lo, hi) in enumerate(fc.slab_rows(n, n_slabs)):                              # slab s holds ITS rows' sum
            part = fc.features_dp(z[lo:hi], dy[lo:hi])
            assert np.abs(slabs[s].cpu().numpy() - part).max() <= 1e-5 * max(np.abs(part).max(), 1.0), (n_slabs, s)
    # empty slabs are written as zeros: 5 rows in 4 slabs of 2 rows
    slabs = torch.full((4, F, dim), float("nan"), device=dev)
    ops.dense_features_bwd((T(z[:5], dev), T(dy[:5], dev), slabs))
    assert not slabs[3].any().item() and torch.isfinite(slabs).all().item()
    assert rel_err(slabs.sum(0).cpu().numpy(), fc.features_dp(z[:5], dy[:5])) <= 1e-5


def test_backward_two_problems_in_one_launch(dev):
    rng = np.random.default_rng(12)
    dim = 32
    za, zb = rng.standard_normal((256, 5)).astype(np.float32), rng.standard_normal((320, 32)).astype(np.float32)
    dya, dyb = rng.uniform(-1, 1, (256, dim)).astype(np.float32), rng.uniform(-1, 1, (320, dim)).astype(np.float32)
    sa, sb = torch.full((2, 5, dim), float("nan"), device=dev), torch.full((3, 32, dim), float("nan"), device=dev)
    ops.dense_features_bwd((T(za, dev), T(dya, dev), sa), (T(zb, dev), T(dyb, dev), sb))
    one_a = ops.dense_features_bwd((T(za, dev), T(dya, dev), torch.empty_like(sa)))[0]
    one_b = ops.dense_features_bwd((T(zb, dev), T(dyb, dev), torch.empty_like(sb)))[0]
    assert torch.equal(sa, one_a) and torch.equal(sb, one_b)
    assert rel_err(sa.sum(0).cpu().numpy(), fc.features_dp(za, dya)) <= 1e-5
    assert rel_err(sb.sum(0).cpu().numpy(), fc.features_dp(zb, dyb)) <= 1e-5


# ------------------------------------------------------------------------------------------ 3. equivalence
def test_equals_gather_then_torch_f32_arithmetic_then_the_add(dev):
    rng = np.random.default_rng(21)
    n, F, dim = 256, 5, 128
    feat, ids, mean, inv_std, proj, _ = _problem(rng, n, F, dim)
    ids = np.where(ids == 50, 7, ids)
    table = T(rng.standard_normal((50, dim)).astype(np.float32), dev)
    d = [T(a, dev) for a in (feat, ids, mean, inv_std, proj)]
    out = ops.embedding_gather(table, d[1])
    ops.dense_features((d[0], d[1], d[2], d[3], d[4], out, True, None), clip=2.5)
    valid = (d[1] >= 0)[:, None]
    z = torch.where(valid, ((d[0][d[1].clamp(min=0)] - d[2]) * d[3]).clamp(-2.5, 2.5), torch.zeros((), device=dev))
    acc = torch.zeros(n, dim, device=dev)
    for f in range(F):                             # one rounded product and one rounded add per f, as the kernel does
        acc = acc + z[:, f:f + 1] * d[4][f][None, :]
    want = ops.embedding_gather(table, d[1]) + acc
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------ 4. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=200, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR_SGD if opt == "sgd" else LR, optimizer=opt, batch_size=batch, **kw)


def _feature_trainer(dev, opt="adagrad", seed=1001, fu=5, fi=5, clip=1.5, **kw):
    tr = TwoTowerTrainer(_cfg(opt, n_user_features=fu, n_item_features=fi, feature_clip=clip, **kw), dev, seed=seed)
    if fu:
        tr.set_user_features(tr.synthetic_user_features(seed))
    if fi:
        tr.set_item_features(tr.synthetic_item_features(seed))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def _features64(tr):
    n = lambda t: t.cpu().numpy().astype(np.float64)
    return {side: (n(getattr(tr, f"{side}_features")), n(getattr(tr, f"{side}_feature_mean")), n(getattr(tr, f"{side}_feature_inv_std")),
                   n(getattr(tr, f"P_{side}")), tr.cfg.feature_clip) for side, _, _, _ in tr._feature_sides}


def _check_step(tr, r, loss, step, batch):
    print(f"step {step}: loss {loss} (f64 {r['loss']})")
    assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    checks = [("due", n64(tr.user_tower.demb), r["due"]), ("die", n64(tr.item_tower.demb), r["die"]),
              ("dP_user", n64(tr._fslabs_user).sum(0), r["dp"]["user"]), ("dP_item", n64(tr._fslabs_item).sum(0), r["dp"]["item"])]
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(tw.n_layers):
            checks += [(f"dw[{t}][{l}]", n64(tw.dw_slabs[l]).sum(0), r["dw"][t][l]), (f"db[{t}][{l}]", n64(tw.db_slabs[l]).sum(0), r["db"][t][l])]
    last = f"db[1][{tr.item_tower.n_layers - 1}]"
    for what, got, want in checks:
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        if what == last:
            # the item tower's last bias shifts every logit of a row alike: its gradient, the column sums of dc, is ZERO (the f64
            # value is rounding noise); the bar is taken from the scale of the rows the device sums (test_gpu_history.py)
            assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
            scale = np.abs(r["dc"]).max()
        print(f"step {step}: {what} error {err / scale:.2e} of max |g|")
        assert scale > 0 and err <= 1e-4 * scale, (step, what, err)


@pytest.mark.parametrize("opt,extras", [("sgd", False), ("adagrad", True), ("adam", False)])
def test_trainer_matches_the_f64_restatement_and_trains(dev, opt, extras):
    """Both sides F = 5 (clip 1.5, so some values are clamped); ``extras``: the category and the title feature on as well.  Three
    steps: loss and every gradient - both projection kernels' included - within the project's bars (relative <= 1e-4 of max |g|)
    of the f64 autograd restatement given the device's ReLU masks.  Then steps through ``step()``: the projection kernels move,
    the feature matrices do not."""
    seed, batch = 1001, 256
    kw = dict(n_category_buckets=30, n_title_buckets=100, title_max_tokens=4) if extras else {}
    tr = _feature_trainer(dev, opt, seed, **kw)
    assert not tr.fuse_lookup and len(tr._segs) == 10
    assert tr.P_user.data_ptr() == tr.dense_flat.data_ptr() + 4 * (tr.user_tower.end_offset + Tower.param_count(tr.cfg, tr.cfg.item_dims))
    feats0 = (tr.user_features.clone(), tr.item_features.clone())
    zu = fc.normalise(tr.user_features.cpu().numpy(), np.arange(300), tr.user_feature_mean.cpu().numpy(), tr.user_feature_inv_std.cpu().numpy(), 1.5)[0]
    assert (np.abs(zu) == 1.5).any() and (np.abs(zu) < 1.5).any()
    for step in range(3):
        u, i = tr.synthetic_batch(seed, step, "Z")
        cat = tr.synthetic_categories(seed, step) if extras else None
        ids, rows, plans = [u, i], [300, 200], [tr.user_plan, tr.item_plan]
        if extras:
            ids.append(cat); rows.append(30); plans.append(tr.cat_plan)
        ops.sparse_plan_batched(plans, ids, rows)
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
        towers, feats = _towers64(tr), _features64(tr)
        category = (tr.cat_table.cpu().numpy(), cat.cpu().numpy()) if extras else None
        title = (tr.title_table.cpu().numpy(), tr.item_titles.cpu().numpy(), "mean") if extras else None
        loss = tr.forward_backward(u, i, category_ids=cat).item()
        tr.check_ids()
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
        r = fc.step_f64(before["user_table"], before["item_table"], towers, u.cpu().numpy(), i.cpu().numpy(), feats, 0.1, masks,
                        category=category, title=title)
        _check_step(tr, r, loss, step, batch)
        # the kept normalised rows are the restatement's, bit for bit
        want_z = fc.normalise(tr.item_features.cpu().numpy(), i.cpu().numpy(), tr.item_feature_mean.cpu().numpy(),
                              tr.item_feature_inv_std.cpu().numpy(), 1.5)[0]
        assert not _bad(tr._fz_item.cpu().numpy(), want_z)[0]
        tr.apply_gradients()
    p0 = (tr.P_user.clone(), tr.P_item.clone())
    losses = []
    for step in range(3, 9):
        u, i = tr.synthetic_batch(seed, 0, "Z")
        losses.append(tr.step(u, i, **({"category_ids": tr.synthetic_categories(seed, 0)} if extras else {})).item())
    tr.check_ids()
    print(f"6 steps on one batch: {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(p0[0], tr.P_user) and not torch.equal(p0[1], tr.P_item)
    assert torch.equal(feats0[0], tr.user_features) and torch.equal(feats0[1], tr.item_features)


def test_mixed_sampling_step_matches_the_f64_restatement(dev):
    """candidate_sampling='mixed', N = 64: the item side looks its features up by ``cand_ids`` - the sampled rows too - and the
    backward launch reduces B rows on the user side and B + N on the item side."""
    seed, batch, n_neg = 77, 256, 64
    tr = _feature_trainer(dev, "sgd", seed, candidate_sampling="mixed", n_sampled_negatives=n_neg)
    assert tuple(tr._fz_item.shape) == (batch + n_neg, 5) and tuple(tr._fz_user.shape) == (batch, 5)
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
        towers, feats = _towers64(tr), _features64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        cand = tr.cand_ids.cpu().numpy()
        assert np.array_equal(cand[:batch], i.cpu().numpy()) and len(cand) == batch + n_neg
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
        r = fc.step_f64(before["user_table"], before["item_table"], towers, u.cpu().numpy(), i.cpu().numpy(), feats, 0.1, masks,
                        cand_ids=cand)
        _check_step(tr, r, loss, step, batch)
        want_z = fc.normalise(tr.item_features.cpu().numpy(), cand, tr.item_feature_mean.cpu().numpy(),
                              tr.item_feature_inv_std.cpu().numpy(), 1.5)[0]
        assert not _bad(tr._fz_item.cpu().numpy(), want_z)[0]
        tr.apply_gradients(step_ids=[u, i])
    p0 = tr.P_item.clone()
    tr.step(*tr.synthetic_batch(seed, 2, "Z"))
    tr.evaluate(*tr.synthetic_batch(seed, 3, "Z"))
    tr.check_ids()
    assert not torch.equal(p0, tr.P_item)


def test_one_sided_features_and_the_setters_refusals(dev):
    seed = 5
    tr = _feature_trainer(dev, "adagrad", seed, fu=0, fi=3, clip=0.0)
    assert tr.user_features is None and tr.P_user is None and len(tr._segs) == 9
    assert tr.dense_flat.numel() == 2 * Tower.param_count(tr.cfg, [64, 32]) + 3 * 32
    # until the setter runs the matrix is zeros (mean 0, inv_std 1): the feature adds nothing
    fresh = TwoTowerTrainer(_cfg("adagrad", n_item_features=3), dev, seed=seed)
    plain = TwoTowerTrainer(_cfg("adagrad"), dev, seed=seed)
    u, i = fresh.synthetic_batch(seed, 0, "Z")
    assert fresh.evaluate(u, i).item() == pytest.approx(plain.evaluate(u, i).item(), rel=1e-6)
    assert torch.equal(fresh.item_tower.acts[0], ops.embedding_gather(plain.item_table, i) + 0.0)
    l0 = tr.step(u, i).item()
    assert np.isfinite(l0)
    with pytest.raises(ValueError, match="n_user_features == 0"):
        tr.set_user_features(torch.zeros(300, 5))
    with pytest.raises(ValueError, match=r"\[200, 3\]"):
        tr.set_item_features(torch.zeros(200, 4))
    bad = np.zeros((200, 3), dtype=np.float32)
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        tr.set_item_features(bad)
    with pytest.raises(ValueError, match="both or neither"):
        tr.set_item_features(np.zeros((200, 3), dtype=np.float32), mean=np.zeros(3))
    with pytest.raises(ValueError, match="finite entries"):
        tr.set_item_features(np.zeros((200, 3), dtype=np.float32), mean=np.zeros(3), inv_std=np.array([1.0, np.inf, 1.0]))
    x = np.random.default_rng(1).standard_normal((200, 3)).astype(np.float32)
    tr.set_item_features(x, mean=np.array([1.0, 2.0, 3.0]), inv_std=np.array([0.5, 0.25, 2.0]))      # given statistics are taken as they are
    assert tr.item_feature_mean.tolist() == [1.0, 2.0, 3.0] and tr.item_feature_inv_std.tolist() == [0.5, 0.25, 2.0]
    tr.set_item_features(torch.from_numpy(x).to(dev))                                                 # adapted; a device tensor is fine
    m, s = ops.adapt_normalization(x)
    assert np.array_equal(tr.item_feature_mean.cpu().numpy(), m) and np.array_equal(tr.item_feature_inv_std.cpu().numpy(), s)


# ------------------------------------------------------------------------------------------ 5. feature off
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_feature_off_is_the_trainer_as_it_was(dev, opt):
    seed = 31
    a, b = TwoTowerTrainer(_cfg(opt), dev, seed=seed), TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    assert a.fuse_lookup and a._feature_sides == [] and a.P_user is None and a.user_features is None and a._fz_item is None
    assert a.dense_flat.numel() == Tower.param_count(a.cfg, a.cfg.user_dims) + Tower.param_count(a.cfg, a.cfg.item_dims)
    assert len(a._segs) == 8 and (a._adam_segs is None or len(a._adam_segs) == 8)
    for s in range(3):
        a.step(*a.synthetic_batch(seed, s, "Z")); b.step(*b.synthetic_batch(seed, s, "Z"))
    a.check_ids()
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) and not [k for k in sa if "feature" in k]
    for k, v in sa.items():
        if torch.is_tensor(v):
            assert torch.equal(v, sb[k]), k
    assert (sa["config"]["n_user_features"], sa["config"]["n_item_features"], sa["config"]["feature_clip"]) == (0, 0, 0.0)


# ------------------------------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17
    kw = dict(dropout_rate=0.1)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _feature_trainer(dev, opt, seed, **kw)
    run(a, range(4))
    b = _feature_trainer(dev, opt, seed, **kw)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert (sd["config"]["n_user_features"], sd["config"]["n_item_features"], sd["config"]["feature_clip"]) == (5, 5, 1.5)
    assert tuple(sd["user_features"].shape) == (300, 5) and tuple(sd["item_feature_inv_std"].shape) == (5,)
    assert sd["dense"].numel() == 2 * Tower.param_count(b.cfg, [64, 32]) + 2 * 5 * 32
    cfg_c = TwoTowerConfig(**{**sd["config"], "feature_clip": 0.0})                  # the clip is the checkpoint's
    c = TwoTowerTrainer(cfg_c, dev, seed=seed + 1)                                    # other initial values, no features set
    c.load_state_dict(sd)
    assert c.cfg.feature_clip == 1.5
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "user_features", "item_features", "user_feature_mean", "user_feature_inv_std",
             "item_feature_mean", "item_feature_inv_std", "loss"]
    names += ["user_accum", "item_accum", "dense_accum"] if opt == "adagrad" else ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.P_user, b.P_user)
    # with the feature into a config without it, and the other way round; another F; a checkpoint from before the feature loads
    other = TwoTowerTrainer(_cfg(opt, **kw), dev, seed=seed)
    with pytest.raises(ValueError, match="n_user_features"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="n_user_features"):
        c.load_state_dict(other.state_dict())
    half = TwoTowerTrainer(_cfg(opt, n_user_features=5, **kw), dev, seed=seed)
    with pytest.raises(ValueError, match="n_item_features"):
        half.load_state_dict(sd)
    wider = TwoTowerTrainer(_cfg(opt, n_user_features=5, n_item_features=6, **kw), dev, seed=seed)
    with pytest.raises(ValueError, match="n_item_features"):
        wider.load_state_dict(sd)
    old = dict(other.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if k not in ("n_user_features", "n_item_features", "feature_clip")}
    other.load_state_dict(old)


# ------------------------------------------------------------------------------------------ 7. inference
def _tower64(tw, x):
    for l in range(tw.n_layers):
        x = x @ tw.w[l].cpu().numpy().astype(np.float64) + tw.b[l].cpu().numpy().astype(np.float64)
        if l < tw.n_layers - 1:
            x = np.maximum(x, 0)
    return x


def test_inference_paths_add_the_features(dev):
    """``user_embeddings`` (700 ids at batch 256: three chunks, the last ragged), ``item_corpus_embeddings``, ``evaluate`` and
    ``evaluate_topk`` feed the towers the id rows + the projected features: the tower inputs bit for bit the restatement, the
    embeddings within 1e-4 of the f64 tower on them; the serving index goes through the same path."""
    from two_tower_amazon_recommender_amd import serving
    from two_tower_amazon_recommender_amd.metrics import FactorizedTopK
    seed = 23
    tr = _feature_trainer(dev, "sgd", seed)
    for s in range(3):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    n = lambda t: t.cpu().numpy()
    fu = (n(tr.user_features), n(tr.user_feature_mean), n(tr.user_feature_inv_std), n(tr.P_user))
    fi = (n(tr.item_features), n(tr.item_feature_mean), n(tr.item_feature_inv_std), n(tr.P_item))
    user_in = lambda ids: fc.features_forward(fu[0], ids, fu[1], fu[2], fu[3], 1.5, True, n(tr.user_table)[ids])[0]
    item_in = lambda ids: fc.features_forward(fi[0], ids, fi[1], fi[2], fi[3], 1.5, True, n(tr.item_table)[ids])[0]
    u, i = tr.synthetic_batch(seed, 1, "Z")
    tr.evaluate(u, i)
    assert not _bad(n(tr.user_tower.acts[0]), user_in(n(u)))[0] and not _bad(n(tr.item_tower.acts[0]), item_in(n(i)))[0]
    tr.user_tower.acts[0].zero_()
    corpus = tr.item_corpus_embeddings()
    tr.evaluate_topk(u, i, FactorizedTopK(ks=(5,), temperature=0.1), corpus=corpus)
    assert not _bad(n(tr.user_tower.acts[0]), user_in(n(u)))[0]
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 300, 700)).to(dev)
    emb = tr.user_embeddings(ids)
    tr.check_ids()
    assert not _bad(n(tr.user_tower.acts[0][:188]), user_in(n(ids)[512:]))[0]
    want_q = _tower64(tr.user_tower, user_in(n(ids)).astype(np.float64))
    want_c = _tower64(tr.item_tower, item_in(np.arange(200)).astype(np.float64))
    assert emb.shape == (700, 32) and corpus.shape == (200, 32)
    assert np.abs(n(emb) - want_q).max() <= 1e-4 * np.abs(want_q).max()
    assert np.abs(n(corpus) - want_c).max() <= 1e-4 * np.abs(want_c).max()
    plain = TwoTowerTrainer(_cfg("sgd"), dev, seed=seed)
    k = plain.dense_flat.numel()
    plain.load_state_dict({**plain.state_dict(), "user_table": tr.user_table, "item_table": tr.item_table, "dense": tr.dense_flat[:k]})
    assert (plain.user_embeddings(ids) - emb).abs().max().item() > 1e-3                 # the features do reach the queries
    assert (plain.item_corpus_embeddings() - corpus).abs().max().item() > 1e-3          # ... and the candidates
    index = serving.BruteForce(k=5).index_from_trainer(tr)
    scores, items = index(ids[:16])
    want = (torch.from_numpy(want_q[:16]) @ torch.from_numpy(want_c).T).topk(5, dim=1)
    assert np.abs(n(scores) - want.values.numpy()).max() <= 1e-4 * np.abs(want.values.numpy()).max() + 1e-6


# ------------------------------------------------------------------------------------------ 8-10. custom op, CLIs, refusals
def test_custom_op_passes_opcheck_equals_the_ops_call_and_differentiates_proj(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(3)
    feat, ids, mean, inv_std, proj, _ = _problem(rng, 77, 5, 32)
    ids = np.where(ids == 50, 4, ids)
    d = [T(a, dev) for a in (feat, ids, mean, inv_std)]
    for norm, clip in ((True, 2.5), (False, 0.0)):
        p = T(proj, dev).requires_grad_(True)
        args = (d[0], d[1], d[2] if norm else None, d[3] if norm else None, p, clip)
        torch.library.opcheck(torch.ops.twotower.dense_features, args)
        out = torch.ops.twotower.dense_features(*args)
        z = torch.empty(77, 5, device=dev)
        (want,) = ops.dense_features((d[0], d[1], args[2], args[3], p.detach(), None, False, z), clip=clip)
        assert torch.equal(out, want)
        dy = T(rng.uniform(-1, 1, (77, 32)).astype(np.float32), dev)
        out.backward(dy)
        (slabs,) = ops.dense_features_bwd((z, dy, None))
        assert torch.equal(p.grad, slabs.sum(0))
        assert rel_err(p.grad.cpu().numpy(), fc.features_dp(z.cpu().numpy(), dy.cpu().numpy())) <= 1e-5
        torch.library.opcheck(torch.ops.twotower.dense_features_bwd, (d[0], d[1], args[2], args[3], p.detach(), dy, clip))
    with pytest.raises(ValueError, match="both or neither"):
        torch.ops.twotower.dense_features(d[0], d[1], d[2], None, T(proj, dev), 0.0)


def test_train_cli_runs_with_rating_stats_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow as pa
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  features:\n    numeric:\n      source: rating_stats\n      clip: 3.0\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    rng = np.random.default_rng(4)
    pairs = tmp_path / "pairs.parquet"
    uu, ii = rng.integers(0, 300, 600), rng.integers(0, 200, 600)
    uu[0], ii[0] = 299, 199
    pq.write_table(pa.table({"user_idx": uu, "item_idx": ii, "rating": rng.integers(1, 6, 600).astype(np.float64)}), pairs)
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    ext = tmp_path / "item_features.npy"
    np.save(ext, rng.standard_normal((200, 7)).astype(np.float32))
    runs = (("synthetic", ["--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200", "--side-features", "rating_stats"], (5, 5, 3.0)),
            ("parquet", ["--data", str(pairs), "--feature-clip", "2.0"], (5, 5, 2.0)),                  # the YAML's source, the CLI's clip
            ("external", ["--data", str(pairs), "--item-features", str(ext)], (5, 7, 3.0)),            # the file wins on its side
            ("only-external", ["--data", str(pairs), "--side-features", "none", "--item-features", str(ext)], (0, 7, 3.0)))
    for name, source, (fu, fi, clip) in runs:
        ck, recs = tmp_path / f"{name}.pt", tmp_path / f"{name}.parquet"
        with contextlib.redirect_stdout(io.StringIO()):                    # 600 pairs, 10 % held out: 2 training steps
            assert train.main(["--config", str(cfgp), *source, "--optimizer", "adam", "--save", str(ck)]) == 0
        sd = torch.load(ck, weights_only=True)
        assert sd["step_index"] == 2 and sd["adam_step"] == 3, name
        assert (sd["config"]["n_user_features"], sd["config"]["n_item_features"], sd["config"]["feature_clip"]) == (fu, fi, clip), name
        assert tuple(sd["item_features"].shape) == (200, fi) and ("user_features" in sd) == bool(fu), name
        if fu:
            assert tuple(sd["user_features"].shape) == (300, 5) and sd["user_features"][:, 0].sum().item() == 540, name   # counts: the training split only
        assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + (fu + fi) * 32, name
        assert sd["dense_m"][-fi * 32:].any().item(), name                   # the item projection kernel was trained
        assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
        got = pq.read_table(recs).to_pydict()
        assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all(), name
    norate = tmp_path / "norate.parquet"
    pq.write_table(pa.table({"user_idx": uu, "item_idx": ii}), norate)
    with pytest.raises(SystemExit, match="rating"):
        train.main(["--config", str(cfgp), "--data", str(norate)])
    with pytest.raises(NotImplementedError, match="numeric side features"):
        train.main(["--config", str(cfgp), "--data", str(pairs), "--distributed"])


def test_refusals(dev):
    tr = _feature_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="numeric side features"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="numeric side features"):
        ShardedTwoTowerTrainer(_cfg("sgd", n_item_features=4), dev, seed=1)
    with pytest.raises(NotImplementedError, match="dense segment"):           # 4-layer towers: 16 segments already
        TwoTowerTrainer(_cfg("sgd", tower_dims=(64, 64, 64, 32), n_user_features=2), dev, seed=1)
    d = [torch.zeros(10, 5, device=dev), torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(5, 32, device=dev)]
    with pytest.raises(RuntimeError, match="proj must be"):
        ops.dense_features((d[0], d[1], None, None, torch.zeros(4, 32, device=dev), None, False, None))
    with pytest.raises(ValueError, match="accumulate=True"):
        ops.dense_features((d[0], d[1], None, None, d[2], None, True, None))
    with pytest.raises(RuntimeError, match="z_out must be"):
        ops.dense_features((d[0], d[1], None, None, d[2], None, False, torch.zeros(4, 4, device=dev)))
    with pytest.raises(ValueError, match="F must be in 1..32"):
        ops.dense_features((torch.zeros(10, 33, device=dev), d[1], None, None, torch.zeros(33, 32, device=dev), None, False, None))
    with pytest.raises(RuntimeError, match="dp_slabs must be"):
        ops.dense_features_bwd((torch.zeros(4, 5, device=dev), torch.zeros(4, 32, device=dev), torch.zeros(2, 5, 16, device=dev)))

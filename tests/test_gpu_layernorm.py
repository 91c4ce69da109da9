"""Layer normalisation of the tower hidden layers on the GPU: the two kernels against the f64 restatement of
tests/layernorm_check.py (bars: tests/test_layernorm_cpu.py shows the f32 arithmetic stays 4x below them), the dropout stream,
the trainer's step against f64 autograd with every optimizer, mixed sampling, asymmetric towers, the inference paths,
checkpoints, refusals, the custom op and the CLIs."""
import contextlib
import io

import numpy as np
import pytest
import torch

import layernorm_check as lc
from oracle.synth import dropout_keep
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TID_DROPOUT_BASE, TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

# SGD's rate: the loss is the SUM over the batch and the normalised hidden activations have unit scale whatever the embeddings'
# (U(-0.05, 0.05) at the start), so at temperature 0.1 the gradients reach 1e4 where the plain towers' reach 1e2: the 1e-4 of
# the other features' tests would move every weight by ~1 per step (measured: loss 7359 -> 3416 -> 25081, a saturated softmax)
LR, LR_SGD = 0.001, 0.000001
rel_err = lc.rel_err


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(a, dev):
    """[n + 1, D] device buffer, rows 0..n-1 = a, row n NaN; returns (whole, view of the first n rows)."""
    whole = torch.full((a.shape[0] + 1, a.shape[1]), float("nan"), device=dev)
    whole[:-1].copy_(T(a, dev))
    return whole, whole[:-1]


def _nan_rows(n, d, dev):
    whole = torch.full((n + 1, d), float("nan"), device=dev)
    return whole, whole[:-1]


def _unpack_bits(bits, d):
    """[n, d/32] int32 words -> [n, d] bool, bit c % 32 of word c / 32."""
    w = bits.cpu().numpy().view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(bool).reshape(w.shape[0], d)


# ------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("n,d", lc.SHAPES)
def test_forward_matches_f64(dev, n, d):
    p = lc.problem(n, d)
    z, gamma, beta = T(p["z"], dev), T(p["gamma"], dev), T(p["beta"], dev)
    for eps in lc.EPSILONS:
        whole, y = _nan_rows(n, d, dev)
        ops.layer_norm2((z, gamma, beta, y, None), eps=eps)
        want, _, _ = lc.layer_forward(p["z"], p["gamma"], p["beta"], eps)
        err = rel_err(y.cpu().numpy(), want)
        print(f"forward ({n}, {d}) eps {eps}: {err:.2e}")
        assert torch.isfinite(y).all() and err <= 1e-5, err
        assert torch.isnan(whole[-1]).all()
        whole_r, yr = _nan_rows(n, d, dev)
        bits_whole = torch.full((n + 1, d // 32), -1, dtype=torch.int32, device=dev)
        ops.layer_norm2((z, gamma, beta, yr, bits_whole[:-1]), eps=eps, relu=True)
        assert torch.equal(yr, torch.clamp_min(y, 0.0))                      # max(y, 0), bit for bit
        assert np.array_equal(_unpack_bits(bits_whole[:-1], d), (yr > 0).cpu().numpy())
        assert torch.isnan(whole_r[-1]).all() and (bits_whole[-1] == -1).all()


# ------------------------------------------------------------------------------------------ 2. dropout
@pytest.mark.parametrize("n,d", [(37, 32), (130, 96), (257, 256), (64, 512)])
def test_dropout_is_the_dense_layers_stream(dev, n, d):
    rate, seed, tid, row0 = 0.25, 1234, TID_DROPOUT_BASE + 3, 5 * n
    off = row0 * d
    p = lc.problem(n, d)
    z, gamma, beta = T(p["z"], dev), T(p["gamma"], dev), T(p["beta"], dev)
    (plain,) = ops.layer_norm2((z, gamma, beta, None, None), relu=True)
    bits = ops.relu_bits_like(n, d, dev)
    (y,) = ops.layer_norm2((z, gamma, beta, None, bits), relu=True, dropout=(rate, seed, tid, off))
    keep, scale32 = dropout_keep(seed, tid, row0, n, d, rate)
    keep_t = T(keep, dev)
    assert 0.6 < keep.mean() < 0.9
    assert torch.equal(y == 0, ~keep_t | (plain == 0))                        # the dropped set is exactly dropout_keep's
    scale = torch.tensor(scale32, dtype=torch.float32, device=dev)
    assert torch.equal(y[keep_t], (plain * scale)[keep_t])                    # kept: y_nodrop * 1 / (1 - rate) in f32, bit for bit
    assert np.array_equal(_unpack_bits(bits, d), (y > 0).cpu().numpy())
    # the mask ops.dense_fwd applies for the same (seed, tensor id, offset): an identity layer with bias 1 keeps 1 / (1 - rate)
    x = torch.zeros(n, 32, device=dev)
    w, b = torch.zeros(32, d, device=dev), torch.ones(d, device=dev)
    dense = ops.dense_fwd(x, w, b, relu=True, dropout=(rate, seed, tid, off))
    assert torch.equal(dense > 0, keep_t)
    # two problems, a tensor id each, one counter offset
    keep2 = T(dropout_keep(seed, tid + 1, row0, n, d, rate)[0], dev)
    ya, yb = ops.layer_norm2((z, gamma, beta, None, None), (z, gamma, beta, None, None), relu=True, dropout=(rate, seed, (tid, tid + 1), off))
    assert torch.equal(ya, y) and torch.equal(yb == 0, ~keep2 | (plain == 0))


# ------------------------------------------------------------------------------------------ 3. backward
def _run_bwd(dev, p, eps, n_slabs, pad=0, alias=False):
    n, d = p["z"].shape
    z, gamma = T(p["z"], dev), T(p["gamma"], dev)
    dn_whole, dn = _guarded(p["dn"], dev)
    dz_whole, dz = (dn_whole, dn) if alias else _nan_rows(n, d, dev)
    stride = 2 * d + pad
    slabs = torch.full((n_slabs, stride), float("nan"), device=dev)
    flat = slabs.view(-1)
    ((out, dgs, dbs),) = ops.layer_norm_bwd2((z, gamma, dn, dz, flat, flat[d:]), eps=eps, n_slabs=n_slabs, slab_stride=stride)
    assert out.data_ptr() == dz.data_ptr() and torch.isnan(dz_whole[-1]).all()
    if pad:
        assert torch.isnan(slabs[:, 2 * d:]).all()                            # nothing behind 2 * dim floats of a slab is touched
    return dz.clone(), dgs.cpu().numpy(), dbs.cpu().numpy()


@pytest.mark.parametrize("n,d", lc.SHAPES)
def test_backward_matches_f64(dev, n, d):
    p = lc.problem(n, d)
    for eps in lc.EPSILONS:
        ref = lc.layer_backward(p["z"], p["gamma"], p["dn"], eps)
        first = None
        for ns in (1, ops.layer_norm_num_slabs(n), n // 32 + 5):
            dz, dgs, dbs = _run_bwd(dev, p, eps, ns, pad=0 if ns == 1 else 12)
            errs = dict(dz=rel_err(dz.cpu().numpy(), ref["dz"]), dgamma=rel_err(dgs.astype(np.float64).sum(0), ref["dgamma"]),
                        dbeta=rel_err(dbs.astype(np.float64).sum(0), ref["dbeta"]))
            print(f"backward ({n}, {d}) eps {eps} slabs {ns}:", {k: f"{v:.2e}" for k, v in errs.items()})
            assert max(errs.values()) <= 1e-5, errs
            first = dz if first is None else first
            assert torch.equal(dz, first)                                     # dz does not depend on the slab count
            for s, rows in enumerate(lc.slab_rows(n, ns)):                    # slab s: the sums of its own rows
                part = lc.layer_backward(p["z"], p["gamma"], p["dn"], eps, rows=rows)
                if rows[0] == rows[1]:
                    assert not dgs[s].any() and not dbs[s].any()
                else:
                    assert np.abs(dgs[s] - part["dgamma"]).max() <= 1e-5 * np.abs(ref["dgamma"]).max()
                    assert np.abs(dbs[s] - part["dbeta"]).max() <= 1e-5 * np.abs(ref["dbeta"]).max()
        alias, ags, abs_ = _run_bwd(dev, p, eps, ops.layer_norm_num_slabs(n), alias=True)
        sep, sgs, sbs = _run_bwd(dev, p, eps, ops.layer_norm_num_slabs(n))
        assert torch.equal(alias, sep) and np.array_equal(ags, sgs) and np.array_equal(abs_, sbs)   # dz aliased onto dn: the same bits


def test_backward_writes_empty_slabs_as_exact_zeros(dev):
    p = {k: (v[:5] if v.ndim == 2 else v) for k, v in lc.problem(37, 32).items()}
    dz, dgs, dbs = _run_bwd(dev, p, 1e-3, 4, pad=8)
    assert lc.slab_rows(5, 4)[3] == (5, 5) and not dgs[3].any() and not dbs[3].any() and dgs[:3].any(1).all()
    ref = lc.layer_backward(p["z"], p["gamma"], p["dn"], 1e-3)
    assert rel_err(dgs.astype(np.float64).sum(0), ref["dgamma"]) <= 1e-5 and rel_err(dz.cpu().numpy(), ref["dz"]) <= 1e-5


# ------------------------------------------------------------------------------------------ 4. two problems
@pytest.mark.parametrize("d", [32, 96, 128])
def test_two_problems_of_different_rows_equal_two_launches_and_repeat(dev, d):
    pa, pb = lc.problem(256, d), lc.problem(352, d)
    ta, tb = ({k: T(v, dev) for k, v in p.items()} for p in (pa, pb))
    fwd_prob = lambda t: (t["z"], t["gamma"], t["beta"], None, ops.relu_bits_like(t["z"].shape[0], d, dev))

    def fwd(probs):
        ps = [fwd_prob(t) for t in probs]
        ys = ops.layer_norm2(*ps, relu=True)
        return [y.clone() for y in ys] + [q[4].clone() for q in ps]
    both, again = fwd((ta, tb)), fwd((ta, tb))
    single = fwd((ta,)) + fwd((tb,))
    for x, y in zip(both, again):
        assert torch.equal(x, y)
    assert torch.equal(both[0], single[0]) and torch.equal(both[1], single[2])
    assert torch.equal(both[2], single[1]) and torch.equal(both[3], single[3])
    ns = ops.layer_norm_num_slabs(352)

    def bwd(probs):
        stride = 2 * d * len(probs)
        slabs = torch.full((ns, stride), float("nan"), device=dev)
        flat = slabs.view(-1)
        outs = ops.layer_norm_bwd2(*[(t["z"], t["gamma"], t["dn"], None, flat[2 * d * i:], flat[2 * d * i + d:]) for i, t in enumerate(probs)],
                                   n_slabs=ns, slab_stride=stride)
        assert torch.isfinite(slabs).all()
        return [o[0].clone() for o in outs], slabs.clone()
    (dza, dzb), s2 = bwd((ta, tb))
    (dza2, dzb2), s2b = bwd((ta, tb))
    (dza1,), sa = bwd((ta,))
    (dzb1,), sb = bwd((tb,))
    assert torch.equal(dza, dza2) and torch.equal(dzb, dzb2) and torch.equal(s2, s2b)
    assert torch.equal(dza, dza1) and torch.equal(dzb, dzb1)
    assert torch.equal(s2[:, :2 * d], sa) and torch.equal(s2[:, 2 * d:], sb)


# ------------------------------------------------------------------------------------------ 5. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=200, layer_norm=True, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR_SGD if opt == "sgd" else LR, optimizer=opt, batch_size=batch,
                          layer_norm=layer_norm, **kw)


EXTRAS = dict(n_category_buckets=30, n_title_buckets=100, title_max_tokens=4, n_user_features=5, n_item_features=5, feature_clip=1.5,
              user_history_len=5, normalize_embeddings=True, rating_weight=0.5, rating_hidden=64, cross_layers=2)


def _trainer(dev, opt="adagrad", seed=1001, **kw):
    tr = TwoTowerTrainer(_cfg(opt, **kw), dev, seed=seed)
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


def _n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _params64(tr):
    tws = (tr.user_tower, tr.item_tower)
    p = dict(towers=tuple(([_n64(w) for w in tw.w], [_n64(b) for b in tw.b]) for tw in tws),
             cross=tuple(([_n64(w) for w in tw.cross_w], [_n64(b) for b in tw.cross_b]) for tw in tws),
             norms=tuple(([_n64(g) for g in tw.ln_gamma], [_n64(b) for b in tw.ln_beta]) for tw in tws))
    if tr.rating_on:
        p["head"] = tuple(_n64(t) for t in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating))
    return p


def _scale32(rate):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))


def _reference_step(tr, u, i, params, ratings=None, cand=None):
    """``layernorm_check.step_f64`` on the device's summed input rows x_0 (the table rows themselves where layer 0 gathers them
    inside its launch and acts[0] is not written) and its activation masks (sign of the hidden activations times the dropout
    scale), the parameters as they were before the step."""
    if tr.fuse_lookup:
        x0u, x0i = _n64(tr.user_table[u]), _n64(tr.item_table[i if cand is None else torch.from_numpy(cand).to(i.device)])
    else:
        x0u, x0i = _n64(tr.user_tower.acts[0]), _n64(tr.item_tower.acts[0])
    scale = _scale32(tr.cfg.dropout_rate) if tr.cfg.dropout_rate > 0 else 1.0
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() * scale for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    kw = {}
    if tr.rating_on:
        kw = dict(head=params["head"], ratings=ratings.cpu().numpy(), rating_weight=tr.cfg.rating_weight, head_mask=(tr._r_h > 0).cpu().numpy())
    return lc.step_f64(x0u, x0i, params["cross"], params["towers"], params["norms"],
                       tr.cfg.layer_norm_epsilon, tr.cfg.temperature, masks,
                       normalize_eps=tr.cfg.normalize_eps if tr.cfg.normalize_embeddings else None,
                       item_ids=None if cand is None else i.cpu().numpy(), cand_ids=cand, **kw)


def _norm_grads(tr):
    """The summed norm slabs as ([dgamma per layer] per tower, [dbeta per layer] per tower)."""
    seg = tr.layout.segment("norm")
    s = tr._ln_slabs.view(tr._ln_nslabs, -1).cpu().numpy().astype(np.float64).sum(0)
    cut = lambda name: s[tr.layout.blocks[name].offset - seg.lo:tr.layout.blocks[name].end - seg.lo]
    sides = (("user", tr.user_tower), ("item", tr.item_tower))
    return ([[cut(f"norm.{side}.g{l}") for l in range(tw.n_layers - 1)] for side, tw in sides],
            [[cut(f"norm.{side}.b{l}") for l in range(tw.n_layers - 1)] for side, tw in sides])


def _check_step(tr, r, loss, step, batch):
    """The bars of tests/test_gpu_cross.py::_check_step - loss within 1e-4 relative and 1e-4 per pair, every gradient within
    1e-4 of its max |g| - with its treatment of the item tower's last bias, for the dgamma / dbeta of the summed norm slabs too."""
    print(f"step {step}: loss {loss} (f64 {r['loss']})")
    assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
    checks = [("due", _n64(tr.user_tower.demb), r["dx0"][0]), ("die", _n64(tr.item_tower.demb), r["dx0"][1])]
    dg, db = _norm_grads(tr)
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(tw.n_layers):
            checks += [(f"dw[{t}][{l}]", _n64(tw.dw_slabs[l]).sum(0), r["dw"][t][l]), (f"db[{t}][{l}]", _n64(tw.db_slabs[l]).sum(0), r["db"][t][l])]
        for l in range(tw.n_layers - 1):
            checks += [(f"dgamma[{t}][{l}]", dg[t][l], r["dgamma"][t][l]), (f"dbeta[{t}][{l}]", db[t][l], r["dbeta"][t][l])]
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


@pytest.mark.parametrize("opt,dims,extra", [("sgd", (64, 32), {}), ("adagrad", (64, 32), {}), ("adam", (64, 32), {}),
                                            ("sgd", (64, 64, 32), {}), ("adagrad", (64, 64, 32), {}), ("adam", (64, 64, 32), {}),
                                            ("adagrad", (64, 32), EXTRAS), ("adagrad", (64, 64, 32), dict(dropout_rate=0.25))])
def test_trainer_matches_the_f64_restatement_and_trains(dev, opt, dims, extra):
    seed, batch = 1001, 256
    extras = "rating_weight" in extra
    tr = _trainer(dev, opt, seed, tower_dims=dims, **extra)
    n_seg = 4 * len(dims) + (6 if extras else 0) + 1
    assert len(tr._segs) == n_seg and (tr._adam_segs is None or len(tr._adam_segs) == n_seg) and (not extras or n_seg == 15)
    assert tr.use_composite is False and tr.bwd2_ws is None                   # step() never takes tt_train_step_f32
    # at construction gamma is 1 and beta is 0 - with a seed and without one - behind everything else
    hidden = sum(dims[:-1])
    tail = tr.dense_flat[-4 * hidden:]
    assert (tail[:2 * hidden] == 1).all() and (tail[2 * hidden:] == 0).all()
    assert all((g == 1).all() and (b == 0).all() for tw in (tr.user_tower, tr.item_tower) for g, b in zip(tw.ln_gamma, tw.ln_beta))
    assert tr.user_tower.ln_gamma[0].data_ptr() == tail.data_ptr() and len(tr.item_tower.ln_beta) == len(dims) - 1
    unseeded = TwoTowerTrainer(_cfg(opt, tower_dims=dims, **extra), dev)
    assert (unseeded.dense_flat[-4 * hidden:-2 * hidden] == 1).all() and (unseeded.dense_flat[-2 * hidden:] == 0).all()
    del unseeded
    # the towers' parameters and the tables are those of the trainer without the option
    plain = TwoTowerTrainer(_cfg(opt, tower_dims=dims, layer_norm=False, **extra), dev, seed=seed)
    assert torch.equal(tr.dense_flat[:plain.dense_flat.numel()], plain.dense_flat) and torch.equal(tr.user_table, plain.user_table)
    assert torch.equal(tr.item_table, plain.item_table) and tr.l2_penalty().item() == plain.l2_penalty().item()
    del plain
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
        if tr.cfg.dropout_rate > 0:                                           # the device's masks are the restated stream's
            for t, tw in enumerate((tr.user_tower, tr.item_tower)):
                for l in range(tw.n_layers - 1):
                    n = tw.dims[l + 1]
                    keep, _ = dropout_keep(tr.dropout_seed, TID_DROPOUT_BASE + 2 * l + t, step * batch, batch, n, tr.cfg.dropout_rate)
                    assert not (tw.acts[l + 1].cpu().numpy() != 0)[~keep].any()
        r = _reference_step(tr, u, i, params, ratings=kw.get("ratings"))
        _check_step(tr, r, loss, step, batch)
        tr.apply_gradients()
    p0 = tr.dense_flat[-4 * hidden:].clone()
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
    for tw in (tr.user_tower, tr.item_tower):                                 # every gamma and every beta has moved
        for g, b in zip(tw.ln_gamma, tw.ln_beta):
            assert not (g == 1).any() and not (b == 0).any()
    assert not torch.equal(p0, tr.dense_flat[-4 * hidden:])
    state = [tr.dense_flat, tr.user_table, tr.item_table] + [x for x in (tr.dense_accum, tr.dense_m, tr.dense_v) if x is not None]
    assert all(torch.isfinite(x).all() for x in state)
    # gamma and beta are not counted in the penalty
    want = sum((w.double() ** 2).sum().item() for tw in (tr.user_tower, tr.item_tower) for w in list(tw.w) + list(tw.cross_w))
    if extras:
        want += sum((w.double() ** 2).sum().item() for w in (tr.P_user, tr.P_item, tr.W1_rating, tr.w2_rating))
    assert tr.l2_penalty().item() == pytest.approx(1e-6 * want, rel=1e-9) and tr.l2_penalty().item() != reg0


# ------------------------------------------------------------------------------------------ 6. mixed sampling
def _inference_loss(tr, u, i):
    p = _params64(tr)
    eps, neps = tr.cfg.layer_norm_epsilon, tr.cfg.normalize_eps if tr.cfg.normalize_embeddings else None
    q = lc.tower_forward(_n64(tr.user_table[u]), p["cross"][0], p["towers"][0], p["norms"][0], eps, neps)
    c = lc.tower_forward(_n64(tr.item_table[i]), p["cross"][1], p["towers"][1], p["norms"][1], eps, neps)
    s = torch.from_numpy(q @ c.T / tr.cfg.temperature)
    return float((torch.logsumexp(s, dim=1) - s.diagonal()).sum())


def test_mixed_sampling_step_matches_the_f64_restatement(dev):
    """candidate_sampling='mixed', N = 64: the item tower's normalisation runs over B + N rows, the user tower's over B."""
    seed, batch, n_neg = 77, 256, 64
    tr = _trainer(dev, "sgd", seed, candidate_sampling="mixed", n_sampled_negatives=n_neg)
    assert tr.item_tower.pre[0].shape[0] == batch + n_neg and tr.user_tower.pre[0].shape[0] == batch
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        params = _params64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        cand = tr.cand_ids.cpu().numpy()
        assert np.array_equal(cand[:batch], i.cpu().numpy()) and len(cand) == batch + n_neg
        r = _reference_step(tr, u, i, params, cand=cand)
        _check_step(tr, r, loss, step, batch)
        tr.apply_gradients(step_ids=[u, i])
    g0 = tr.item_tower.ln_gamma[0].clone()
    tr.step(*tr.synthetic_batch(seed, 2, "Z"))
    # evaluate: the in-batch loss over the first B rows of the longer item tower (a partial-row pass)
    u, i = tr.synthetic_batch(seed, 3, "Z")
    loss = tr.evaluate(u, i).item()
    tr.check_ids()
    assert not torch.equal(g0, tr.item_tower.ln_gamma[0])
    want = _inference_loss(tr, u, i)
    print(f"mixed evaluate: {loss} (f64 {want})")
    assert abs(loss - want) <= 1e-4 * abs(want) and abs(loss - want) / batch <= 1e-4


# ------------------------------------------------------------------------------------------ 7. inference
@pytest.mark.parametrize("dims,head", [((64, 32), True), ((64, 64, 32), False)])
def test_inference_paths_match_the_f64_restatement(dev, dims, head):
    seed, batch = 23, 256
    tr = _trainer(dev, "adagrad", seed, tower_dims=dims, **(dict(rating_weight=0.5, rating_hidden=64) if head else {}))
    for s in range(2):
        kw = {"ratings": _ratings(dev, seed, s)} if head else {}
        tr.step(*tr.synthetic_batch(seed, s, "Z"), **kw)
    p = _params64(tr)
    eps = tr.cfg.layer_norm_epsilon
    tower = lambda t, x0: lc.tower_forward(x0, p["cross"][t], p["towers"][t], p["norms"][t], eps)
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 300, 300)).to(dev)        # 256 + a partial chunk of 44
    got = tr.user_embeddings(ids).cpu().numpy()
    eu = rel_err(got, tower(0, _n64(tr.user_table[ids])))
    corpus = tr.item_corpus_embeddings().cpu().numpy()                                        # 200 items: one partial chunk
    ei = rel_err(corpus, tower(1, _n64(tr.item_table)))
    u, i = tr.synthetic_batch(seed, 5, "Z")
    loss, want = tr.evaluate(u, i, **({"ratings": _ratings(dev, seed, 5)} if head else {})).item(), _inference_loss(tr, u, i)
    tr.check_ids()
    print(f"dims {dims}: user_embeddings {eu:.2e} item_corpus_embeddings {ei:.2e} evaluate {loss} (f64 {want})")
    assert eu <= 1e-4 and ei <= 1e-4 and got.shape == (300, 32) and corpus.shape == (200, 32)
    assert abs(loss - want) <= 1e-4 * abs(want) and abs(loss - want) / batch <= 1e-4
    if head:
        pred = tr.predict_ratings(u[:100], i[:100]).cpu().numpy()
        q, c = tower(0, _n64(tr.user_table[u[:100]])), tower(1, _n64(tr.item_table[i[:100]]))
        w1, b1, w2, b2 = p["head"]
        want_pred = np.maximum(b1 + q @ w1[:32] + c @ w1[32:], 0.0) @ w2 + b2
        ep = rel_err(pred, want_pred)
        print(f"predict_ratings {ep:.2e}")
        assert ep <= 1e-4
    # evaluate_topk: layer 0 gathers the user rows itself, the normalisation launch follows it - the embeddings above
    from two_tower_amazon_recommender_amd import metrics
    m = metrics.FactorizedTopK(ks=(10,))
    tr.evaluate_topk(u, i, m, corpus=torch.from_numpy(corpus).to(dev))
    tr.check_ids()
    q_topk = tr.user_tower.acts[-1].clone()
    assert torch.equal(q_topk, tr.user_embeddings(u))
    # a partial-row pass of a tower equals the full pass on those rows
    full = tr.user_tower.forward().clone()
    part = tr.user_tower.forward(rows=100).clone()
    assert torch.equal(part, full[:100])


# ------------------------------------------------------------------------------------------ 8. asymmetric towers
@pytest.mark.parametrize("udims,idims", [((64, 32), (96, 32)), ((64, 64, 32), (64, 32))])
def test_asymmetric_towers_match_the_f64_restatement(dev, udims, idims):
    seed, batch = 5, 256
    tr = _trainer(dev, "adagrad", seed, tower_dims=udims, item_tower_dims=list(idims))
    assert not tr.cfg.symmetric and len(tr._segs) == 2 * (len(udims) + len(idims)) + 1
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        ops.sparse_plan_batched([tr.user_plan, tr.item_plan], [u, i], [300, 200])
        params = _params64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        _check_step(tr, _reference_step(tr, u, i, params), loss, step, batch)
        tr.apply_gradients()
    loss, want = tr.evaluate(u, i).item(), _inference_loss(tr, u, i)
    assert abs(loss - want) <= 1e-4 * abs(want) and abs(loss - want) / batch <= 1e-4


# ------------------------------------------------------------------------------------------ 9. checkpoints
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _trainer(dev, opt, seed)
    run(a, range(4))
    b = _trainer(dev, opt, seed)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["layer_norm"] is True and sd["config"]["layer_norm_epsilon"] == 1e-3
    assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + 4 * 64
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values
    c.load_state_dict(sd)
    assert torch.equal(c.dense_flat, sd["dense"]) and torch.equal(c.user_tower.ln_gamma[0], b.user_tower.ln_gamma[0])
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    names = ["user_table", "item_table", "dense_flat", "loss"]
    names += ["user_accum", "item_accum", "dense_accum"] if opt == "adagrad" else ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]
    for k in names:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.user_tower.ln_gamma[0], b.user_tower.ln_gamma[0])
    # a checkpoint without the option - one from before the field existed too - loads into a trainer without it; a mismatch is refused
    off = TwoTowerTrainer(_cfg(opt, layer_norm=False), dev, seed=seed)
    old = dict(off.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if k not in ("layer_norm", "layer_norm_epsilon")}
    off.load_state_dict(old)
    with pytest.raises(ValueError, match="layer_norm"):
        off.load_state_dict(sd)
    with pytest.raises(ValueError, match="layer_norm"):
        c.load_state_dict(old)
    with pytest.raises(ValueError, match="layer_norm_epsilon"):
        _trainer(dev, opt, seed, layer_norm_epsilon=1e-5).load_state_dict(sd)
    sd2 = dict(off.state_dict())
    sd2["config"] = dict(sd2["config"], layer_norm_epsilon=1e-5)                    # without the option the epsilon does not matter
    off.load_state_dict(sd2)


# ------------------------------------------------------------------------------------------ 10. refusals
def test_trainer_and_op_refusals(dev):
    tr = _trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="layer normalisation"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="layer normalisation"):
        ShardedTwoTowerTrainer(_cfg("sgd"), dev, seed=1)
    with pytest.raises(ValueError, match="multiples of 32"):
        TwoTowerTrainer(_cfg("sgd", tower_dims=(48, 32)), dev, seed=1)
    TwoTowerTrainer(_cfg("sgd", tower_dims=(48, 32), layer_norm=False), dev, seed=1)      # without the option 48 is as fine as before
    with pytest.raises(ValueError, match="hidden layer"):
        TwoTowerTrainer(_cfg("sgd", tower_dims=(32,)), dev, seed=1)
    # step() runs the Python sequence: the composite call's description is never built
    assert tr.use_composite is False
    tr.step(*tr.synthetic_batch(1, 0, "Z"))
    tr.check_ids()
    assert tr._cstep is None and tr.use_composite is False
    z = torch.zeros(64, 32, device=dev)
    g, b = torch.ones(32, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(ValueError, match="alias"):
        ops.layer_norm2((z, g, b, z, None))
    with pytest.raises(ValueError, match="alias"):
        ops.layer_norm_bwd2((z, g, z.clone(), z, None, None))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.layer_norm2((z[:, :16].contiguous(), g[:16].contiguous(), b[:16].contiguous(), None, None))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.layer_norm2((torch.zeros(64, 64, device=dev)[:, :32], g, b, None, None))
    with pytest.raises(RuntimeError, match="dtype"):
        ops.layer_norm2((z.double(), g, b, None, None))
    with pytest.raises(RuntimeError, match="gamma"):
        ops.layer_norm2((z, torch.ones(64, device=dev), b, None, None))
    with pytest.raises(ValueError, match="eps"):
        ops.layer_norm2((z, g, b, None, None), eps=0.0)
    with pytest.raises(RuntimeError, match="slab_stride"):
        ops.layer_norm_bwd2((z, g, z.clone(), None, torch.zeros(200, device=dev), torch.zeros(200, device=dev)), n_slabs=2, slab_stride=48)
    assert ops.layer_norm2((z[:0], g, b, None, None))[0].shape == (0, 32)     # no rows: no launch


# ------------------------------------------------------------------------------------------ 11. custom op
@pytest.mark.parametrize("relu", [False, True])
def test_custom_op_passes_opcheck_and_differentiates_every_input(dev, relu):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    n, d, eps = 77, 160, 1e-3
    p = lc.problem(n, d)
    args = tuple(T(p[k], dev).requires_grad_(True) for k in ("z", "gamma", "beta"))
    torch.library.opcheck(torch.ops.twotower.layer_norm, args + (eps, relu))
    y = torch.ops.twotower.layer_norm(*args, eps, relu)
    (want,) = ops.layer_norm2(tuple(a.detach() for a in args) + (None, None), eps=eps, relu=relu)
    assert torch.equal(y, want)
    y.backward(T(p["dn"], dev))
    ref = tuple(torch.tensor(p[k].astype(np.float64), requires_grad=True) for k in ("z", "gamma", "beta"))
    y64 = torch.nn.functional.layer_norm(ref[0], (d,), ref[1], ref[2], eps)
    y64 = torch.relu(y64) if relu else y64
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) <= 1e-5
    assert np.array_equal(y.detach().cpu().numpy() > 0, y64.detach().numpy() > 0)
    y64.backward(torch.tensor(p["dn"].astype(np.float64)))
    for a, r, k in zip(args, ref, ("dz", "dgamma", "dbeta")):
        err = rel_err(a.grad.cpu().numpy(), r.grad.numpy())
        print(f"custom op relu={relu}: {k} {err:.2e}")
        assert err <= 1e-5, (k, err)
    torch.library.opcheck(torch.ops.twotower.layer_norm_bwd, (args[0].detach(), args[1].detach(), y.detach(), T(p["dn"], dev), eps, relu))


# ------------------------------------------------------------------------------------------ 12. CLIs
def test_train_cli_trains_and_saves_and_recommend_needs_only_the_checkpoint(dev, tmp_path):
    import json
    import pyarrow.parquet as pq
    from two_tower_amazon_recommender_amd import config as cfgmod, recommend, train
    base = ("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n  l2_regularization: 1e-6\n"
            "  training:\n    batch_size: 256\n    learning_rate: 0.01\n    epochs: 2\n"
            "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text(base)
    ck = tmp_path / "ck.pt"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):            # 1100 pairs, 40 % held out: 2 training steps per epoch, 1 validation batch
        assert train.main(["--config", str(cfgp), "--synthetic", "1100", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--val-fraction", "0.4", "--layer-norm", "--save", str(ck)]) == 0
    hist = json.loads(out.getvalue().strip().splitlines()[-1])["history"]
    print(hist)
    assert all(np.isfinite(h["val_loss_per_pair"]) for h in hist) and len(hist) == 2
    assert hist[1]["train_loss_per_pair"] < hist[0]["train_loss_per_pair"]                    # the loss falls
    sd = torch.load(ck, weights_only=True)
    assert (sd["config"]["layer_norm"], sd["config"]["layer_norm_epsilon"], sd["step_index"]) == (True, 1e-3, 4)
    assert sd["dense"].numel() == 2 * (32 * 64 + 64 + 64 * 32 + 32) + 4 * 64
    assert (sd["dense"][-256:-128] != 1).any().item() and sd["dense"][-128:].any().item()     # gamma and beta were trained
    # a YAML with model.layer_norm gives the same config
    with_block = cfgmod.model_config_from_dict(cfgmod.load_yaml(_write(tmp_path / "ln.yaml", base.replace(
        "  training:", "  layer_norm:\n    enabled: true\n  training:"))), 300, 200)[0]
    assert with_block.layer_norm is True and with_block.layer_norm_epsilon == sd["config"]["layer_norm_epsilon"]
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


def _write(path, text):
    path.write_text(text)
    return path

"""Global-norm gradient clipping and the learning-rate schedule on the GPU: the two clip launches against the f64 restatement
of tests/clip_check.py (bar 1e-5 of the norm: tests/test_clip_cpu.py shows the kernel's summation order in f32 stays 4x below
it), the in-place scale bit for bit, and the trainer - a huge clip norm changes nothing, a clip to exactly a quarter is the
step at a quarter of the rate, the norm covers every buffer by the per-occurrence rules, the schedule reaches the kernels, the
composite call and the checkpoint - with the refusals, the custom op and the CLI."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

import clip_check as cc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

NAN = float("nan")


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ 1. the op against f64
class Device:
    """The buffers of a ``clip_check.problem`` on the device, every one inside a NaN-filled allocation: a guard row in front of
    and behind a row buffer, four guard floats around a dense buffer, and NaN in the padding between two slabs."""

    def __init__(self, bufs, dense, dev):
        self.wholes, self.real, self.rows, self.dense, self.keep = [], [], [], [], []
        for g, weight, ids, mode in bufs:
            whole = torch.full((g.shape[0] + 2, g.shape[1]), NAN, device=dev)
            whole[1:-1].copy_(T(g, dev))
            real = torch.zeros_like(whole, dtype=torch.bool)
            real[1:-1] = True
            ids_d = T(ids, dev)
            self.keep.append(ids_d)                                          # (the descriptors hold raw pointers)
            self.rows.append(ops.make_clip_rows(whole[1:-1], weight, ids_d, mode))
            self.wholes.append(whole); self.real.append(real)
        for slabs, count, n_slabs, stride in dense:
            host = np.full((n_slabs, stride), np.nan, dtype=np.float32)
            host[:, :count] = slabs[:, :count]
            whole = torch.full((8 + n_slabs * stride,), NAN, device=dev)
            whole[4:-4].copy_(T(host.reshape(-1), dev))
            real = torch.zeros_like(whole, dtype=torch.bool)
            real[4:-4].view(n_slabs, stride)[:, :count] = True
            self.dense.append(ops.make_clip_dense(whole[4:-4], count, n_slabs, stride))
            self.wholes.append(whole); self.real.append(real)
        self.before = [w.clone() for w in self.wholes]

    def restore(self):
        for w, b in zip(self.wholes, self.before):
            w.copy_(b)

    def clip(self, c):
        return ops.clip_global_norm_(self.rows, self.dense, c).cpu().numpy()

    def check_scaled(self, scale):
        """Every real element is its value before times ``scale`` (one f32 product), everything around it has its bits."""
        s = torch.tensor(float(scale), device=self.wholes[0].device)
        for k, (w, b, real) in enumerate(zip(self.wholes, self.before, self.real)):
            assert torch.equal(bits(w), bits(torch.where(real, b * s, b))), k
            assert torch.isnan(w[~real]).all(), k


@pytest.mark.parametrize("rows,dim", [(r, d) for r in cc.ROWS for d in cc.DIMS])
def test_norm_and_in_place_scale_match_the_f64_restatement(dev, rows, dim):
    bufs, dense = cc.problem(rows, dim)
    ref = cc.global_norm(bufs, dense)
    d = Device(bufs, dense, dev)
    c = ref / 3
    norm, scale = d.clip(c)
    print(f"rows {rows} dim {dim}: norm {norm!r} (f64 {ref!r}, rel {abs(norm - ref) / ref:.2e}) scale {scale!r}")
    assert abs(norm - ref) <= 1e-5 * ref
    assert scale == cc.scale_of(norm, c) and 0.3 < scale < 0.4
    d.check_scaled(scale)
    after = [w.clone() for w in d.wholes]
    # the same inputs again: the same bits
    d.restore()
    norm2, scale2 = d.clip(c)
    assert norm2.tobytes() == norm.tobytes() and scale2.tobytes() == scale.tobytes()
    assert all(torch.equal(bits(a), bits(w)) for a, w in zip(after, d.wholes))
    # c >= norm: scale is exactly 1 and nothing changes
    for big in (float(norm), 10.0 * ref, 1e30):
        d.restore()
        n3, s3 = d.clip(big)
        assert n3.tobytes() == norm.tobytes() and s3 == 1.0
        assert all(torch.equal(bits(b), bits(w)) for b, w in zip(d.before, d.wholes))


def test_zero_gradients_an_inf_and_rows_that_do_not_count(dev):
    bufs, dense = cc.problem(65, 36)
    zero = ([(np.zeros_like(g), w, ids, m) for g, w, ids, m in bufs], [(np.zeros_like(s), c, n, st) for s, c, n, st in dense])
    d = Device(*zero, dev)
    norm, scale = d.clip(1.0)
    assert norm == 0.0 and scale == 1.0
    d.check_scaled(1.0)
    assert all((w[r] == 0).all() for w, r in zip(d.wholes, d.real))          # no NaN reached the buffers
    # rows whose factor is 0 (empty bags and skipped slots of the buffers without a constant weight) hold 1e30: the norm does not move
    ref = cc.global_norm(bufs, dense)
    poisoned, n_poisoned = [], 0
    for g, w, ids, m in bufs:
        f = cc.row_factors(g.shape[0], w, ids, m)
        g = g.copy()
        g[f == 0] = 1e30
        n_poisoned += int((f == 0).sum())
        poisoned.append((g, w, ids, m))
    assert n_poisoned > 50
    clean, dirty = Device(bufs, dense, dev), Device(poisoned, dense, dev)
    (n0, s0), (n1, s1) = clean.clip(ref / 2), dirty.clip(ref / 2)
    assert n0.tobytes() == n1.tobytes() and s0.tobytes() == s1.tobytes() and abs(n1 - ref) <= 1e-5 * ref
    dirty.check_scaled(s1)                                                   # (row buffers are scaled in full)
    # one inf in one buffer: norm inf, scale NaN, every gradient NaN - loud, as TF's
    for k in (0, len(bufs)):                                                 # in a row buffer, in a dense segment
        d = Device(bufs, dense, dev)
        d.wholes[k].view(-1)[d.real[k].view(-1).nonzero()[3]] = float("inf")
        norm, scale = d.clip(1.0)
        assert np.isinf(norm) and norm > 0 and np.isnan(scale)
        assert all(torch.isnan(w).all() for w in d.wholes)


def test_no_buffers_and_empty_buffers_report_norm_0_scale_1(dev):
    stats = torch.full((2,), NAN, device=dev)
    assert ops.clip_global_norm_([], [], 1.0, stats=stats) is stats and stats.tolist() == [0.0, 1.0]
    empty = torch.zeros(0, 8, device=dev)
    stats.fill_(NAN)
    ops.clip_global_norm_([ops.make_clip_rows(empty)], [ops.make_clip_dense(torch.zeros(4, device=dev), 0)], 2.0, stats=stats)
    assert stats.tolist() == [0.0, 1.0]
    g = torch.ones(3, 8, device=dev)
    with pytest.raises(ValueError, match="clip_norm"):
        ops.clip_global_norm_([ops.make_clip_rows(g)], [], 0.0)
    with pytest.raises(ValueError, match="at most 24"):
        ops.clip_global_norm_([ops.make_clip_rows(g)] * 25, [], 1.0)
    with pytest.raises(RuntimeError, match="slot_ids"):
        ops.make_clip_rows(g, 1.0, torch.zeros(7, dtype=torch.int64, device=dev), "sum")
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.clip_global_norm_([ops.make_clip_rows(torch.ones(3, 6, device=dev))], [], 1.0)
    assert (g == 1).all()


# ------------------------------------------------------------------------------------------ 2. the trainer
BATCH = 64
FEATURES = dict(n_category_buckets=7, n_title_buckets=50, title_max_tokens=3, n_user_features=3, n_item_features=3, user_history_len=4,
                rating_weight=0.5, rating_hidden=32, cross_layers=1, layer_norm=True)
MIXED = dict(FEATURES, n_category_buckets=0, user_history_len=0, candidate_sampling="mixed", n_sampled_negatives=32)
VARIANTS = {"sum": dict(FEATURES, history_pooling="sum", title_pooling="sum"), "mean": dict(FEATURES),
            "sqrtn": dict(FEATURES, history_pooling="sqrtn", title_pooling="sqrtn"),
            "attention": dict(FEATURES, history_pooling="attention"), "mixed": MIXED}
RATES = {"sgd": 1e-4, "adagrad": 1e-3, "adam": 1e-3}


def _cfg(opt, **kw):
    base = dict(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], temperature=0.5, l2_regularization=1e-6,
                learning_rate=RATES[opt], optimizer=opt, batch_size=BATCH)
    base.update(kw)
    return TwoTowerConfig(**base)


def _trainer(dev, opt="sgd", seed=31, **kw):
    tr = TwoTowerTrainer(_cfg(opt, **kw), dev, seed=seed)
    if tr.user_features is not None:
        tr.set_user_features(tr.synthetic_user_features(seed))
    if tr.item_features is not None:
        tr.set_item_features(tr.synthetic_item_features(seed))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    if tr.user_history is not None:
        pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(4)]
        u, i = (torch.cat([p[k] for p in pairs]).cpu().numpy() for k in (0, 1))
        tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, tr.cfg.user_history_len), dev))
    return tr


def _batch(tr, seed, step):
    """Power-law ids (duplicates occur) with what the model's features need beside them."""
    u, i = tr.synthetic_batch(seed, step, "Z")
    kw = {}
    if tr.cat_table is not None:
        kw["category_ids"] = tr.synthetic_categories(seed, step)
    if tr.rating_on:
        rng = np.random.default_rng(1000 * seed + step)
        r = rng.integers(1, 6, BATCH).astype(np.float32)
        r[rng.random(BATCH) < 0.1] = np.nan
        kw["ratings"] = T(r, tr.dev)
    return u, i, kw


def _state(tr):
    out = {"dense_flat": tr.dense_flat}
    for name in ("dense_accum", "dense_m", "dense_v"):
        if getattr(tr, name) is not None:
            out[name] = getattr(tr, name)
    for t in tr.tables.values():
        for k, v in (("table", t.table), ("accum", t.accum), ("m", t.m), ("v", t.v)):
            if v is not None:
                out[f"{t.prefix}_{k}"] = v
    return out


def _assert_same_state(a, b):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.isfinite(sa[k]).all(), k
        assert torch.equal(bits(sa[k]), bits(sb[k])), k


def _run(tr, seed, steps):
    for s in steps:
        u, i, kw = _batch(tr, seed, s)
        tr.step(u, i, **kw)
    tr.check_ids()
    return tr


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("variant", ["sum", "mean", "attention", "mixed"])
def test_a_huge_clip_norm_changes_no_bit_of_the_step(dev, opt, variant):
    seed = 31
    off = _run(_trainer(dev, opt, seed, **VARIANTS[variant]), seed, range(2))
    on = _run(_trainer(dev, opt, seed, global_clipnorm=1e30, **VARIANTS[variant]), seed, range(2))
    _assert_same_state(on, off)
    assert torch.equal(on.loss, off.loss)
    norm, scale = on.grad_norm.item(), on.clip_scale.item()
    print(f"{opt} {variant}: grad_norm {norm}")
    assert np.isfinite(norm) and norm > 0 and scale == 1.0
    assert not torch.equal(on.user_table, _trainer(dev, opt, seed, **VARIANTS[variant]).user_table)      # (it did train)
    with pytest.raises(ValueError, match="no step has been clipped"):
        off.grad_norm
    assert off.clip_gradients() is None                                      # off: nothing happens


def _gradient_tensors(tr):
    """Every gradient buffer of the step by the name the trainer keeps it under (the slot rows: the kept ones only)."""
    out = [tr.user_tower.demb, tr.item_tower.demb]
    for tw in (tr.user_tower, tr.item_tower):
        out += list(tw.dw_slabs) + list(tw.db_slabs)
    out += [fs.slabs for fs in tr.sides.values()]
    out += [x for x in (tr._r_kslabs, tr._r_bslabs, tr._c_slabs, tr._ln_slabs, tr._ha_slabs) if x is not None]
    if tr.history_slot_grads is not None:
        out.append(tr.history_slot_grads[tr.history_ids >= 0])
    return out


@pytest.mark.parametrize("variant", ["sum", "mean", "sqrtn", "attention", "mixed"])
def test_a_clip_to_a_quarter_is_the_step_at_a_quarter_of_the_rate_bit_for_bit(dev, variant):
    """scale = 0.25 commutes with every rounding between the gradient buffers and the parameters (SGD, no l2 term, which the clip
    does not see): a buffer scaled twice, or not at all, shows as a different bit somewhere."""
    seed, lr = 47, 1e-4
    kw = dict(VARIANTS[variant], l2_regularization=0.0, dropout_rate=0.0, learning_rate=lr)
    a = _run(_trainer(dev, "sgd", seed, global_clipnorm=1e30, **kw), seed, [0])
    n = a.grad_norm.item()
    smallest = min(g[g != 0].abs().min().item() for g in _gradient_tensors(a) if (g != 0).any())
    print(f"{variant}: grad_norm {n}, smallest non-zero gradient entry {smallest:.3e}")
    assert smallest > 1e-30 and np.isfinite(n)
    b = _run(_trainer(dev, "sgd", seed, global_clipnorm=n / 4, **kw), seed, [0])
    assert b.grad_norm.item() == n and b.clip_scale.item() == 0.25
    c = _run(_trainer(dev, "sgd", seed, **dict(kw, learning_rate=lr / 4)), seed, [0])
    _assert_same_state(b, c)
    fresh = _trainer(dev, "sgd", seed, **kw)
    for k, v in _state(fresh).items():                                       # every table and the dense parameters have moved
        assert not torch.equal(v, _state(b)[k]), k


def _host(t):
    return t.detach().cpu().numpy().copy()


def _reference_buffers(tr):
    """The step's gradient as section 1 of the definition counts it, from the buffers as they stand behind forward_backward:
    one entry per TABLE (a buffer that several tables consume appears once for each) and one per dense segment."""
    cfg, b = tr.cfg, tr.cfg.batch_size
    ud, idm = _host(tr.user_tower.demb), _host(tr.item_tower.demb)
    bufs = [(ud, 1.0, None, "rows"), (idm, 1.0, None, "rows")]               # the user and the item id table
    if tr.cat_table is not None:
        bufs.append((idm, 1.0, None, "rows"))
    if tr.title_table is not None:
        bufs.append((idm, 0.0, _host(tr.title_ids).reshape(idm.shape[0], cfg.title_max_tokens), cfg.title_pooling))
    if tr.history_table is not None:
        ids = _host(tr.history_ids)
        if cfg.history_pooling == "attention":
            bufs.append((_host(tr.history_slot_grads), 0.0, ids, "mask"))
        else:
            bufs.append((ud, 0.0, ids.reshape(b, cfg.user_history_len), cfg.history_pooling))
    dense = []
    for side, tw in (("user", tr.user_tower), ("item", tr.item_tower)):
        for l in range(tw.n_layers):
            for slabs in (tw.dw_slabs[l], tw.db_slabs[l]):
                count = slabs[0].numel()
                dense.append((_host(slabs), count, tw.n_slabs, count))
    for fs in tr.sides.values():
        dense.append((_host(fs.slabs), fs.slabs[0].numel(), fs.n_slabs, fs.slabs[0].numel()))
    if tr.rating_on:
        for slabs in (tr._r_kslabs, tr._r_bslabs):
            dense.append((_host(slabs), slabs.shape[1], slabs.shape[0], slabs.shape[1]))
    lay = tr.layout
    if cfg.cross_layers:
        kernels, biases = lay.segment("cross.kernels"), lay.segment("cross.biases")
        flat = _host(tr._c_slabs)
        dense.append((flat, kernels.size, tr._c_nslabs, kernels.stride))
        dense.append((flat[biases.lo - kernels.lo:], biases.size, tr._c_nslabs, kernels.stride))
    if cfg.history_attention:
        dense.append((_host(tr._ha_slabs), tr._ha_slabs.shape[1], tr._ha_slabs.shape[0], tr._ha_slabs.shape[1]))
    if cfg.layer_norm:
        norm = lay.segment("norm")
        dense.append((_host(tr._ln_slabs), norm.size, tr._ln_nslabs, norm.stride))
    assert len(dense) == len(lay.segments)
    return bufs, dense


@pytest.mark.parametrize("variant", ["sum", "mean", "sqrtn", "attention", "mixed"])
def test_grad_norm_covers_every_buffer_by_the_per_occurrence_rules(dev, variant):
    seed = 53
    tr = _trainer(dev, "adagrad", seed, global_clipnorm=1e30, **VARIANTS[variant])
    _run(tr, seed, [0])                                                      # (a step first: the attention vector leaves zero)
    u, i, kw = _batch(tr, seed, 1)
    tr.forward_backward(u, i, **kw)
    bufs, dense = _reference_buffers(tr)
    ref = cc.global_norm(bufs, dense)
    tr.clip_gradients()
    got = tr.grad_norm.item()
    parts = {m: cc.global_norm([x for x in bufs if x[3] == m], []) for m in sorted({x[3] for x in bufs})}
    print(f"{variant}: grad_norm {got!r} (f64 {ref!r}, rel {abs(got - ref) / ref:.2e}); rows {parts}, dense {cc.global_norm([], dense)}")
    assert abs(got - ref) <= 1e-5 * ref
    assert all(v > 0 for v in parts.values()) and cc.global_norm([], dense) > 0                        # every kind is there
    if variant == "attention":                                               # the skipped slots' rows are stale: they must not count
        skipped = tr.history_ids < 0
        assert 0 < skipped.sum().item() < skipped.numel()
        tr.history_slot_grads[skipped] = 1e30
        tr.clip_gradients()
        assert tr.grad_norm.item() == got and tr.clip_scale.item() == 1.0
        assert (tr.history_slot_grads[skipped] == 1e30).all()
    tr.apply_gradients(step_ids=[u, i] + ([kw["category_ids"]] if "category_ids" in kw else []))
    tr.check_ids()
    assert all(torch.isfinite(v).all() for v in _state(tr).values())


# ------------------------------------------------------------------------------------------ 3. the schedule on the device
SCHEDULE = dict(lr_warmup_steps=2, lr_decay="linear", lr_decay_steps=4)


@pytest.mark.parametrize("clip", [0.0, 5.0])
def test_the_schedule_reaches_the_kernels_the_composite_call_and_the_checkpoint(dev, clip):
    seed, peak = 61, 2e-4
    opt = "adagrad" if clip else "sgd"
    kw = dict(l2_regularization=0.0, learning_rate=peak, global_clipnorm=clip, **SCHEDULE)
    a = _trainer(dev, opt, seed, **kw)
    want = [peak * f for f in (0.5, 1.0, 1.0, 0.75, 0.5, 0.25, 0.0, 0.0)]
    assert [a.learning_rate_at(k) for k in range(8)] == pytest.approx(want, rel=1e-15, abs=0.0) and a.cfg.learning_rate == peak
    # step 0 is the step of a fresh trainer at the constant rate lr_0, bit for bit
    const = _trainer(dev, opt, seed, **dict(kw, learning_rate=a.learning_rate_at(0), lr_warmup_steps=0, lr_decay="none"))
    _run(a, seed, [0]); _run(const, seed, [0])
    _assert_same_state(a, const)
    assert a.learning_rate == want[0] and const.learning_rate == want[0]
    # only a schedule: the composite call is still taken; with clipping the step is the Python sequence
    assert (a._cstep is not None) == (clip == 0.0) and (a.use_composite and a.fuse_lookup)
    for k in range(1, 5):
        _run(a, seed, [k])
        assert a.learning_rate == pytest.approx(want[k], rel=1e-15) and a.step_index == k + 1
    # checkpoint after 3 steps, reload into a trainer with other initial values, two more steps: the uninterrupted run's bits
    b = _run(_trainer(dev, opt, seed, **kw), seed, range(3))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["step_index"] == 3 and sd["config"]["lr_warmup_steps"] == 2 and sd["config"]["global_clipnorm"] == clip
    c = _trainer(dev, opt, seed + 1, **kw)
    c.load_state_dict(sd)
    assert c.learning_rate == a.learning_rate_at(3) == pytest.approx(want[3], rel=1e-15)
    _run(c, seed, [3, 4])
    _assert_same_state(a, c)
    assert c.learning_rate == a.learning_rate == pytest.approx(want[4], rel=1e-15)
    # a checkpoint from before the keys existed loads (as a constant rate, unclipped, into a trainer without the options)
    plain = _trainer(dev, opt, seed, l2_regularization=0.0, learning_rate=peak)
    old = dict(plain.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if not (k.startswith("lr_") or k == "global_clipnorm")}
    assert len(old["config"]) == len(sd["config"]) - 5 and set(old) == set(sd)
    plain.load_state_dict(old)
    assert plain.learning_rate == peak and TwoTowerConfig(**old["config"]).global_clipnorm == 0.0


# ------------------------------------------------------------------------------------------ 4. refusals, the custom op, the CLI
def test_refusals_and_the_step_never_takes_the_composite_call_when_it_clips(dev):
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    for kw, what in ((dict(global_clipnorm=1.0), "gradient clipping"), (dict(lr_warmup_steps=3), "learning-rate schedule")):
        tr = _trainer(dev, "sgd", 7, **kw)
        with pytest.raises(NotImplementedError, match=what):
            tr.capture_graph()
        with pytest.raises(NotImplementedError, match=what):
            ShardedTwoTowerTrainer(_cfg("sgd", **kw), dev, seed=7)
    with pytest.raises(ValueError, match="global_clipnorm"):
        TwoTowerTrainer(_cfg("sgd", global_clipnorm=-1.0), dev)
    with pytest.raises(ValueError, match="lr_decay_steps"):
        TwoTowerTrainer(_cfg("sgd", lr_decay="cosine"), dev)
    off, on = _trainer(dev, "adagrad", 7), _trainer(dev, "adagrad", 7, global_clipnorm=0.5)
    _run(off, 7, range(2)); _run(on, 7, range(2))
    assert off._cstep is not None and on._cstep is None and on.use_composite       # the option, not a switch, keeps it off the call
    assert 0.0 < on.clip_scale.item() < 1.0 and on.grad_norm.item() > 0.5
    assert not torch.equal(on.user_table, off.user_table)


def test_custom_op_agrees_with_the_op_and_with_torch(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(5)
    host = [rng.standard_normal(s).astype(np.float32) for s in ((37, 5), (4096,), (3, 7, 11), (1,))]
    ref = float(np.sqrt(sum((h.astype(np.float64) ** 2).sum() for h in host)))
    a, b = [T(h, dev) for h in host], [T(h, dev) for h in host]
    stats = torch.ops.twotower.clip_by_global_norm_(a, ref / 2)
    want = ops.clip_global_norm_([], [ops.make_clip_dense(t.view(-1), t.numel()) for t in b], ref / 2)
    assert torch.equal(stats, want) and all(torch.equal(x, y) for x, y in zip(a, b))
    norm, scale = stats.tolist()
    assert abs(norm - ref) <= 1e-5 * ref and scale == cc.scale_of(norm, ref / 2)
    for x, h in zip(a, host):
        assert torch.equal(x, T(h, dev) * scale)
    p = [torch.nn.Parameter(T(h, dev)) for h in host]                               # torch.nn.utils.clip_grad_norm_'s result
    for q, h in zip(p, host):
        q.grad = T(h, dev).clone()
    total = torch.nn.utils.clip_grad_norm_(p, ref / 2).item()
    assert abs(total - norm) <= 1e-5 * ref
    assert all(torch.allclose(q.grad, x, rtol=1e-5, atol=0) for q, x in zip(p, a))
    with pytest.raises(RuntimeError, match="dtype"):
        torch.ops.twotower.clip_by_global_norm_([torch.zeros(4, device=dev, dtype=torch.float64)], 1.0)


def test_train_cli_clips_warms_up_decays_and_logs(dev, tmp_path):
    from two_tower_amazon_recommender_amd import train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n  l2_regularization: 1e-6\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.01\n    epochs: 2\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck = tmp_path / "ck.pt"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):            # 1100 pairs, 40 % held out: 2 training steps per epoch, 4 in all
        assert train.main(["--config", str(cfgp), "--synthetic", "1100", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--val-fraction", "0.4", "--global-clipnorm", "1", "--lr-warmup-steps", "3", "--lr-decay", "cosine",
                           "--lr-decay-steps", "auto", "--save", str(ck)]) == 0
    hist = json.loads(out.getvalue().strip().splitlines()[-1])["history"]
    print(hist)
    assert len(hist) == 2 and all(np.isfinite(h["train_loss_per_pair"]) for h in hist)
    assert hist[0]["lr"] == pytest.approx(0.01 * 2 / 3, rel=1e-15) and hist[1]["lr"] == 0.01   # steps 1 and 3 of a 3-step warm-up
    assert all(np.isfinite(h["grad_norm"]) and h["grad_norm"] > 1.0 for h in hist)               # (the summed loss: well above c = 1)
    sd = torch.load(ck, weights_only=True)
    got = {k: sd["config"][k] for k in ("global_clipnorm", "lr_warmup_steps", "lr_decay", "lr_decay_steps", "lr_min_ratio")}
    assert got == dict(global_clipnorm=1.0, lr_warmup_steps=3, lr_decay="cosine", lr_decay_steps=1, lr_min_ratio=0.0)
    assert sd["step_index"] == 4
    # --resume continues the schedule at the saved step: one more epoch runs steps 4 and 5, behind the decay's end
    cfgp.write_text(cfgp.read_text().replace("epochs: 2", "epochs: 3"))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert train.main(["--config", str(cfgp), "--synthetic", "1100", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--val-fraction", "0.4", "--global-clipnorm", "1", "--lr-warmup-steps", "3", "--lr-decay", "cosine",
                           "--lr-decay-steps", "1", "--lr-min-ratio", "0.5", "--resume", str(ck)]) == 0
    hist = json.loads(out.getvalue().strip().splitlines()[-1])["history"]
    assert len(hist) == 1 and hist[0]["epoch"] == 3 and hist[0]["lr"] == pytest.approx(0.005, rel=1e-15)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        train.main(["--config", str(cfgp), "--synthetic", "1100", "--distributed", "--global-clipnorm", "1"])

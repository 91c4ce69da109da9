"""Row-wise Adagrad on the GPU (csrc/rowwise.hip, tt_rowwise_adagrad_step_f32): the sparse update against the f32 restatement
of tests/rowwise_check.py BIT FOR BIT (every device operation is correctly rounded, and so is NumPy's; the order of the row's
sum of squares is part of the contract), laziness (table AND accumulator), runs that cross 64-slot blocks, rows of more than two
chunks per lane (the kernels' other instantiations), every feature of the trainer beside an Adagrad trainer, skipped ids, the dense
segments riding in the call against tt_dense_update_f32, one call for three tables and four segments, the trainer (the update
against the restatement fed the device's own gradients; the dense state against an Adagrad trainer), checkpoints, the refusal
of graph capture, the custom op, and the CLI."""
import contextlib
import io

import numpy as np
import pytest
import torch

import rowwise_check as rc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR, EPS = 0.01, 1e-7


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ids(kind, rows, n, rng):
    if kind == "U":
        return rng.integers(0, rows, n).astype(np.int64)
    return np.minimum((rows * rng.random(n) ** 4).astype(np.int64), rows - 1)        # power law: floor(rows * u^4)


def _state(rows, dim, rng):
    """(w, a): embedding-scale parameters and one accumulator per row, at and above Keras's initial 0.1."""
    return rng.uniform(-0.05, 0.05, (rows, dim)).astype(np.float32), rng.uniform(0.1, 0.3, rows).astype(np.float32)


def _device_sparse(dev, state, ids, grads, lr=LR):
    """One tt_rowwise_adagrad_step_f32 call for one table from a copy of ``state``; returns [w, a] as NumPy arrays."""
    d = [T(a, dev) for a in state]
    plan = ops.SparsePlan(len(ids), dev).run(T(ids, dev), state[0].shape[0])
    ops.rowwise_adagrad_step_([(d[0], d[1], T(grads, dev), plan)], [], lr, EPS)
    return [t.cpu().numpy() for t in d]


def _restated_sparse(state, ids, grads, lr=LR):
    w, a = (x.copy() for x in state)
    uniq = rc.sparse_rowwise_adagrad(w, a, ids, grads, lr, EPS)
    return [w, a], uniq


def _assert_bits(got, want, what, names=("w", "a")):
    for g, w, name in zip(got, want, names):
        bad = rc.bits(g) != rc.bits(w)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ------------------------------------------------------------------------------------------ sparse, bit-exact and lazy
@pytest.mark.parametrize("kind", ["U", "Z"])
@pytest.mark.parametrize("rows,dim,n", [
    (10_000, 4, 256),                # one lane per row: no butterfly
    (10_000, 32, 256),               # a partial group (8 lanes)
    (5_000, 96, 1024),               # 32 lanes, 24 chunks: idle lanes
    (5_000, 128, 2048),              # a full group
    (2_000, 256, 1024),              # two chunks per lane
])
def test_sparse_update_is_bit_exact_and_lazy(dev, rows, dim, n, kind):
    rng = np.random.default_rng(rows + n + dim)
    state = _state(rows, dim, rng)
    ids = _ids(kind, rows, n, rng)
    grads = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    got = _device_sparse(dev, state, ids, grads)
    want, uniq = _restated_sparse(state, ids, grads)
    _assert_bits(got, want, "whole arrays")                                 # touched rows AND everything else
    rest = np.setdiff1d(np.arange(rows), uniq)
    assert len(rest)
    _assert_bits([a[rest] for a in got], [a[rest] for a in state], "untouched rows: table and accumulator")
    for g, s in zip(got, state):
        assert (rc.bits(g[uniq]) != rc.bits(s[uniq])).any()                # the touched rows did change
    assert (got[1][uniq] > state[1][uniq]).all()


# ------------------------------------------------------------------------------------------ runs that cross 64-slot blocks
@pytest.mark.parametrize("dim,n,one_row", [(128, 4096, False), (96, 4096, False), (128, 4096, True), (96, 4096, True),
                                           (128, 20000, False)])       # 20000 ids: the rocPRIM plan
def test_runs_that_cross_blocks_are_bit_exact_and_reproducible(dev, dim, n, one_row):
    """20 rows: ~205 slots per id, every run crosses 64-slot boundaries and the second launch does all the work; one_row: a
    single run spans every block."""
    rows = 20
    rng = np.random.default_rng(dim + n + one_row)
    ids = np.full(n, 7, dtype=np.int64) if one_row else _ids("U", rows, n, rng)
    state = _state(rows, dim, rng)
    grads = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    got = _device_sparse(dev, state, ids, grads)
    want, uniq = _restated_sparse(state, ids, grads)
    assert len(uniq) == (1 if one_row else rows)
    _assert_bits(got, want, "long runs")
    again = _device_sparse(dev, state, ids, grads)
    _assert_bits(again, got, "second call from the same state")


@pytest.mark.parametrize("dim,n", [(160, 512), (384, 512), (512, 700)])
def test_rows_of_more_than_two_chunks_per_lane_are_bit_exact_inside_and_across_blocks(dev, dim, n):
    """The kernels' other instantiations: dim 160 (two chunks per lane, the second on 8 lanes only), 384 (three chunks, run by
    the four-chunk instantiation) and 512 (four chunks) - power-law ids over 1000 rows (runs inside a block), then 20 rows
    (every run crosses blocks: the second launch)."""
    for rows in (1000, 20):
        rng = np.random.default_rng(dim + rows)
        state = _state(rows, dim, rng)
        ids = _ids("Z" if rows == 1000 else "U", rows, n, rng)
        grads = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
        got = _device_sparse(dev, state, ids, grads)
        want, uniq = _restated_sparse(state, ids, grads)
        _assert_bits(got, want, f"{rows} rows")
        assert (rc.bits(got[0][uniq]) != rc.bits(state[0][uniq])).any()


def test_rows_wider_than_512_floats_are_refused(dev):
    t, a, g = torch.zeros(10, 516, device=dev), torch.full((10,), 0.1, device=dev), torch.ones(4, 516, device=dev)
    plan = ops.SparsePlan(4, dev).run(torch.arange(4, device=dev), 10)
    with pytest.raises(NotImplementedError, match="516"):
        ops.rowwise_adagrad_step_([(t, a, g, plan)], [], LR, EPS)
    assert not t.any().item() and (a == 0.1).all().item()


# ------------------------------------------------------------------------------------------ skipped ids
def test_out_of_range_and_padding_ids_are_skipped(dev):
    rows, dim, n = 500, 64, 2048
    rng = np.random.default_rng(3)
    ids = _ids("Z", rows, n, rng)
    ids[rng.random(n) < 0.2] = -1
    ids[rng.random(n) < 0.1] = rows
    ids[rng.random(n) < 0.1] = rows + 12345
    ids[:3] = [-1, rows, 0]
    ok = (ids >= 0) & (ids < rows)
    assert 0 < ok.sum() < n
    state = _state(rows, dim, rng)
    grads = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    got = _device_sparse(dev, state, ids, grads)
    want, uniq = _restated_sparse(state, ids[ok], grads[ok])               # the restatement on the valid pairs only
    _assert_bits(got, want, "valid pairs only")
    rest = np.setdiff1d(np.arange(rows), uniq)
    _assert_bits([a[rest] for a in got], [a[rest] for a in state], "rows of no valid id")
    nothing = np.where(rng.random(n) < 0.5, -1, rows + rng.integers(0, 1000, n)).astype(np.int64)
    _assert_bits(_device_sparse(dev, state, nothing, grads), state, "a batch of skipped ids only")


def test_ops_refuses_a_wrong_accumulator_and_mismatched_dims(dev):
    t, g = torch.zeros(10, 32, device=dev), torch.zeros(4, 32, device=dev)
    plan = ops.SparsePlan(4, dev)
    with pytest.raises(RuntimeError, match="row_accum"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10, 32, device=dev), g, plan)], [], LR, EPS)       # [rows, dim]: Adagrad's
    with pytest.raises(RuntimeError, match="row_accum"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(9, device=dev), g, plan)], [], LR, EPS)
    with pytest.raises(RuntimeError, match="row_accum"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10, device=dev, dtype=torch.float64), g, plan)], [], LR, EPS)
    with pytest.raises(RuntimeError, match="same dim"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10, device=dev), g, plan),
                                   (torch.zeros(10, 64, device=dev), torch.zeros(10, device=dev), torch.zeros(4, 64, device=dev), plan)],
                                  [], LR, EPS)
    with pytest.raises(RuntimeError, match="same dim"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10, device=dev), torch.zeros(5, 32, device=dev), plan)], [], LR, EPS)
    assert not t.any().item()


# ------------------------------------------------------------------------------------------ dense segments riding in the call
def _dense_problem(dev, count, n_slabs, rng, offset=0, stride_pad=0):
    """Device buffers of one segment: parameter / accumulator at ``offset`` floats into their allocations (1: not 16-byte
    aligned)."""
    stride = count + stride_pad
    host = dict(w=rng.uniform(-0.3, 0.3, count).astype(np.float32), acc=rng.uniform(0.1, 0.2, count).astype(np.float32),
                slabs=(rng.standard_normal((n_slabs, stride)) * 0.01).astype(np.float32))
    dev_t = {}
    for k in ("w", "acc"):
        buf = torch.zeros(count + offset + 8, device=dev)
        buf[offset:offset + count] = T(host[k], dev)
        dev_t[k] = buf[offset:offset + count]
    dev_t["slabs"] = T(host["slabs"], dev)
    return host, dev_t, stride


def _segs(probs, n_slabs, l2s):
    return [ops.make_dense_seg(d["w"], d["acc"], d["slabs"], n_slabs, l2, slab_stride=stride) for (_, d, stride), l2 in zip(probs, l2s)]


@pytest.mark.parametrize("n_slabs", [1, 5, 32])
@pytest.mark.parametrize("l2", [0.0, 1e-6])
def test_dense_segments_equal_the_adagrad_path_bit_for_bit(dev, n_slabs, l2):
    """Segments: a [128, 256] kernel, its bias, 7 elements (the scalar path) and a 4k-element segment whose pointers are offset
    by one float (unaligned: the scalar path) - all in ONE call without tables (n_tables = 0) - against tt_dense_update_f32
    (Adagrad) on the same inputs and against the restatement."""
    def fresh():
        rng = np.random.default_rng(100 * n_slabs + int(l2 > 0))
        return [_dense_problem(dev, 128 * 256, n_slabs, rng), _dense_problem(dev, 256, n_slabs, rng, stride_pad=8),
                _dense_problem(dev, 7, n_slabs, rng), _dense_problem(dev, 4 * 1024, n_slabs, rng, offset=1, stride_pad=4)]
    probs, twin = fresh(), fresh()
    assert probs[3][1]["w"].data_ptr() % 16 == 4
    ops.rowwise_adagrad_step_([], _segs(probs, n_slabs, [l2] * 4), LR, EPS)
    ops.dense_update_(_segs(twin, n_slabs, [l2] * 4), "adagrad", LR, EPS)
    for i, ((h, d, stride), (_, e, _)) in enumerate(zip(probs, twin)):
        count = len(h["w"])
        got = [d[k].cpu().numpy() for k in ("w", "acc")]
        _assert_bits(got, [e[k].cpu().numpy() for k in ("w", "acc")], f"segment {i} against tt_dense_update_f32", ("w", "acc"))
        w, acc = h["w"].copy(), h["acc"].copy()
        rc.dense_adagrad(w, acc, h["slabs"][:, :count], l2, LR, EPS)
        _assert_bits(got, [w, acc], f"segment {i} restated", ("w", "acc"))
        assert (rc.bits(w) != rc.bits(h["w"])).any()


# ------------------------------------------------------------------------------------------ one call for everything
def test_three_tables_and_four_segments_in_one_call_equal_the_separate_calls(dev):
    dim, n = 64, 2048
    rng = np.random.default_rng(21)
    rows = (3000, 100, 30)
    states = [_state(r, dim, rng) for r in rows]
    idss = [_ids(k, r, n, rng) for k, r in zip("UZZ", rows)]
    gradss = [(rng.standard_normal((n, dim)) * 0.01).astype(np.float32) for _ in rows]
    counts, n_slabs, l2s = (64 * 128, 128, 128 * 64, 64), 4, (1e-6, 0.0, 1e-6, 0.0)

    def fresh_segs():
        r = np.random.default_rng(22)
        return [_dense_problem(dev, c, n_slabs, r) for c in counts]
    # everything in ONE call
    dts = [[T(a, dev) for a in st] for st in states]
    plans = [ops.SparsePlan(n, dev) for _ in rows]
    ops.sparse_plan_batched(plans, [T(i, dev) for i in idss], rows)
    all_probs = fresh_segs()
    ops.rowwise_adagrad_step_([(d[0], d[1], T(g, dev), p) for d, g, p in zip(dts, gradss, plans)], _segs(all_probs, n_slabs, l2s), LR, EPS)
    # ... against single-table (n_segs = 0) and dense-only (n_tables = 0) calls, and the restatement
    for t in range(3):
        single = _device_sparse(dev, states[t], idss[t], gradss[t])
        _assert_bits([x.cpu().numpy() for x in dts[t]], single, f"table {t}")
        _assert_bits(single, _restated_sparse(states[t], idss[t], gradss[t])[0], f"table {t} restated")
    only = fresh_segs()
    ops.rowwise_adagrad_step_([], _segs(only, n_slabs, l2s), LR, EPS)
    for i, ((_, a, _), (_, b, _)) in enumerate(zip(all_probs, only)):
        _assert_bits([a[k].cpu().numpy() for k in ("w", "acc")], [b[k].cpu().numpy() for k in ("w", "acc")], f"segment {i}", ("w", "acc"))
    h, d, _ = only[0]
    w, acc = h["w"].copy(), h["acc"].copy()
    rc.dense_adagrad(w, acc, h["slabs"], 1e-6, LR, EPS)
    _assert_bits([d[k].cpu().numpy() for k in ("w", "acc")], [w, acc], "segment 0 restated", ("w", "acc"))


# ------------------------------------------------------------------------------------------ trainer
def _cfg(n_users, n_items, dim, tower_dims, batch, opt="rowwise_adagrad", dropout=0.0, cats=0, lr=LR, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=lr, optimizer=opt, batch_size=batch, dropout_rate=dropout,
                          n_category_buckets=cats, **kw)


def _table_names(tr):
    return ["user", "item"] + (["cat"] if tr.cat_table is not None else [])


def _snapshot(tr):
    names = ["dense_flat", "dense_accum"]
    for p in _table_names(tr):
        names += [f"{p}_table", f"{p}_row_accum"]
    return {k: getattr(tr, k).cpu().numpy().copy() for k in names}


def _half_step(tr, seed, step, cats):
    """The sort plans and ``forward_backward`` of one synthetic batch; returns the ids per table (NumPy)."""
    du, di = tr.synthetic_batch(seed, step)
    plans, ids, rows, kw = [tr.user_plan, tr.item_plan], [du, di], [tr.cfg.n_users, tr.cfg.n_items], {}
    if cats:
        dc = tr.synthetic_categories(seed, step)
        plans.append(tr.cat_plan); ids.append(dc); rows.append(cats)
        kw["category_ids"] = dc
    ops.sparse_plan_batched(plans, ids, rows)
    tr.forward_backward(du, di, **kw)
    return [i.cpu().numpy() for i in ids]


@pytest.mark.parametrize("cats", [0, 30])
def test_trainer_update_matches_the_restatement_and_the_dense_state_an_adagrad_trainer(dev, cats):
    shape, seed = (3000, 2000, 64, [128, 64], 256), 1001
    tr = TwoTowerTrainer(_cfg(*shape, cats=cats), dev, seed=seed)
    twin = TwoTowerTrainer(_cfg(*shape, opt="adagrad", cats=cats), dev, seed=seed)
    assert tr.user_accum is None and tr.item_accum is None and tr.user_row_accum.shape == (3000,)
    assert (tr.user_row_accum == 0.1).all().item() and (tr.dense_accum == 0.1).all().item()
    assert torch.equal(tr.dense_flat, twin.dense_flat) and torch.equal(tr.user_table, twin.user_table)
    for step in range(3):
        ids = _half_step(tr, seed, step, cats)
        snap = _snapshot(tr)
        due, die = tr.user_tower.demb.cpu().numpy().copy(), tr.item_tower.demb.cpu().numpy().copy()
        if step == 0:                    # the gradients of step 1 are those of the Adagrad trainer: nothing in front of the optimizer differs
            _half_step(twin, seed, step, cats)
            assert torch.equal(tr.user_tower.demb, twin.user_tower.demb) and torch.equal(tr.item_tower.demb, twin.item_tower.demb)
            for a, b in zip((tr.user_tower, tr.item_tower), (twin.user_tower, twin.item_tower)):
                for l in range(a.n_layers):
                    assert torch.equal(a.dw_slabs[l], b.dw_slabs[l]) and torch.equal(a.db_slabs[l], b.db_slabs[l])
        tr.apply_gradients()
        tr.check_ids()
        after = _snapshot(tr)
        for p, i, g in zip(_table_names(tr), ids, (due, die, die)):
            rc.sparse_rowwise_adagrad(snap[f"{p}_table"], snap[f"{p}_row_accum"], i, g, LR, EPS)
            for k in (f"{p}_table", f"{p}_row_accum"):
                bad = rc.bits(after[k]) != rc.bits(snap[k])
                assert not bad.any(), (step, k, int(bad.sum()))
        assert (rc.bits(after["dense_flat"]) != rc.bits(snap["dense_flat"])).any()
        if step == 0:
            twin.apply_gradients()
            assert torch.equal(tr.dense_flat, twin.dense_flat) and torch.equal(tr.dense_accum, twin.dense_accum)
            assert not torch.equal(tr.user_table, twin.user_table)          # another optimizer on the tables


def test_trainer_trains_on_a_repeated_batch(dev):
    seed = 5
    tr = TwoTowerTrainer(_cfg(3000, 2000, 64, [128, 64], 256, lr=0.05), dev, seed=seed)
    batch = tr.synthetic_batch(seed, 0)
    losses = [tr.step(*batch).item() for _ in range(30)]
    tr.check_ids()
    print(f"rowwise_adagrad: loss {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------ every feature of the trainer
FEATURES = dict(n_category_buckets=7, n_title_buckets=50, title_max_tokens=3, n_user_features=3, n_item_features=3, user_history_len=4,
                rating_weight=0.5, rating_hidden=32, cross_layers=1, layer_norm=True)
VARIANTS = {"mean": dict(FEATURES), "attention": dict(FEATURES, history_pooling="attention"),
            "mixed": dict(FEATURES, n_category_buckets=0, user_history_len=0, candidate_sampling="mixed", n_sampled_negatives=32),
            "clipped-with-a-schedule": dict(FEATURES, global_clipnorm=0.25, lr_warmup_steps=2)}


def _featured_trainer(dev, opt, seed, **kw):
    cfg = TwoTowerConfig(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], temperature=0.5, l2_regularization=1e-6,
                         learning_rate=LR, optimizer=opt, batch_size=64, **kw)
    tr = TwoTowerTrainer(cfg, dev, seed=seed)
    tr.set_user_features(tr.synthetic_user_features(seed))
    tr.set_item_features(tr.synthetic_item_features(seed))
    tr.set_item_titles(tr.synthetic_item_titles(seed))
    if tr.user_history is not None:
        pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(4)]
        u, i = (torch.cat([p[k] for p in pairs]).cpu().numpy() for k in (0, 1))
        tr.set_user_histories(T(data.user_histories(u, i, cfg.n_users, cfg.user_history_len), dev))
    return tr


def _featured_step(tr, seed, step):
    u, i = tr.synthetic_batch(seed, step, "Z")
    kw = {}
    if tr.cat_table is not None:
        kw["category_ids"] = tr.synthetic_categories(seed, step)
    rng = np.random.default_rng(1000 * seed + step)
    kw["ratings"] = T(rng.integers(1, 6, 64).astype(np.float32), tr.dev)
    return tr.step(u, i, **kw).item()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_feature_trains_its_tables_row_wise_and_its_dense_parameters_as_adagrad_does(dev, variant):
    """Category, title and history tables, numeric features, rating head, cross layer, layer normalisation (and mixed negative
    sampling, the attention pool, clipping with a warm-up): after the first step from one seed every dense parameter and its
    accumulator - projections, head, cross kernels, gammas, attention vector - equal the Adagrad trainer's bit for bit (the
    gradients are the same and the dense segments take the same update); every table moved and keeps one accumulator per row."""
    seed = 31
    tr, twin = (_featured_trainer(dev, opt, seed, **VARIANTS[variant]) for opt in ("rowwise_adagrad", "adagrad"))
    before = {p: t.table.clone() for p, t in tr.tables.items()}
    losses = [_featured_step(tr, seed, 0)]
    assert _featured_step(twin, seed, 0) == losses[0]
    assert torch.equal(tr.dense_flat, twin.dense_flat) and torch.equal(tr.dense_accum, twin.dense_accum)
    assert (tr.dense_accum > 0.1).any().item()
    for p, t in tr.tables.items():
        assert t.accum is None and t.row_accum.shape == (t.table.shape[0],), p
        assert (t.table != before[p]).any().item() and (t.row_accum > 0.1).any().item() and (t.row_accum >= 0.1).all().item(), p
        assert not torch.equal(t.table, twin.tables[p].table), p
    losses += [_featured_step(tr, seed, s) for s in (1, 2)]
    tr.check_ids()
    assert np.isfinite(losses).all()
    for t in tr.tables.values():
        assert torch.isfinite(t.table).all().item() and torch.isfinite(t.row_accum).all().item() and (t.row_accum >= 0.1).all().item()


# ------------------------------------------------------------------------------------------ checkpoint
def test_checkpoint_carries_the_row_accumulators(dev):
    seed = 17

    def fresh(opt="rowwise_adagrad"):
        return TwoTowerTrainer(_cfg(800, 700, 32, [64, 32], 256, opt, dropout=0.1, cats=30), dev, seed=seed)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s), category_ids=tr.synthetic_categories(seed, s))
    a = fresh()
    run(a, range(4))
    b = fresh()
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["step_index"] == 2 and "user_accum" not in sd and "user_m" not in sd
    for k, rows in (("user_row_accum", 800), ("item_row_accum", 700), ("cat_row_accum", 30)):
        assert sd[k].shape == (rows,) and (sd[k] > 0.1).any().item() and (sd[k] >= 0.1).all().item(), k
    assert (sd["dense_accum"] > 0.1).any().item()
    c = fresh()
    c.load_state_dict(sd)
    run(c, range(2, 4))
    for k in _snapshot(a):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert torch.equal(a.loss, c.loss)
    with pytest.raises(ValueError, match="optimizer"):
        fresh("adagrad").load_state_dict(sd)
    with pytest.raises(ValueError, match="optimizer"):
        fresh().load_state_dict(fresh("adagrad").state_dict())
    fresh_again = fresh()
    fresh_again.load_state_dict(sd)
    fresh_again.init_synthetic(seed)                                        # resets the row accumulators too
    assert (fresh_again.user_row_accum == 0.1).all().item() and (fresh_again.cat_row_accum == 0.1).all().item()


# ------------------------------------------------------------------------------------------ refusals, the custom op, the CLI
def test_graph_capture_is_refused(dev):
    tr = TwoTowerTrainer(_cfg(300, 200, 32, [64, 32], 256), dev, seed=1)
    with pytest.raises(NotImplementedError, match="rowwise_adagrad"):
        tr.capture_graph()


def test_custom_op_passes_opcheck_and_equals_the_ops_call(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rows, dim, n = 500, 64, 300
    rng = np.random.default_rng(31)
    state = _state(rows, dim, rng)
    ids = _ids("Z", rows, n, rng)
    grads = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    d = [T(a, dev) for a in state]
    torch.library.opcheck(torch.ops.twotower.sparse_rowwise_adagrad_, (d[0].clone(), d[1].clone(), T(grads, dev), T(ids, dev), LR, EPS))
    torch.ops.twotower.sparse_rowwise_adagrad_(d[0], d[1], T(grads, dev), T(ids, dev), LR, EPS)
    _assert_bits([t.cpu().numpy() for t in d], _device_sparse(dev, state, ids, grads), "op against ops.rowwise_adagrad_step_")
    cpu = [torch.from_numpy(a.copy()) for a in state]
    with pytest.raises((NotImplementedError, RuntimeError)):                # no CPU kernel, no fallback
        torch.ops.twotower.sparse_rowwise_adagrad_(cpu[0], cpu[1], torch.from_numpy(grads), torch.from_numpy(ids), LR, EPS)
    assert np.array_equal(cpu[0].numpy(), state[0]) and np.array_equal(cpu[1].numpy(), state[1])


def test_train_cli_runs_saves_resumes_and_composes_with_clipping_and_a_schedule(dev, tmp_path):
    from two_tower_amazon_recommender_amd import train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  dropout_rate: 0.1\n  l2_regularization: 1e-6\n  training:\n    batch_size: 256\n    learning_rate: 0.01\n"
                    "    epochs: 1\n  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck, ck2, ck3 = tmp_path / "rw.pt", tmp_path / "rw2.pt", tmp_path / "rw3.pt"
    common = ["--config", str(cfgp), "--synthetic", "5000", "--synthetic-users", "600", "--synthetic-items", "500", "--seed", "42",
              "--optimizer", "rowwise_adagrad"]
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(common + ["--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    steps = 5000 * 9 // 10 // 256
    assert sd["config"]["optimizer"] == "rowwise_adagrad" and sd["step_index"] == steps and sd["epoch"] == 1
    assert "user_accum" not in sd and sd["user_row_accum"].shape == (600,) and sd["item_row_accum"].shape == (500,)
    for k in ("user_row_accum", "item_row_accum", "dense_accum"):
        assert (sd[k] > 0.1).any().item() and torch.isfinite(sd[k]).all().item(), k
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(common + ["--epochs", "2", "--resume", str(ck), "--save", str(ck2)]) == 0
    sd2 = torch.load(ck2, weights_only=True)
    assert sd2["step_index"] == 2 * steps and sd2["epoch"] == 2
    assert (sd2["user_row_accum"] >= sd["user_row_accum"]).all().item() and (sd2["user_row_accum"] > sd["user_row_accum"]).any().item()
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(common + ["--global-clipnorm", "0.5", "--lr-decay", "cosine", "--lr-decay-steps", "auto", "--lr-warmup-steps", "3",
                                   "--save", str(ck3)]) == 0
    sd3 = torch.load(ck3, weights_only=True)
    assert sd3["step_index"] == steps and torch.isfinite(sd3["user_table"]).all().item()
    assert not torch.equal(sd3["user_table"], sd["user_table"])             # the clip and the schedule did act

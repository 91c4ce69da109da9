"""The pairwise retrieval losses (csrc/pairwise.hip) on the device against the f64 restatement of tests/pairwise_check.py:
the two C entries, run-to-run bits, the custom ops and tasks.Retrieval(loss=...), the trainer, its refusals and the CLI."""
import functools

import numpy as np
import pytest
import torch

import pairwise_check as pc
from two_tower_amazon_recommender_amd import ops

pytestmark = pytest.mark.gpu

INV_T = 10.0
# (nq, nc, dim, diag_offset): ragged tiles both ways, nc > nq with an offset, every dim, one tile, a split boundary, no negatives
SHAPES = [(33, 33, 32, 0), (100, 131, 128, 31), (257, 300, 256, 0), (64, 64, 64, 0), (96, 160, 64, 64), (130, 515, 128, 7),
          (300, 557, 256, 257), (1, 1, 32, 0), (32, 64, 32, 32)]
OPTIONS = ["none", "weight", "prob", "ids", "hard1", "hard5", "all", "scale2"]
KINDS = ["logistic", "hinge"]
REDUCTIONS = ["mean", "sum"]


def _inputs(shape, seed):
    nq, nc, d, off = shape
    rng = np.random.default_rng(seed)
    q = (rng.uniform(-1, 1, (nq, d)) / np.sqrt(d)).astype(np.float32)
    c = (rng.uniform(-1, 1, (nc, d)) / np.sqrt(d)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, nq).astype(np.float32)
    w[rng.random(nq) < 0.15] = 0.0                       # exact zeros
    p = rng.uniform(1e-4, 0.2, nc).astype(np.float32)
    ids = np.arange(nc, dtype=np.int64) + 1000
    dup = rng.random(nc) < 0.10                          # ~10 % duplicated ids, duplicates of positives among them
    ids[dup] = ids[rng.integers(0, nc, int(dup.sum()))]
    if nq > 2:
        ids[(off + 1) % nc] = ids[off]                   # a duplicate of query 0's positive, for certain
    return q, c, w, p, ids


def _thresholds(dev, q, c, k, p, ids, off):
    tq, tc = torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev)
    ws = torch.empty(ops.retrieval_workspace_bytes(q.shape[0], c.shape[0], q.shape[1]), dtype=torch.uint8, device=dev)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    return ops.retrieval_hard_negative_thresholds(tq, tc, INV_T, k, ws, cand_prob=t(p), cand_ids=t(ids), diag_offset=off).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs of a shape whose hard-negative thresholds (k = 1, 5; alone and with every option) keep 2e-5 clear of every logit
    in the f64 reference - a condition on the inputs: the first seed that meets it.  Returns the inputs and, per option, the
    keyword arguments of the restatement with the hinge margin pick_margin gives for that option's pairs."""
    dev = torch.device("cuda:0")
    off = shape[3]
    for seed in range(20):
        q, c, w, p, ids = _inputs(shape, 1000 * shape[0] + seed)
        thr = {"hard1": _thresholds(dev, q, c, 1, None, None, off), "hard5": _thresholds(dev, q, c, 5, None, None, off),
               "all": _thresholds(dev, q, c, 5, p, ids, off)}
        gaps = []
        for name, t in thr.items():
            s, _, cand, _ = pc.pairs(q, c, INV_T, p if name == "all" else None, ids if name == "all" else None, None, off)
            gaps.append(pc.thr_gap(s, pc.thr_natural(t), cand))
        if min(gaps) >= pc.GAP:
            break
    else:
        raise AssertionError(f"{shape}: no seed keeps the hard-negative thresholds 2e-5 clear of the logits")
    opts = {"none": {}, "weight": dict(w=w), "prob": dict(p=p), "ids": dict(ids=ids), "hard1": dict(thr=thr["hard1"]),
            "hard5": dict(thr=thr["hard5"]), "all": dict(w=w, p=p, ids=ids, thr=thr["all"]), "scale2": {}}
    ref = {}
    for name, kw in opts.items():
        rkw = dict(inv_t=INV_T, off=off, w=kw.get("w"), p=kw.get("p"), ids=kw.get("ids"), thr=pc.thr_natural(kw.get("thr")))
        _, _, valid, x = pc.pairs(q, c, INV_T, rkw["p"], rkw["ids"], rkw["thr"], off)
        ref[name] = (rkw, pc.pick_margin(x, valid))
    return q, c, opts, ref


def _run(dev, q, c, off, kind, margin, reduction, kw, grad=True, grad_scale=1.0):
    """One call of the entry with NaN guard rows behind every output; returns (loss, per_row, dq, dc) as NumPy."""
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tq, tc = t(q), t(c)
    ws = torch.empty(ops.retrieval_pairwise_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    per_row, loss, dq, dc = nan(nq + 1), nan(2), nan(nq + 1, d), nan(nc + 1, d)
    args = dict(kind=kind, margin=margin, reduction=reduction, sample_weight=t(kw.get("w")), cand_prob=t(kw.get("p")),
                cand_ids=t(kw.get("ids")), diag_offset=off, hard_thr=t(kw.get("thr")))
    if grad:
        ops.retrieval_pairwise_fwd_bwd(tq, tc, INV_T, ws, per_row[:nq], loss[:1], dq[:nq], dc[:nc], grad_scale=grad_scale, **args)
    else:
        ops.retrieval_pairwise_fwd(tq, tc, INV_T, ws, per_row[:nq], loss[:1], **args)
    torch.cuda.synchronize()
    assert torch.isnan(per_row[nq]) and torch.isnan(loss[1]) and torch.isnan(dq[nq]).all() and torch.isnan(dc[nc]).all(), "guard"
    if not grad:
        assert torch.isnan(dq).all() and torch.isnan(dc).all()
    return float(loss[0]), per_row[:nq].cpu().numpy(), dq[:nq].cpu().numpy(), dc[:nc].cpu().numpy()


def _check_loss(got, got_rows, want, want_rows, nq, what):
    d = abs(got - want)
    print(f"{what}: loss {got!r} ref {want!r} |d| {d:.3e}; per_row max|d| {np.abs(got_rows - want_rows).max():.3e}")
    assert d <= 1e-4 * abs(want) and d / nq <= 1e-4, (what, got, want)
    assert np.abs(got_rows - want_rows).max() <= 1e-4 * max(1.0, np.abs(want_rows).max()), what


def _check_grad(got, want, what):
    err, bar = np.abs(got - want).max(), 1e-4 * np.abs(want).max() + 1e-6
    print(f"{what}: max|d| {err:.3e} bar {bar:.3e}")
    assert err <= bar, (what, err, bar)


# ------------------------------------------------------------------------------------------------- 1. kernel parity
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entries_match_the_f64_restatement(dev, shape, kind):
    nq, nc, d, off = shape
    q, c, opts, ref = _case(shape)
    for name in OPTIONS:
        kw, (rkw, margin) = opts[name], ref[name]
        gs = 2.0 if name == "scale2" else 1.0
        for reduction in REDUCTIONS:
            what = f"{shape} {kind} {reduction} {name}"
            rl, rrows, _ = pc.loss(q, c, kind, margin, reduction, **rkw)
            rdq, rdc = pc.grads(q, c, kind, margin, reduction, grad_scale=gs, **rkw)
            loss, rows, dq, dc = _run(dev, q, c, off, kind, margin, reduction, kw, grad=True, grad_scale=gs)
            _check_loss(loss, rows, rl, rrows, nq, what + " fwd_bwd")
            _check_grad(dq, rdq, what + " dq")
            _check_grad(dc, rdc, what + " dc")
            loss_f, rows_f, _, _ = _run(dev, q, c, off, kind, margin, reduction, kw, grad=False)
            _check_loss(loss_f, rows_f, rl, rrows, nq, what + " fwd")
            assert loss_f == loss and np.array_equal(rows_f, rows), what + ": the forward entry's bits differ from the training entry's"


def test_a_row_without_negatives_has_no_loss_and_no_gradient(dev):
    q, c, _, _ = _case((1, 1, 32, 0))
    for kind in KINDS:
        loss, rows, dq, dc = _run(dev, q, c, 0, kind, 0.5, "mean", {})
        assert loss == 0.0 and rows[0] == 0.0 and not dq.any() and not dc.any()
    # every negative an accidental hit: the same
    q, c, _, _ = _case((33, 33, 32, 0))
    ids = np.zeros(33, dtype=np.int64)
    loss, rows, dq, dc = _run(dev, q, c, 0, "logistic", 0.5, "mean", dict(ids=ids))
    assert loss == 0.0 and not rows.any() and not dq.any() and not dc.any()


def test_workspace_is_no_larger_than_the_scorers(dev):
    for shape in SHAPES + [(8192, 8192, 64, 0), (8192, 8192, 128, 0), (8192, 8192, 256, 0), (4096, 12288, 128, 0)]:
        nq, nc, d, _ = shape
        assert 0 < ops.retrieval_pairwise_workspace_bytes(nq, nc, d) <= ops.retrieval_workspace_bytes(nq, nc, d), shape


# ------------------------------------------------------------------------------------------------- 2. run-to-run bits
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits_and_grad_scale_scales(dev, kind):
    shape = (130, 515, 128, 7)
    q, c, opts, ref = _case(shape)
    kw, (_, margin) = opts["all"], ref["all"]
    a = _run(dev, q, c, 7, kind, margin, "mean", kw)
    b = _run(dev, q, c, 7, kind, margin, "mean", kw)
    assert a[0] == b[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1:], b[1:]))
    s2 = _run(dev, q, c, 7, kind, margin, "mean", kw, grad_scale=2.0)
    assert s2[0] == a[0] and np.array_equal(s2[1], a[1])
    assert np.allclose(s2[2], 2 * a[2], rtol=1e-6, atol=1e-9) and np.allclose(s2[3], 2 * a[3], rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------- 3. custom op and task
def _task_loss(kind, margin, reduction="mean"):
    from two_tower_amazon_recommender_amd import tasks
    return tasks.PairwiseLogisticLoss(reduction=reduction) if kind == "logistic" else tasks.PairwiseHingeLoss(margin, reduction=reduction)


@pytest.mark.parametrize("kind", KINDS)
def test_retrieval_task_autograd_and_value_paths(dev, kind):
    from two_tower_amazon_recommender_amd import tasks
    shape = (100, 131, 128, 31)
    q, c, opts, ref = _case(shape)
    kw, (rkw, margin) = opts["all"], ref["all"]
    rkw = dict(rkw, thr=None)
    _, _, valid, x = pc.pairs(q, c, INV_T, rkw["p"], rkw["ids"], None, 31)
    margin = pc.pick_margin(x, valid)
    t = lambda a: torch.from_numpy(a).to(dev)
    tq, tc = t(q).requires_grad_(True), t(c).requires_grad_(True)
    task = tasks.Retrieval(loss=_task_loss(kind, margin), temperature=1.0 / INV_T, remove_accidental_hits=True)
    call = lambda a, b: task(a, b, sample_weight=t(kw["w"]), candidate_sampling_probability=t(kw["p"]), candidate_ids=t(kw["ids"]),
                             diag_offset=31)
    loss = call(tq, tc)
    (3.0 * loss).backward()
    rl, rrows, _ = pc.loss(q, c, kind, margin, "mean", **rkw)
    rdq, rdc = pc.grads(q, c, kind, margin, "mean", grad_scale=3.0, **rkw)
    _check_loss(float(loss.detach()), task.last_per_example_loss.cpu().numpy(), rl, rrows, 100, f"task {kind}")
    _check_grad(tq.grad.cpu().numpy(), rdq, f"task {kind} q.grad")
    _check_grad(tc.grad.cpu().numpy(), rdc, f"task {kind} c.grad")
    with torch.no_grad():
        assert float(call(tq, tc)) == float(loss.detach())
    # the custom op itself, sum reduction
    out = torch.ops.twotower.retrieval_pairwise_loss(t(q), t(c), None, None, None, INV_T, 31, 0, kind, 0.5 if kind == "logistic"
                                                     else ref["none"][1], "sum")
    rl, _, _ = pc.loss(q, c, kind, ref["none"][1], "sum", inv_t=INV_T, off=31)
    assert abs(float(out[0]) - rl) <= 1e-4 * abs(rl)


def test_retrieval_task_num_hard_negatives_and_batch_metrics(dev):
    from two_tower_amazon_recommender_amd import tasks
    from two_tower_amazon_recommender_amd.metrics import TopKCategoricalAccuracy
    shape = (130, 515, 128, 7)
    q, c, opts, ref = _case(shape)
    t = lambda a: torch.from_numpy(a).to(dev)
    rkw, margin = ref["hard5"]
    tq, tc = t(q).requires_grad_(True), t(c).requires_grad_(True)
    loss = tasks.Retrieval(loss=tasks.PairwiseHingeLoss(margin), temperature=1.0 / INV_T, num_hard_negatives=5)(tq, tc, diag_offset=7)
    loss.backward()
    rl, _, n = pc.loss(q, c, "hinge", margin, "mean", **rkw)
    assert (n == 5).all()
    rdq, rdc = pc.grads(q, c, "hinge", margin, "mean", **rkw)
    assert abs(float(loss.detach()) - rl) <= 1e-4 * abs(rl)
    _check_grad(tq.grad.cpu().numpy(), rdq, "hard negatives q.grad")
    _check_grad(tc.grad.cpu().numpy(), rdc, "hard negatives c.grad")
    accs = []
    for lo in (tasks.BPRLoss(), None):
        m = TopKCategoricalAccuracy(3)
        tasks.Retrieval(loss=lo, temperature=1.0 / INV_T, batch_metrics=[m])(t(q), t(c), diag_offset=7)
        accs.append(float(m.result()))
    assert accs[0] == accs[1]
    with pytest.raises(NotImplementedError):
        tasks.Retrieval(loss=tasks.BPRLoss(), batch_metrics=[TopKCategoricalAccuracy(3)], num_hard_negatives=5)


# ------------------------------------------------------------------------------------------------- 4. trainer
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer  # noqa: E402

LR, LR_SGD, W_RATING, HID = 0.001, 0.0001, 0.5, 64
MARGIN = 0.5            # pick_margin's first candidate: every step asserts that the f64 pairs keep 2e-5 clear of it


def _cfg(opt, loss_kind, batch=256, **kw):
    return TwoTowerConfig(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], temperature=0.1, l2_regularization=1e-6,
                          learning_rate=LR_SGD if opt == "sgd" else LR, optimizer=opt, batch_size=batch, retrieval_loss=loss_kind,
                          pairwise_margin=MARGIN, **kw)


def _cut64(tr, t):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    return flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))


def _reference_step(tr, u, i, before, towers, ratings=None, head=None, cand=None, sample_weight=None):
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
    cfg = tr.cfg
    r = pc.step_f64(before["user_table"], before["item_table"], towers, u.cpu().numpy(), i.cpu().numpy(),
                    "logistic" if cfg.retrieval_loss == "bpr" else "hinge", cfg.pairwise_margin, cfg.pairwise_reduction, cfg.temperature,
                    masks, normalize_eps=cfg.normalize_eps if cfg.normalize_embeddings else None, sample_weight=sample_weight,
                    cand_ids=cand, head=head, ratings=None if ratings is None else ratings.cpu().numpy(),
                    rating_weight=cfg.rating_weight, head_mask=(tr._r_h > 0).cpu().numpy() if head is not None else None)
    if cfg.retrieval_loss == "hinge":         # the condition on the inputs: no pair within 2e-5 of the kink
        assert pc.pick_margin(r["x"], r["valid"]) == cfg.pairwise_margin
    return r


def _check_step(tr, r, loss, step, batch):
    """The bars of tests/test_gpu_features.py::_check_step: loss within 1e-4 relative and 1e-4 per pair, every gradient within 1e-4
    of its max |g|; the item tower's last bias gradient is zero (every row's logit gradients sum to zero) and is treated as there."""
    print(f"step {step}: loss {loss} (f64 {r['loss']})")
    assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    checks = [("due", n64(tr.user_tower.demb), r["due"]), ("die", n64(tr.item_tower.demb), r["die"])]
    if tr.rating_on:
        d, hd = tr.cfg.tower_dims[-1], tr.cfg.rating_hidden
        ks, bs = n64(tr._r_kslabs).sum(0), n64(tr._r_bslabs).sum(0)
        dw1, db1, dw2, db2 = r["dhead"]
        checks += [("dW1", ks[:2 * d * hd].reshape(2 * d, hd), dw1), ("dw2", ks[2 * d * hd:], dw2.reshape(-1)), ("db1", bs[:hd], db1),
                   ("db2", bs[hd:], db2.reshape(-1))]
        lr = tr.rating_loss.item()
        assert abs(lr - r["rating_loss"]) <= 1e-4 * abs(r["rating_loss"]) and abs(lr - r["rating_loss"]) <= 1e-4, (lr, r["rating_loss"])
    for t, tw in enumerate((tr.user_tower, tr.item_tower)):
        for l in range(tw.n_layers):
            checks += [(f"dw[{t}][{l}]", n64(tw.dw_slabs[l]).sum(0), r["dw"][t][l]), (f"db[{t}][{l}]", n64(tw.db_slabs[l]).sum(0), r["db"][t][l])]
    last = f"db[1][{tr.item_tower.n_layers - 1}]"
    last_user = f"db[0][{tr.user_tower.n_layers - 1}]"
    for what, got, want in checks:
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        if what == last and not tr.cfg.normalize_embeddings:
            if not tr.rating_on:
                assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
            scale = max(scale, np.abs(r["dc"]).max()) if tr.rating_on else np.abs(r["dc"]).max()
        if what == last_user and not tr.cfg.normalize_embeddings and scale <= 1e-9 * np.abs(r["dq"]).max():
            # the same cancellation on the user side: a hinge whose pairs are ALL inside the margin has h_ij = r_i for every pair,
            # so the column sums of dq - this bias gradient - are sum_i r_i (sum_{j != i} c_j - n_i c_i) = 0 with n_i = B - 1; the
            # f64 value is rounding noise, and the bar is taken from the scale of the rows the device sums, as for the item side
            scale = np.abs(r["dq"]).max()
        print(f"step {step}: {what} error {err / scale:.2e} of max |g| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (step, what, err, scale)


def _ratings(dev, seed, step, batch=256):
    rng = np.random.default_rng(1000 * seed + step)
    r = rng.integers(1, 6, batch).astype(np.float32)
    r[rng.random(batch) < 0.1] = np.nan
    return torch.from_numpy(r).to(dev)


def _three_steps(dev, opt, loss_kind, seed=1001, **kw):
    batch = 256
    tr = TwoTowerTrainer(_cfg(opt, loss_kind, **kw), dev, seed=seed)
    assert tr.pairwise_ws is not None and tr.pairwise_kind == ("logistic" if loss_kind == "bpr" else "hinge")
    lse0 = tr.lse.clone()
    for step in range(3):
        u, i = tr.synthetic_batch(seed, step, "Z")
        t = _ratings(dev, seed, step) if tr.rating_on else None
        if not tr.mixed:
            ops.sparse_plan_batched([tr.user_plan, tr.item_plan], [u, i], [300, 200])
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
        towers = tuple(([_cut64(tr, w) for w in tw.w], [_cut64(tr, b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))
        head = tuple(_cut64(tr, x) for x in (tr.W1_rating, tr.b1_rating, tr.w2_rating, tr.b2_rating)) if tr.rating_on else None
        loss = tr.forward_backward(u, i, **({"ratings": t} if tr.rating_on else {})).item()
        tr.check_ids()
        cand = tr.cand_ids.cpu().numpy() if tr.mixed else None
        r = _reference_step(tr, u, i, before, towers, ratings=t, head=head, cand=cand)
        _check_step(tr, r, loss, step, batch)
        assert abs(tr.per_row.sum().item() - r["loss"]) <= 1e-4 * abs(r["loss"])
        if tr.cfg.global_clipnorm > 0:
            _check_clip(tr, r)
        tr.apply_gradients(**({"step_ids": [u, i]} if tr.mixed else {}))
    assert torch.equal(tr.lse.view(torch.int32), lse0.view(torch.int32))          # the softmax's lse is not touched
    return tr


def _check_clip(tr, r):
    """The clip launches behind a pairwise step: the norm over the dense gradients and the embedding gradient rows (one per
    occurrence, as Keras counts IndexedSlices.values: tests/clip_check.py), the scale c / max(norm, c), every gradient scaled."""
    sq = sum(float((g ** 2).sum()) for side in r["dw"] + r["db"] for g in side)
    sq += float((r["due"] ** 2).sum()) + float((r["die"] ** 2).sum())
    due = tr.user_tower.demb.clone()
    norm, scale = tr.clip_gradients().tolist()
    c = tr.cfg.global_clipnorm
    print(f"clip: norm {norm!r} (f64 {np.sqrt(sq)!r}) scale {scale!r}")
    assert abs(norm - np.sqrt(sq)) <= 1e-4 * np.sqrt(sq) and scale < 1.0 and abs(scale - c / norm) <= 1e-6
    assert torch.allclose(tr.user_tower.demb, due * scale, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("loss_kind", ["bpr", "hinge"])
def test_trainer_matches_the_f64_restatement_and_trains(dev, loss_kind, opt):
    seed = 1001
    tr = _three_steps(dev, opt, loss_kind, seed)
    u, i = tr.synthetic_batch(seed, 0, "Z")
    losses = [tr.step(u, i).item() for _ in range(30)]
    tr.check_ids()
    print(f"30 steps on one batch: {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    # evaluate: the forward entry on another batch, against the restatement
    u, i = tr.synthetic_batch(seed, 5, "Z")
    before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table")}
    towers = tuple(([_cut64(tr, w) for w in tw.w], [_cut64(tr, b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))
    sw = torch.linspace(0.5, 1.5, 256, device=dev)
    got = tr.evaluate(u, i, sample_weight=sw).item()
    r = _reference_step(tr, u, i, before, towers, sample_weight=sw.cpu().numpy())
    assert abs(got - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(got - r["loss"]) / 256 <= 1e-4, (got, r["loss"])


@pytest.mark.parametrize("variant,loss_kind,opt", [("normalize", "bpr", "adagrad"), ("mixed", "hinge", "sgd"), ("rating", "bpr", "sgd"),
                                                   ("clip", "hinge", "adagrad")])
def test_trainer_step_under_the_other_options(dev, variant, loss_kind, opt):
    kw = {"normalize": dict(normalize_embeddings=True), "mixed": dict(candidate_sampling="mixed", n_sampled_negatives=64),
          "rating": dict(rating_weight=W_RATING, rating_hidden=HID), "clip": dict(global_clipnorm=0.05)}[variant]
    tr = _three_steps(dev, opt, loss_kind, 77, **kw)
    u, i = tr.synthetic_batch(77, 4, "Z")
    tr.step(u, i, **({"ratings": _ratings(dev, 77, 4)} if variant == "rating" else {}))
    tr.evaluate(u, i, **({"ratings": _ratings(dev, 77, 4)} if variant == "rating" else {}))
    tr.check_ids()
    assert torch.isfinite(tr.loss).all() and torch.isfinite(tr.dense_flat).all()


@pytest.mark.parametrize("loss_kind", ["bpr", "hinge"])
def test_checkpoint_round_trip_continues_bit_identically(dev, loss_kind):
    seed = 17

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    kw = dict(pairwise_reduction="sum")
    a = TwoTowerTrainer(_cfg("adagrad", loss_kind, **kw), dev, seed=seed)
    run(a, range(4))
    b = TwoTowerTrainer(_cfg("adagrad", loss_kind, **kw), dev, seed=seed)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert (sd["config"]["retrieval_loss"], sd["config"]["pairwise_margin"], sd["config"]["pairwise_reduction"]) == (loss_kind, MARGIN, "sum")
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)
    assert c.cfg.retrieval_loss == loss_kind
    c.load_state_dict(sd)
    run(c, range(2, 4))
    for k in ("user_table", "item_table", "dense_flat", "user_accum", "item_accum", "dense_accum", "loss", "per_row"):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    # a checkpoint from before the option: its config builds a softmax trainer
    old = {k: v for k, v in sd["config"].items() if k not in ("retrieval_loss", "pairwise_margin", "pairwise_reduction")}
    assert TwoTowerConfig(**old).retrieval_loss == "softmax"


def test_option_off_allocates_nothing_and_keeps_the_step(dev):
    """With the option off the trainer is the one it was (the launch sequence itself is pinned by tests/test_gpu_trainer_trace.py)."""
    tr = TwoTowerTrainer(_cfg("adagrad", "softmax"), dev, seed=3)
    assert tr.pairwise_ws is None and tr.pairwise_kind is None
    ref = TwoTowerTrainer(TwoTowerConfig(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], temperature=0.1,
                                         l2_regularization=1e-6, learning_rate=LR, optimizer="adagrad", batch_size=256), dev, seed=3)
    for s in range(2):
        la, lb = tr.step(*tr.synthetic_batch(3, s, "Z")).clone(), ref.step(*ref.synthetic_batch(3, s, "Z")).clone()
        assert torch.equal(la, lb)
    assert torch.equal(tr.dense_flat, ref.dense_flat) and torch.equal(tr.lse, ref.lse)
    assert set(tr.state_dict()) == set(ref.state_dict())


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(dev):
    from two_tower_amazon_recommender_amd import tasks, train
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(ValueError, match="scorer_precision='f32'"):
        TwoTowerTrainer(TwoTowerConfig(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 128], batch_size=256,
                                       retrieval_loss="bpr", scorer_precision="bf16x3"), dev)
    with pytest.raises(ValueError, match="retrieval_loss must be one of"):
        TwoTowerTrainer(_cfg("sgd", "triplet"), dev)
    with pytest.raises(NotImplementedError, match="pairwise retrieval loss"):
        TwoTowerTrainer(_cfg("sgd", "hinge"), dev, seed=1).capture_graph()
    with pytest.raises(NotImplementedError, match="pairwise retrieval loss.*row-sharded"):
        ShardedTwoTowerTrainer(_cfg("sgd", "bpr"), dev)
    with pytest.raises(NotImplementedError, match="exact f32 only"):
        tasks.Retrieval(loss=tasks.BPRLoss(), precision="bf16x3")
    with pytest.raises(NotImplementedError):
        tasks.Retrieval(loss=object())
    q = torch.zeros(4, 48, device=dev)
    with pytest.raises(ValueError, match="dim 48"):
        tasks.Retrieval(loss=tasks.PairwiseHingeLoss(0.3))(q, q)
    with pytest.raises(ValueError, match="kind"):
        ops.retrieval_pairwise_fwd(q, q, 1.0, torch.empty(256, dtype=torch.uint8, device=dev), torch.empty(4, device=dev),
                                   torch.empty(1, device=dev), kind="triplet")


# ------------------------------------------------------------------------------------------------- 6. CLI
def test_train_cli_runs_two_epochs_with_the_hinge_loss(dev, tmp_path):
    import contextlib
    import io
    import pyarrow as pa
    import pyarrow.parquet as pq
    from two_tower_amazon_recommender_amd import train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 2\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n    loss:\n      kind: bpr\n      reduction: sum\n")
    rng = np.random.default_rng(4)
    pairs = tmp_path / "pairs.parquet"
    uu, ii = rng.integers(0, 300, 600), rng.integers(0, 200, 600)
    uu[0], ii[0] = 299, 199
    pq.write_table(pa.table({"user_idx": uu, "item_idx": ii}), pairs)
    ck = tmp_path / "hinge.pt"
    with contextlib.redirect_stdout(io.StringIO()):                        # 600 pairs, 10 % held out: 2 training steps per epoch
        assert train.main(["--config", str(cfgp), "--data", str(pairs), "--retrieval-loss", "hinge", "--pairwise-margin", "0.25",
                           "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 4
    assert (sd["config"]["retrieval_loss"], sd["config"]["pairwise_margin"], sd["config"]["pairwise_reduction"]) == ("hinge", 0.25, "sum")
    with pytest.raises(NotImplementedError, match="row-sharded"):
        train.main(["--config", str(cfgp), "--data", str(pairs), "--distributed"])
    with pytest.raises(SystemExit, match="f32"):
        train.main(["--config", str(cfgp), "--data", str(pairs), "--scorer-precision", "bf16x3"])

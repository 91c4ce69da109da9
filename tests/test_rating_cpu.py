"""The rating head without a GPU: the NumPy restatement of tests/rating_check.py against torch-CPU autograd and central finite
differences, the loss's conventions (NaN = no label, the divisor is n), the YAML block, the config's refusals and the CLIs'
argument refusals."""
import numpy as np
import pytest
import torch

import rating_check as rc
from two_tower_amazon_recommender_amd import config as cfgmod
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig


def _problem(n=7, d=4, h=8, seed=0):
    rng = np.random.default_rng(seed)
    q, c = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    w1, b1 = rng.standard_normal((2 * d, h)) * 0.5, rng.standard_normal(h) * 0.3
    w2, b2 = rng.standard_normal(h), np.array([3.0])
    rating = rng.integers(1, 6, n).astype(np.float64)
    rating[2] = np.nan
    sw = rng.uniform(0.5, 2.0, n)
    sw[4] = 0.0
    return q, c, w1, b1, w2, b2, rating, sw


def _loss(q, c, w1, b1, w2, b2, rating, sw):
    return rc.rating_loss(rc.head_forward(q, c, w1, b1, w2, b2)[0], rating, sw)


def test_backward_equals_torch_autograd_of_the_forward_math():
    q, c, w1, b1, w2, b2, rating, sw = _problem()
    n = len(rating)
    weight = 0.5
    pred, h, _ = rc.head_forward(q, c, w1, b1, w2, b2)
    got = rc.head_backward(q, c, h, pred, rating, w1, w2, 2.0 * weight / n, sw)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, c, w1, b1, w2, b2)]
    hid = torch.relu(t[3] + torch.cat([t[0], t[1]], dim=1) @ t[2])
    tp = hid @ t[4] + t[5]
    valid = torch.tensor(np.isfinite(rating))
    e = torch.where(valid, tp - torch.tensor(np.nan_to_num(rating)), torch.zeros_like(tp))
    loss = (torch.tensor(sw) * e * e).sum() / n
    (weight * loss).backward()
    assert abs(float(loss.detach()) - rc.rating_loss(pred, rating, sw)) <= 1e-12 * abs(float(loss.detach()))
    assert abs(got["se"] / n - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for g, k in zip(t, ("dq", "dc", "dw1", "db1", "dw2", "db2")):
        want = g.grad.numpy()
        assert np.abs(np.asarray(got[k]).reshape(want.shape) - want).max() <= 1e-12 * np.abs(want).max(), k


def test_f32_evaluation_meets_the_kernel_bars_at_every_gpu_shape():
    """The bars of tests/test_gpu_rating.py (1e-5 of max|ref|) can be met in float32 on its own problems, every hidden width
    included: the same math as torch-CPU f32 operations against the f64 restatement, the backward from the f32 h and pred (the
    GPU test hands the restatement the device's)."""
    import test_gpu_rating as tg
    assert sorted({h for _, _, h in tg.SHAPES}) == list(range(32, 257, 32))
    f = torch.from_numpy
    for n, d, h in tg.SHAPES:
        q, c, w1, b1, w2, b2, rating, sw = tg._problem(n, d, h)
        tq, tc, tw1, tb1, tw2, tb2 = (f(a).requires_grad_() for a in (q, c, w1, b1, w2, b2))
        hid = torch.relu(torch.addmm(tb1, torch.cat([tq, tc], dim=1), tw1))
        pred = torch.mv(hid, tw2) + tb2
        want_pred, want_h, _ = rc.head_forward(q, c, w1, b1, w2, b2)
        errs = dict(pred=tg.rel_err(pred.detach().numpy(), want_pred), h=tg.rel_err(hid.detach().numpy(), want_h))
        valid = torch.isfinite(f(rating))
        e = torch.where(valid, pred - torch.nan_to_num(f(rating)), torch.zeros_like(pred))
        se = (f(sw) * e * e).sum()
        scale = 2.0 * 0.5 / n
        (0.5 * scale * se).backward()
        ref = rc.head_backward(q, c, hid.detach().numpy(), pred.detach().numpy(), rating, w1, w2, scale, sw)
        for k, t in (("dq", tq), ("dc", tc), ("dw1", tw1), ("db1", tb1), ("dw2", tw2)):
            errs[k] = tg.rel_err(t.grad.numpy(), ref[k])
        errs["db2"] = tg.rel_err(tb2.grad.numpy(), np.array([ref["db2"]]))
        errs["se"] = tg.rel_err(np.array([se.item()]), np.array([ref["se"]]))
        print(f"({n}, {d}, {h}): " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-5, (n, d, h, errs)


def test_backward_equals_central_finite_differences():
    args = list(_problem())
    q, c, w1, b1, w2, b2, rating, sw = args
    n = len(rating)
    pred, h, a = rc.head_forward(q, c, w1, b1, w2, b2)
    assert np.abs(a).min() > 1e-3                       # no pre-activation at the kink: the differences are clean
    got = rc.head_backward(q, c, h, pred, rating, w1, w2, 2.0 / n, sw)          # rating_weight 1: the gradient of L_r itself
    eps = 1e-6
    for idx, k in enumerate(("dq", "dc", "dw1", "db1", "dw2", "db2")):
        base = args[idx]
        num = np.zeros_like(base)
        for pos in np.ndindex(base.shape):
            up, dn = base.copy(), base.copy()
            up[pos] += eps; dn[pos] -= eps
            num[pos] = (_loss(*args[:idx], up, *args[idx + 1:]) - _loss(*args[:idx], dn, *args[idx + 1:])) / (2 * eps)
        want = np.asarray(got[k]).reshape(base.shape)
        assert np.abs(num - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0), k


def test_missing_labels_and_zero_weights_give_exactly_zero_gradient_rows_and_the_divisor_is_n():
    q, c, w1, b1, w2, b2, rating, sw = _problem()
    n = len(rating)
    pred, h, _ = rc.head_forward(q, c, w1, b1, w2, b2)
    got = rc.head_backward(q, c, h, pred, rating, w1, w2, 2.0 / n, sw)
    for row in (2, 4):                                  # the NaN rating, the zero weight
        assert got["g"][row] == 0 and not got["dq"][row].any() and not got["dc"][row].any()
    assert got["dq"][0].any() and got["dc"][0].any()
    valid = np.isfinite(rating)
    e = pred[valid] - rating[valid]
    assert rc.rating_loss(pred, rating) == pytest.approx((e * e).sum() / n, rel=1e-14)          # n = 7, not the 6 labels
    assert rc.rating_loss(pred, rating) != pytest.approx((e * e).mean(), rel=1e-3)
    assert rc.rating_loss(pred, np.full(n, np.nan)) == 0.0
    assert rc.slab_rows(10, 4) == [(0, 3), (3, 6), (6, 9), (9, 10)] and rc.slab_rows(3, 5)[3:] == [(3, 3), (3, 3)]


def test_step_f64_total_is_retrieval_plus_weighted_rating_loss():
    rng = np.random.default_rng(3)
    b, dim, d, h = 6, 4, 4, 8
    ut, it = rng.standard_normal((10, dim)) * 0.1, rng.standard_normal((9, dim)) * 0.1
    towers = tuple(([rng.standard_normal((dim, d)) * 0.5], [np.zeros(d)]) for _ in range(2))
    head = (rng.standard_normal((2 * d, h)) * 0.5, rng.standard_normal(h) * 0.1, rng.standard_normal(h), np.array([3.0]))
    u, i = rng.integers(0, 10, b), rng.integers(0, 9, b)
    rating = np.array([1.0, 5.0, np.nan, 3.0, 4.0, 2.0])
    q, c = ut[u] @ towers[0][0][0], it[i] @ towers[1][0][0]
    pred, hid, _ = rc.head_forward(q, c, *head)
    r = rc.step_f64(ut, it, towers, u, i, head, rating, 0.5, 0.1, ([], []), hid > 0)
    assert r["rating_loss"] == pytest.approx(rc.rating_loss(pred, rating), rel=1e-12)
    want = rc.head_backward(q, c, hid, pred, rating, head[0], head[2], 2.0 * 0.5 / b)
    for k in ("dw1", "db1", "dw2"):
        assert np.abs(r[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    r0 = rc.step_f64(ut, it, towers, u, i, head, rating, 0.0, 0.1, ([], []), hid > 0)
    assert r0["loss"] == r["loss"] and np.abs(r["dq"] - r0["dq"] - want["dq"]).max() <= 1e-12 * np.abs(want["dq"]).max()


def test_tensor_ids_collide_with_none_of_the_trainers():
    from two_tower_amazon_recommender_amd import trainer
    assert (trainer.TID_RATING_W1, trainer.TID_RATING_W2) == (rc.TID_RATING_W1, rc.TID_RATING_W2) == (40, 41)
    others = {v for k, v in vars(trainer).items() if k.startswith("TID_") and "RATING" not in k and "BASE" not in k}
    dense = {trainer.TID_DENSE_BASE + 2 * l + t for l in range(8) for t in range(2)}
    dropout = {trainer.TID_DROPOUT_BASE + 2 * l + t for l in range(8) for t in range(2)}
    assert not {40, 41} & (others | dense | dropout) and (others | dense | dropout) <= rc.TRAINER_TIDS_IN_USE


DOC = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "training": {"batch_size": 256},
                 "retrieval": {"temperature": 0.1}}}


def _doc(**ranking):
    return {"model": {**DOC["model"], "ranking": ranking}}


def test_config_reads_the_ranking_block():
    cfg, _ = cfgmod.model_config_from_dict(DOC, 10, 10)
    assert cfg.rating_weight == 0.0 and cfg.rating_hidden == 128             # no block: no head
    cfg, _ = cfgmod.model_config_from_dict(_doc(weight=0.5, hidden_dim=64), 10, 10)
    assert (cfg.rating_weight, cfg.rating_hidden) == (0.5, 64)
    cfg.validate()
    cfg, _ = cfgmod.model_config_from_dict(_doc(weight=2), 10, 10)
    assert (cfg.rating_weight, cfg.rating_hidden) == (2.0, 128)
    for bad in (dict(weight=-0.1), dict(weight=float("nan")), dict(weight="much"), dict(weight=True), dict(weight=0.5, hidden_dim=48),
                dict(weight=0.5, hidden_dim=0), dict(weight=0.5, hidden_dim=288), dict(weight=0.5, hidden_dim=64.0)):
        with pytest.raises(ValueError, match="model.ranking"):
            cfgmod.model_config_from_dict(_doc(**bad), 10, 10)


def test_validate_refuses_bad_fields():
    TwoTowerConfig(10, 10, rating_weight=0.5, rating_hidden=256).validate()
    TwoTowerConfig(10, 10).validate()
    for kw in (dict(rating_weight=-1.0), dict(rating_weight=float("inf")), dict(rating_weight=float("nan")), dict(rating_weight="1"),
               dict(rating_weight=True)):
        with pytest.raises(ValueError, match="rating_weight"):
            TwoTowerConfig(10, 10, **kw).validate()
    for h in (0, 16, 48, 257, 512, 64.0, True):
        with pytest.raises(ValueError, match="rating_hidden"):
            TwoTowerConfig(10, 10, rating_weight=0.5, rating_hidden=h).validate()


def test_ranking_task_is_the_contracts_loss():
    from two_tower_amazon_recommender_amd import tasks
    _, _, _, _, _, _, rating, sw = _problem()
    pred = torch.tensor(np.random.default_rng(1).uniform(1, 5, len(rating)), requires_grad=True)
    seen = []

    class Metric:
        def update_state(self, labels, predictions):
            seen.append((labels, predictions))
    task = tasks.Ranking(loss=tasks.MeanSquaredError(), metrics=[Metric()])
    loss = task(torch.tensor(rating), pred, sample_weight=torch.tensor(sw))
    assert loss.item() == pytest.approx(rc.rating_loss(pred.detach().numpy(), rating, sw), rel=1e-12) and len(seen) == 1
    loss.backward()
    assert pred.grad[2].item() == 0 and pred.grad[4].item() == 0 and pred.grad[0].item() != 0
    with pytest.raises(NotImplementedError):
        tasks.Ranking(loss="hinge")
    with pytest.raises(TypeError):
        tasks.Ranking(metrics=[object()])


def test_cli_argument_refusals(tmp_path):
    import yaml
    from two_tower_amazon_recommender_amd import recommend, train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text(yaml.safe_dump(DOC))
    base = ["--config", str(cfgp), "--synthetic", "600"]
    with pytest.raises(SystemExit, match="rating-weight"):
        train.main(base + ["--rating-weight", "-1"])
    with pytest.raises(SystemExit, match="rating-hidden"):
        train.main(base + ["--rating-weight", "0.5", "--rating-hidden", "48"])
    with pytest.raises(SystemExit, match="needs a rating head"):
        train.main(base + ["--rating-hidden", "64"])
    with pytest.raises(NotImplementedError, match="rating head"):
        train.main(base + ["--rating-weight", "0.5", "--distributed"])
    bad = tmp_path / "bad.yaml"
    bad.write_text(yaml.safe_dump(_doc(weight=0.5, hidden_dim=100)))
    with pytest.raises(ValueError, match="model.ranking.hidden_dim"):
        train.main(["--config", str(bad), "--synthetic", "600"])
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"")
    with pytest.raises(SystemExit):                      # argparse: not one of score / rating
        recommend.parse(["--checkpoint", str(ck), "--all-users", "--rank-by", "stars"])
    args = recommend.parse(["--checkpoint", str(ck), "--all-users", "--rank-by", "rating"])
    assert args.predict_ratings and args.rank_by == "rating"
    args = recommend.parse(["--checkpoint", str(ck), "--all-users"])
    assert not args.predict_ratings and args.rank_by == "score"

"""L2-normalised tower outputs on the GPU: the two kernels of csrc/normalize.hip against an f64 NumPy restatement of
tf.math.l2_normalize and its gradient, the clamped branch, bit identity, the custom op, the trainer against the oracle's own
pieces with the normalisation restated between them, the embeddings the trainer hands to serving, checkpoints and the CLI."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

from oracle import synth, two_tower as tt
from two_tower_amazon_recommender_amd import ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
EPS = 1e-12
SENTINEL = -12345.0
SHAPES = [(1, 4), (7, 32), (777, 64), (1025, 128), (513, 256), (33, 1000)]


# ------------------------------------------------------------------------------------------ the f64 restatement
def l2n(x, eps=EPS):
    """tf.math.l2_normalize(x, axis=1, epsilon=eps): x * rsqrt(max(sum x^2, eps))."""
    s = (x * x).sum(axis=1, keepdims=True)
    return x / np.sqrt(np.maximum(s, eps))


def l2n_grad(x, dy, eps=EPS):
    """Gradient of l2n: where the sum of squares is clamped the function is linear (x / sqrt(eps))."""
    s = (x * x).sum(axis=1, keepdims=True)
    t = (x * dy).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(s, eps))
    return np.where(s >= eps, inv * (dy - x * (t * inv * inv)), dy * inv)


def _inputs(rows, dim, seed):
    """x rows N(0,1) * 10^U(-3,3), dy N(0,1), as f32."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, dim)) * 10.0 ** rng.uniform(-3, 3, (rows, 1))
    return x.astype(np.float32), rng.standard_normal((rows, dim)).astype(np.float32)


def _guarded(rows, dim, dev):
    """([rows, dim] view to write into, the 64 sentinel rows behind it)."""
    buf = torch.full((rows + 64, dim), SENTINEL, device=dev)
    return buf[:rows], buf[rows:]


def _check_y(y, x, eps, what):
    err = np.abs(y.cpu().numpy().astype(np.float64) - l2n(x.astype(np.float64), eps)).max()
    print(f"{what}: max |y - y64| = {err / U24:.2f} * 2^-24")
    assert err <= 16 * U24, (what, err / U24)


def _check_dx(dx, x, dy, eps, what):
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    bar = 32 * U24 * np.linalg.norm(dy64, axis=1) / np.linalg.norm(x64, axis=1)
    err = np.abs(dx.cpu().numpy().astype(np.float64) - l2n_grad(x64, dy64, eps)).max(axis=1)
    print(f"{what}: max |dx - dx64| / (2^-24 |dy| / |x|) = {(err / (bar / 32)).max():.2f}")
    assert (err <= bar).all(), (what, (err / (bar / 32)).max())


# ------------------------------------------------------------------------------------------ 1. kernels against f64
@pytest.mark.parametrize("rows,dim", SHAPES)
def test_kernels_match_the_f64_restatement_and_stay_inside_their_rows(dev, rows, dim):
    (xa, dya), (xb, dyb) = _inputs(rows, dim, 10 + dim), _inputs(rows, dim, 20 + dim)
    txa, txb, tdya, tdyb = (torch.from_numpy(a).to(dev) for a in (xa, xb, dya, dyb))
    (ya, ga), (yb, gb) = _guarded(rows, dim, dev), _guarded(rows, dim, dev)
    ops.l2_normalize2((txa, txb), (ya, yb), EPS)                   # both towers in one launch
    (dxa, ha), (dxb, hb) = _guarded(rows, dim, dev), _guarded(rows, dim, dev)
    ops.l2_normalize_bwd2((txa, txb), (tdya, tdyb), (dxa, dxb), EPS)
    for guard in (ga, gb, ha, hb):
        assert (guard == SENTINEL).all()
    for y, dx, x, dy, nm in ((ya, dxa, xa, dya, "a"), (yb, dxb, xb, dyb, "b")):
        _check_y(y, x, EPS, f"({rows}, {dim}) {nm}")
        _check_dx(dx, x, dy, EPS, f"({rows}, {dim}) {nm}")
    # the one-tower wrappers are the same launch with one problem
    assert torch.equal(ops.l2_normalize(txa), ya) and torch.equal(ops.l2_normalize_bwd(txa, tdya), dxa)


# ------------------------------------------------------------------------------------------ 2. the clamped branch
def _two_ulp(got, want64):
    want32 = want64.astype(np.float32)
    return (np.abs(got.astype(np.float64) - want64) <= 2 * np.spacing(np.abs(want32)).astype(np.float64)).all()


@pytest.mark.parametrize("dim", [32, 128, 1000])
def test_clamped_branch(dev, dim):
    rng = np.random.default_rng(dim)
    unit = rng.standard_normal((3, dim))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    x = np.stack([np.zeros(dim), unit[0] * 1e-8, unit[1] * 1e-3, unit[2] * 3.0]).astype(np.float32)
    dy = rng.standard_normal((4, dim)).astype(np.float32)
    tx, tdy = torch.from_numpy(x).to(dev), torch.from_numpy(dy).to(dev)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    for eps, clamped in ((1e-12, [True, True, False, False]), (1e-4, [True, True, True, False])):
        s = (x64 * x64).sum(axis=1)
        assert list(s < eps) == clamped and (np.abs(s / eps - 1) > 0.01).all()     # no row within 1 % of the switch
        y = ops.l2_normalize(tx, eps=eps).cpu().numpy()
        dx = ops.l2_normalize_bwd(tx, tdy, eps=eps).cpu().numpy()
        assert not y[0].any()                                                         # a zero row stays zero (no 0 * inf)
        _check_y(torch.from_numpy(y), x, eps, f"dim {dim} eps {eps}")
        inv = 1.0 / np.sqrt(np.float64(np.float32(eps)))                              # eps as the kernel receives it
        for r in range(4):
            if clamped[r]:      # linear: dx = dy * (1 / sqrt(eps)), one rounding of the factor and one of the product
                assert _two_ulp(dx[r], dy64[r] * inv), (dim, eps, r)
            else:
                _check_dx(torch.from_numpy(dx[r:r + 1]), x[r:r + 1], dy[r:r + 1], eps, f"dim {dim} eps {eps} row {r}")


# ------------------------------------------------------------------------------------------ 3. bit identity
@pytest.mark.parametrize("rows,dim", [(777, 64), (1025, 128)])
def test_bit_identity_across_runs_problem_counts_and_aliasing(dev, rows, dim):
    (xa, dya), (xb, dyb) = _inputs(rows, dim, 1), _inputs(rows, dim, 2)
    txa, txb, tdya, tdyb = (torch.from_numpy(a).to(dev) for a in (xa, xb, dya, dyb))
    new = lambda: torch.full((rows, dim), SENTINEL, device=dev)      # noqa: E731
    y2 = ops.l2_normalize2((txa, txb), (new(), new()), EPS)
    y2again = ops.l2_normalize2((txa, txb), (new(), new()), EPS)
    y1 = (ops.l2_normalize2((txa,), (new(),), EPS)[0], ops.l2_normalize2((txb,), (new(),), EPS)[0])
    d2 = ops.l2_normalize_bwd2((txa, txb), (tdya, tdyb), (new(), new()), EPS)
    d2again = ops.l2_normalize_bwd2((txa, txb), (tdya, tdyb), (new(), new()), EPS)
    d1 = (ops.l2_normalize_bwd2((txa,), (tdya,), (new(),), EPS)[0], ops.l2_normalize_bwd2((txb,), (tdyb,), (new(),), EPS)[0])
    alias = (tdya.clone(), tdyb.clone())
    ops.l2_normalize_bwd2((txa, txb), alias, alias, EPS)              # dx written over dy
    for i in range(2):
        assert torch.equal(y2[i], y2again[i]) and torch.equal(y2[i], y1[i])
        assert torch.equal(d2[i], d2again[i]) and torch.equal(d2[i], d1[i]) and torch.equal(d2[i], alias[i])


# ------------------------------------------------------------------------------------------ 4. the custom op
@pytest.mark.parametrize("rows,dim", [(64, 32), (130, 128)])
def test_custom_op_passes_opcheck_and_its_gradient_matches_f64_autograd(dev, rows, dim):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    x, dy = _inputs(rows, dim, 5)
    tx = torch.from_numpy(x).to(dev).requires_grad_()
    torch.library.opcheck(torch.ops.twotower.l2_normalize, (tx, EPS))
    torch.library.opcheck(torch.ops.twotower.l2_normalize, (tx.detach(),))
    torch.library.opcheck(torch.ops.twotower.l2_normalize_bwd, (tx.detach(), torch.from_numpy(dy).to(dev), EPS))
    y = torch.ops.twotower.l2_normalize(tx, EPS)
    y.backward(torch.from_numpy(dy).to(dev))
    x64 = torch.from_numpy(x).double().requires_grad_()
    y64 = x64 * torch.rsqrt(torch.clamp((x64 * x64).sum(dim=1, keepdim=True), min=EPS))
    y64.backward(torch.from_numpy(dy).double())
    bar = 32 * U24 * np.linalg.norm(dy.astype(np.float64), axis=1) / np.linalg.norm(x.astype(np.float64), axis=1)
    assert (np.abs(y.detach().cpu().numpy() - y64.detach().numpy()).max()) <= 16 * U24
    assert (np.abs(tx.grad.cpu().numpy() - x64.grad.numpy()).max(axis=1) <= bar).all()
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.twotower.l2_normalize(torch.zeros(4, 32))              # CPU tensor: no kernel, no fallback


# ------------------------------------------------------------------------------------------ 5. trainer against the oracle
def _cfg(n_users, n_items, dim, tower_dims, batch, opt, item_tower_dims=None, dropout=0.0, precision="f32", normalize=True):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=tower_dims, item_tower_dims=item_tower_dims,
                          temperature=0.1, l2_regularization=1e-6, learning_rate=0.001, optimizer=opt, batch_size=batch,
                          dropout_rate=dropout, scorer_precision=precision, normalize_embeddings=normalize)


def oracle_forward(state, uid, iid, dropout=None):
    ud, idr, _ = (None, None, 1.0) if dropout is None else dropout
    ua = tt.tower_fwd(tt.embedding_gather(state.user_table, uid), state.user_tower.weights, state.user_tower.biases, ud)
    ia = tt.tower_fwd(tt.embedding_gather(state.item_table, iid), state.item_tower.weights, state.item_tower.biases, idr)
    return ua, ia


def oracle_train_step_normalized(state, uid, iid, lr, optimizer, temperature, l2, relu_masks, dropout=None, eps=1e-7):
    """oracle.two_tower.train_step with an f64 normalise between tower_fwd and retrieval_loss / retrieval_grad and its gradient
    between retrieval_grad and tower_bwd; every other piece is the oracle's own function."""
    ua, ia = oracle_forward(state, uid, iid, dropout)
    q, c = l2n(ua[-1]), l2n(ia[-1])
    loss, _, _ = tt.retrieval_loss(q, c, temperature=temperature)
    dq, dc = tt.retrieval_grad(q, c, temperature=temperature)
    dscale = 1.0 if dropout is None else dropout[2]
    due, udw, udb = tt.tower_bwd(ua, state.user_tower.weights, l2n_grad(ua[-1], dq), relu_masks[0], dscale)
    die, idw, idb = tt.tower_bwd(ia, state.item_tower.weights, l2n_grad(ia[-1], dc), relu_masks[1], dscale)
    for tw, dws in ((state.user_tower, udw), (state.item_tower, idw)):
        for l, w in enumerate(tw.weights):
            dws[l] = dws[l] + 2 * l2 * w
    if optimizer == "sgd":
        tt.sparse_sgd(state.user_table, uid, due, lr)
        tt.sparse_sgd(state.item_table, iid, die, lr)
    else:
        tt.sparse_adagrad(state.user_table, state.user_accum, uid, due, lr, eps)
        tt.sparse_adagrad(state.item_table, state.item_accum, iid, die, lr, eps)
    for tw, dws, dbs in ((state.user_tower, udw, udb), (state.item_tower, idw, idb)):
        for l in range(len(tw.weights)):
            if optimizer == "sgd":
                tt.dense_sgd(tw.weights[l], dws[l], lr)
                tt.dense_sgd(tw.biases[l], dbs[l], lr)
            else:
                tt.dense_adagrad(tw.weights[l], tw.w_accum[l], dws[l], lr, eps)
                tt.dense_adagrad(tw.biases[l], tw.b_accum[l], dbs[l], lr, eps)
    return dict(loss=loss, due=due, die=die, q=q, c=c)


def _loss_close(got, want, batch):
    return abs(got - want) / batch <= 1e-4 and abs(got - want) <= 1e-4 * abs(want)


@pytest.mark.parametrize("name,shape,item_dims,opt,variant,dropout,precision", [
    ("ragged-777", (3000, 2000, 64, [96, 64], 777), None, "adagrad", "Z", 0.0, "f32"),
    ("1024-sgd", (5000, 5000, 128, [256, 128], 1024), None, "sgd", "U", 0.0, "f32"),
    ("1024-sgd-bf16x3", (5000, 5000, 128, [256, 128], 1024), None, "sgd", "U", 0.0, "bf16x3"),
    ("asymmetric-dropout", (2000, 2000, 32, [64, 32], 256), [32], "adagrad", "Z", 0.1, "f32"),
])
def test_normalized_train_steps_match_the_oracle(dev, name, shape, item_dims, opt, variant, dropout, precision):
    n_users, n_items, dim, tower_dims, batch = shape
    seed = 1001
    cfg = _cfg(n_users, n_items, dim, tower_dims, batch, opt, item_dims, dropout, precision)
    tr = TwoTowerTrainer(cfg, dev, seed=seed)
    ref = tt.synthetic_state(seed, n_users, n_items, dim, tower_dims, dtype=np.float64, optimizer=opt, item_tower_dims=item_dims)
    init = copy.deepcopy(ref)
    for step in range(3):
        uid = synth.batch_ids(seed, synth.TID_USER_IDS, step, batch, n_users, variant)
        iid = synth.batch_ids(seed, synth.TID_ITEM_IDS, step, batch, n_items, variant)
        du, di = tr.synthetic_batch(seed, step, variant)
        assert np.array_equal(du.cpu().numpy(), uid) and np.array_equal(di.cpu().numpy(), iid)
        if step == 0:
            # forward only (no dropout), before anything is updated: the normalised loss, and a trainer with the switch off
            # still returns the un-normalised one
            ua, ia = oracle_forward(ref, uid, iid)
            want_eval = tt.retrieval_loss(l2n(ua[-1]), l2n(ia[-1]), temperature=0.1)[0]
            want_raw = tt.retrieval_loss(ua[-1], ia[-1], temperature=0.1)[0]
            got_eval = tr.evaluate(du, di).item()
            off = TwoTowerTrainer(_cfg(n_users, n_items, dim, tower_dims, batch, opt, item_dims, dropout, precision, normalize=False),
                                  dev, seed=seed)
            got_raw = off.evaluate(du, di).item()
            print(f"{name}: evaluate {got_eval} (oracle {want_eval}); switch off {got_raw} (oracle {want_raw})")
            assert _loss_close(got_eval, want_eval, batch), (got_eval, want_eval)
            assert _loss_close(got_raw, want_raw, batch), (got_raw, want_raw)
            assert not _loss_close(got_raw, want_eval, batch) and not _loss_close(got_eval, want_raw, batch)
            del off
        loss = tr.step(du, di).item()
        towers = (tr.user_tower, tr.item_tower)
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in towers)
        drop = None
        if dropout:
            per_tower = [[synth.dropout_keep(seed, synth.dropout_tid(t, l), step * batch, batch, tw.dims[l + 1], dropout)
                          for l in range(tw.n_layers - 1)] for t, tw in enumerate(towers)]
            drop = (per_tower[0], per_tower[1], per_tower[0][0][1])
        r = oracle_train_step_normalized(ref, uid, iid, 0.001, opt, 0.1, 1e-6, masks, drop)
        tr.check_ids()
        print(f"{name} step {step}: loss {loss} (oracle {r['loss']})")
        assert _loss_close(loss, r["loss"], batch), (step, loss, r["loss"])
        norms = tr.user_tower.unit.double().norm(dim=1).cpu().numpy()
        assert np.abs(norms - 1).max() <= 1e-6, np.abs(norms - 1).max()
        for got, want in ((tr.user_tower.demb, r["due"]), (tr.item_tower.demb, r["die"])):
            err = np.abs(got.cpu().numpy() - want).max()
            print(f"{name} step {step}: demb error {err / np.abs(want).max():.2e} of max |want|")
            assert err <= 1e-4 * np.abs(want).max(), (step, err, np.abs(want).max())

    def close(got, want, want0, what):
        got = got.cpu().numpy()
        bar = 1e-4 * np.abs(want - want0).max() + 4 * float(np.spacing(np.float32(np.abs(want).max())))
        err = np.abs(got - want).max()
        print(f"{name} {what}: error {err:.3e}, bar {bar:.3e} (largest change {np.abs(want - want0).max():.3e})")
        assert err <= bar, (what, err, bar)
    close(tr.user_table, ref.user_table, init.user_table, "user table")
    close(tr.item_table, ref.item_table, init.item_table, "item table")
    for tower, rt, rt0, tn in ((tr.user_tower, ref.user_tower, init.user_tower, "user"), (tr.item_tower, ref.item_tower, init.item_tower, "item")):
        for l in range(tower.n_layers):
            close(tower.w[l], rt.weights[l], rt0.weights[l], f"{tn} w[{l}]")
            close(tower.b[l], rt.biases[l], rt0.biases[l], f"{tn} b[{l}]")


# ------------------------------------------------------------------------------------------ 6. serving consistency
def test_embeddings_handed_to_serving_are_the_normalised_tower_outputs(dev):
    from two_tower_amazon_recommender_amd.serving import BruteForce
    n_users, n_items, dim, tower_dims, batch, seed = 5000, 5000, 128, [256, 128], 1024, 1001
    tr = TwoTowerTrainer(_cfg(n_users, n_items, dim, tower_dims, batch, "sgd"), dev, seed=seed)
    ref = tt.synthetic_state(seed, n_users, n_items, dim, tower_dims, dtype=np.float64)
    bar = 16 * U24 + 1e-5
    corpus = tr.item_corpus_embeddings().cpu().numpy().astype(np.float64)
    want = l2n(tt.tower_fwd(ref.item_table, ref.item_tower.weights, ref.item_tower.biases)[-1])
    assert np.abs(np.linalg.norm(corpus, axis=1) - 1).max() <= 1e-6
    assert np.abs(corpus - want).max() <= bar, np.abs(corpus - want).max()
    ids = np.random.default_rng(3).integers(0, n_users, 1500)                    # more than one batch, a ragged tail
    users = tr.user_embeddings(torch.from_numpy(ids).to(dev)).cpu().numpy().astype(np.float64)
    want = l2n(tt.tower_fwd(ref.user_table[ids], ref.user_tower.weights, ref.user_tower.biases)[-1])
    assert np.abs(np.linalg.norm(users, axis=1) - 1).max() <= 1e-6
    assert np.abs(users - want).max() <= bar, np.abs(users - want).max()
    scores, items = BruteForce(k=10).index_from_trainer(tr)(torch.from_numpy(ids).to(dev))
    assert (items >= 0).all() and scores.min().item() >= -1 - 1e-5 and scores.max().item() <= 1 + 1e-5
    tr.check_ids()


# ------------------------------------------------------------------------------------------ 7. checkpoint
def test_checkpoint_carries_the_switch(dev):
    seed = 17

    def fresh(normalize):
        return TwoTowerTrainer(_cfg(800, 700, 32, [64, 32], 256, "adagrad", dropout=0.2, normalize=normalize), dev, seed=seed)
    a = fresh(True)
    for s in range(2):
        a.step(*a.synthetic_batch(seed, s))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    sd["config"] = dict(sd["config"])
    assert sd["config"]["normalize_embeddings"] is True and sd["config"]["normalize_eps"] == 1e-12
    want = a.step(*a.synthetic_batch(seed, 2)).clone()
    b = fresh(False)                                  # the checkpoint, not the loading run, says what the model is
    b.load_state_dict(sd)
    assert b.cfg.normalize_embeddings is True
    got = b.step(*b.synthetic_batch(seed, 2))
    assert torch.equal(got, want)
    assert torch.equal(a.user_table, b.user_table) and torch.equal(a.dense_flat, b.dense_flat)
    old = dict(sd, config={k: v for k, v in sd["config"].items() if k not in ("normalize_embeddings", "normalize_eps")})
    c = fresh(True)
    c.load_state_dict(old)                            # a checkpoint from before the switch existed
    assert c.cfg.normalize_embeddings is False
    plain = fresh(False)
    plain.load_state_dict(old)
    assert torch.equal(c.step(*c.synthetic_batch(seed, 2)), plain.step(*plain.synthetic_batch(seed, 2)))
    assert not torch.equal(c.loss, want)


# ------------------------------------------------------------------------------------------ 8. CLI
CLI_SEED = 42


def _train_and_recommend(tmp_path, tag, *extra):
    """One epoch of Adagrad at learning rate 1.0: with accumulators starting at 0.1 the first updates move every parameter by
    up to ~1, several times the Glorot limit, so the raw towers' outputs (and their dot products) grow far past 1 whether the
    run goes on learning or collapses onto its biases, while the normalised model's scores cannot leave [-1, 1].  (An f64
    restatement of this run with the oracle's train_step left |score| >= 19 at four seeds; at 0.3 the raw scores depend on
    the batch order: from 0.02 to 1.6.)"""
    import pyarrow.parquet as pq
    from two_tower_amazon_recommender_amd import recommend, train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  dropout_rate: 0.0\n  l2_regularization: 1e-6\n  training:\n    batch_size: 256\n    learning_rate: 1.0\n"
                    "    epochs: 1\n  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck, out = tmp_path / f"{tag}.pt", tmp_path / f"{tag}.parquet"
    with contextlib.redirect_stdout(io.StringIO()):
        assert train.main(["--config", str(cfgp), "--synthetic", "100000", "--synthetic-users", "600", "--synthetic-items", "500",
                           "--seed", str(CLI_SEED), "--save", str(ck), *extra]) == 0
        assert recommend.main(["--checkpoint", str(ck), "--k", "5", "--all-users", "--out", str(out)]) == 0
    scores = pq.read_table(out).column("score").to_numpy()
    assert len(scores) == 600 * 5
    return torch.load(ck, weights_only=True), scores


def test_train_and_recommend_cli_serve_cosine_scores(dev, tmp_path):
    sd, scores = _train_and_recommend(tmp_path, "unit", "--normalize-embeddings")
    assert sd["config"]["normalize_embeddings"] is True
    print(f"normalised: scores in [{scores.min()}, {scores.max()}]")
    assert scores.min() >= -1 - 1e-5 and scores.max() <= 1 + 1e-5
    sd, raw = _train_and_recommend(tmp_path, "raw")
    assert sd["config"]["normalize_embeddings"] is False
    print(f"switch off: scores in [{raw.min()}, {raw.max()}]")
    assert raw.max() > 1 + 1e-5 or raw.min() < -1 - 1e-5        # dot products of the raw tower outputs are not bounded

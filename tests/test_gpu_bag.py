"""The pooled item-title feature on the GPU (csrc/bag.hip): the forward pass, its backward launch and the bag table's update
against the restatements of tests/bag_check.py BIT FOR BIT, then the trainer - invariance against the category feature, parity
with the f64 autograd restatement, training, checkpoints, the item corpus - the custom op, the CLIs and the refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import bag_check as bc
from two_tower_amazon_recommender_amd import ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bad(got, want):
    b = bc.bits(got) != bc.bits(want)
    return int(b.sum()), np.argwhere(b)[:4].tolist()


def _tokens(rng, n_rows, L, buckets):
    """Padding anywhere (also in the middle), all-padding rows, repeated tokens inside a row."""
    tok = rng.integers(0, buckets, (n_rows, L)).astype(np.int32)
    tok[rng.random((n_rows, L)) < 0.3] = -1
    tok[rng.random(n_rows) < 0.1] = -1
    if L >= 3:
        rep = rng.random(n_rows) < 0.3
        tok[rep, 2] = tok[rep, 0]
        tok[0, 1] = -1                                  # padding between two tokens
        tok[0, 0], tok[0, 2] = 1, 2
    return tok


def _device_forward(dev, table, tokens, bag_rows, pooling, accumulate, base):
    n_bags = len(tokens) if bag_rows is None else len(bag_rows)
    L = tokens.shape[1]
    out = T(base, dev) if accumulate else torch.full((n_bags, table.shape[1]), 7.0, device=dev)
    ids = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
    inv = torch.full((n_bags,), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.embedding_bag(T(table, dev), T(tokens, dev), None if bag_rows is None else T(bag_rows, dev), pooling, out=out,
                      accumulate=accumulate, batch_ids=ids, inv=inv, oob_flag=flag)
    return out.cpu().numpy(), ids.cpu().numpy(), inv.cpu().numpy(), int(flag.item())


# ------------------------------------------------------------------------------------------ 1. forward, bit-exact
@pytest.mark.parametrize("dim", [4, 36, 128, 256])
def test_forward_is_bit_exact(dev, dim):
    """dim x L {1, 3, 16, 33} x n_bags {1, 63, 257} x three poolings x accumulate x identity / indirect bag rows.  The table
    holds a row of -0.0 (the sum starts AT the first valid row) and the indirect bag rows hold -1 (an empty bag)."""
    rng = np.random.default_rng(dim)
    buckets = 97
    table = rng.standard_normal((buckets, dim)).astype(np.float32)
    table[5] = -0.0
    for L in (1, 3, 16, 33):
        for n_bags in (1, 63, 257):
            n_rows = 50
            for indirect in (False, True):
                tokens = _tokens(rng, n_rows if indirect else n_bags, L, buckets)
                tokens[-1, 0] = 5                                   # a bag whose first (or only) valid row is the -0.0 row
                tokens[-1, 1:] = -1
                bag_rows = None
                if indirect:
                    bag_rows = rng.integers(0, n_rows, n_bags).astype(np.int64)
                    bag_rows[rng.random(n_bags) < 0.1] = -1
                    bag_rows[0] = n_rows - 1
                base = rng.standard_normal((n_bags, dim)).astype(np.float32)
                for pooling in bc.POOLINGS:
                    for accumulate in (False, True):
                        want = bc.bag_forward(table, tokens, bag_rows, pooling, accumulate, base)
                        got = _device_forward(dev, table, tokens, bag_rows, pooling, accumulate, base)
                        what = (dim, L, n_bags, indirect, pooling, accumulate)
                        assert got[3] == want[3] == 0, what
                        assert np.array_equal(got[1], want[1]), what
                        assert not _bad(got[2], want[2])[0], (what, "inv", _bad(got[2], want[2]))
                        assert not _bad(got[0], want[0])[0], (what, "out", _bad(got[0], want[0]))


def test_forward_edge_cases_flag_and_outputs(dev):
    """Out-of-range tokens and bag rows set the flag and are skipped, the rest stays exact; -1 never sets it; an all-padding bag
    and a -1 bag row leave an accumulated row untouched and write +0 otherwise; optional outputs may be left out."""
    rng = np.random.default_rng(9)
    buckets, dim, L, n_rows = 60, 128, 16, 40
    table = rng.standard_normal((buckets, dim)).astype(np.float32)
    tokens = _tokens(rng, n_rows, L, buckets)
    tokens[3] = -1
    tokens[4, :] = 11                                               # one token repeated in every slot
    bag_rows = np.array([3, -1, 4, 0, 7, 4, 39], dtype=np.int64)
    base = rng.standard_normal((len(bag_rows), dim)).astype(np.float32)
    for pooling in bc.POOLINGS:
        for accumulate in (False, True):
            want = bc.bag_forward(table, tokens, bag_rows, pooling, accumulate, base)
            got = _device_forward(dev, table, tokens, bag_rows, pooling, accumulate, base)
            assert got[3] == 0 and np.array_equal(got[1], want[1]) and not _bad(got[2], want[2])[0] and not _bad(got[0], want[0])[0]
            assert got[2][0] == 0 and got[2][1] == 0 and (got[1].reshape(-1, L)[:2] == -1).all()
            if accumulate:
                assert not _bad(got[0][:2], base[:2])[0]
            else:
                assert not bc.bits(got[0][:2]).any()                # +0, every bit clear
    # the flag: a token == buckets, a token < -1, a bag row == n_rows, a bag row < -1 - one at a time, then a clean run
    for kind in ("token_high", "token_low", "row_high", "row_low", "clean"):
        tk, br = tokens.copy(), bag_rows.copy()
        if kind == "token_high":
            tk[0, 5] = buckets
        elif kind == "token_low":
            tk[7, 0] = -2
        elif kind == "row_high":
            br[4] = n_rows
        elif kind == "row_low":
            br[4] = -3
        want = bc.bag_forward(table, tk, br, "mean", True, base)
        got = _device_forward(dev, table, tk, br, "mean", True, base)
        assert got[3] == want[3] == (0 if kind == "clean" else 1), kind
        assert np.array_equal(got[1], want[1]) and not _bad(got[2], want[2])[0] and not _bad(got[0], want[0])[0], kind
    # no optional output, no flag, a fresh out
    out = ops.embedding_bag(T(table, dev), T(tokens, dev), pooling="sqrtn")
    assert not _bad(out.cpu().numpy(), bc.bag_forward(table, tokens, pooling="sqrtn")[0])[0]
    with pytest.raises(ValueError, match="pooling"):
        ops.embedding_bag(T(table, dev), T(tokens, dev), pooling="max")
    with pytest.raises(ValueError, match="accumulate"):
        ops.embedding_bag(T(table, dev), T(tokens, dev), accumulate=True)


# ------------------------------------------------------------------------------------------ 2. backward + update, bit-exact
def _update_problem(rng, n_bags=512, L=16, buckets=50, rows=60, dim=128):
    """8192 slots over 50 buckets: every run of equal tokens crosses 64-slot blocks; token 7 fills 200 more slots; rows 50..59 of
    the table are never touched."""
    tokens = _tokens(rng, n_bags, L, buckets)
    tokens[100:300, 4] = 7
    table = rng.uniform(-0.05, 0.05, (rows, dim)).astype(np.float32)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    return table, tokens, dy


@pytest.fixture(scope="module")
def update_problem():
    return _update_problem(np.random.default_rng(77))


def _device_update(dev, opt, state, tokens, dy, pooling, step=7):
    """forward (for batch_ids / inv) -> plan -> backward launch -> the optimizer, from a copy of ``state``."""
    n_bags, L = tokens.shape
    d = [T(a, dev) for a in state]
    plan = ops.BagPlan(n_bags, L, dev)
    ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
    inv = torch.empty(n_bags, device=dev)
    ops.embedding_bag(d[0], T(tokens, dev), pooling=pooling, batch_ids=ids, inv=inv)
    plan.run(ids, state[0].shape[0])
    dyt = T(dy, dev)
    gs = plan.backward(dyt, inv, None if pooling == "sum" else torch.empty_like(dyt))
    if opt == "sgd":
        ops.sparse_sgd_(d[0], gs, plan, LR)
    elif opt == "adagrad":
        ops.sparse_adagrad_(d[0], d[1], gs, plan, LR)
    else:
        ops.adam_step_([(d[0], d[1], d[2], gs, plan)], [], ops.AdamHyper(lr=LR, step=step))
    return [t.cpu().numpy() for t in d], gs.cpu().numpy(), plan, ids.cpu().numpy(), inv.cpu().numpy()


def test_backward_gs_and_order_bags_are_bit_exact(dev, update_problem):
    table, tokens, dy = update_problem
    n_bags, L = tokens.shape
    for pooling in bc.POOLINGS:
        _, gs, plan, ids, inv = _device_update(dev, "sgd", [table], tokens, dy, pooling)
        _, want_ids, want_inv, _ = bc.bag_forward(table, tokens, pooling=pooling)
        assert np.array_equal(ids, want_ids) and not _bad(inv, want_inv)[0]
        assert not _bad(gs, bc.bag_gs(dy, want_inv, pooling))[0], pooling
        order = plan.order.cpu().numpy()
        assert np.array_equal(plan.order_bags.cpu().numpy(), order // L)
        # the plan itself: the valid slots, sorted stably by token, come first
        valid = np.flatnonzero(want_ids >= 0)
        assert np.array_equal(order[:len(valid)], valid[np.argsort(want_ids[valid], kind="stable")])
    # gs may be dy itself (in place); gs = None leaves dy alone and still fills order_bags
    dyt, invt = T(dy, dev), T(want_inv, dev)
    ob = torch.full_like(plan.order_bags, -1)
    ops.embedding_bag_bwd(dyt, invt, plan.order, L, ob, gs=dyt)
    assert not _bad(dyt.cpu().numpy(), bc.bag_gs(dy, want_inv, "sqrtn"))[0] and torch.equal(ob, plan.order_bags)
    dyt, ob = T(dy, dev), torch.full_like(plan.order_bags, -1)
    g, _ = ops.embedding_bag_bwd(dyt, None, plan.order, L, ob)
    assert g is dyt and not _bad(dyt.cpu().numpy(), dy)[0] and torch.equal(ob, plan.order_bags)


@pytest.mark.parametrize("opt,pooling", [("sgd", "sum"), ("sgd", "mean"), ("adagrad", "mean"), ("adam", "mean"), ("adam", "sqrtn")])
def test_update_is_bit_exact_lazy_and_reproducible(dev, update_problem, opt, pooling):
    table, tokens, dy = update_problem
    rng = np.random.default_rng(5)
    state = [table]
    if opt == "adagrad":
        state = [table, np.full_like(table, 0.1)]
    elif opt == "adam":
        state = [table, (rng.standard_normal(table.shape) * 0.01).astype(np.float32),
                 ((rng.standard_normal(table.shape) * 0.01) ** 2).astype(np.float32)]
    got, gs, _, ids, inv = _device_update(dev, opt, state, tokens, dy, pooling)
    assert (np.bincount(ids[ids >= 0]) >= 129).any()                       # a token repeated at least 129 times
    want = [a.copy() for a in state]
    touched = bc.bag_update(opt, want, ids, gs, tokens.shape[1], LR, step=7)    # fed the device's own gradient rows
    for g, w, name in zip(got, want, ("table", "state 1", "state 2")):
        assert not _bad(g, w)[0], (opt, pooling, name, _bad(g, w))
    rest = np.setdiff1d(np.arange(len(table)), touched)
    assert len(rest) >= 10
    for g, s0 in zip(got, state):
        assert not _bad(g[rest], s0[rest])[0]                              # untouched rows keep their bits
        assert (bc.bits(g[touched]) != bc.bits(s0[touched])).any()
    again = _device_update(dev, opt, state, tokens, dy, pooling)[0]
    for g, a in zip(got, again):
        assert not _bad(g, a)[0]                                           # two runs are bit-identical


# ------------------------------------------------------------------------------------------ 3. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=3000, n_items=2000, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **kw)


def _names(tr, title=True):
    names = ["user_table", "item_table", "dense_flat"]
    opt = tr.cfg.optimizer
    if opt == "adagrad":
        names += ["user_accum", "item_accum", "dense_accum"]
    if opt == "adam":
        names += ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]
    if title:
        names += ["title_table"] + {"sgd": [], "adagrad": ["title_accum"], "adam": ["title_m", "title_v"]}[opt]
    return names


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_trainer_with_one_token_sum_pooling_is_the_category_feature_bit_for_bit(dev, monkeypatch, opt):
    """L = 1, sum pooling, every item's token = its category: the pooled row IS the category row, its gradient the item-tower
    input gradient - so loss and every parameter equal the category-feature trainer's on the unfused path, bit for bit."""
    monkeypatch.setenv("TT_FUSE_LOOKUP", "0")
    monkeypatch.setenv("TT_COMPOSITE_STEP", "0")
    seed, nb = 31, 30
    a = TwoTowerTrainer(_cfg(opt, n_category_buckets=nb), dev, seed=seed)
    b = TwoTowerTrainer(_cfg(opt, n_title_buckets=nb, title_max_tokens=1, title_pooling="sum"), dev, seed=seed)
    assert not a.fuse_lookup and not a.use_composite and not b.fuse_lookup
    b.title_table.copy_(a.cat_table)                                        # the same initial table
    init = a.cat_table.clone()
    item_cat = torch.from_numpy(np.random.default_rng(seed).integers(0, nb, 2000)).to(dev)
    b.set_item_titles(item_cat.to(torch.int32).view(-1, 1))
    for step in range(3):
        u, i = a.synthetic_batch(seed, step, "Z")
        la = a.step(u, i, category_ids=item_cat[i]).clone()
        lb = b.step(u, i).clone()
        assert torch.equal(la, lb), (step, la.item(), lb.item())
    a.check_ids(); b.check_ids()
    pairs = [(k, k) for k in _names(a, title=False)] + [("cat_table", "title_table")]
    pairs += {"sgd": [], "adagrad": [("cat_accum", "title_accum")], "adam": [("cat_m", "title_m"), ("cat_v", "title_v")]}[opt]
    for ka, kb in pairs:
        assert torch.equal(getattr(a, ka), getattr(b, kb)), (ka, kb)
    assert not torch.equal(b.title_table, init)


def _title_trainer(dev, opt="adagrad", seed=1001, pooling="mean", L=5, buckets=300, **kw):
    tr = TwoTowerTrainer(_cfg(opt, n_title_buckets=buckets, title_max_tokens=L, title_pooling=pooling, **kw), dev, seed=seed)
    tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def test_trainer_matches_the_f64_restatement_and_trains(dev):
    """L = 5, mean pooling: loss and every gradient within the project's bars (relative <= 1e-4, max-abs <= 1e-4 * max|ref|;
    DESIGN section 2) of the f64 autograd restatement given the device's ReLU masks; then 20 steps lower the loss.
    One gradient is identically zero - the item tower's last bias, which the softmax cannot see - and is held to the same
    1e-4 of the scale of the rows its sum is taken over (max|dc|)."""
    seed, batch, L = 1001, 256, 5
    tr = _title_trainer(dev, "sgd", seed)
    titles = tr.item_titles.cpu().numpy()
    assert (titles == -1).any() and (titles >= 0).sum(1).min() >= 1 and (titles >= 0).sum(1).max() == L
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table", "title_table")}
        towers = _towers64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
        r = bc.step_f64(before["user_table"], before["item_table"], before["title_table"], towers, u.cpu().numpy(), i.cpu().numpy(),
                        titles, "mean", 0.1, masks)
        print(f"step {step}: loss {loss} (f64 {r['loss']})")
        assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
        # the title table's gradient as the device holds it: the bags' scaled rows, one per valid slot
        tr.title_plan.run(tr.title_ids, tr.cfg.n_title_buckets)
        gs = tr.title_plan.backward(tr.item_tower.demb, tr.title_inv, tr.title_gs).cpu().numpy().astype(np.float64)
        ids, g = bc.slot_gradients(tr.title_ids.cpu().numpy(), gs, L)
        g_title = np.zeros_like(before["title_table"])
        np.add.at(g_title, ids, g)
        checks = [("due", tr.user_tower.demb.cpu().numpy(), r["due"]), ("die", tr.item_tower.demb.cpu().numpy(), r["die"]),
                  ("title_table", g_title, r["title_table"])]
        for t, tw in enumerate((tr.user_tower, tr.item_tower)):
            for l in range(tw.n_layers):
                checks += [(f"dw[{t}][{l}]", tw.dw_slabs[l].cpu().numpy().astype(np.float64).sum(0), r["dw"][t][l]),
                           (f"db[{t}][{l}]", tw.db_slabs[l].cpu().numpy().astype(np.float64).sum(0), r["db"][t][l])]
        last = f"db[1][{tr.item_tower.n_layers - 1}]"
        for what, got, want in checks:
            err = np.abs(got - want).max()
            scale = np.abs(want).max()
            if what == last:
                # the item tower's last bias shifts every logit of a row alike, so the in-batch softmax does not see it: its
                # gradient, the column sums of dc, is ZERO (the f64 value is rounding noise) and has no scale of its own;
                # the scale of what the device sums - the rows of dc - is the one the bar is taken from
                assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
                scale = np.abs(r["dc"]).max()
            print(f"step {step}: {what} error {err / scale:.2e} of max |g|")
            assert scale > 0 and err <= 1e-4 * scale, (step, what, err)
        tr.apply_gradients(step_ids=[u, i])        # (no plan launch ran: the optimizer launch sorts the ids itself)
    tr2 = _title_trainer(dev, "adam", seed)
    batch0 = tr2.synthetic_batch(seed, 0)
    t0 = tr2.title_table.clone()
    losses = [tr2.step(*batch0).item() for _ in range(20)]
    tr2.check_ids()
    print(f"20 steps: {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(t0, tr2.title_table)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s))
    a = _title_trainer(dev, opt, seed, dropout_rate=0.1)
    run(a, range(4))
    b = _title_trainer(dev, opt, seed, dropout_rate=0.1)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["n_title_buckets"] == 300 and sd["config"]["title_max_tokens"] == 5 and sd["config"]["title_pooling"] == "mean"
    assert sd["item_titles"].dtype == torch.int32 and tuple(sd["item_titles"].shape) == (2000, 5)
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values, no titles set
    c.load_state_dict(sd)
    run(c, range(2, 4))
    for k in _names(a) + ["item_titles", "loss"]:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    plain = TwoTowerTrainer(_cfg(opt), dev, seed=seed)
    with pytest.raises(ValueError, match="n_title_buckets"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="n_title_buckets"):
        c.load_state_dict(plain.state_dict())
    old = {k: v for k, v in plain.state_dict().items()}
    old["config"] = {k: v for k, v in old["config"].items() if not k.startswith(("n_title", "title_"))}
    plain.load_state_dict(old)                                                       # a checkpoint from before the feature


def test_item_corpus_embeddings_equal_the_training_path(dev):
    """700 items at batch 256 (three chunks, the last ragged): the corpus rows of a batch's items against the item-tower outputs
    of ``evaluate`` on that batch (1e-4 of max|ref|: two GEMM launch shapes), and the tower INPUT rows - item row + pooled
    titles - of both paths against the restatement, bit for bit."""
    seed = 23
    tr = _title_trainer(dev, "sgd", seed, n_items=700, pooling="sqrtn")
    for s in range(3):
        tr.step(*tr.synthetic_batch(seed, s))
    u, i = tr.synthetic_batch(seed, 5)
    table, titles, items = tr.title_table.cpu().numpy(), tr.item_titles.cpu().numpy(), tr.item_table.cpu().numpy()
    tr.evaluate(u, i)
    want_in = bc.bag_forward(table, titles, i.cpu().numpy(), "sqrtn", True, items[i.cpu().numpy()])[0]
    assert not _bad(tr.item_tower.acts[0].cpu().numpy(), want_in)[0]
    c_train = tr.item_tower.acts[-1].clone()
    corpus = tr.item_corpus_embeddings()
    tr.check_ids()
    last = bc.bag_forward(table, titles[512:], None, "sqrtn", True, items[512:])[0]
    assert not _bad(tr.item_tower.acts[0][:188].cpu().numpy(), last)[0]
    assert corpus.shape == (700, 32)
    err = (corpus[i] - c_train).abs().max().item()
    assert err <= 1e-4 * c_train.abs().max().item(), err
    plain = TwoTowerTrainer(_cfg("sgd", n_items=700), dev, seed=seed)
    plain.load_state_dict({**plain.state_dict(), "user_table": tr.user_table, "item_table": tr.item_table, "dense": tr.dense_flat})
    assert (plain.item_corpus_embeddings() - corpus).abs().max().item() > 1e-3      # the titles do reach the corpus


def test_evaluate_between_backward_and_update_leaves_the_update_alone(dev):
    """An inference pass writes none of the buffers a train step keeps for ``apply_gradients`` - the titles' and the history's
    slot tokens and pooling scales: forward_backward, evaluate on ANOTHER batch, apply_gradients trains every table and
    dense_flat to the bits of the same step without the evaluate in between."""
    seed, b, lh = 29, 64, 5
    cfg = _cfg("sgd", batch=b, n_users=300, n_items=200, n_title_buckets=50, title_max_tokens=4, user_history_len=lh, history_pooling="mean")
    rng = np.random.default_rng(seed)
    histories = rng.integers(-1, cfg.n_items, (cfg.n_users, lh)).astype(np.int32)

    def fresh():
        tr = TwoTowerTrainer(TwoTowerConfig(**cfg.__dict__), dev, seed=seed)
        tr.set_item_titles(tr.synthetic_item_titles(seed))
        tr.set_user_histories(T(histories, dev))
        return tr
    a, c = fresh(), fresh()
    (u0, i0), (u1, i1) = a.synthetic_batch(seed, 0, "Z"), a.synthetic_batch(seed, 1, "Z")
    assert not torch.equal(i0, i1) and not torch.equal(u0, u1)
    a.forward_backward(u0, i0)
    a.apply_gradients(step_ids=[u0, i0])
    c.forward_backward(u0, i0)
    c.evaluate(u1, i1)
    c.apply_gradients(step_ids=[u0, i0])
    a.check_ids(); c.check_ids()
    assert set(a.tables) == {"user", "item", "title", "history"}
    init = fresh()
    for k in [f"{p}_table" for p in a.tables] + ["dense_flat"]:
        assert torch.equal(getattr(a, k), getattr(c, k)), k
        assert not torch.equal(getattr(a, k), getattr(init, k)), k             # (and the step did train it)


# ------------------------------------------------------------------------------------------ 4. custom op, CLIs, refusals
def test_custom_op_passes_opcheck_and_equals_the_ops_call(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(3)
    table = T(rng.standard_normal((80, 64)).astype(np.float32), dev)
    tokens = T(_tokens(rng, 33, 6, 80), dev)
    rows = T(rng.integers(-1, 33, 50).astype(np.int64), dev)
    for args in ((table, tokens, None, "mean"), (table, tokens, rows, "sqrtn")):
        torch.library.opcheck(torch.ops.twotower.embedding_bag, args)
        assert torch.equal(torch.ops.twotower.embedding_bag(*args), ops.embedding_bag(table, tokens, args[2], args[3]))


def test_train_cli_runs_with_titles_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  features:\n    title:\n      max_tokens: 6\n      pooling: sqrtn\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck, recs = tmp_path / "title.pt", tmp_path / "recs.parquet"
    with contextlib.redirect_stdout(io.StringIO()):                        # 600 pairs, 10 % held out: 2 training steps
        assert train.main(["--config", str(cfgp), "--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200",
                           "--optimizer", "adam", "--title-buckets", "100", "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 2 and sd["adam_step"] == 3
    assert (sd["config"]["n_title_buckets"], sd["config"]["title_max_tokens"], sd["config"]["title_pooling"]) == (100, 6, "sqrtn")
    assert tuple(sd["title_table"].shape) == (100, 32) and tuple(sd["item_titles"].shape) == (200, 6)
    assert sd["title_m"].any().item() and (sd["item_titles"] >= 0).any().item()
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
    got = pq.read_table(recs).to_pydict()
    assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all()


def test_graph_capture_and_the_sharded_trainer_refuse_the_feature(dev):
    tr = _title_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="title"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises((NotImplementedError, ValueError), match="title"):
        ShardedTwoTowerTrainer(_cfg("sgd", n_title_buckets=100), dev, seed=1)
    with pytest.raises(ValueError, match="n_title_buckets"):
        TwoTowerTrainer(_cfg("sgd"), dev, seed=1).set_item_titles(torch.zeros(2000, 16, dtype=torch.int32, device=dev))

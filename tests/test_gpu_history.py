"""The pooled user-history feature on the GPU (tt_history_bag_fwd_f32, csrc/bag.hip): the leave-one-out / base-row forward launch
against the restatement of tests/history_check.py BIT FOR BIT and against the existing bag and gather launches, the flags, the
history table's update, then the trainer - parity with the f64 autograd restatement, training, checkpoints, the inference
paths - the custom op, the CLIs and the refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import bag_check as bc
import history_check as hc
from two_tower_amazon_recommender_amd import data, ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bad(got, want):
    b = bc.bits(got) != bc.bits(want)
    return int(b.sum()), np.argwhere(b)[:4].tolist()


def _problem(rng, n_rows, n_bags, L, rows, indirect):
    """(tokens [n_rows, L], bag_rows or None, exclude [n_bags]).  Tokens lie in [0, rows - 1): token rows - 1 stands in no bag.
    Bags 0..7 are the special cases (bag b pools token row b, bag 7 - indirect only - the row -1):
      0 padding in the middle, an exclude value that is in range and matches nothing     4 as 1, but exclude = -1
      1 one token in every slot, excluded: a repeated match and an emptied bag           5 exclude >= rows (matches nothing, no flag)
      2 the match in the first valid slot (L >= 3: behind a padding slot)                6 random tokens, the in-range no-match value
      3 the match in the last valid slot (L >= 3: in front of a padding slot)
    The other bags exclude a slot of their own row (a padding slot: -1) half of the time, a random item otherwise."""
    tok = rng.integers(0, rows - 1, (n_rows, L)).astype(np.int32)
    tok[rng.random((n_rows, L)) < 0.25] = -1
    tok[8:][rng.random(n_rows - 8) < 0.1] = -1
    tok[0:7] = rng.integers(0, rows - 1, (7, L))
    tok[1], tok[4] = 11, 12
    tok[2, -1] = tok[2, 0]                                  # (L >= 3: the match found first is not the only one)
    tok[2, 1:-1] = np.where(tok[2, 1:-1] == tok[2, 0], tok[2, 0] + 1, tok[2, 1:-1])
    if L >= 3:
        tok[0, 1] = -1
        tok[2, 0], tok[2, 1], tok[2, -1] = -1, 21, 22
        tok[2, 2:-1] = np.where(tok[2, 2:-1] == 21, 23, tok[2, 2:-1])
        tok[3, -1], tok[3, -2] = -1, 31
        tok[3, :-2] = np.where(tok[3, :-2] == 31, 32, tok[3, :-2])
    bag_rows = None
    if indirect:
        bag_rows = rng.integers(0, n_rows, n_bags).astype(np.int64)
        bag_rows[rng.random(n_bags) < 0.08] = -1
        bag_rows[:8] = [0, 1, 2, 3, 4, 5, 6, -1]
    br = np.arange(n_bags) if bag_rows is None else bag_rows
    own = tok[np.maximum(br, 0), rng.integers(0, L, n_bags)].astype(np.int64)
    exclude = np.where(rng.random(n_bags) < 0.5, own, rng.integers(0, rows, n_bags))
    first3 = tok[3][tok[3] >= 0]
    exclude[:7] = [rows - 1, 11, tok[2][tok[2] >= 0][0], first3[-1], -1, rows + 5, rows - 1]
    return tok, bag_rows, exclude.astype(np.int64)


def _assert_cases(tok, bag_rows, exclude, rows, L):
    """The inputs hold every case the kernel can meet (those that exist at this L)."""
    per, _ = hc.mask_tokens(tok, bag_rows, None)
    valid = per >= 0
    match = valid & (per.astype(np.int64) == exclude[:, None])
    nv, nm = valid.sum(1), match.sum(1)
    first = np.argmax(valid, 1)
    last = L - 1 - np.argmax(valid[:, ::-1], 1)
    rng_ = np.arange(len(per))
    assert ((nv > 0) & (nm == 0)).any()                                             # a bag with no match
    assert ((nv > 0) & match[rng_, first]).any() and ((nv > 0) & match[rng_, last]).any()   # first / last valid slot
    assert ((nv > 0) & (nm == nv)).any()                                            # all valid slots match: an emptied bag
    assert ((exclude == -1) & (nv > 0)).any() and ((exclude >= rows) & (nv > 0)).any()
    if bag_rows is not None:
        assert (bag_rows == -1).any()
    if L >= 3:
        assert (nm >= 2).any()                                                      # a repeated match
        assert (valid[:, :-2] & ~valid[:, 1:-1] & valid[:, 2:]).any()               # padding in the middle of a row
        assert ((nv > 1) & (nm == 1) & match[rng_, first] & (first > 0)).any()
        assert ((nv > 1) & (nm == 1) & match[rng_, last] & (last < L - 1)).any()


def _device_forward(dev, table_t, tokens, bag_rows, exclude, base_t, pooling, accumulate, out0):
    n_bags = len(tokens) if bag_rows is None else len(bag_rows)
    L = tokens.shape[1]
    out = T(out0, dev) if accumulate else torch.full((n_bags, table_t.shape[1]), 7.0, device=dev)
    ids = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
    inv = torch.full((n_bags,), -7.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.history_bag(table_t, T(tokens, dev), T(bag_rows, dev), T(exclude, dev), base_t, pooling, out=out, accumulate=accumulate,
                    batch_ids=ids, inv=inv, oob_flag=flag)
    return out.cpu().numpy(), ids.cpu().numpy(), inv.cpu().numpy(), int(flag.item())


# ------------------------------------------------------------------------------------------ 1. forward, bit-exact
@pytest.mark.parametrize("dim", [4, 36, 128, 256, 516, 1024])
def test_forward_is_bit_exact(dev, dim):
    """dim (every lane-group width, a partly filled group, NV 1..4) x {37, 300} bags x L {1, 7, 37} x three poolings x
    {plain, accumulate, base} x identity / indirect bag rows (50 token rows), always with ``exclude``."""
    rng = np.random.default_rng(dim)
    rows, n_rows = 97, 50
    table = rng.standard_normal((rows, dim)).astype(np.float32)
    table[5] = -0.0
    base_table = rng.standard_normal((40, dim)).astype(np.float32)
    base_table[2] = -0.0
    table_t, base_table_t = T(table, dev), T(base_table, dev)
    for L in (1, 7, 37):
        for n_bags in (37, 300):
            for indirect in (False, True):
                tok, bag_rows, exclude = _problem(rng, n_rows if indirect else n_bags, n_bags, L, rows, indirect)
                _assert_cases(tok, bag_rows, exclude, rows, L)
                base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
                base_ids[1] = 2                                      # the emptied bag's base row is the -0.0 row: written as it is
                out0 = rng.standard_normal((n_bags, dim)).astype(np.float32)
                for pooling in hc.POOLINGS:
                    for mode in ("plain", "accumulate", "base"):
                        base = (base_table, base_ids) if mode == "base" else None
                        base_t = (base_table_t, T(base_ids, dev)) if mode == "base" else None
                        acc = mode == "accumulate"
                        want = hc.history_forward(table, tok, bag_rows, exclude, base, pooling, acc, out0)
                        got = _device_forward(dev, table_t, tok, bag_rows, exclude, base_t, pooling, acc, out0)
                        what = (dim, L, n_bags, indirect, pooling, mode)
                        assert got[3] == want[3] == 0, what                 # (an exclude value >= rows sets no flag)
                        assert np.array_equal(got[1], want[1]), what
                        assert not _bad(got[2], want[2])[0], (what, "inv", _bad(got[2], want[2]))
                        assert not _bad(got[0], want[0])[0], (what, "out", _bad(got[0], want[0]))
                        # the emptied bag: scale 0; the base row, the untouched row, or +0
                        assert got[2][1] == 0 and (got[1].reshape(n_bags, L)[1] == -1).all(), what
                        row1 = {"plain": np.zeros(dim, np.float32), "accumulate": out0[1], "base": base_table[2]}[mode]
                        assert not _bad(got[0][1], row1)[0], what


# ------------------------------------------------------------------------------------------ 2. against the existing launches
@pytest.mark.parametrize("dim", [36, 128, 516])
def test_equivalences_with_the_existing_kernels(dev, dim):
    rng = np.random.default_rng(100 + dim)
    rows, n_rows, n_bags, L = 97, 50, 300, 7
    table_t = T(rng.standard_normal((rows, dim)).astype(np.float32), dev)
    base_table_t = T(rng.standard_normal((40, dim)).astype(np.float32), dev)
    tok, bag_rows, exclude = _problem(rng, n_rows, n_bags, L, rows, True)
    per, _ = hc.mask_tokens(tok, bag_rows, exclude)                          # the pre-masked matrix, one row per bag
    base_ids = T(rng.integers(-1, 40, n_bags).astype(np.int64), dev)
    tok_t, br_t, ex_t, per_t = T(tok, dev), T(bag_rows, dev), T(exclude, dev), T(per, dev)

    def run(fn, *a, **kw):
        out = kw.pop("out", None)
        out = torch.full((n_bags, dim), 7.0, device=dev) if out is None else out
        ids = torch.full((n_bags * L,), -7, dtype=torch.int64, device=dev)
        inv = torch.full((n_bags,), -7.0, device=dev)
        fn(*a, out=out, batch_ids=ids, inv=inv, **kw)
        return out, ids, inv

    for pooling in hc.POOLINGS:
        # exclude=None, base=None: the bag launch itself
        a = run(ops.history_bag, table_t, tok_t, br_t, pooling=pooling)
        b = run(ops.embedding_bag, table_t, tok_t, br_t, pooling=pooling)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), pooling
        # with exclude: the bag launch on the pre-masked token matrix (plain and accumulating)
        a = run(ops.history_bag, table_t, tok_t, br_t, ex_t, pooling=pooling)
        b = run(ops.embedding_bag, table_t, per_t, None, pooling=pooling)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), pooling
        o0 = torch.randn(n_bags, dim, device=dev)
        a = run(ops.history_bag, table_t, tok_t, br_t, ex_t, pooling=pooling, accumulate=True, out=o0.clone())
        b = run(ops.embedding_bag, table_t, per_t, None, pooling=pooling, accumulate=True, out=o0.clone())
        assert all(torch.equal(x, y) for x, y in zip(a, b)), pooling
        # with base: the gather launch followed by the accumulating bag launch
        for ex, tk, br in ((None, tok_t, br_t), (ex_t, per_t, None)):
            a = run(ops.history_bag, table_t, tok_t, br_t, ex, (base_table_t, base_ids), pooling=pooling)
            g = ops.embedding_gather(base_table_t, base_ids)
            b = run(ops.embedding_bag, table_t, tk, br, pooling=pooling, accumulate=True, out=g)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (pooling, ex is None)


# ------------------------------------------------------------------------------------------ 3. flags
def test_flags_and_argument_checks(dev):
    rng = np.random.default_rng(9)
    rows, dim, L, n_rows, n_bags = 60, 128, 7, 50, 37
    table = rng.standard_normal((rows, dim)).astype(np.float32)
    base_table = rng.standard_normal((40, dim)).astype(np.float32)
    table_t, base_table_t = T(table, dev), T(base_table, dev)
    tok, bag_rows, exclude = _problem(rng, n_rows, n_bags, L, rows, True)
    base_ids = rng.integers(0, 40, n_bags).astype(np.int64)
    for kind in ("token_high", "token_low", "row_high", "row_low", "base_high", "base_low", "base_minus_one", "clean"):
        tk, br, bi = tok.copy(), bag_rows.copy(), base_ids.copy()
        if kind == "token_high":
            tk[6, 2] = rows
        elif kind == "token_low":
            tk[6, 0] = -2
        elif kind == "row_high":
            br[9] = n_rows
        elif kind == "row_low":
            br[9] = -3
        elif kind == "base_high":
            bi[4] = 40
        elif kind == "base_low":
            bi[4] = -2
        elif kind == "base_minus_one":
            bi[4] = -1
        want = hc.history_forward(table, tk, br, exclude, (base_table, bi), "mean")
        got = _device_forward(dev, table_t, tk, br, exclude, (base_table_t, T(bi, dev)), "mean", False, None)
        assert got[3] == want[3] == (0 if kind in ("clean", "base_minus_one") else 1), kind
        assert np.array_equal(got[1], want[1]) and not _bad(got[2], want[2])[0] and not _bad(got[0], want[0])[0], kind
        if kind.startswith("base_"):            # a zero base row: the row is the pooled term alone
            alone = hc.history_forward(table, tk, br, exclude, None, "mean")[0][4]
            assert np.array_equal(got[0][4], np.float32(0) + alone), kind
        if kind.startswith("row_"):             # an empty bag: the base row itself
            assert not _bad(got[0][9], base_table[bi[9]])[0] and got[2][9] == 0, kind
    # no optional output, a fresh out
    out = ops.history_bag(table_t, T(tok, dev), T(bag_rows, dev), T(exclude, dev), (base_table_t, T(base_ids, dev)), "sqrtn")
    assert not _bad(out.cpu().numpy(), hc.history_forward(table, tok, bag_rows, exclude, (base_table, base_ids), "sqrtn")[0])[0]
    with pytest.raises(ValueError, match="pooling"):
        ops.history_bag(table_t, T(tok, dev), pooling="max")
    with pytest.raises(ValueError, match="accumulate"):
        ops.history_bag(table_t, T(tok, dev), T(bag_rows, dev), base=(base_table_t, T(base_ids, dev)), accumulate=True, out=out)
    with pytest.raises(RuntimeError, match="exclude"):
        ops.history_bag(table_t, T(tok, dev), T(bag_rows, dev), T(exclude[:-1], dev))
    with pytest.raises(RuntimeError, match="base"):
        ops.history_bag(table_t, T(tok, dev), T(bag_rows, dev), base=(base_table_t, T(base_ids[:-1], dev)))


# ------------------------------------------------------------------------------------------ 4. the update
@pytest.fixture(scope="module")
def update_problem():
    """512 bags, L 16, 60 rows (rows 50..59 stand in no bag), dim 128.  Item 49 stands only in bags that exclude it: its row gets
    no gradient.  Item 7 fills 200 more slots (runs of equal tokens across the 64-slot blocks)."""
    rng = np.random.default_rng(77)
    n_bags, L, rows, dim = 512, 16, 60, 128
    tok = rng.integers(0, 50, (n_bags, L)).astype(np.int32)
    tok[rng.random((n_bags, L)) < 0.3] = -1
    tok[100:300, 4] = 7
    own = tok[np.arange(n_bags), rng.integers(0, L, n_bags)].astype(np.int64)
    exclude = np.where(rng.random(n_bags) < 0.5, own, rng.integers(0, 50, n_bags))
    exclude[(tok == 49).any(1)] = 49
    table = rng.uniform(-0.05, 0.05, (rows, dim)).astype(np.float32)
    dy = (rng.standard_normal((n_bags, dim)) * 0.01).astype(np.float32)
    return table, tok, exclude.astype(np.int64), dy


@pytest.mark.parametrize("opt,pooling", [("sgd", "sum"), ("adagrad", "mean"), ("adam", "sqrtn")])
def test_update_after_the_excluding_forward_is_bit_exact(dev, update_problem, opt, pooling):
    table, tok, exclude, dy = update_problem
    n_bags, L = tok.shape
    rng = np.random.default_rng(5)
    state = [table]
    if opt == "adagrad":
        state = [table, np.full_like(table, 0.1)]
    elif opt == "adam":
        state = [table, (rng.standard_normal(table.shape) * 0.01).astype(np.float32),
                 ((rng.standard_normal(table.shape) * 0.01) ** 2).astype(np.float32)]
    d = [T(a, dev) for a in state]
    plan = ops.BagPlan(n_bags, L, dev)
    ids = torch.empty(n_bags * L, dtype=torch.int64, device=dev)
    inv = torch.empty(n_bags, device=dev)
    ops.history_bag(d[0], T(tok, dev), exclude=T(exclude, dev), pooling=pooling, batch_ids=ids, inv=inv)
    plan.run(ids, table.shape[0])
    dyt = T(dy, dev)
    gs = plan.backward(dyt, inv, None if pooling == "sum" else torch.empty_like(dyt))
    if opt == "sgd":
        ops.sparse_sgd_(d[0], gs, plan, LR)
    elif opt == "adagrad":
        ops.sparse_adagrad_(d[0], d[1], gs, plan, LR)
    else:
        ops.adam_step_([(d[0], d[1], d[2], gs, plan)], [], ops.AdamHyper(lr=LR, step=7))
    _, want_ids, want_inv, _ = hc.history_forward(table, tok, None, exclude, None, pooling)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and not _bad(inv.cpu().numpy(), want_inv)[0]
    want_gs = bc.bag_gs(dy, want_inv, pooling)
    assert not _bad(gs.cpu().numpy(), want_gs)[0]
    assert (tok == 49).any() and not (want_ids == 49).any() and (want_ids == 48).any()
    assert ((tok.reshape(-1) >= 0) & (want_ids == -1)).sum() > 100                     # slots that lost their gradient
    want = [a.copy() for a in state]
    touched = bc.bag_update(opt, want, want_ids, want_gs, L, LR, step=7)
    for g, w, name in zip(d, want, ("table", "state 1", "state 2")):
        assert not _bad(g.cpu().numpy(), w)[0], (opt, pooling, name, _bad(g.cpu().numpy(), w))
    rest = np.setdiff1d(np.arange(len(table)), touched)
    assert 49 in rest and len(rest) == 11
    for g, s0 in zip(d, state):
        g = g.cpu().numpy()
        assert not _bad(g[rest], s0[rest])[0]                                          # row 49 and rows 50..59 keep their bits
        assert (bc.bits(g[touched]) != bc.bits(s0[touched])).any()


# ------------------------------------------------------------------------------------------ 5. trainer
def _cfg(opt, batch=256, dim=32, tower_dims=(64, 32), n_users=300, n_items=2000, **kw):
    return TwoTowerConfig(n_users=n_users, n_items=n_items, embedding_dim=dim, tower_dims=list(tower_dims), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **kw)


def _history_trainer(dev, opt="adagrad", seed=1001, pooling="mean", L=5, batches=2, **kw):
    """Histories from the pairs of the first synthetic batches (``data.user_histories``, file order): the steps' positives are
    in them."""
    tr = TwoTowerTrainer(_cfg(opt, user_history_len=L, history_pooling=pooling, **kw), dev, seed=seed)
    pairs = [tr.synthetic_batch(seed, s, "Z") for s in range(batches)]
    u = torch.cat([p[0] for p in pairs]).cpu().numpy()
    i = torch.cat([p[1] for p in pairs]).cpu().numpy()
    tr.set_user_histories(T(data.user_histories(u, i, tr.cfg.n_users, L), dev))
    if tr.title_table is not None:
        tr.set_item_titles(tr.synthetic_item_titles(seed))
    return tr


def _towers64(tr):
    flat = tr.dense_flat.cpu().numpy().astype(np.float64)
    cut = lambda t: flat[t.storage_offset():t.storage_offset() + t.numel()].reshape(tuple(t.shape))
    return tuple(([cut(w) for w in tw.w], [cut(b) for b in tw.b]) for tw in (tr.user_tower, tr.item_tower))


def test_trainer_matches_the_f64_restatement_and_trains(dev):
    """L = 5, mean pooling: loss and every gradient - the history table's included - within the project's bars (relative
    <= 1e-4, max-abs <= 1e-4 * max|ref|) of the f64 autograd restatement given the device's ReLU masks; then
    20 Adam steps lower the loss.  The item tower's last bias gradient is identically zero under the in-batch softmax and is
    held to 1e-4 of the scale of the rows its sum is taken over (max|dc|), as in the title feature's test."""
    seed, batch, L = 1001, 256, 5
    tr = _history_trainer(dev, "sgd", seed)
    assert not tr.fuse_lookup
    hist = tr.user_history.cpu().numpy()
    for step in range(2):
        u, i = tr.synthetic_batch(seed, step, "Z")
        un, inn = u.cpu().numpy(), i.cpu().numpy()
        valid = hist[un] >= 0
        match = valid & (hist[un] == inn[:, None])
        print(f"step {step}: {int(match.any(1).sum())} bags lost a slot, {int((match.sum(1) == valid.sum(1)).sum())} were emptied")
        assert match.any() and (valid.any(1) & (match.sum(1) == valid.sum(1))).any() and (valid & ~match).any()
        before = {k: getattr(tr, k).cpu().numpy().astype(np.float64) for k in ("user_table", "item_table", "history_table")}
        towers = _towers64(tr)
        loss = tr.forward_backward(u, i).item()
        tr.check_ids()
        masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (tr.user_tower, tr.item_tower))
        r = hc.step_f64(before["user_table"], before["item_table"], before["history_table"], towers, un, inn, hist, "mean", 0.1, masks)
        print(f"step {step}: loss {loss} (f64 {r['loss']})")
        assert abs(loss - r["loss"]) <= 1e-4 * abs(r["loss"]) and abs(loss - r["loss"]) / batch <= 1e-4, (loss, r["loss"])
        # the leave-one-out rule reached the device's slots
        assert np.array_equal(tr.history_ids.cpu().numpy().reshape(batch, L), np.where(valid & ~match, hist[un], -1))
        # the history table's gradient as the device holds it: the bags' scaled rows, one per kept slot
        tr.history_plan.run(tr.history_ids, tr.cfg.n_items)
        gs = tr.history_plan.backward(tr.user_tower.demb, tr.history_inv, tr.history_gs).cpu().numpy().astype(np.float64)
        ids, g = bc.slot_gradients(tr.history_ids.cpu().numpy(), gs, L)
        g_hist = np.zeros_like(before["history_table"])
        np.add.at(g_hist, ids, g)
        g_user = np.zeros_like(before["user_table"])
        np.add.at(g_user, un, tr.user_tower.demb.cpu().numpy().astype(np.float64))
        checks = [("due", tr.user_tower.demb.cpu().numpy(), r["due"]), ("die", tr.item_tower.demb.cpu().numpy(), r["die"]),
                  ("history_table", g_hist, r["history_table"]), ("user_table", g_user, r["user_table"])]
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
    tr2 = _history_trainer(dev, "adam", seed)
    batch0 = tr2.synthetic_batch(seed, 0, "Z")
    t0 = tr2.history_table.clone()
    losses = [tr2.step(*batch0).item() for _ in range(20)]
    tr2.check_ids()
    print(f"20 steps: {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not torch.equal(t0, tr2.history_table)


def _names(tr):
    opt = tr.cfg.optimizer
    names = ["user_table", "item_table", "dense_flat", "history_table", "user_history", "title_table", "item_titles", "loss"]
    if opt == "adagrad":
        names += ["user_accum", "item_accum", "dense_accum", "history_accum", "title_accum"]
    if opt == "adam":
        names += ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "history_m", "history_v", "title_m", "title_v"]
    return names


# ------------------------------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_checkpoint_round_trip_continues_bit_identically(dev, opt):
    seed = 17
    kw = dict(dropout_rate=0.1, n_title_buckets=300, title_max_tokens=5)

    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(seed, s, "Z"))
    a = _history_trainer(dev, opt, seed, **kw)
    run(a, range(4))
    b = _history_trainer(dev, opt, seed, **kw)
    run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.state_dict().items()}
    assert sd["config"]["user_history_len"] == 5 and sd["config"]["history_pooling"] == "mean"
    assert sd["user_history"].dtype == torch.int32 and tuple(sd["user_history"].shape) == (300, 5)
    assert tuple(sd["history_table"].shape) == (2000, 32)
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=seed + 1)          # other initial values, no histories set
    c.load_state_dict(sd)
    run(c, range(2, 4))
    a.check_ids(); c.check_ids()
    for k in _names(a):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert not torch.equal(a.history_table, b.history_table)
    # a mismatch of user_history_len is refused in either direction; a checkpoint from before the feature loads
    other = TwoTowerTrainer(_cfg(opt, **kw), dev, seed=seed)
    other.set_item_titles(other.synthetic_item_titles(seed))
    with pytest.raises(ValueError, match="user_history_len"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="user_history_len"):
        c.load_state_dict(other.state_dict())
    longer = TwoTowerTrainer(_cfg(opt, user_history_len=6, **kw), dev, seed=seed)
    with pytest.raises(ValueError, match="user_history_len"):
        longer.load_state_dict(sd)
    sums = TwoTowerTrainer(_cfg(opt, user_history_len=5, history_pooling="sum", **kw), dev, seed=seed)
    with pytest.raises(ValueError, match="history_pooling"):
        sums.load_state_dict(sd)
    old = dict(other.state_dict())
    old["config"] = {k: v for k, v in old["config"].items() if k not in ("user_history_len", "history_pooling")}
    other.load_state_dict(old)


# ------------------------------------------------------------------------------------------ 7. inference
def test_inference_paths_pool_the_full_history(dev):
    """``evaluate``, ``user_embeddings`` (700 ids at batch 256: three chunks, the last ragged) and ``evaluate_topk`` feed the user
    tower user row + the pooled FULL history - nothing left out - bit for bit the restatement; a trainer loaded without the
    feature gives other embeddings."""
    from two_tower_amazon_recommender_amd.metrics import FactorizedTopK
    seed = 23
    tr = _history_trainer(dev, "sgd", seed, pooling="sqrtn", batches=3)
    for s in range(3):
        tr.step(*tr.synthetic_batch(seed, s, "Z"))
    u, i = tr.synthetic_batch(seed, 1, "Z")
    table, hist, users = tr.history_table.cpu().numpy(), tr.user_history.cpu().numpy(), tr.user_table.cpu().numpy()
    un = u.cpu().numpy()
    assert (hist[un] == i.cpu().numpy()[:, None]).any()                       # the positives are there - and stay in
    want = hc.history_forward(table, hist, un, None, (users, un), "sqrtn")[0]
    train_in = hc.history_forward(table, hist, un, i.cpu().numpy(), (users, un), "sqrtn")[0]
    assert _bad(want, train_in)[0] > 0
    tr.evaluate(u, i)
    assert not _bad(tr.user_tower.acts[0].cpu().numpy(), want)[0]
    q_eval = tr.user_tower.acts[-1].clone()
    tr.user_tower.acts[0].zero_()
    tr.evaluate_topk(u, i, FactorizedTopK(ks=(5,), temperature=0.1))
    assert not _bad(tr.user_tower.acts[0].cpu().numpy(), want)[0]
    ids = torch.from_numpy(np.random.default_rng(seed).integers(0, 300, 700)).to(dev)
    emb = tr.user_embeddings(ids)
    tr.check_ids()
    idn = ids.cpu().numpy()
    last = hc.history_forward(table, hist, idn[512:], None, (users, idn[512:]), "sqrtn")[0]
    assert not _bad(tr.user_tower.acts[0][:188].cpu().numpy(), last)[0]
    assert emb.shape == (700, 32)
    err = (tr.user_embeddings(u) - q_eval).abs().max().item()
    assert err <= 1e-4 * q_eval.abs().max().item(), err
    plain = TwoTowerTrainer(_cfg("sgd"), dev, seed=seed)
    plain.load_state_dict({**plain.state_dict(), "user_table": tr.user_table, "item_table": tr.item_table, "dense": tr.dense_flat})
    assert (plain.user_embeddings(ids) - emb).abs().max().item() > 1e-3       # the histories do reach the queries


# ------------------------------------------------------------------------------------------ 8-10. custom op, CLIs, refusals
def test_custom_op_passes_opcheck_and_equals_the_ops_call(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(3)
    table = T(rng.standard_normal((80, 64)).astype(np.float32), dev)
    base_table = T(rng.standard_normal((30, 64)).astype(np.float32), dev)
    tok, bag_rows, exclude = _problem(rng, 33, 50, 6, 80, True)
    tok_t, rows, ex = T(tok, dev), T(bag_rows, dev), T(exclude, dev)
    base_ids = T(rng.integers(0, 30, 50).astype(np.int64), dev)
    for args in ((table, tok_t, None, None, None, None, "mean"), (table, tok_t, rows, ex, None, None, "sum"),
                 (table, tok_t, rows, ex, base_table, base_ids, "sqrtn")):
        torch.library.opcheck(torch.ops.twotower.history_bag, args)
        base = None if args[4] is None else (args[4], args[5])
        assert torch.equal(torch.ops.twotower.history_bag(*args), ops.history_bag(table, tok_t, args[2], args[3], base, args[6]))
    with pytest.raises(ValueError, match="go together"):
        torch.ops.twotower.history_bag(table, tok_t, rows, ex, base_table, None, "mean")


def test_train_cli_runs_with_histories_and_recommend_serves_from_the_checkpoint(dev, tmp_path):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow as pa
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  features:\n    history:\n      max_items: 9\n      pooling: sqrtn\n"
                    "  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    rng = np.random.default_rng(4)
    pairs = tmp_path / "pairs.parquet"
    uu, ii = rng.integers(0, 300, 600), rng.integers(0, 200, 600)
    uu[0], ii[0] = 299, 199
    pq.write_table(pa.table({"user_idx": uu, "item_idx": ii, "timestamp": rng.integers(0, 1000, 600).astype(np.float64)}), pairs)
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    for name, source in (("synthetic", ["--synthetic", "600", "--synthetic-users", "300", "--synthetic-items", "200"]),
                         ("parquet", ["--data", str(pairs)])):
        ck, recs = tmp_path / f"{name}.pt", tmp_path / f"{name}.parquet"
        with contextlib.redirect_stdout(io.StringIO()):                    # 600 pairs, 10 % held out: 2 training steps
            assert train.main(["--config", str(cfgp), *source, "--optimizer", "adam", "--history-len", "4", "--save", str(ck)]) == 0
        sd = torch.load(ck, weights_only=True)
        assert sd["step_index"] == 2 and sd["adam_step"] == 3, name
        assert (sd["config"]["user_history_len"], sd["config"]["history_pooling"]) == (4, "sqrtn"), name   # the CLI's length, the YAML's pooling
        assert tuple(sd["history_table"].shape) == (200, 32) and tuple(sd["user_history"].shape) == (300, 4), name
        assert sd["user_history"].dtype == torch.int32 and (sd["user_history"] >= 0).any().item() and sd["history_m"].any().item(), name
        assert int((sd["user_history"] >= 0).sum()) <= 540                 # the training split only
        assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
        got = pq.read_table(recs).to_pydict()
        assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all(), name
    assert recommend.main(["--checkpoint", str(ck), "--all-users", "--k", "3", "--out", str(recs)]) == 0
    got = pq.read_table(recs).to_pydict()
    assert len(got["item_idx"]) == 900 and set(got["user_idx"]) == set(range(300))


def test_refusals(dev):
    tr = _history_trainer(dev, "sgd", 1)
    with pytest.raises(NotImplementedError, match="history"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises((NotImplementedError, ValueError), match="history"):
        ShardedTwoTowerTrainer(_cfg("sgd", user_history_len=4), dev, seed=1)
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerTrainer(_cfg("sgd", user_history_len=4, candidate_sampling="mixed", n_sampled_negatives=64), dev, seed=1)
    with pytest.raises(ValueError, match="user_history_len"):
        TwoTowerTrainer(_cfg("sgd"), dev, seed=1).set_user_histories(torch.zeros(300, 5, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="int32"):
        tr.set_user_histories(torch.zeros(300, 4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="int32"):
        tr.set_user_histories(torch.zeros(300, 5, dtype=torch.int64, device=dev))

"""Mixed negative sampling on the GPU (csrc/sample.hip): the sampler launch against the restatement of tests/sample_check.py
BIT FOR BIT, then the trainer - one mixed step against the f64 restatement, the custom-op path, the updates of exactly the
candidates' rows, the title feature, reproducibility and resume, training, the refusals and the CLI."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import adam_check as ac
import bag_check as bc
import sample_check as sc
from oracle import synth, two_tower as tt
from two_tower_amazon_recommender_amd import ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

LR = 0.001
ID_SENTINEL, PROB_SENTINEL, PAD = -7777, -7.5, 64
BS = (0, 1, 64, 255)
NS = (0, 1, 63, 257, 4096)
STARTS = (0, (1 << 33) + 5)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_differ(got, want):
    return int((ac.bits(got) != ac.bits(want)).sum())


# ------------------------------------------------------------------------------------------ 1. the sampler, bit for bit
def _run_sampler(dev, pos, n_items, n_neg, start, sampler, alias_dev, freq_dev, sp_dev, seed=77, tid=10):
    n = len(pos) + n_neg
    out_ids = torch.full((n + PAD,), ID_SENTINEL, dtype=torch.int64, device=dev)
    out_prob = torch.full((n + PAD,), PROB_SENTINEL, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.sample_candidates(T(pos, dev), n_items, n_neg, out_ids, out_prob, sampler=sampler, alias=alias_dev, item_freq=freq_dev,
                          sampler_prob=sp_dev, seed=seed, tensor_id=tid, start=start, oob_flag=flag)
    return out_ids.cpu().numpy(), out_prob.cpu().numpy(), int(flag.item())


def _check_sampler(got, want_ids, want_prob, want_flag, what):
    ids, prob, flag = got
    n = len(want_ids)
    assert flag == want_flag, what
    assert np.array_equal(ids[:n], want_ids), (what, np.flatnonzero(ids[:n] != want_ids)[:4])
    assert (ids[n:] == ID_SENTINEL).all() and len(ids) == n + PAD, what
    if want_prob is None:
        assert (prob == np.float32(PROB_SENTINEL)).all(), what                # never touched without the frequencies
    else:
        assert not _bits_differ(prob[:n], want_prob), (what, np.flatnonzero(ac.bits(prob[:n]) != ac.bits(want_prob))[:4])
        assert (prob[n:] == np.float32(PROB_SENTINEL)).all(), what


@pytest.mark.parametrize("sampler", ["uniform", "alias"])
@pytest.mark.parametrize("n_items", [1, 7, 1000])
def test_sampler_is_bit_exact(dev, n_items, sampler):
    """B x N x start x (probabilities off | on | on with sampler_prob); buffers 64 entries too long, pre-filled with a sentinel."""
    rng = np.random.default_rng(n_items)
    freq = rng.random(n_items).astype(np.float32)
    freq /= freq.sum()
    freq[rng.random(n_items) < 0.2] = 0.0
    weights = 1.0 / np.arange(1, n_items + 1) ** 1.1
    weights[n_items // 2] = 0.0 if n_items > 1 else 1.0
    alias = alias_dev = None
    sp = np.full(n_items, 1.0 / n_items, dtype=np.float32) if sampler == "uniform" else (weights / weights.sum()).astype(np.float32)
    if sampler == "alias":
        alias = ops.build_alias_table(weights)
        alias_dev = (T(alias[0], dev), T(alias[1], dev))
        if n_items > 1:
            assert (alias[0] < 1).any() and (alias[1] != np.arange(n_items)).any()
    freq_dev, sp_dev = T(freq, dev), T(sp, dev)
    for b in BS:
        for n in NS:
            if b + n == 0:
                continue
            pos = rng.integers(0, n_items, b).astype(np.int64)
            for start in STARTS:
                for mode in ("off", "freq", "freq+sampler_prob"):
                    want = sc.candidates(pos, n_items, n, 77, 10, start, alias, None if mode == "off" else freq,
                                         sp if mode == "freq+sampler_prob" else None)
                    got = _run_sampler(dev, pos, n_items, n, start, sampler, alias_dev, None if mode == "off" else freq_dev,
                                       sp_dev if mode == "freq+sampler_prob" else None)
                    _check_sampler(got, *want, (n_items, sampler, b, n, start, mode))
                    assert want[2] == 0
    if sampler == "alias" and n_items == 1000:           # the alias branch is taken, and items of weight 0 are never drawn
        ids = sc.draw(77, 10, 0, 4096, n_items, alias)
        buckets = sc.draw(77, 10, 0, 4096, n_items)
        assert (ids != buckets).any() and (ids == buckets).any() and not (ids == n_items // 2).any()


def test_sampler_is_bit_exact_over_two_to_the_32_items(dev):
    """n_items = 2^32 (uniform sampler): ids beyond 2^31, and the probability vectors indexed by them.  ONE 16 GiB f32 vector
    stands for item_freq and sampler_prob: a constant everywhere but at the ids the restatement expects, which hold distinct
    values - an index computed wrongly reads the constant."""
    n_items = 1 << 32
    rng = np.random.default_rng(32)
    base = np.float32(2.0 ** -33)
    vec = torch.full((n_items,), float(base), device=dev)
    for b in BS:
        for n in NS:
            if b + n == 0:
                continue
            pos = rng.integers(0, n_items, b).astype(np.int64)
            for start in STARTS:
                ids = np.concatenate([pos, sc.draw(77, 10, start, n, n_items)])
                if n >= 63:
                    assert ids[b:].max() >= 1 << 31 and ids[b:].min() < 1 << 31                      # both halves of the range
                vals = (base * (1.0 + rng.random(len(ids)))).astype(np.float32)
                vec[T(ids, dev)] = T(vals, dev)
                at = vec[T(ids, dev)].cpu().numpy()                 # (equal ids hold the last value written)
                for mode in ("off", "freq", "freq+sampler_prob"):
                    want_prob = None if mode == "off" else sc.mixture_prob(ids, b, n, n_items, at, at if mode == "freq+sampler_prob" else None)
                    got = _run_sampler(dev, pos, n_items, n, start, "uniform", None, None if mode == "off" else vec,
                                       vec if mode == "freq+sampler_prob" else None)
                    _check_sampler(got, ids, want_prob, 0, ("2^32", b, n, start, mode))
                vec[T(ids, dev)] = float(base)
    del vec
    torch.cuda.empty_cache()


@pytest.mark.parametrize("sampler", ["uniform", "alias"])
def test_bad_positive_ids_raise_the_flag_and_pass_through(dev, sampler):
    n_items, n = 1000, 63
    rng = np.random.default_rng(3)
    freq = (rng.random(n_items) / n_items).astype(np.float32)
    alias = alias_dev = sp = None
    if sampler == "alias":
        w = rng.random(n_items)
        alias = ops.build_alias_table(w)
        alias_dev, sp = (T(alias[0], dev), T(alias[1], dev)), (w / w.sum()).astype(np.float32)
    for bad in (-1, n_items, None):
        pos = rng.integers(0, n_items, 64).astype(np.int64)
        if bad is not None:
            pos[17] = bad
        want = sc.candidates(pos, n_items, n, 5, 10, 9, alias, freq, sp)
        got = _run_sampler(dev, pos, n_items, n, 9, sampler, alias_dev, T(freq, dev), None if sp is None else T(sp, dev), seed=5)
        _check_sampler(got, *want, (sampler, bad))
        assert want[2] == (0 if bad is None else 1)
        if bad is not None:
            assert got[0][17] == bad and got[1][17] == 1.0
        got = _run_sampler(dev, pos, n_items, n, 9, sampler, alias_dev, None, None, seed=5)        # the flag without frequencies
        _check_sampler(got, want[0], None, want[2], (sampler, bad, "off"))


def test_custom_op_passes_opcheck_and_equals_the_ops_call(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(4)
    n_items = 300
    w = rng.random(n_items)
    thr, idx = (T(a, dev) for a in ops.build_alias_table(w))
    freq, sp = T((rng.random(n_items) / n_items).astype(np.float32), dev), T((w / w.sum()).astype(np.float32), dev)
    pos = T(rng.integers(0, n_items, 33).astype(np.int64), dev)
    for args in ((pos, n_items, 50, 3, 10, 7, None, None, None, None), (pos, n_items, 50, 3, 10, 7, None, None, freq, None),
                 (pos, n_items, 50, 3, 10, 7, thr, idx, freq, sp)):
        torch.library.opcheck(torch.ops.twotower.sample_candidates, args)
        ids, prob = torch.ops.twotower.sample_candidates(*args)
        alias = None if args[6] is None else (np.asarray(thr.cpu()), np.asarray(idx.cpu()))
        want = sc.candidates(pos.cpu().numpy(), n_items, 50, 3, 10, 7, alias, None if args[8] is None else freq.cpu().numpy(),
                             None if args[9] is None else sp.cpu().numpy())
        assert np.array_equal(ids.cpu().numpy(), want[0])
        assert prob.numel() == 0 if want[1] is None else not _bits_differ(prob.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------ the trainer
N_USERS, N_ITEMS, DIM, DIMS, B, SEED = 300, 500, 32, (64, 32), 64, 1001


def _cfg(opt="sgd", n_neg=37, sampler="uniform", batch=B, n_items=N_ITEMS, **kw):
    mixed = dict(candidate_sampling="mixed", n_sampled_negatives=n_neg, negative_sampler=sampler) if n_neg else {}
    return TwoTowerConfig(n_users=N_USERS, n_items=n_items, embedding_dim=DIM, tower_dims=list(DIMS), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=batch, **mixed, **kw)


def _item_freq(n_items=N_ITEMS, seed=SEED):
    """The share of every item in 20,000 power-law 'training pairs' (zero for most of the tail)."""
    counts = np.bincount(synth.ids_powerlaw(seed, synth.TID_ITEM_IDS, 20000, n_items), minlength=n_items).astype(np.float64)
    return (counts / counts.sum()).astype(np.float32)


def _expected_candidates(tr, item_ids, step):
    cfg = tr.cfg
    alias = sp = None
    if cfg.negative_sampler == "unigram":
        f = tr.item_freq.cpu().numpy().astype(np.float64)
        w = f ** cfg.unigram_power
        alias, sp = ops.build_alias_table(w), (w / w.sum()).astype(np.float32)
    freq = None if tr.item_freq is None else tr.item_freq.cpu().numpy()
    return sc.candidates(item_ids, cfg.n_items, cfg.n_sampled_negatives, tr.dropout_seed, sc.TID_SAMPLED_NEGATIVES,
                         step * cfg.n_sampled_negatives, alias, freq, sp)


def _loss_close(got, want, batch):
    return abs(got - want) / batch <= 1e-4 and abs(got - want) <= 1e-4 * abs(want)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("correction", ["off", "uniform", "unigram"])
@pytest.mark.parametrize("n_neg", [1, 37, 256])
def test_one_mixed_step_matches_the_f64_restatement(dev, n_neg, correction, normalize):
    """forward_backward at B = 64 against sample_check.mixed_step in f64 given the device's ReLU masks: loss (|d| / B <= 1e-4 and
    relative <= 1e-4), dq, dc, both towers' weight gradients and both demb (max error <= 1e-4 of max |reference|); the device's
    candidate list equals the restatement's draw exactly.  correction: off | on with the uniform | the unigram sampler."""
    sampler = "unigram" if correction == "unigram" else "uniform"
    tr = TwoTowerTrainer(_cfg("sgd", n_neg, sampler, normalize_embeddings=normalize), dev, seed=SEED)
    if correction != "off":
        tr.set_item_frequencies(_item_freq())
    step = 2
    tr.step_index = step                                                       # the sampler's counter is step * N
    u, i = tr.synthetic_batch(SEED, step, "Z")
    uid, iid = u.cpu().numpy(), i.cpu().numpy()
    ref = tt.synthetic_state(SEED, N_USERS, N_ITEMS, DIM, list(DIMS), dtype=np.float64)
    loss = tr.forward_backward(u, i).item()
    tr.check_ids()
    want_ids, want_prob, _ = _expected_candidates(tr, iid, step)
    cand = tr.cand_ids.cpu().numpy()
    assert np.array_equal(cand, want_ids) and len(cand) == B + n_neg
    if correction != "off":
        assert not _bits_differ(tr.cand_prob.cpu().numpy(), want_prob)
    # accidental hits and duplicates do occur: in-batch ones from the power-law positives, and (N >= 37) sampled ids that are
    # some query's positive or repeat each other
    hits = (cand[:B, None] == cand[None, :])
    hits[np.arange(B), np.arange(B)] = False
    assert hits[:, :B].any()
    if n_neg >= 37:
        assert hits[:, B:].any() and len(np.unique(cand[B:])) < n_neg
    ut, it = tr.user_tower, tr.item_tower
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (ut, it))
    r = sc.mixed_step(ref, uid, cand, 0.1, None if correction == "off" else want_prob.astype(np.float64), masks, normalize)
    print(f"N={n_neg} {correction} normalize={normalize}: loss {loss} (f64 {r['loss']})")
    assert _loss_close(loss, r["loss"], B), (loss, r["loss"])
    dq, dc = (ut.dunit, it.dunit) if normalize else (ut.dz[-1], it.dz[-1])
    checks = [("dq", dq.cpu().numpy(), r["dq"]), ("dc", dc.cpu().numpy(), r["dc"]),
              ("due", ut.demb.cpu().numpy(), r["due"]), ("die", it.demb.cpu().numpy(), r["die"])]
    for name, tw, dws, dbs in (("user", ut, r["udw"], r["udb"]), ("item", it, r["idw"], r["idb"])):
        for l in range(tw.n_layers):
            checks += [(f"{name} dw[{l}]", tw.dw_slabs[l].cpu().numpy().astype(np.float64).sum(0), dws[l]),
                       (f"{name} db[{l}]", tw.db_slabs[l].cpu().numpy().astype(np.float64).sum(0), dbs[l])]
    assert it.demb.shape[0] == B + n_neg and ut.demb.shape[0] == B
    for what, got, want in checks:
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        if what == f"item db[{it.n_layers - 1}]" and not normalize:
            # the item tower's last bias shifts every logit of a row alike: its gradient, the column sums of dc, is ZERO (the
            # f64 value is rounding noise); the scale of what the device sums - the rows of dc - is the one the bar is taken from
            assert scale <= 1e-9 * np.abs(r["dc"]).max(), (what, scale)
            scale = np.abs(r["dc"]).max()
        print(f"  {what}: error {err / scale:.2e} of max |g|")
        assert scale > 0 and err <= 1e-4 * scale, (what, err, scale)


@pytest.mark.parametrize("normalize", [False, True])
def test_custom_op_task_returns_the_trainers_loss(dev, normalize):
    """tasks.Retrieval on the trainer's own tower outputs, candidate ids and mixture probabilities: the same loss, same bar."""
    from two_tower_amazon_recommender_amd import tasks
    tr = TwoTowerTrainer(_cfg("sgd", 37, "unigram", normalize_embeddings=normalize), dev, seed=SEED)
    tr.set_item_frequencies(_item_freq())
    u, i = tr.synthetic_batch(SEED, 0, "Z")
    loss = tr.forward_backward(u, i).item()
    q, c = (tr.user_tower.unit, tr.item_tower.unit) if normalize else (tr.user_tower.acts[-1], tr.item_tower.acts[-1])
    assert q.shape[0] == B and c.shape[0] == B + 37
    task = tasks.Retrieval(temperature=0.1, remove_accidental_hits=True)
    got = task(q.clone(), c.clone(), candidate_ids=tr.cand_ids, candidate_sampling_probability=tr.cand_prob).item()
    print(f"normalize={normalize}: trainer {loss}, task {got}")
    assert _loss_close(got, loss, B), (got, loss)
    plain = tasks.Retrieval(temperature=0.1, remove_accidental_hits=True)(q.clone(), c.clone(), candidate_ids=tr.cand_ids).item()
    assert not _loss_close(plain, loss, B)                                      # the correction does reach the trainer's scorer


def _state_names(opt, title=False):
    per = {"sgd": [""], "adagrad": ["", "accum"], "adam": ["", "m", "v"]}[opt]
    name = lambda t, s: f"{t}_table" if s == "" else f"{t}_{s}"
    return {t: [name(t, s) for s in per] for t in (("user", "item", "title") if title else ("user", "item"))}


def _two_ulp(got, want):
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2 * np.spacing(np.abs(want))).all()


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adam"])
def test_step_updates_exactly_the_candidates_rows(dev, opt):
    """One step(): only the user rows of user_ids and the item rows of cand_ids change, in every table and optimizer state; a
    sampled-only item's row does change; fed the device's gradient rows, the new rows equal the per-optimizer restatements
    (SGD bit for bit, Adagrad within 2 ulp, lazy Adam bit for bit)."""
    n_neg = 100
    tr = TwoTowerTrainer(_cfg(opt, n_neg), dev, seed=SEED)
    names = _state_names(opt)
    before = {k: getattr(tr, k).cpu().numpy().copy() for ks in names.values() for k in ks}
    dense0 = tr.dense_flat.clone()
    u, i = tr.synthetic_batch(SEED, 0, "Z")
    tr.step(u, i)
    tr.check_ids()
    cand = tr.cand_ids.cpu().numpy()
    assert np.array_equal(cand, _expected_candidates(tr, i.cpu().numpy(), 0)[0]) and tr.step_index == 1
    assert not torch.equal(dense0, tr.dense_flat)
    only_sampled = np.setdiff1d(cand[B:], cand[:B])
    assert len(only_sampled) >= 10
    for side, ids, tower in (("user", u.cpu().numpy(), tr.user_tower), ("item", cand, tr.item_tower)):
        g = tower.demb.cpu().numpy()
        assert g.shape[0] == len(ids)
        want = [before[k].copy() for k in names[side]]
        if opt == "sgd":
            tt.sparse_sgd(want[0], ids, g, LR)
        elif opt == "adagrad":
            tt.sparse_adagrad(want[0], want[1], ids, g, LR, tr.cfg.adagrad_epsilon)
        else:
            ac.sparse_adam(want[0], want[1], want[2], ids, g, LR, 1, tr.cfg.adam_beta1, tr.cfg.adam_beta2, tr.cfg.adam_epsilon)
        touched = np.unique(ids)
        rest = np.setdiff1d(np.arange(len(before[names[side][0]])), touched)
        assert len(rest) >= 50
        for k, w in zip(names[side], want):
            got = getattr(tr, k).cpu().numpy()
            assert not _bits_differ(got[rest], before[k][rest]), (opt, k, "a row outside the step's ids changed")
            if opt == "adagrad":
                assert _two_ulp(got, w), (opt, k)
            else:
                assert not _bits_differ(got, w), (opt, k, _bits_differ(got, w))
        if side == "item":
            t0, t1 = before["item_table"], tr.item_table.cpu().numpy()
            assert (ac.bits(t1[only_sampled]) != ac.bits(t0[only_sampled])).any(axis=1).all()       # every sampled-only row moved
    if opt == "adam":
        assert tr.adam_step == 2


def test_title_feature_pools_the_candidates_titles(dev):
    """L = 3, 97 buckets: the item tower's input rows - the sampled items' too - are item row + pooled title over cand_ids, bit
    for bit; the title table changes only in tokens of candidate items."""
    n_neg, L, buckets = 37, 3, 97
    tr = TwoTowerTrainer(_cfg("adagrad", n_neg, n_title_buckets=buckets, title_max_tokens=L, title_pooling="mean"), dev, seed=SEED)
    tr.set_item_titles(tr.synthetic_item_titles(SEED))
    titles = tr.item_titles.cpu().numpy()
    item0, title0 = tr.item_table.cpu().numpy().copy(), tr.title_table.cpu().numpy().copy()
    u, i = tr.synthetic_batch(SEED, 0, "Z")
    tr.step(u, i)
    tr.check_ids()
    cand = tr.cand_ids.cpu().numpy()
    want_in, want_slots, _, _ = bc.bag_forward(title0, titles, cand, "mean", True, item0[cand])
    got_in = tr.item_tower.acts[0].cpu().numpy()
    assert got_in.shape == (B + n_neg, DIM) and not _bits_differ(got_in, want_in)
    assert not _bits_differ(got_in[B:], want_in[B:]) and np.array_equal(tr.title_ids.cpu().numpy(), want_slots)
    changed = np.flatnonzero((ac.bits(tr.title_table.cpu().numpy()) != ac.bits(title0)).any(axis=1))
    tokens = np.unique(want_slots[want_slots >= 0])
    only_sampled = np.setdiff1d(np.unique(titles[cand[B:]]), np.unique(titles[cand[:B]]))
    only_sampled = only_sampled[only_sampled >= 0]
    assert len(changed) and np.isin(changed, tokens).all() and len(tokens) < buckets
    assert len(only_sampled) and np.isin(only_sampled, changed).all()          # tokens only sampled items carry are trained


def _run(tr, steps, seed=SEED):
    for s in steps:
        tr.step(*tr.synthetic_batch(seed, s, "Z"))


def _tables(tr):
    names = ["user_table", "item_table", "dense_flat", "loss"]
    names += {"sgd": [], "adagrad": ["user_accum", "item_accum", "dense_accum"],
              "adam": ["user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v"]}[tr.cfg.optimizer]
    return {k: getattr(tr, k) for k in names}


@pytest.mark.parametrize("opt,sampler", [("adagrad", "uniform"), ("adam", "unigram")])
def test_runs_are_reproducible_and_resume_draws_the_same_negatives(dev, opt, sampler):
    def make(seed):
        tr = TwoTowerTrainer(_cfg(opt, 37, sampler, dropout_rate=0.1), dev, seed=seed)
        return tr
    freq = _item_freq()
    a, a2, b = make(SEED), make(SEED), make(SEED)
    for tr in (a, a2, b):
        tr.set_item_frequencies(freq)
    _run(a, range(6)); _run(a2, range(6)); _run(b, range(3))
    for k, v in _tables(a).items():
        assert torch.equal(v, getattr(a2, k)), k
    sd = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in b.state_dict().items()}
    assert (sd["config"]["candidate_sampling"], sd["config"]["n_sampled_negatives"], sd["config"]["negative_sampler"],
            sd["config"]["unigram_power"]) == ("mixed", 37, sampler, 0.75)
    assert torch.equal(sd["item_freq"], T(freq, dev)) and sd["step_index"] == 3
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=SEED + 1)          # other initial values, no frequencies set
    c.load_state_dict(sd)
    assert c.item_freq is not None and (c.alias is not None) == (sampler == "unigram")
    _run(c, range(3, 6))
    for k, v in _tables(a).items():
        assert torch.equal(v, getattr(c, k)), k
    assert torch.equal(a.cand_ids, c.cand_ids) and torch.equal(a.cand_prob, c.cand_prob)


def test_in_batch_checkpoints_load_and_train_as_before(dev):
    a, b = TwoTowerTrainer(_cfg("adagrad", 0), dev, seed=SEED), TwoTowerTrainer(_cfg("adagrad", 0), dev, seed=SEED)
    assert not a.mixed and a.cand_ids is None and a.item_tower.rows == B
    _run(a, range(4)); _run(b, range(2))
    sd = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in b.state_dict().items()}
    assert sd["config"]["candidate_sampling"] == "in_batch" and "item_freq" not in sd
    old = dict(sd)                                                              # a checkpoint from before the fields existed
    old["config"] = {k: v for k, v in sd["config"].items()
                     if k not in ("candidate_sampling", "n_sampled_negatives", "negative_sampler", "unigram_power")}
    for ck in (sd, old):
        c = TwoTowerTrainer(TwoTowerConfig(**ck["config"]), dev, seed=SEED + 1)
        assert c.cfg.candidate_sampling == "in_batch"
        c.load_state_dict(ck)
        _run(c, range(2, 4))
        for k, v in _tables(a).items():
            assert torch.equal(v, getattr(c, k)), k


def test_mixed_training_lowers_the_validation_loss_and_pushes_the_tail_down(dev):
    """4 fixed batches whose items all lie in the first 2000 of 3000 items, 40 steps: the in-batch loss evaluate() reports
    falls below its initial value, and the mean logit of the 1000 items no batch ever holds against the training queries is
    lower than after an in-batch run of the same length and seed (a sign test)."""
    n_items, head, steps = 3000, 2000, 40
    def make(n_neg):
        mixed = dict(candidate_sampling="mixed", n_sampled_negatives=n_neg) if n_neg else {}
        return TwoTowerTrainer(TwoTowerConfig(n_users=N_USERS, n_items=n_items, embedding_dim=DIM, tower_dims=list(DIMS),
                                              temperature=0.1, learning_rate=0.01, optimizer="adam", batch_size=B, **mixed), dev, seed=SEED)
    batches = []
    for s in range(4):
        u = torch.empty(B, dtype=torch.int64, device=dev)
        i = torch.empty(B, dtype=torch.int64, device=dev)
        ops.fill_ids_(u, SEED, synth.TID_USER_IDS, N_USERS, "U", start=s * B)
        ops.fill_ids_(i, SEED, synth.TID_ITEM_IDS, head, "U", start=s * B)
        batches.append((u, i))
    train, val = batches, batches[0]                    # the in-batch loss of a training batch, through evaluate()
    assert max(int(i.max()) for _, i in batches) < head
    tail_mean = {}
    for n_neg in (0, 256):
        tr = make(n_neg)
        v0 = tr.evaluate(*val).item()
        for s in range(steps):
            tr.step(*train[s % 4])
        tr.check_ids()
        v1 = tr.evaluate(*val).item()
        q = tr.user_embeddings(torch.cat([u for u, _ in train]))
        c = tr.item_corpus_embeddings()[head:]
        tail_mean[n_neg] = (q.double() @ c.double().t()).mean().item() / 0.1
        print(f"N={n_neg}: validation loss {v0:.3f} -> {v1:.3f}; mean tail logit {tail_mean[n_neg]:.4f}")
        assert np.isfinite(v1) and v1 < v0, (n_neg, v0, v1)
    assert tail_mean[256] < tail_mean[0], tail_mean


def test_refusals(dev):
    with pytest.raises(ValueError, match="n_category_buckets"):
        TwoTowerTrainer(_cfg("sgd", 37, n_category_buckets=30), dev, seed=1)
    tr = TwoTowerTrainer(_cfg("sgd", 37), dev, seed=1)
    with pytest.raises(NotImplementedError, match="mixed"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="mixed"):
        ShardedTwoTowerTrainer(_cfg("sgd", 37), dev, seed=1)
    u, i = tr.synthetic_batch(1, 0)
    for kw in (dict(candidate_ids=i), dict(candidate_sampling_probability=torch.full((B,), 0.01, device=dev))):
        with pytest.raises(ValueError, match="mixed"):
            tr.step(u, i, **kw)
        with pytest.raises(ValueError, match="mixed"):
            tr.forward_backward(u, i, **kw)
    assert tr.step_index == 0
    uni = TwoTowerTrainer(_cfg("sgd", 37, "unigram"), dev, seed=1)
    with pytest.raises(ValueError, match="set_item_frequencies"):
        uni.step(u, i)
    with pytest.raises(ValueError, match="in_batch"):
        TwoTowerTrainer(_cfg("sgd", 0), dev, seed=1).set_item_frequencies(_item_freq())
    with pytest.raises(ValueError, match="n_items"):
        tr.set_item_frequencies(np.ones(N_ITEMS + 1))
    tr.step(u, i, sample_weight=torch.ones(B, device=dev))                      # sample_weight is passed through
    tr.check_ids()


@pytest.mark.parametrize("sampler", ["uniform", "unigram"])
def test_train_cli_runs_mixed_and_recommend_serves_from_the_checkpoint(dev, tmp_path, sampler):
    from two_tower_amazon_recommender_amd import recommend, train
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    ck, recs = tmp_path / "mixed.pt", tmp_path / "recs.parquet"
    with contextlib.redirect_stdout(io.StringIO()):                        # 4096 pairs, 10 % held out: 14 training steps
        assert train.main(["--config", str(cfgp), "--synthetic", "4096", "--synthetic-users", "300", "--synthetic-items", "500",
                           "--candidate-sampling", "mixed", "--sampled-negatives", "64", "--negative-sampler", sampler,
                           "--correct-sampling-bias", "--save", str(ck)]) == 0
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 14
    assert (sd["config"]["candidate_sampling"], sd["config"]["n_sampled_negatives"], sd["config"]["negative_sampler"]) == ("mixed", 64, sampler)
    assert tuple(sd["item_freq"].shape) == (500,) and abs(sd["item_freq"].sum().item() - 1.0) < 1e-5
    users = tmp_path / "users.npy"
    np.save(users, np.arange(7, dtype=np.int64))
    assert recommend.main(["--checkpoint", str(ck), "--users-file", str(users), "--k", "5", "--out", str(recs)]) == 0
    got = pq.read_table(recs).to_pydict()
    assert len(got["item_idx"]) == 35 and set(got["user_idx"]) == set(range(7)) and np.isfinite(got["score"]).all()

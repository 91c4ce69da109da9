"""The streaming frequency estimator on the GPU (csrc/freq.hip): the launch against the restatement of tests/freq_check.py BIT
FOR BIT on the sketch words and the probabilities, then the trainer - in-batch steps against a plain trainer that is handed the
restatement's probabilities, a mixed step against the f64 restatement, resume, the refusals, the custom op and the CLI."""
import contextlib
import copy
import io
import itertools
import json

import numpy as np
import pytest
import torch

import freq_check as fc
import sample_check as sc
from oracle import two_tower as tt
from two_tower_amazon_recommender_amd import ops
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

SEED, TID = 77, fc.TID_FREQ_HASH_BASE
WORD_SENTINEL, PROB_SENTINEL, PAD = -7777, -7.5, 64
NS = (1, 63, 64, 257, 4096)
UPDATES = ("none", "half", "all")
MIXES = ("off", "uniform", "sampler_prob")
PATTERNS = ("equal", "three", "uniform", "out_of_range")
HASHES = (1, 2, 3, 4)
SLOTS = (1, 7, 1024, 1 << 20)
N_ITEMS = (1, 7, 1000)
FIRST_STEPS = (1, (1 << 31) - 21)
STEPS = 20
COMBOS = list(itertools.product(NS, UPDATES, MIXES, PATTERNS))          # 180: every one is run, 20 per case below


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ids(rng, pattern, n, n_items, k):
    if pattern == "equal":
        return np.full(n, rng.integers(0, n_items), dtype=np.int64)
    if pattern == "three":
        return rng.choice(rng.integers(0, n_items, 3), n).astype(np.int64)
    ids = rng.integers(0, n_items, n).astype(np.int64)
    if pattern == "out_of_range":                  # one id out of range at each end (a single id: the ends take turns)
        if n == 1:
            ids[0] = -1 if k % 2 else n_items
        else:
            ids[rng.integers(0, n)], ids[rng.integers(0, n)] = -1, n_items
            ids[0] = -1
            ids[-1] = n_items
    return ids


def _sketch(dev, hashes, slots):
    """A zeroed sketch cut out of a buffer that is PAD words longer; the tail holds a sentinel."""
    flat = torch.full((hashes * slots + PAD,), WORD_SENTINEL, dtype=torch.int64, device=dev)
    flat[:hashes * slots] = 0
    return flat, flat[:hashes * slots].view(hashes, slots)


@pytest.mark.parametrize("first_step", FIRST_STEPS)
@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("hashes", HASHES)
def test_kernel_is_bit_exact_over_twenty_steps(dev, hashes, slots, first_step):
    """20 consecutive steps carried in one sketch.  The 32 cases walk through all 180 combinations of n, n_update, mix and id
    pattern (each more than three times, under different sketch shapes) and all three n_items; mix falls back to off where it
    is not legal (n_update == 0 or == n).  Every step's probabilities and - small sketches: every step, all: after the last -
    the sketch words equal the restatement's; the 64 entries behind both buffers keep their sentinel."""
    case = (HASHES.index(hashes) * len(SLOTS) + SLOTS.index(slots)) * len(FIRST_STEPS) + FIRST_STEPS.index(first_step)
    n_items = N_ITEMS[case % 3]
    rng = np.random.default_rng(1000 + case)
    alpha = (0.01, 0.3, 1.0)[(case // 3) % 3]
    sp = rng.random(n_items).astype(np.float32)
    sp /= sp.sum(dtype=np.float32)
    sp_dev = T(sp, dev)
    flat, sketch = _sketch(dev, hashes, slots)
    last, delta = fc.new_sketch(hashes, slots)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    raised = 0
    for k in range(STEPS):
        n, upd, mix, pattern = COMBOS[(case * STEPS + k) % len(COMBOS)]
        n_update = {"none": 0, "half": n // 2, "all": n}[upd]
        mixed = mix != "off" and 1 <= n_update < n
        ids = _ids(rng, pattern, n, n_items, k)
        t = first_step + k
        out = torch.full((n + PAD,), PROB_SENTINEL, device=dev)
        got = ops.frequency_estimate_(sketch, T(ids, dev), n_update, t, alpha, n_items, out, seed=SEED, tensor_id=TID,
                                      sampler_prob=sp_dev if mixed and mix == "sampler_prob" else None, mix=mixed, oob_flag=flag)
        want, want_flag = fc.call(last, delta, ids, n_update, t, alpha, n_items, SEED, TID,
                                  sampler_prob=sp if mixed and mix == "sampler_prob" else None, mix=mixed)
        raised |= want_flag
        what = (case, k, n, upd, mix, pattern, n_items, alpha)
        o = out.cpu().numpy()
        assert got.data_ptr() == out.data_ptr() and got.numel() == n
        assert np.array_equal(_bits(o[:n]), _bits(want)), (what, np.flatnonzero(_bits(o[:n]) != _bits(want))[:4])
        assert (o[n:] == np.float32(PROB_SENTINEL)).all(), what
        assert int(flag.item()) == raised, what
        if slots <= 1024 or k == STEPS - 1:
            assert np.array_equal(sketch.cpu().numpy(), fc.pack(last, delta)), what
    assert (flat[hashes * slots:] == WORD_SENTINEL).all().item()
    l, d = ops.unpack_frequency_sketch(sketch)
    assert np.array_equal(l.cpu().numpy(), last) and np.array_equal(_bits(d.cpu().numpy()), _bits(delta))


def test_every_combination_is_run():
    seen = {COMBOS[(case * STEPS + k) % len(COMBOS)] for case in range(len(HASHES) * len(SLOTS) * len(FIRST_STEPS)) for k in range(STEPS)}
    assert seen == set(COMBOS)


def test_an_empty_call_leaves_everything_untouched(dev):
    flat, sketch = _sketch(dev, 2, 64)
    sketch.fill_(12345)
    out = torch.full((PAD,), PROB_SENTINEL, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.frequency_estimate_(sketch, torch.empty(0, dtype=torch.int64, device=dev), 0, 3, 0.1, 10, out, seed=SEED, tensor_id=TID,
                                  oob_flag=flag)
    assert got.numel() == 0 and (out == PROB_SENTINEL).all().item() and (sketch == 12345).all().item() and flag.item() == 0
    assert (flat[128:] == WORD_SENTINEL).all().item()


def test_custom_op_passes_opcheck_and_equals_the_ops_call(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(4)
    n_items = 300
    sp = T((rng.random(n_items) / n_items).astype(np.float32), dev)
    ids = T(rng.integers(0, n_items, 97).astype(np.int64), dev)
    for n_update, spd, mix in ((97, None, False), (0, None, False), (40, None, True), (40, sp, True)):
        a, b = ops.new_frequency_sketch(2, 512, dev), ops.new_frequency_sketch(2, 512, dev)
        out = torch.empty(97, device=dev)
        for t in (1, 2, 5):
            prob = torch.ops.twotower.frequency_estimate_(a, ids, n_update, t, 0.2, n_items, SEED, TID, spd, mix)
            ops.frequency_estimate_(b, ids, n_update, t, 0.2, n_items, out, seed=SEED, tensor_id=TID, sampler_prob=spd, mix=mix)
            assert torch.equal(prob, out) and torch.equal(a, b)
        torch.library.opcheck(torch.ops.twotower.frequency_estimate_, (a.clone(), ids, n_update, 9, 0.2, n_items, SEED, TID, spd, mix))


# ------------------------------------------------------------------------------------------ the trainer
N_USERS, N_IT, DIM, DIMS, B, TSEED, LR, ALPHA = 300, 1000, 32, (64, 32), 256, 1001, 0.001, 0.05


def _cfg(opt="sgd", streaming=True, n_neg=0, sampler="uniform", **kw):
    mixed = dict(candidate_sampling="mixed", n_sampled_negatives=n_neg, negative_sampler=sampler) if n_neg else {}
    est = dict(sampling_bias_estimator="streaming", freq_alpha=ALPHA) if streaming else {}
    return TwoTowerConfig(n_users=N_USERS, n_items=N_IT, embedding_dim=DIM, tower_dims=list(DIMS), temperature=0.1,
                          l2_regularization=1e-6, learning_rate=LR, optimizer=opt, batch_size=B, **mixed, **est, **kw)


def _state(tr):
    names = ["user_table", "item_table", "dense_flat", "loss"]
    names += {"sgd": [], "adagrad": ["user_accum", "item_accum", "dense_accum"]}[tr.cfg.optimizer]
    return {k: getattr(tr, k) for k in names}


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_in_batch_steps_equal_a_plain_trainer_fed_the_restatements_probabilities(dev, opt):
    """Batch 256, towers [64, 32], 1000 items, power-law ids (duplicates in every batch).  Both trainers go through the same
    kernels with the same cand_prob, so losses, tables and dense_flat are bit-identical after each of 3 steps; evaluate reads
    the sketch without changing it."""
    est, plain = TwoTowerTrainer(_cfg(opt), dev, seed=TSEED), TwoTowerTrainer(_cfg(opt, streaming=False), dev, seed=TSEED)
    assert plain.freq_sketch is None and plain.freq_prob is None and "freq_sketch" not in plain.state_dict()
    assert tuple(est.freq_sketch.shape) == (2, 2 * N_IT) and est.freq_sketch.dtype == torch.int64
    last, delta = fc.new_sketch(2, 2 * N_IT)
    for s in range(3):
        u, i = est.synthetic_batch(TSEED, s, "Z")
        iid = i.cpu().numpy()
        assert len(np.unique(iid)) < B
        want, _ = fc.call(last, delta, iid, B, s + 1, ALPHA, N_IT, TSEED, TID)
        la = est.step(u, i).item()
        lb = plain.step(u, i, candidate_sampling_probability=T(want, dev)).item()
        assert np.array_equal(_bits(est.freq_prob.cpu().numpy()), _bits(want)), s
        assert np.array_equal(est.freq_sketch.cpu().numpy(), fc.pack(last, delta)), s
        assert la == lb and np.isfinite(la), (s, la, lb)
        for k, v in _state(est).items():
            assert torch.equal(v, getattr(plain, k)), (s, k)
    est.check_ids()
    # forward_backward runs the estimator itself (step 4 of the stream), like step
    u, i = est.synthetic_batch(TSEED, 3, "Z")
    want, _ = fc.call(last, delta, i.cpu().numpy(), B, 4, ALPHA, N_IT, TSEED, TID)
    la = est.forward_backward(u, i).item()
    lb = plain.forward_backward(u, i, candidate_sampling_probability=T(want, dev)).item()
    assert la == lb and np.array_equal(est.freq_sketch.cpu().numpy(), fc.pack(last, delta))
    # evaluate: estimated at the present step, nothing updated
    before = est.freq_sketch.clone()
    u, i = est.synthetic_batch(TSEED, 9, "Z")
    iid = i.cpu().numpy()
    want, _ = fc.call(last, delta, iid, 0, est.step_index, ALPHA, N_IT, TSEED, TID)
    va = est.evaluate(u, i).item()
    vb = plain.evaluate(u, i, candidate_sampling_probability=T(want, dev)).item()
    assert va == vb and torch.equal(before, est.freq_sketch)
    got = est.estimated_item_probability(i[:77])
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[:77])) and torch.equal(before, est.freq_sketch)
    assert (want < 1.0).any() and (want > 1.0 / est.step_index).any()            # seen and never-seen items both occur


def _loss_close(got, want, batch):
    return abs(got - want) / batch <= 1e-4 and abs(got - want) <= 1e-4 * abs(want)


@pytest.mark.parametrize("sampler", ["uniform", "unigram"])
def test_one_mixed_step_takes_the_estimators_mixture_probability(dev, sampler):
    """N = 64 sampled negatives.  Two earlier batches are fed to the trainer's sketch and to the restatement's, then one
    forward_backward at step index 2: ``cand_prob`` equals the restatement bit for bit, and the loss equals
    sample_check.mixed_step in f64 with that probability (|d| / B <= 1e-4 and relative <= 1e-4, test_gpu_sample.py's bars)."""
    n_neg = 64
    tr = TwoTowerTrainer(_cfg("sgd", n_neg=n_neg, sampler=sampler), dev, seed=TSEED)
    alias = sp = None
    if sampler == "unigram":
        counts = np.bincount(np.random.default_rng(3).zipf(1.3, 20000) % N_IT, minlength=N_IT).astype(np.float64)
        freq = (counts / counts.sum()).astype(np.float32)          # (f32: the trainer forms the sampler's weights from what it is given)
        tr.set_item_frequencies(freq)
        w = freq.astype(np.float64) ** tr.cfg.unigram_power
        alias, sp = ops.build_alias_table(w), (w / w.sum()).astype(np.float32)
    last, delta = fc.new_sketch(2, 2 * N_IT)
    for s in range(2):
        _, i = tr.synthetic_batch(TSEED, s, "Z")
        ops.frequency_estimate_(tr.freq_sketch, i, B, s + 1, ALPHA, N_IT, tr.freq_prob, seed=TSEED, tensor_id=TID)
        fc.update(last, delta, i.cpu().numpy(), s + 1, ALPHA, N_IT, TSEED, TID)
    step = 2
    tr.step_index = step
    u, i = tr.synthetic_batch(TSEED, step, "Z")
    ref = tt.synthetic_state(TSEED, N_USERS, N_IT, DIM, list(DIMS), dtype=np.float64)
    loss = tr.forward_backward(u, i).item()
    tr.check_ids()
    cand = sc.candidates(i.cpu().numpy(), N_IT, n_neg, TSEED, sc.TID_SAMPLED_NEGATIVES, step * n_neg, alias)[0]
    assert np.array_equal(tr.cand_ids.cpu().numpy(), cand)
    want, _ = fc.call(last, delta, cand, B, step + 1, ALPHA, N_IT, TSEED, TID, sampler_prob=sp, mix=True)
    assert np.array_equal(_bits(tr.cand_prob.cpu().numpy()), _bits(want))
    assert np.array_equal(tr.freq_sketch.cpu().numpy(), fc.pack(last, delta))
    ut, it = tr.user_tower, tr.item_tower
    masks = tuple([(t.acts[l + 1] > 0).cpu().numpy() for l in range(t.n_layers - 1)] for t in (ut, it))
    r = sc.mixed_step(ref, u.cpu().numpy(), cand, 0.1, want.astype(np.float64), masks, False)
    print(f"{sampler}: loss {loss} (f64 {r['loss']})")
    assert _loss_close(loss, r["loss"], B), (loss, r["loss"])


@pytest.mark.parametrize("opt,n_neg", [("adagrad", 0), ("sgd", 64)])
def test_resume_continues_the_sketch(dev, opt, n_neg):
    """3 steps, save, load into a fresh trainer, 3 more: bit-identical to 6 uninterrupted steps, sketch included."""
    def run(tr, steps):
        for s in steps:
            tr.step(*tr.synthetic_batch(TSEED, s, "Z"))
    a, b = TwoTowerTrainer(_cfg(opt, n_neg=n_neg), dev, seed=TSEED), TwoTowerTrainer(_cfg(opt, n_neg=n_neg), dev, seed=TSEED)
    run(a, range(6)); run(b, range(3))
    sd = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in b.state_dict().items()}
    c4 = sd["config"]
    assert (c4["sampling_bias_estimator"], c4["freq_alpha"], c4["freq_hashes"], c4["freq_slots"]) == ("streaming", ALPHA, 2, 0)
    assert sd["freq_sketch"].dtype == torch.int64 and tuple(sd["freq_sketch"].shape) == (2, 2 * N_IT) and sd["step_index"] == 3
    c = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev, seed=TSEED + 1)
    c.load_state_dict(sd)
    run(c, range(3, 6))
    for k, v in _state(a).items():
        assert torch.equal(v, getattr(c, k)), k
    assert torch.equal(a.freq_sketch, c.freq_sketch) and (a.freq_sketch != 0).any().item()
    assert torch.equal(a.freq_prob, c.freq_prob) if not n_neg else torch.equal(a.cand_prob, c.cand_prob)
    # a trainer without the estimator ignores the sketch; one with another sketch shape, or no sketch to continue on, refuses
    TwoTowerTrainer(_cfg(opt, streaming=False, n_neg=n_neg), dev, seed=1).load_state_dict(sd)
    with pytest.raises(ValueError, match="freq_sketch"):
        TwoTowerTrainer(_cfg(opt, n_neg=n_neg, freq_hashes=3), dev, seed=1).load_state_dict(sd)
    with pytest.raises(ValueError, match="freq_sketch"):
        TwoTowerTrainer(_cfg(opt, n_neg=n_neg), dev, seed=1).load_state_dict({k: v for k, v in sd.items() if k != "freq_sketch"})


def test_refusals(dev):
    tr = TwoTowerTrainer(_cfg("sgd"), dev, seed=1)
    with pytest.raises(NotImplementedError, match="step number is a launch argument"):
        tr.capture_graph()
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="streaming"):
        ShardedTwoTowerTrainer(_cfg("sgd"), dev, seed=1)
    u, i = tr.synthetic_batch(1, 0)
    p = torch.full((B,), 0.01, device=dev)
    for call in (tr.step, tr.forward_backward, tr.evaluate):
        with pytest.raises(ValueError, match="streaming"):
            call(u, i, candidate_sampling_probability=p)
    assert tr.step_index == 0 and not tr.freq_sketch.any().item()
    with pytest.raises(ValueError, match="estimator"):
        TwoTowerTrainer(_cfg("sgd", streaming=False), dev, seed=1).estimated_item_probability(i)
    mixed = TwoTowerTrainer(_cfg("sgd", n_neg=64), dev, seed=1)
    with pytest.raises(ValueError, match="mixed"):
        mixed.step(u, i, candidate_sampling_probability=p)
    uni = TwoTowerTrainer(_cfg("sgd", n_neg=64, sampler="unigram"), dev, seed=1)
    with pytest.raises(ValueError, match="set_item_frequencies"):        # the unigram sampler still needs its alias table
        uni.step(u, i)
    mixed.step(u, i)                                                       # the uniform sampler needs nothing
    mixed.check_ids()


def test_train_cli_runs_with_the_streaming_estimator(dev, tmp_path):
    from two_tower_amazon_recommender_amd import train
    import pyarrow as pa
    import pyarrow.parquet as pq
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  l2_regularization: 1e-6\n  training:\n    batch_size: 256\n    learning_rate: 0.001\n    epochs: 1\n"
                    "  retrieval:\n    candidate_sampling: in_batch\n    temperature: 0.1\n")
    rng = np.random.default_rng(4)
    pairs = tmp_path / "pairs.parquet"
    uu, ii = rng.integers(0, 300, 900), rng.integers(0, 200, 900)
    uu[0], ii[0] = 299, 199
    pq.write_table(pa.table({"user_idx": uu, "item_idx": ii}), pairs)
    ck = tmp_path / "freq.pt"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):                                  # 900 pairs, 30 % held out: 2 training steps, 1 validation batch
        assert train.main(["--config", str(cfgp), "--data", str(pairs), "--val-fraction", "0.3", "--sampling-bias-estimator", "streaming",
                           "--freq-alpha", "0.05", "--freq-slots", "512", "--save", str(ck)]) == 0
    rec = json.loads(buf.getvalue().strip().splitlines()[-1])["history"][-1]
    assert np.isfinite(rec["train_loss_per_pair"]) and np.isfinite(rec["val_loss_per_pair"]), rec
    assert set(rec) <= {"epoch", "train_loss_per_pair", "pairs_per_sec", "lr", "val_loss_per_pair"}      # nothing new is logged
    sd = torch.load(ck, weights_only=True)
    assert sd["step_index"] == 2 and tuple(sd["freq_sketch"].shape) == (2, 512) and (sd["freq_sketch"] != 0).any().item()
    assert (sd["config"]["sampling_bias_estimator"], sd["config"]["freq_alpha"], sd["config"]["freq_slots"]) == ("streaming", 0.05, 512)

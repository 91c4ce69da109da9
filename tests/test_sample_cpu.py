"""Mixed negative sampling without a GPU: the entry point's argument checks, the alias table, the restatement's own draw
statistics (so that the GPU tests can be bit-exact and need none), the config plumbing and the CLI's refusal."""
import copy

import numpy as np
import pytest

import sample_check as sc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod, ops
from two_tower_amazon_recommender_amd.trainer import TID_SAMPLED_NEGATIVES, TwoTowerConfig


def test_tensor_id_of_the_restatement_is_the_trainers():
    assert sc.TID_SAMPLED_NEGATIVES == TID_SAMPLED_NEGATIVES


# ------------------------------------------------------------------------------------------ argument refusals
def _call(n_pos=4, n_items=10, n_neg=4, sampler=0, thr=None, idx=None, freq=None, sp=None, pos=1, ids=1, prob=None):
    """Pointers are never dereferenced before the checks pass; 64 stands for 'some non-null pointer'."""
    p = lambda v: None if not v else 64
    return _lib.load().tt_sample_candidates_i64(p(pos), n_pos, n_items, n_neg, sampler, p(thr), p(idx), p(freq), p(sp), 1, 10, 0,
                                                p(ids), p(prob), None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(n_items=0), "n_items"), (dict(n_items=-3), "n_items"), (dict(n_items=(1 << 32) + 1), "n_items"),
    (dict(n_pos=-1), "n_pos"), (dict(n_neg=-1), "n_neg"), (dict(n_pos=0, n_neg=0), ">= 1"),
    (dict(sampler=2), "sampler"), (dict(sampler=-1), "sampler"),
    (dict(sampler=1), "alias"), (dict(sampler=1, thr=1), "alias"), (dict(sampler=1, idx=1), "alias"),
    (dict(sampler=1, thr=1, idx=1, n_items=1 << 31), "2^31"),
    (dict(sp=1), "sampler_prob without item_freq"),
    (dict(ids=0), "null"), (dict(pos=0), "null"), (dict(freq=1), "cand_prob"),
])
def test_bad_arguments_are_refused_before_any_launch(kw, word):
    lib = _lib.load()
    assert _call(**kw) == _lib.TT_ERR_INVALID_ARG, kw
    msg = lib.tt_last_error().decode()
    assert "tt_sample_candidates_i64" in msg and word in msg, (kw, msg)


def test_the_python_wrapper_refuses_cpu_tensors_and_bad_names():
    import torch
    ids, out = torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_candidates(ids, 10, 4, out, seed=1, tensor_id=10, start=0)
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.twotower.sample_candidates(ids, 10, 4, 1, 10, 0, None, None, None, None)


# ------------------------------------------------------------------------------------------ the alias table
def _targets():
    rng = np.random.default_rng(5)
    zeros = rng.random(64)
    zeros[rng.random(64) < 0.4] = 0.0
    one_hot = np.zeros(17)
    one_hot[11] = 3.0
    return {"uniform": np.ones(50), "one-hot": one_hot, "power-law": 1.0 / np.arange(1, 1001) ** 1.1, "with zeros": zeros,
            "single": np.array([0.25])}


@pytest.mark.parametrize("name", list(_targets()))
def test_alias_table_implies_its_target_distribution(name):
    w = _targets()[name]
    thr, idx = ops.build_alias_table(w)
    n = len(w)
    assert thr.dtype == np.float32 and idx.dtype == np.int32 and thr.shape == idx.shape == (n,)
    assert (thr >= 0).all() and (thr <= 1).all() and (idx >= 0).all() and (idx < n).all()
    assert np.array_equal(thr.astype(np.float64) * 2.0 ** 24, np.rint(thr.astype(np.float64) * 2.0 ** 24))    # on the 2^-24 grid
    p, indegree = sc.alias_distribution(thr, idx)
    target = w / w.sum()
    bound = (1 + indegree) * 2.0 ** -24 / n
    worst = np.abs(p - target) / bound
    print(f"{name}: largest error {np.abs(p - target).max():.3e}, {worst.max():.3f} of its bound; sum - 1 = {p.sum() - 1:.2e}")
    assert (np.abs(p - target) <= bound).all(), (name, int(worst.argmax()), worst.max())
    assert abs(p.sum() - 1.0) <= 4 * n * np.finfo(np.float64).eps
    assert (p[w == 0] == 0).all()                                     # an item of weight 0 is never drawn
    again = ops.build_alias_table(w * 7.0)                            # deterministic, and normalised
    assert np.array_equal(again[1], idx) and np.abs(again[0] - thr).max() <= 2.0 ** -24


def test_alias_table_rejects_negative_and_all_zero_weights():
    for bad in ([0.5, -0.1, 0.6], [0.0, 0.0, 0.0], [], [1.0, float("nan")]):
        with pytest.raises(ValueError):
            ops.build_alias_table(np.asarray(bad, dtype=np.float64))


# ------------------------------------------------------------------------------------------ the restatement's draws
@pytest.mark.parametrize("sampler", ["uniform", "alias"])
def test_restatement_draws_follow_their_distribution(sampler):
    """200,000 draws over 40 items: every item's count within 5 standard deviations of n * p_k (binomial).  Fixed seed."""
    n_items, n, seed = 40, 200_000, 20201
    if sampler == "uniform":
        alias, p = None, np.full(n_items, 1.0 / n_items)
    else:
        w = 1.0 / np.arange(1, n_items + 1) ** 1.2
        alias = ops.build_alias_table(w)
        p = sc.alias_distribution(*alias)[0]
    ids = sc.draw(seed, sc.TID_SAMPLED_NEGATIVES, 12345, n, n_items, alias)
    assert ids.min() >= 0 and ids.max() < n_items
    counts = np.bincount(ids, minlength=n_items)
    z = (counts - n * p) / np.sqrt(n * p * (1 - p))
    print(f"{sampler}: largest |z| {np.abs(z).max():.2f}")
    assert (np.abs(z) <= 5).all(), z
    # the stream is a function of the counter: a window of it is the same draws
    assert np.array_equal(sc.draw(seed, sc.TID_SAMPLED_NEGATIVES, 12345 + 100, 50, n_items, alias), ids[100:150])


def test_restatement_probability_is_the_mixture_formula():
    n_items, b, n = 7, 3, 5
    freq = np.array([0.5, 0.25, 0.125, 0.125, 0, 0, 0], dtype=np.float32)
    ids, prob, flag = sc.candidates([0, 7, -1], n_items, n, 1, 10, 0, item_freq=freq)
    assert flag == 1 and list(ids[:3]) == [0, 7, -1] and prob[1] == 1.0 and prob[2] == 1.0
    want0 = (3 * 0.5 + 5 / 7) / 8
    assert abs(float(prob[0]) - want0) <= 4 * np.finfo(np.float32).eps * want0
    sp = np.full(n_items, 1.0 / n_items, dtype=np.float32)
    assert np.array_equal(sc.candidates([0, 1, 2], n_items, n, 1, 10, 0, item_freq=freq, sampler_prob=sp)[1],
                          sc.candidates([0, 1, 2], n_items, n, 1, 10, 0, item_freq=freq)[1])
    assert sc.candidates([0], n_items, n, 1, 10, 0)[1] is None


# ------------------------------------------------------------------------------------------ config
def _doc(**retrieval):
    return {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                      "training": {"batch_size": 256, "learning_rate": 0.001},
                      "retrieval": {"temperature": 0.1, **retrieval}}}


def test_config_reads_mixed_sampling():
    cfg, _ = cfgmod.model_config_from_dict(_doc(candidate_sampling="mixed"), 100, 100)
    assert (cfg.candidate_sampling, cfg.n_sampled_negatives, cfg.negative_sampler, cfg.unigram_power) == ("mixed", 256, "uniform", 0.75)
    cfg.validate()
    cfg, _ = cfgmod.model_config_from_dict(_doc(candidate_sampling="mixed", num_sampled_negatives=64, negative_sampler="unigram",
                                                unigram_power=0.5), 100, 100)
    assert (cfg.n_sampled_negatives, cfg.negative_sampler, cfg.unigram_power) == (64, "unigram", 0.5)
    cfg.validate()
    cfg, _ = cfgmod.model_config_from_dict(_doc(candidate_sampling="in_batch", num_sampled_negatives=64), 100, 100)
    assert (cfg.candidate_sampling, cfg.n_sampled_negatives) == ("in_batch", 0)
    cfg, _ = cfgmod.model_config_from_dict(_doc(), 100, 100)
    assert (cfg.candidate_sampling, cfg.n_sampled_negatives) == ("in_batch", 0)
    for other in ("uniform", "sampled", "Mixed", ""):
        with pytest.raises(NotImplementedError, match="in_batch"):
            cfgmod.model_config_from_dict(_doc(candidate_sampling=other), 100, 100)


def test_validate_checks_the_sampling_fields():
    base = TwoTowerConfig(n_users=100, n_items=100, embedding_dim=32, tower_dims=[64, 32], batch_size=256)
    base.validate()
    assert (base.candidate_sampling, base.n_sampled_negatives, base.negative_sampler, base.unigram_power) == ("in_batch", 0, "uniform", 0.75)

    def bad(match, **kw):
        cfg = copy.copy(base)
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match=match):
            cfg.validate()
    bad("n_sampled_negatives", candidate_sampling="mixed", n_sampled_negatives=0)
    bad("n_sampled_negatives", candidate_sampling="in_batch", n_sampled_negatives=8)
    bad("65536", candidate_sampling="mixed", n_sampled_negatives=65536 - 255)
    bad("negative_sampler", candidate_sampling="mixed", n_sampled_negatives=8, negative_sampler="zipf")
    bad("candidate_sampling", candidate_sampling="uniform")
    bad("n_category_buckets", candidate_sampling="mixed", n_sampled_negatives=8, n_category_buckets=30)
    bad("unigram_power", unigram_power=-1.0)
    ok = copy.copy(base)
    ok.candidate_sampling, ok.n_sampled_negatives, ok.negative_sampler = "mixed", 65536 - 256, "unigram"
    ok.validate()


# ------------------------------------------------------------------------------------------ CLI
def test_train_cli_refuses_distributed_with_mixed_sampling_before_touching_a_device(tmp_path):
    import yaml
    from two_tower_amazon_recommender_amd import train
    for doc, extra in ((_doc(), ["--candidate-sampling", "mixed"]), (_doc(candidate_sampling="mixed"), [])):
        cfgp = tmp_path / "cfg.yaml"
        cfgp.write_text(yaml.safe_dump(doc))
        with pytest.raises(NotImplementedError, match="mixed"):
            train.main(["--config", str(cfgp), "--synthetic", "600", "--distributed", "--device", "cuda:99"] + extra)
    args = train.parse(["--config", "x", "--candidate-sampling", "mixed", "--sampled-negatives", "64", "--negative-sampler", "unigram",
                        "--unigram-power", "0.5"])
    assert (args.candidate_sampling, args.sampled_negatives, args.negative_sampler, args.unigram_power) == ("mixed", 64, "unigram", 0.5)

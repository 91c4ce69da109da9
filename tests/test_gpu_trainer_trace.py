"""The op sequence of every entry point of ``TwoTowerTrainer`` against a recorded trace, the way ``test_tower_drivers_cpu.py``
holds the tower drivers to theirs - here on the GPU, with the real launches passing through.

A recorder wraps every function of the ``ops`` module (and the sort plans' ``run``; a call made from inside another op is part
of that op), counts the composite C call as the one entry ``tt_train_step_f32``, and lists, per case and entry point, the names
in the order the trainer called them.  Host-side shape queries (``*_num_slabs``, ``*_supported``, ``*_bytes``, ...) launch
nothing and are left out.

``tests/golden/trainer_op_traces.json`` was recorded with this recorder from the trainer as it stood BEFORE the input builder,
the step body and the optimizer dispatch became one each.  It is a record of that behaviour and is never regenerated from the
code under test.  Where the trainer differs from it on purpose the file says so itself (``_intended_difference``): a rewrite
rule and the exact (case, entry point) pairs it applies to.  Everywhere else the traces must be equal, name for name."""
import json
import os

import numpy as np
import pytest
import torch

from two_tower_amazon_recommender_amd import data, metrics, ops, trainer
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_op_traces.json")
SEED, BATCH, HIST = 23, 64, 5
BASE = dict(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], batch_size=BATCH)
MIXED = dict(candidate_sampling="mixed", n_sampled_negatives=16)
TITLE = dict(n_title_buckets=50, title_max_tokens=4)
FEATURES = dict(n_user_features=3, n_item_features=2)
# the config of test_all_features_checkpoint_round_trip_is_bit_identical (test_gpu_trainer.py)
ALL = dict(n_category_buckets=7, user_history_len=HIST, history_pooling="attention", rating_weight=0.5, rating_hidden=32,
           cross_layers=2, normalize_embeddings=True, **TITLE, **FEATURES)
OPTIMIZERS = ("sgd", "adagrad", "adam", "rowwise_adagrad")

# case -> config fields; "env": the environment the trainer is built under; "freq": set_item_frequencies runs
CASES = {
    **{f"plain_{o}": dict(optimizer=o) for o in OPTIMIZERS},
    "no_composite": dict(env={"TT_COMPOSITE_STEP": "0"}),
    "no_fuse_lookup": dict(env={"TT_FUSE_LOOKUP": "0"}),
    "asymmetric": dict(tower_dims=[64, 32], item_tower_dims=[96, 64, 32]),
    "category": dict(n_category_buckets=7),
    "title": dict(TITLE),
    "history_mean": dict(user_history_len=HIST, history_pooling="mean"),
    "history_attention": dict(user_history_len=HIST, history_pooling="attention"),
    "features": dict(FEATURES),
    "rating": dict(rating_weight=0.5, rating_hidden=32),
    "cross2": dict(cross_layers=2),
    "layer_norm": dict(layer_norm=True),
    "normalize": dict(normalize_embeddings=True),
    "clipnorm": dict(global_clipnorm=1.0),
    "streaming": dict(sampling_bias_estimator="streaming"),
    "mixed_uniform": dict(MIXED),
    "mixed_unigram": dict(MIXED, negative_sampler="unigram", freq=True),
    "mixed_title_features": dict(MIXED, **TITLE, **FEATURES),
    "mixed_normalize": dict(MIXED, normalize_embeddings=True),
    **{f"mixed_{o}": dict(MIXED, optimizer=o) for o in OPTIMIZERS[1:]},
    **{f"all_features_{o}": dict(ALL, optimizer=o) for o in OPTIMIZERS},
}

# launch nothing: shape and capability queries of the host side
_QUERIES = ("_num_slabs", "_supported", "_bytes", "_workspace", "_max_ids", "_max_lds_ids")


class Recorder:
    """Pass-through: every public function of ``ops`` (and ``SparsePlan.run``) appends its name, then runs.  Calls made while
    another recorded call runs are not listed.  ``tt_train_step_f32`` of the library the trainer loads is listed under that name."""

    def __init__(self):
        self.names, self._depth, self._saved = [], 0, []

    def _wrap(self, name, fn):
        def call(*args, **kwargs):
            if self._depth == 0:
                self.names.append(name)
            self._depth += 1
            try:
                return fn(*args, **kwargs)
            finally:
                self._depth -= 1
        return call

    def _set(self, obj, attr, value):
        self._saved.append((obj, attr, getattr(obj, attr)))
        setattr(obj, attr, value)

    def __enter__(self):
        for name, fn in sorted(vars(ops).items()):
            if (callable(fn) and not isinstance(fn, type) and not name.startswith("_") and getattr(fn, "__module__", None) == ops.__name__
                    and not name.endswith(_QUERIES)):
                self._set(ops, name, self._wrap(name, fn))
        self._set(ops.SparsePlan, "run", self._wrap("SparsePlan.run", ops.SparsePlan.run))
        lib, rec = trainer._lib.load(), self

        class Library:
            """The loaded library with the composite entry recorded; everything else is the library's own."""

            def __getattr__(self, attr):
                fn = getattr(lib, attr)
                return rec._wrap(attr, fn) if attr == "tt_train_step_f32" else fn

        proxy = Library()
        self._set(trainer._lib, "load", lambda: proxy)
        return self

    def __exit__(self, *exc):
        for obj, attr, value in reversed(self._saved):
            setattr(obj, attr, value)
        self._saved = []

    def take(self):
        names, self.names = self.names, []
        return names


def build_trainer(case, dev):
    case = dict(case)
    env, freq = case.pop("env", {}), case.pop("freq", False)
    cfg = TwoTowerConfig(**{**BASE, **case})
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tr = TwoTowerTrainer(cfg, dev, seed=SEED)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if cfg.user_history_len:
        pairs = [tr.synthetic_batch(SEED, s, "Z") for s in range(4)]
        u, i = (torch.cat([p[k] for p in pairs]).cpu().numpy() for k in (0, 1))
        tr.set_user_histories(torch.from_numpy(data.user_histories(u, i, cfg.n_users, cfg.user_history_len)).to(dev))
    if cfg.n_title_buckets:
        tr.set_item_titles(tr.synthetic_item_titles(SEED))
    if cfg.n_user_features:
        tr.set_user_features(tr.synthetic_user_features(SEED))
    if cfg.n_item_features:
        tr.set_item_features(tr.synthetic_item_features(SEED))
    if freq:
        tr.set_item_frequencies(np.arange(1, cfg.n_items + 1, dtype=np.float64) / (cfg.n_items * (cfg.n_items + 1) / 2))
    return tr


def batch_kw(tr, step, u, i):
    """The keyword arguments a batch of ``tr`` needs: the pairs' categories and ratings where the model has the feature."""
    kw = {}
    if tr.cat_table is not None:
        kw["category_ids"] = tr.synthetic_categories(SEED, step)
    if tr.rating_on:
        kw["ratings"] = ((u + 2 * i) % 5 + 1).to(torch.float32)
    return kw


def run_entry_points(tr, rec):
    """Every entry point once, in a fixed order; returns entry point -> op names."""
    cfg, out = tr.cfg, {}
    batches = [tr.synthetic_batch(SEED, s, "Z") for s in range(4)]
    kws = [batch_kw(tr, s, *b) for s, b in enumerate(batches)]
    many = torch.cat([batches[0][0], batches[1][0][:BATCH // 2]])              # 1.5 batches
    many_items = torch.cat([batches[0][1], batches[1][1][:BATCH // 2]])
    item_cats = torch.arange(cfg.n_items, device=tr.dev) % cfg.n_category_buckets if cfg.n_category_buckets else None
    rec.take()
    tr.step(*batches[0], **kws[0])
    out["step"] = rec.take()
    tr.step(*batches[1], **kws[1])
    out["step_again"] = rec.take()
    tr.evaluate(*batches[2], **kws[2])
    out["evaluate"] = rec.take()
    tr.user_embeddings(many)
    out["user_embeddings"] = rec.take()
    corpus = tr.item_corpus_embeddings(item_cats)
    out["item_corpus_embeddings"] = rec.take()
    tr.evaluate_topk(*batches[2], metrics.FactorizedTopK(ks=(1, 5)), corpus=corpus)
    out["evaluate_topk"] = rec.take()
    if tr.rating_on:
        cats = None if item_cats is None else item_cats[many_items]
        tr.predict_ratings(many, many_items, cats)
        out["predict_ratings"] = rec.take()
    u, i = batches[3]
    tr.forward_backward(u, i, **kws[3])
    tr.clip_gradients()
    tr.apply_gradients(step_ids=[u, i] + ([kws[3]["category_ids"]] if "category_ids" in kws[3] else []))
    out["forward_backward_clip_apply"] = rec.take()
    tr.check_ids()
    return out


def trace_case(name, dev):
    tr = build_trainer(CASES[name], dev)
    with Recorder() as rec:
        return run_entry_points(tr, rec)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _expected(want, rewrites):
    """The recorded names with the intended differences applied: every rule replaces each occurrence of its ``old`` run of names
    by its ``new`` one, and must find one."""
    for rule in rewrites:
        old, new, got, k = rule["old"], rule["new"], [], 0
        while k < len(want):
            if want[k:k + len(old)] == old:
                got += new
                k += len(old)
            else:
                got.append(want[k])
                k += 1
        assert got != want, f"the rule {rule['what']!r} found nothing to rewrite"
        want = got
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_op_trace(name, dev, golden):
    got, want = trace_case(name, dev), golden[name]
    assert sorted(got) == sorted(want)
    for entry in want:
        rewrites = [r for r in golden["_intended_difference"] if [name, entry] in r["where"]]
        assert got[entry] == _expected(want[entry], rewrites), f"{name}: {entry}"


def test_golden_has_no_stale_case(golden):
    assert sorted(k for k in golden if not k.startswith("_")) == sorted(CASES)
    for rule in golden["_intended_difference"]:
        for case, entry in rule["where"]:
            assert entry in golden[case], (case, entry)


def test_the_intended_differences_are_the_inference_gathers_alone(golden):
    """What may differ from the record: inference passes that materialise both sides at equal row counts - mixed sampling's
    ``evaluate`` and ``predict_ratings`` - take one ``embedding_gather2`` where they took two ``embedding_gather``; and
    ``predict_ratings`` with the history feature gathers the item rows in front of the user side's history launch, like every
    other pass, where it ran the two launches (which write different buffers) the other way round."""
    rules = {r["what"]: r for r in golden["_intended_difference"]}
    assert sorted(rules) == ["gather2", "item_gather_first"]
    assert rules["gather2"]["old"] == ["embedding_gather", "embedding_gather"] and rules["gather2"]["new"] == ["embedding_gather2"]
    mixed = [[c, "evaluate"] for c in sorted(CASES) if c.startswith("mixed_")]
    assert sorted(rules["gather2"]["where"]) == sorted(mixed + [["rating", "predict_ratings"]])
    first = rules["item_gather_first"]
    assert first["old"] == ["history_attention", "embedding_gather"] and first["new"] == ["embedding_gather", "history_attention"]
    assert sorted(first["where"]) == [[f"all_features_{o}", "predict_ratings"] for o in sorted(OPTIMIZERS)]

"""The dense numeric side features without a GPU: the data layer (rating statistics against pandas), the normalisation's
statistics, the NumPy restatement of tests/features_check.py against torch f64, config / YAML / CLI parsing and every refusal,
the C entry points' argument errors (returned before any launch), the ABI mirrors and the custom op's registration."""
import ctypes as C
import dataclasses
import pathlib
import re

import numpy as np
import pytest
import torch

import features_check as fc
from two_tower_amazon_recommender_amd import _lib, data, ops
from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, FeatureSide, TwoTowerConfig, TwoTowerTrainer

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------ data layer
def _ratings(seed=5, n=4000, n_users=700, n_items=300):
    """~4000 synthetic rows.  Users 0..49 have exactly one rating (their std does not exist), user n_users - 1 and item
    n_items - 1 have no row at all, 30 ratings are NaN (left out, as pandas' aggregations do)."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([np.arange(50), rng.integers(50, n_users - 1, n - 50)])
    i = rng.integers(0, n_items - 1, n)
    r = rng.integers(1, 6, n).astype(np.float64) + rng.integers(0, 2, n) * 0.5
    r[rng.choice(np.arange(50, n), 30, replace=False)] = np.nan
    return u, i, r, n_users, n_items


def test_rating_features_equal_the_pandas_groupby():
    import pandas as pd
    u, i, r, n_users, n_items = _ratings()
    got_u, got_i = data.rating_features(u, i, r, n_users, n_items)
    assert got_u.dtype == got_i.dtype == np.float32 and got_u.shape == (n_users, 5) and got_i.shape == (n_items, 5)
    df = pd.DataFrame({"u": u, "i": i, "rating": r})
    for key, rows, got in (("u", n_users, got_u), ("i", n_items, got_i)):
        agg = df.groupby(key)["rating"].agg(["count", "mean", "std", "min", "max"]).round(3).reindex(np.arange(rows))
        want = agg.to_numpy(dtype=np.float64)
        want[np.isnan(want[:, 0]), 0] = 0.0                      # an id with no row: count 0
        exists = np.isfinite(want)
        assert exists[:, 0].all() and (~exists[:, 2]).sum() >= (50 if key == "u" else 1)
        assert not exists[rows - 1, 1:].any() and want[rows - 1, 0] == 0
        assert np.array_equal(got[exists], want[exists].astype(np.float32)), key
        # what does not exist takes its column's mean over what does: the normalised value is (up to rounding) 0
        fill = np.array([want[exists[:, c], c].mean() for c in range(5)])
        for c in range(1, 5):
            assert np.allclose(got[~exists[:, c], c], fill[c], rtol=1e-6), (key, c)
        assert np.isfinite(got).all()
    assert got_u[:50, 0].tolist() == [1.0] * 50
    # a column with nothing finite at all: 0
    gu, gi = data.rating_features(np.array([0, 1]), np.array([0, 0]), np.array([3.0, 5.0]), 3, 2)
    assert gu[:, 2].tolist() == [0.0, 0.0, 0.0] and gu[2].tolist() == [0.0, 4.0, 0.0, 4.0, 4.0]
    assert np.allclose(gi[0], [2.0, 4.0, 1.414, 3.0, 5.0]) and gi[1, 0] == 0.0
    with pytest.raises(ValueError, match="length"):
        data.rating_features(np.array([0]), np.array([0, 1]), np.array([1.0]), 2, 2)
    with pytest.raises(ValueError, match="user_idx"):
        data.rating_features(np.array([5]), np.array([0]), np.array([1.0]), 2, 2)


def test_read_ratings_reads_the_column_or_returns_none(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({"user_idx": [0, 1, 2], "item_idx": [0, 1, 1], "rating": [5.0, None, 3.0]}), tmp_path / "a.parquet")
    pq.write_table(pa.table({"user_idx": [0, 1], "item_idx": [0, 1]}), tmp_path / "b.parquet")
    got = data.read_ratings(tmp_path / "a.parquet")
    assert got.dtype == np.float64 and got[0] == 5.0 and np.isnan(got[1]) and got[2] == 3.0
    assert data.read_ratings(tmp_path / "b.parquet") is None


def test_adapt_normalization_is_keras_adapt():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((500, 6)) * [1, 10, 0.01, 3, 1, 1] + [0, 5, -2, 100, 0, 0]).astype(np.float32)
    x[:, 4] = 3.25                                                # a constant column
    x[:, 5] = np.float32(0.1)                                     # ... and one that is not a dyadic number
    mean, inv_std = ops.adapt_normalization(x)
    assert mean.dtype == inv_std.dtype == np.float32 and mean.shape == inv_std.shape == (6,)
    x64 = x.astype(np.float64)
    assert np.array_equal(mean, x64.mean(0).astype(np.float32))
    assert np.array_equal(inv_std, (1.0 / np.maximum(np.sqrt(x64.var(0)), 1e-7)).astype(np.float32))
    assert inv_std[4] == inv_std[5] == np.float32(1e7)
    z, _ = fc.normalise(x, np.arange(500), mean, inv_std)
    assert not z[:, 4:].any()                                     # a constant column: exactly 0
    assert np.abs(z[:, :4].mean(0)).max() < 1e-3 and np.abs(z[:, :4].std(0) - 1).max() < 1e-3
    m2, s2 = ops.adapt_normalization(torch.from_numpy(x))
    assert np.array_equal(m2, mean) and np.array_equal(s2, inv_std)
    for bad in (np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]])):
        with pytest.raises(ValueError, match="non-finite"):
            ops.adapt_normalization(bad)
    with pytest.raises(ValueError, match="rows"):
        ops.adapt_normalization(np.zeros(4))


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("F,dim,clip,norm", [(1, 32, 0.0, True), (5, 32, 2.5, True), (32, 128, 0.0, False), (3, 128, 2.5, False)])
def test_restatement_against_torch_f64(F, dim, clip, norm):
    rng = np.random.default_rng(F * 100 + dim)
    feat = (rng.standard_normal((50, F)) * 3 + 1).astype(np.float32)
    ids = rng.integers(0, 50, 77)
    ids[[3, 9]] = -1
    ids[11] = 50
    mean, inv_std = ops.adapt_normalization(feat) if norm else (None, None)
    proj = rng.uniform(-0.2, 0.2, (F, dim)).astype(np.float32)
    base = rng.standard_normal((77, dim)).astype(np.float32)
    out, z, flag = fc.features_forward(feat, ids, mean, inv_std, proj, clip)
    acc, z2, _ = fc.features_forward(feat, ids, mean, inv_std, proj, clip, accumulate=True, out=base)
    assert flag == 1 and fc.features_forward(feat, np.where(ids == 50, 0, ids), mean, inv_std, proj, clip)[2] == 0
    assert not out[[3, 9, 11]].any() and not z[[3, 9, 11]].any() and np.array_equal(fc.bits(z), fc.bits(z2))
    assert np.array_equal(fc.bits(acc[[3, 9, 11]]), fc.bits(base[[3, 9, 11]]))
    ok = (ids >= 0) & (ids < 50)
    x = torch.from_numpy(feat.astype(np.float64))[torch.from_numpy(np.where(ok, ids, 0))]
    if norm:
        x = (x - torch.from_numpy(mean.astype(np.float64))) * torch.from_numpy(inv_std.astype(np.float64))
    if clip > 0:
        x = x.clamp(-clip, clip)
        assert (np.abs(z) == np.float32(clip)).any() and np.abs(z).max() == np.float32(clip)
    x = x * torch.from_numpy(ok.astype(np.float64))[:, None]
    p = torch.tensor(proj.astype(np.float64), requires_grad=True)
    want = x @ p
    # f32 rounding: z within a few ulp of its f64 value (a subtraction of f32 values, one product); the sum of F products of
    # magnitude <= |z| |P| accumulates at most (F + 2) roundings of 2^-24 relative to sum |z_f P_fd|
    assert np.abs(z - x.numpy()).max() <= 4 * 2.0 ** -24 * max(np.abs(x.numpy()).max(), 1.0) * (np.abs(inv_std).max() if norm else 1.0) * 8
    bound = (F + 2) * 2.0 ** -24 * (np.abs(z.astype(np.float64)) @ np.abs(proj.astype(np.float64))) + 1e-6 * np.abs(want.detach().numpy())
    assert (np.abs(out - want.detach().numpy()) <= bound + 1e-30).all()
    assert np.abs(acc - (base + want.detach().numpy())).max() <= 1e-5 * np.abs(base).max()
    dy = rng.standard_normal((77, dim))
    want.backward(torch.from_numpy(dy))
    dp = fc.features_dp(z, dy)
    assert np.abs(dp - p.grad.numpy()).max() <= 1e-5 * np.abs(p.grad.numpy()).max()
    assert fc.slab_rows(1000, 8) == [(125 * s, 125 * s + 125) for s in range(8)]
    assert fc.slab_rows(130, 3) == [(0, 44), (44, 88), (88, 130)] and fc.slab_rows(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]


def test_step_f64_reduces_to_the_plain_step_without_features_and_sees_the_projection():
    rng = np.random.default_rng(8)
    ut, it = rng.standard_normal((20, 8)) * 0.1, rng.standard_normal((30, 8)) * 0.1
    towers = tuple(([rng.standard_normal((8, 12)) * 0.3, rng.standard_normal((12, 8)) * 0.3], [np.zeros(12), np.zeros(8)]) for _ in range(2))
    u, i = rng.integers(0, 20, 16), rng.permutation(30)[:16]
    masks = ([np.ones((16, 12))], [np.ones((16, 12))])
    plain = fc.step_f64(ut, it, towers, u, i, {}, 0.1, masks)
    feat = rng.standard_normal((20, 3))
    zero = fc.step_f64(ut, it, towers, u, i, {"user": (feat, np.zeros(3), np.ones(3), np.zeros((3, 8)), 0.0)}, 0.1, masks)
    assert zero["loss"] == plain["loss"] and np.array_equal(zero["due"], plain["due"])
    assert np.allclose(zero["dp"]["user"], feat[u].T @ plain["due"], rtol=1e-12, atol=1e-15)      # dP = z^T dL/d(input)
    on = fc.step_f64(ut, it, towers, u, i, {"user": (feat, np.zeros(3), np.ones(3), rng.standard_normal((3, 8)), 0.0)}, 0.1, masks)
    assert on["loss"] != plain["loss"]


# ------------------------------------------------------------------------------------------ config, YAML, CLI
def test_config_validation_yaml_and_cli():
    base = dict(n_users=10, n_items=10)
    TwoTowerConfig(**base, n_user_features=32, n_item_features=1, feature_clip=2.5).validate()
    TwoTowerConfig(**base, n_user_features=5).validate()
    TwoTowerConfig(**base, n_item_features=5, candidate_sampling="mixed", n_sampled_negatives=8).validate()   # mixed sampling works
    for bad in (dict(n_user_features=-1), dict(n_user_features=33), dict(n_item_features=-1), dict(n_item_features=33),
                dict(n_item_features=2.0), dict(n_user_features=True)):
        with pytest.raises(ValueError, match="features"):
            TwoTowerConfig(**base, **bad).validate()
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="feature_clip"):
            TwoTowerConfig(**base, n_user_features=3, feature_clip=bad).validate()
    from two_tower_amazon_recommender_amd import config, train
    doc = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                     "features": {"numeric": {"source": "rating_stats", "clip": 3.0}, "title": {"buckets": 50}}}}
    assert config.numeric_features_from_dict(doc) == {"source": "rating_stats", "clip": 3.0}
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.feature_clip, cfg.n_user_features, cfg.n_item_features, cfg.n_title_buckets) == (3.0, 0, 0, 50)
    doc["model"]["features"]["numeric"] = {"source": "none"}
    assert config.numeric_features_from_dict(doc) == {"source": "none", "clip": 0.0}
    doc["model"]["features"]["numeric"] = {"source": "text_length"}
    with pytest.raises(ValueError, match="source"):
        config.numeric_features_from_dict(doc)
    doc["model"]["features"]["numeric"] = {"source": "rating_stats", "clip": -1}
    with pytest.raises(ValueError, match="clip"):
        config.model_config_from_dict(doc, 10, 10)
    del doc["model"]["features"]
    assert config.numeric_features_from_dict(doc) == {"source": "none", "clip": 0.0}
    assert config.model_config_from_dict(doc, 10, 10)[0].feature_clip == 0.0
    args = train.parse(["--config", "x.yaml", "--side-features", "rating_stats", "--feature-clip", "2.5", "--user-features", "u.npy",
                        "--item-features", "i.npy"])
    assert (args.side_features, args.feature_clip, args.user_features, args.item_features) == ("rating_stats", 2.5, "u.npy", "i.npy")
    args = train.parse(["--config", "x.yaml"])
    assert args.side_features is None and args.feature_clip is None and args.user_features is None and args.item_features is None
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--side-features", "text_length"])


def test_distributed_cli_and_the_sharded_trainer_refuse_the_feature(tmp_path):
    from two_tower_amazon_recommender_amd import train
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n")
    with pytest.raises(NotImplementedError, match="numeric side features"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--side-features", "rating_stats", "--distributed"])
    with pytest.raises(NotImplementedError, match="numeric side features"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--item-features", "i.npy", "--distributed"])
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n"
                    "  features:\n    numeric:\n      source: rating_stats\n")
    with pytest.raises(NotImplementedError, match="numeric side features"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--distributed"])
    for kw in (dict(n_user_features=5), dict(n_item_features=2)):
        with pytest.raises(NotImplementedError, match="numeric side features"):
            ShardedTwoTowerTrainer(TwoTowerConfig(n_users=10, n_items=10, **kw), "cpu", seed=1)


def test_graph_capture_refuses_the_feature():
    class Stub:
        mixed = False
    for kw in (dict(n_user_features=5), dict(n_item_features=2)):
        s = Stub()
        s.cfg = TwoTowerConfig(n_users=10, n_items=10, **kw)
        with pytest.raises(NotImplementedError, match="numeric side features"):
            TwoTowerTrainer.capture_graph(s)


def test_feature_off_keeps_the_fields_in_front_of_the_history_block_and_the_checkpoint_keys():
    cfg = TwoTowerConfig(n_users=10, n_items=10)
    assert (cfg.n_user_features, cfg.n_item_features, cfg.feature_clip) == (0, 0, 0.0)
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]
    k = names.index("user_history_len")
    assert names[k - 3:k] == ["n_user_features", "n_item_features", "feature_clip"]
    assert names[-3:] == ["n_title_buckets", "title_max_tokens", "title_pooling"]

    class Stub:
        pass
    for sides in ((), ("user",), ("user", "item")):
        s = Stub()
        s.cfg = TwoTowerConfig(n_users=10, n_items=10, optimizer="adagrad", n_user_features=5 if "user" in sides else 0,
                               n_item_features=5 if "item" in sides else 0)
        s.dense_flat, s.dense_accum = "dense_flat", "dense_accum"
        s.tables = {p: EmbeddingTable.new(s.cfg, "cpu", p, 0, 10, None) for p in ("user", "item")}     # (the records: CPU tensors)
        s.sides = {side: FeatureSide(side, f"{side}_features", f"{side}_feature_mean", f"{side}_feature_inv_std", None, None, None, 1)
                   for side in sides}
        s.step_index, s.dropout_seed, s.adam_step = 0, 0, 1
        more = {f"{side}{k}" for side in sides for k in ("_features", "_feature_mean", "_feature_inv_std")}
        assert set(TwoTowerTrainer.state_dict(s)) == {"config", "user_table", "item_table", "dense", "step_index", "dropout_seed",
                                                      "user_accum", "item_accum", "dense_accum"} | more


# ------------------------------------------------------------------------------------------ the C ABI
def _fwd_prob(**kw):
    one = 16                                    # a non-null, aligned address that is never dereferenced: every call fails first
    d = dict(feat=one, feat_rows=10, F=5, accumulate=0, ids=one, n=4, mean=one, inv_std=one, proj=one, out=one, z_out=None)
    d.update(kw)
    return _lib.DenseFeaturesFwdArgs(**d)


def test_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    fwd, bwd = lib.tt_dense_features_fwd_f32, lib.tt_dense_features_bwd_f32
    arr = lambda *p: (type(p[0]) * len(p))(*p)
    assert fwd(None, 1, 32, 0.0, None, None) == E and b"null" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob()), 0, 32, 0.0, None, None) == E and b"n_probs" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob()), 3, 32, 0.0, None, None) == E
    assert fwd(arr(_fwd_prob()), 1, 30, 0.0, None, None) == E and b"multiple of 4" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob()), 1, 0, 0.0, None, None) == E and fwd(arr(_fwd_prob()), 1, 2048, 0.0, None, None) == E
    assert fwd(arr(_fwd_prob()), 1, 32, -1.0, None, None) == E and b"clip" in lib.tt_last_error()
    for F in (0, 33, -1):
        assert fwd(arr(_fwd_prob(F=F)), 1, 32, 0.0, None, None) == E and b"F must be in 1..32" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob(), _fwd_prob(F=40)), 2, 32, 0.0, None, None) == E and b"problem 1" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob(mean=None)), 1, 32, 0.0, None, None) == E and b"both or neither" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob(inv_std=None)), 1, 32, 0.0, None, None) == E and b"both or neither" in lib.tt_last_error()
    for k in ("feat", "proj", "out", "ids"):
        assert fwd(arr(_fwd_prob(**{k: None})), 1, 32, 0.0, None, None) == E and b"null" in lib.tt_last_error(), k
    assert fwd(arr(_fwd_prob(out=20)), 1, 32, 0.0, None, None) == E and b"aligned" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob(proj=20)), 1, 32, 0.0, None, None) == E and b"aligned" in lib.tt_last_error()
    assert fwd(arr(_fwd_prob(n=-1)), 1, 32, 0.0, None, None) == E and fwd(arr(_fwd_prob(feat_rows=0)), 1, 32, 0.0, None, None) == E
    assert b"tt_dense_features_fwd_f32" in lib.tt_last_error()               # the messages name the entry that was called
    assert fwd(arr(_fwd_prob(n=0, ids=None), _fwd_prob(n=0)), 2, 32, 0.0, None, None) == _lib.TT_OK    # no rows: nothing launched

    def bp(**kw):
        d = dict(z=16, dy=16, n=4, F=5, n_slabs=2, dp_slabs=16)
        d.update(kw)
        return _lib.DenseFeaturesBwdArgs(**d)
    assert bwd(None, 1, 32, None) == E and bwd(arr(bp()), 3, 32, None) == E and bwd(arr(bp()), 0, 32, None) == E
    assert bwd(arr(bp()), 1, 6, None) == E and b"multiple of 4" in lib.tt_last_error()
    for F in (0, 33):
        assert bwd(arr(bp(F=F)), 1, 32, None) == E and b"F must be in 1..32" in lib.tt_last_error()
    assert bwd(arr(bp(n_slabs=0)), 1, 32, None) == E and b"n_slabs" in lib.tt_last_error()
    assert bwd(arr(bp(n=-1)), 1, 32, None) == E
    for k in ("z", "dy", "dp_slabs"):
        assert bwd(arr(bp(**{k: None})), 1, 32, None) == E and b"null" in lib.tt_last_error(), k
    assert bwd(arr(bp(dy=20)), 1, 32, None) == E and b"aligned" in lib.tt_last_error()
    assert b"tt_dense_features_bwd_f32" in lib.tt_last_error()


def test_slab_query_struct_sizes_and_signatures():
    lib = _lib.load()
    assert lib.tt_dense_features_num_slabs(8192) == 64 and lib.tt_dense_features_num_slabs(77) == 1
    assert lib.tt_dense_features_num_slabs(1000) == 8 and lib.tt_dense_features_num_slabs(129) == 2
    assert lib.tt_dense_features_num_slabs(0) == 1 and lib.tt_dense_features_num_slabs(10 ** 7) == 64
    assert ops.dense_features_num_slabs(8192 + 64) == 64
    assert lib.tt_abi_struct_bytes(14) == C.sizeof(_lib.DenseFeaturesFwdArgs) == 80
    assert lib.tt_abi_struct_bytes(15) == C.sizeof(_lib.DenseFeaturesBwdArgs) == 40
    assert _lib.FEATURES_STRUCT_INDEX == {"DenseFeaturesFwdArgs": 14, "DenseFeaturesBwdArgs": 15}
    assert lib.tt_abi_struct_bytes(13) == -1 and lib.tt_abi_struct_bytes(16) == -1
    header = (ROOT / "include" / "twotower_hip.h").read_text()
    for name in ("tt_dense_features_fwd_f32", "tt_dense_features_bwd_f32", "tt_dense_features_num_slabs"):
        m = re.search(rf"int(?:32_t)? {name}\((.*?)\);", header, re.S)
        params = [p.strip() for p in m.group(1).split(",")]
        kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "tt_stream_t": C.c_void_p}
        want = [("ptr" if "*" in p else kinds[p.split()[0]]) for p in params]
        got = [("ptr" if (a is C.c_void_p and "*" in p) or hasattr(a, "contents") else a) for a, p in zip(_lib.SIGNATURES[name][1], params)]
        assert want == got, name
    # the mirrors' fields are the header's, in order
    for struct, mirror in (("tt_dense_features_fwd_args", _lib.DenseFeaturesFwdArgs), ("tt_dense_features_bwd_args", _lib.DenseFeaturesBwdArgs)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
        assert fields == [f[0] for f in mirror._fields_], struct


def test_ops_and_the_custom_op_exist_and_have_a_meta_implementation():
    from two_tower_amazon_recommender_amd import torch_ops
    assert callable(ops.dense_features) and callable(ops.dense_features_bwd) and ops.MAX_DENSE_FEATURES == 32
    for name in ("dense_features", "dense_features_bwd"):
        assert name in torch_ops.OPS and hasattr(torch.ops.twotower, name)
    feat, proj = torch.empty(100, 5, device="meta"), torch.empty(5, 32, device="meta")
    ids, st = torch.empty(7, dtype=torch.int64, device="meta"), torch.empty(5, device="meta")
    assert torch.ops.twotower.dense_features(feat, ids, st, st, proj, 2.5).shape == (7, 32)
    assert torch.ops.twotower.dense_features(feat, ids, None, None, proj, 0.0).shape == (7, 32)
    assert torch.ops.twotower.dense_features_bwd(feat, ids, st, st, proj, torch.empty(7, 32, device="meta"), 0.0).shape == (5, 32)
    with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel, no fallback
        torch.ops.twotower.dense_features(torch.zeros(10, 5), torch.zeros(2, dtype=torch.int64), None, None, torch.zeros(5, 8), 0.0)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        ops.dense_features((torch.zeros(10, 5), torch.zeros(2, dtype=torch.int64), None, None, torch.zeros(5, 8), None, False, None))
    with pytest.raises(ValueError, match="one or two"):
        ops.dense_features()

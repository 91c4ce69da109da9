"""Layer normalisation of the tower hidden layers, the parts that need no GPU: the restatements of tests/layernorm_check.py
against torch, the f32 error on the GPU tests' problems, the config's refusals, the dense layout, the YAML block and the CLI."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import layernorm_check as lc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod, train
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, dense_layout


# ------------------------------------------------------------------------------------------ 1. the restatements
@pytest.mark.parametrize("n,d", [(37, 32), (130, 96), (33, 1024)])
@pytest.mark.parametrize("eps", lc.EPSILONS)
def test_f64_restatement_is_torch_layer_norm_and_its_autograd(n, d, eps):
    p = lc.problem(n, d)
    z, gamma, beta = (torch.tensor(p[k].astype(np.float64), requires_grad=True) for k in ("z", "gamma", "beta"))
    y = torch.nn.functional.layer_norm(z, (d,), gamma, beta, eps)
    y.backward(torch.tensor(p["dn"].astype(np.float64)))
    got, _, _ = lc.layer_forward(p["z"], p["gamma"], p["beta"], eps)
    assert lc.rel_err(got, y.detach().numpy()) <= 1e-13
    assert np.array_equal(lc.layer_forward(p["z"], p["gamma"], p["beta"], eps, relu=True)[0], np.maximum(got, 0.0))
    b = lc.layer_backward(p["z"], p["gamma"], p["dn"], eps)
    for k, t in (("dz", z), ("dgamma", gamma), ("dbeta", beta)):
        assert lc.rel_err(b[k], t.grad.numpy()) <= 1e-12, k
    # the sums of the slabs' row ranges are the whole sum
    parts = [lc.layer_backward(p["z"], p["gamma"], p["dn"], eps, rows=r) for r in lc.slab_rows(n, 4)]
    assert lc.rel_err(sum(q["dgamma"] for q in parts), b["dgamma"]) <= 1e-13
    assert lc.slab_rows(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)] and lc.slab_rows(0, 2) == [(0, 0), (0, 0)]


@pytest.mark.parametrize("n,d", lc.SHAPES)
def test_f32_restatement_stays_within_the_kernel_bar_with_headroom(n, d):
    """The GPU tests' bar is 1e-5 of max |ref|: the same arithmetic in f32, sums in index order, stays at or below 2.5e-6 on
    exactly their problems - a different reduction order has 4x headroom at least."""
    p = lc.problem(n, d)
    for eps in lc.EPSILONS:
        y32, _, _ = lc.layer_forward_f32(p["z"], p["gamma"], p["beta"], eps)
        y64, _, _ = lc.layer_forward(p["z"], p["gamma"], p["beta"], eps)
        b32, b64 = lc.layer_backward_f32(p["z"], p["gamma"], p["dn"], eps), lc.layer_backward(p["z"], p["gamma"], p["dn"], eps)
        errs = dict(y=lc.rel_err(y32, y64), **{k: lc.rel_err(b32[k], b64[k]) for k in ("dz", "dgamma", "dbeta")})
        print(n, d, eps, {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= 2.5e-6, errs
        assert np.array_equal(y32 > 0, y64 > 0)              # no ReLU sign flips between f32 and f64 on these problems


# ------------------------------------------------------------------------------------------ 2. the config
def _cfg(**kw):
    base = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[64, 32])
    base.update(kw)
    return TwoTowerConfig(**base)


def test_validate_refusals():
    _cfg(layer_norm=True).validate()
    _cfg(layer_norm=True, layer_norm_epsilon=1e-5, tower_dims=[1024, 96, 32]).validate()
    assert TwoTowerConfig.layer_norm is False and TwoTowerConfig.layer_norm_epsilon == 1e-3
    with pytest.raises(ValueError, match="layer_norm must be a bool"):
        _cfg(layer_norm=1).validate()
    for eps in (0.0, -1e-3, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="layer_norm_epsilon"):
            _cfg(layer_norm_epsilon=eps).validate()
    with pytest.raises(ValueError, match="hidden layer"):
        _cfg(layer_norm=True, tower_dims=[32]).validate()
    with pytest.raises(ValueError, match="hidden layer"):
        _cfg(layer_norm=True, tower_dims=[64, 32], item_tower_dims=[32]).validate()
    for dims in ([48, 32], [2048, 32], [64, 16, 32], [36, 32]):
        with pytest.raises(ValueError, match="multiples of 32"):
            _cfg(layer_norm=True, tower_dims=dims).validate()
    with pytest.raises(ValueError, match="multiples of 32"):
        _cfg(layer_norm=True, item_tower_dims=[40, 32]).validate()
    _cfg(tower_dims=[36, 32]).validate()                     # without the option 36 is as fine as before
    _cfg(tower_dims=[32]).validate()
    # the new fields sit in front of cross_layers: every later field keeps its place
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]
    k = names.index("cross_layers")
    assert names[k - 3:k] == ["rating_hidden", "layer_norm", "layer_norm_epsilon"]


# ------------------------------------------------------------------------------------------ 3. the layout
FULL = dict(n_category_buckets=30, n_title_buckets=100, n_user_features=5, n_item_features=5, user_history_len=5,
            history_pooling="attention", rating_weight=0.5, rating_hidden=64, cross_layers=2)


@pytest.mark.parametrize("extra", [{}, FULL, dict(item_tower_dims=[96, 64, 32]), dict(tower_dims=[512, 256, 128], embedding_dim=128)])
def test_norm_block_sits_last_and_moves_nothing(extra):
    off, on = dense_layout(_cfg(**extra)), dense_layout(_cfg(layer_norm=True, **extra))
    cfg = _cfg(layer_norm=True, **extra)
    assert list(on.blocks)[:len(off.blocks)] == list(off.blocks)
    for name, blk in off.blocks.items():
        assert on.blocks[name] == blk, name                                   # every earlier offset, shape and initialiser
    assert on.segments[:-1] == off.segments
    seg = on.segments[-1]
    assert (seg.name, seg.group, seg.l2) == ("norm", "norm", False)
    assert seg.lo == (off.total + 3) // 4 * 4 and seg.lo % 4 == 0 and seg.hi == on.total
    hidden = [cfg.user_dims[:-1], cfg.item_dims[:-1]]
    assert seg.size == seg.stride == 2 * sum(sum(h) for h in hidden)
    # [user gamma_0.. | item gamma_0.. | user beta_0.. | item beta_0..], gammas filled with 1, betas with 0, no initialiser
    want, pos = [], seg.lo
    for kind, fill in (("g", 1.0), ("b", 0.0)):
        for side, dims in zip(("user", "item"), hidden):
            for l, n in enumerate(dims):
                want.append((f"norm.{side}.{kind}{l}", pos, (n,), fill))
                pos += n
    got = [(b.name, b.offset, b.shape, b.fill) for b in on.blocks.values() if b.name.startswith("norm.")]
    assert got == want and pos == on.total
    assert all(b.glorot is None and b.offset % 4 == 0 for b in on.blocks.values() if b.name.startswith("norm."))
    assert all(b.fill == 0.0 for b in off.blocks.values())
    assert cfg.dense_segment_count() == len(off.segments) + 1


def test_segment_counts_and_the_limit_blames_the_norm_block():
    ref = _cfg(tower_dims=[512, 256, 128], embedding_dim=128, layer_norm=True)
    ref.validate()
    assert ref.dense_segment_count() == 13                                    # the reference's towers: 12 + 1
    full = {k: v for k, v in FULL.items() if k != "history_pooling"}
    everything = _cfg(layer_norm=True, normalize_embeddings=True, **full)
    everything.validate()
    assert everything.dense_segment_count() == 15
    # three-layer towers with numeric features and a rating head hold 16 segments: the norm block is the one past the limit
    sixteen = dict(tower_dims=[64, 64, 32], n_user_features=3, n_item_features=3, rating_weight=0.5)
    _cfg(**sixteen).validate()
    with pytest.raises(NotImplementedError, match="layer normalisation adds one dense segment"):
        _cfg(layer_norm=True, **sixteen).validate()
    with pytest.raises(NotImplementedError, match="cross layers"):           # an earlier block crosses it first: blamed instead
        _cfg(layer_norm=True, **sixteen, cross_layers=1).validate()


# ------------------------------------------------------------------------------------------ 4. YAML and CLI
def _doc(block):
    m = dict(embedding_dim=32, user_tower_dims=[64, 32], item_tower_dims=[64, 32])
    if block is not None:
        m["layer_norm"] = block
    return {"model": m}


def test_yaml_block():
    assert cfgmod.layer_norm_from_dict(_doc(None)) == {"enabled": False, "epsilon": 1e-3}
    assert cfgmod.layer_norm_from_dict(_doc({"enabled": True})) == {"enabled": True, "epsilon": 1e-3}
    assert cfgmod.layer_norm_from_dict(_doc({"enabled": True, "epsilon": 1e-5})) == {"enabled": True, "epsilon": 1e-5}
    assert cfgmod.layer_norm_from_dict({}) == {"enabled": False, "epsilon": 1e-3}
    cfg, _ = cfgmod.model_config_from_dict(_doc({"enabled": True, "epsilon": 0.01}), 10, 10)
    assert cfg.layer_norm is True and cfg.layer_norm_epsilon == 0.01
    cfg, _ = cfgmod.model_config_from_dict(_doc(None), 10, 10)
    assert cfg.layer_norm is False and cfg.layer_norm_epsilon == 1e-3
    with pytest.raises(ValueError, match="unknown keys"):
        cfgmod.layer_norm_from_dict(_doc({"enabled": True, "center": False}))
    with pytest.raises(ValueError, match="mapping"):
        cfgmod.layer_norm_from_dict(_doc(True))
    with pytest.raises(ValueError, match="enabled must be a bool"):
        cfgmod.layer_norm_from_dict(_doc({"enabled": 1}))
    for eps in (0, -1.0, "small", True, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            cfgmod.layer_norm_from_dict(_doc({"enabled": True, "epsilon": eps}))


def test_cli_arguments(tmp_path):
    a = train.parse(["--config", "x.yaml"])
    assert a.layer_norm is False and a.layer_norm_epsilon is None
    a = train.parse(["--config", "x.yaml", "--layer-norm", "--layer-norm-epsilon", "1e-5"])
    assert a.layer_norm is True and a.layer_norm_epsilon == 1e-5
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n")
    with pytest.raises(SystemExit, match="needs --layer-norm"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--layer-norm-epsilon", "1e-5"])
    with pytest.raises(SystemExit, match="finite number > 0"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--layer-norm", "--layer-norm-epsilon", "0"])
    with pytest.raises(NotImplementedError, match="layer normalisation"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--layer-norm", "--distributed"])


# ------------------------------------------------------------------------------------------ 5. the C entries
def test_c_entries_validate_before_any_launch_and_the_mirrors_have_the_library_sizes():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    err = lib.tt_last_error
    A = 4096                                                                  # a non-null aligned address, never dereferenced
    fwd = lambda probs, n, dim, eps=1e-3, rate=0.0: lib.tt_layer_norm_fwd_f32(probs, n, dim, eps, 1, rate, 0, 0, None)
    bwd = lambda probs, n, dim, eps=1e-3, ns=1, stride=0: lib.tt_layer_norm_bwd_f32(probs, n, dim, eps, ns, stride, None)
    F, B = _lib.LayerNormFwdArgs, _lib.LayerNormBwdArgs
    one = (F * 1)(F(A, A, A, 2 * A, None, 0, 4))
    assert fwd(None, 1, 32) == E and fwd(one, 3, 32) == E and b"n_probs" in err()
    for dim in (0, 16, 48, 1056):
        assert fwd(one, 1, dim) == E and b"multiple of 32" in err()
    assert fwd(one, 1, 32, eps=0.0) == E and b"eps" in err()
    assert fwd(one, 1, 32, rate=1.0) == E and b"drop_rate" in err()
    assert fwd((F * 1)(F(A, A, A, 2 * A, None, 0, -1)), 1, 32) == E and b"rows" in err()
    assert fwd((F * 1)(F(A, A, A, None, None, 0, 4)), 1, 32) == E and b"null" in err()
    assert fwd((F * 1)(F(A, A + 4, A, 2 * A, None, 0, 4)), 1, 32) == E and b"aligned" in err()
    assert fwd((F * 1)(F(A, A, A, A, None, 0, 4)), 1, 32) == E and b"alias" in err()
    assert b"tt_layer_norm_fwd_f32" in err()
    assert fwd((F * 2)(F(rows=0), F(rows=0)), 2, 1024) == _lib.TT_OK             # no rows: no launch
    ok = (B * 1)(B(A, A, 2 * A, 2 * A, 3 * A, 3 * A, 4))
    assert bwd(None, 1, 32) == E and bwd(ok, 0, 32) == E and b"n_probs" in err()
    assert bwd(ok, 1, 40) == E and b"multiple of 32" in err()
    assert bwd(ok, 1, 32, eps=-1.0) == E and b"eps" in err()
    assert bwd(ok, 1, 32, ns=0) == E and b"n_slabs" in err()
    assert bwd(ok, 1, 32, ns=2, stride=63) == E and b"slab_stride" in err()
    assert bwd((B * 1)(B(A, A, 2 * A, 2 * A, None, 3 * A, 4)), 1, 32) == E and b"null" in err()
    assert bwd((B * 1)(B(A, A, 2 * A, 2 * A + 4, 3 * A, 3 * A, 4)), 1, 32) == E and b"aligned" in err()
    assert bwd((B * 1)(B(A, A, 2 * A, A, 3 * A, 3 * A, 4)), 1, 32) == E and b"alias" in err()
    assert b"tt_layer_norm_bwd_f32" in err()
    assert bwd((B * 2)(B(rows=0), B(rows=0)), 2, 64) == _lib.TT_OK
    assert lib.tt_layer_norm_num_slabs(8192) == 256 and lib.tt_layer_norm_num_slabs(1000) == 32
    assert lib.tt_layer_norm_num_slabs(0) == 1 and lib.tt_layer_norm_num_slabs(1) == 1 and lib.tt_layer_norm_num_slabs(1 << 20) == 256
    assert lib.tt_abi_struct_bytes(21) == C.sizeof(F) == 56 and lib.tt_abi_struct_bytes(22) == C.sizeof(B) == 56
    assert _lib.LAYER_NORM_STRUCT_INDEX == {"LayerNormFwdArgs": 21, "LayerNormBwdArgs": 22}
    assert lib.tt_abi_version() == _lib.ABI_VERSION == 10


def test_custom_ops_are_registered():
    from two_tower_amazon_recommender_amd import torch_ops
    for name in ("layer_norm", "layer_norm_bwd"):
        assert name in torch_ops.OPS and hasattr(torch.ops.twotower, name)

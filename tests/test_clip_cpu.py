"""Global-norm gradient clipping and the learning-rate schedule, the parts that need no GPU: the schedule's closed forms, the
config's refusals, the YAML keys and the CLI, the restatements of tests/clip_check.py against a per-occurrence expansion, the
f32 margin on the GPU test's inputs and the C ABI's refusals."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import clip_check as cc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod, train
from two_tower_amazon_recommender_amd.trainer import _GRAPH_REFUSALS, LR_DECAYS, TwoTowerConfig


def _cfg(**kw):
    base = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[64, 32], learning_rate=0.05)
    base.update(kw)
    return TwoTowerConfig(**base)


# ------------------------------------------------------------------------------------------ 1. the schedule
def closed_form(P, s, W, decay, T, m):
    if s < W:
        return P * (s + 1) / W
    t = s - W
    if decay == "none":
        return P
    if decay == "cosine":
        return P * (m + (1 - m) * 0.5 * (1 + math.cos(math.pi * min(t, T) / T)))
    if decay == "linear":
        return P * (m + (1 - m) * (1 - min(t, T) / T))
    return P * max(m, math.sqrt(max(W, 1) / (s + 1)))


@pytest.mark.parametrize("decay", LR_DECAYS)
@pytest.mark.parametrize("W", [0, 1, 100])
@pytest.mark.parametrize("m", [0.0, 0.1])
def test_learning_rate_at_is_the_closed_form_and_never_rises_after_the_warm_up(decay, W, m):
    P, T = 0.05, 40
    cfg = _cfg(lr_warmup_steps=W, lr_decay=decay, lr_decay_steps=T, lr_min_ratio=m)
    cfg.validate()
    for s in {0, max(W - 1, 0), W, W + T // 2, W + T, W + T + 10}:
        want = closed_form(P, s, W, decay, T, m)
        assert abs(cfg.learning_rate_at(s) - want) <= 1e-15 * abs(want), (s, cfg.learning_rate_at(s), want)
    if W:
        assert cfg.learning_rate_at(0) == P / W and cfg.learning_rate_at(W - 1) == P     # the warm-up ends AT the peak
    rates = [cfg.learning_rate_at(s) for s in range(W, W + T + 20)]
    # (inverse_sqrt as defined starts its decay inside the warm-up's last step: sqrt(W / (W + 1)) of the peak at step W)
    first = P * math.sqrt(max(W, 1) / (W + 1)) if decay == "inverse_sqrt" else P
    assert rates[0] == pytest.approx(first, rel=1e-15) and all(b <= a <= P for a, b in zip(rates, rates[1:]))
    assert min(rates) >= m * P * (1 - 1e-15)
    if decay in ("cosine", "linear"):
        assert rates[T] == pytest.approx(m * P, rel=1e-12, abs=1e-18) and rates[-1] == rates[T]
    assert cfg.lr_schedule_on == (W > 0 or decay != "none")


def test_no_schedule_is_the_configured_rate_itself():
    cfg = _cfg(learning_rate=0.001)
    assert not cfg.lr_schedule_on and all(cfg.learning_rate_at(s) is cfg.learning_rate for s in (0, 1, 10 ** 9))
    assert (TwoTowerConfig.global_clipnorm, TwoTowerConfig.lr_warmup_steps, TwoTowerConfig.lr_decay, TwoTowerConfig.lr_decay_steps,
            TwoTowerConfig.lr_min_ratio) == (0.0, 0, "none", 0, 0.0)
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]               # beside the optimizer's other settings
    k = names.index("global_clipnorm")
    assert names[k - 1] == "adam_epsilon" and names[k:k + 6] == ["global_clipnorm", "lr_warmup_steps", "lr_decay", "lr_decay_steps",
                                                                 "lr_min_ratio", "batch_size"]


# ------------------------------------------------------------------------------------------ 2. the config
def test_validate_refusals():
    _cfg(global_clipnorm=1.0, lr_warmup_steps=3, lr_decay="cosine", lr_decay_steps=1, lr_min_ratio=1.0).validate()
    _cfg(lr_decay="inverse_sqrt").validate()                                   # needs no decay_steps
    for c in (-1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="global_clipnorm"):
            _cfg(global_clipnorm=c).validate()
    for w in (-1, 1.5, True):
        with pytest.raises(ValueError, match="lr_warmup_steps"):
            _cfg(lr_warmup_steps=w).validate()
    for t in (-1, 2.0, True):
        with pytest.raises(ValueError, match="lr_decay_steps"):
            _cfg(lr_decay="linear", lr_decay_steps=t).validate()
    with pytest.raises(ValueError, match="lr_decay must be one of"):
        _cfg(lr_decay="exponential").validate()
    for decay in ("cosine", "linear"):
        with pytest.raises(ValueError, match="lr_decay_steps >= 1"):
            _cfg(lr_decay=decay).validate()
    for m in (-0.1, 1.1, float("nan"), True):
        with pytest.raises(ValueError, match="lr_min_ratio"):
            _cfg(lr_min_ratio=m).validate()
    # both options refuse graph replay
    on = [what for refused, what in _GRAPH_REFUSALS if refused(_cfg(global_clipnorm=1.0, lr_warmup_steps=2))]
    assert len(on) == 2 and "global_clipnorm" in on[0] and "schedule" in on[1]
    assert not [what for refused, what in _GRAPH_REFUSALS if refused(_cfg())]


# ------------------------------------------------------------------------------------------ 3. YAML and CLI
def _doc(training_extra=None):
    tr = {"batch_size": 64, "learning_rate": 0.01, "epochs": 2}
    tr.update(training_extra or {})
    return {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "training": tr,
                      "retrieval": {"temperature": 0.1}}}


def test_yaml_keys():
    cfg, loop = cfgmod.model_config_from_dict(_doc(), 10, 10)
    assert cfg.global_clipnorm == 0.0 and not cfg.lr_schedule_on and "lr_decay_steps" not in loop
    doc = _doc({"global_clipnorm": 2, "lr_schedule": {"warmup_steps": 5, "decay": "cosine", "decay_steps": 70, "min_ratio": 0.1}})
    cfg, _ = cfgmod.model_config_from_dict(doc, 10, 10)
    assert (cfg.global_clipnorm, cfg.lr_warmup_steps, cfg.lr_decay, cfg.lr_decay_steps, cfg.lr_min_ratio) == (2.0, 5, "cosine", 70, 0.1)
    cfg.validate()
    assert cfg.learning_rate == 0.01 and cfg.learning_rate_at(4) == 0.01 and cfg.learning_rate_at(0) == 0.01 / 5
    doc = _doc({"lr_schedule": {"decay": "linear", "decay_steps": "auto"}})
    assert cfgmod.optimization_from_dict(doc)["decay_steps"] == "auto"
    assert cfgmod.model_config_from_dict(doc, 10, 10)[0].lr_decay_steps == 0         # train.py resolves it
    for bad, match in (({"lr_schedule": {"warmup": 3}}, "unknown keys"), ({"lr_schedule": {"decay": "step"}}, "decay must be one of"),
                       ({"lr_schedule": [1]}, "mapping"), ({"lr_schedule": {"warmup_steps": -1}}, "warmup_steps"),
                       ({"lr_schedule": {"decay_steps": "all"}}, "decay_steps"), ({"lr_schedule": {"min_ratio": 2}}, "min_ratio"),
                       ({"global_clipnorm": -1}, "global_clipnorm"), ({"global_clipnorm": "x"}, "global_clipnorm")):
        with pytest.raises(ValueError, match=match):
            cfgmod.optimization_from_dict(_doc(bad))


def test_cli_flags_and_the_distributed_refusals(tmp_path):
    import yaml
    args = train.parse(["--config", "x.yaml", "--global-clipnorm", "1.5", "--lr-warmup-steps", "3", "--lr-decay", "cosine",
                        "--lr-decay-steps", "auto", "--lr-min-ratio", "0.1"])
    assert (args.global_clipnorm, args.lr_warmup_steps, args.lr_decay, args.lr_decay_steps, args.lr_min_ratio) == (1.5, 3, "cosine", "auto", 0.1)
    none = train.parse(["--config", "x.yaml"])
    assert (none.global_clipnorm, none.lr_warmup_steps, none.lr_decay, none.lr_decay_steps, none.lr_min_ratio) == (None,) * 5
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--lr-decay", "exponential"])
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(_doc()))
    for flags in (["--global-clipnorm", "1"], ["--lr-warmup-steps", "3"], ["--lr-decay", "inverse_sqrt"]):
        with pytest.raises(NotImplementedError, match="row-sharded"):            # before any device or process group is touched
            train.main(["--config", str(path), "--synthetic", "1000", "--distributed"] + flags)
    path.write_text(yaml.safe_dump(_doc({"global_clipnorm": 1.0})))
    with pytest.raises(NotImplementedError, match="row-sharded"):
        train.main(["--config", str(path), "--synthetic", "1000", "--distributed"])
    with pytest.raises(SystemExit, match="lr-decay-steps"):
        train.main(["--config", str(path), "--synthetic", "1000", "--lr-decay-steps", "many"])


# ------------------------------------------------------------------------------------------ 4. the restatement
def _tiny(seed=0):
    rng = np.random.default_rng(seed)
    g = lambda n, d: rng.standard_normal((n, d)).astype(np.float32)
    ids = np.array([[3, -1, 7], [-1, -1, -1], [0, 1, 2], [5, -1, -1]], dtype=np.int64)          # bags of 2, 0, 3 and 1 kept slots
    slot_ids = np.array([4, -1, 9, -1, -1, 2], dtype=np.int64)
    masked = g(6, 4)
    masked[[1, 3, 4]] = 1e30                                                                    # stale rows of skipped slots
    bufs = [(g(4, 8), 1.0, ids, "sum"), (g(4, 8), 1.0, ids, "mean"), (g(4, 8), 0.0, ids, "sqrtn"), (masked, 0.0, slot_ids, "mask"),
            (g(5, 4), 2.0, None, "rows"), (g(4, 4), 2.0, ids, "mean")]
    dense = [(g(3, 7), 5, 3, 7), (g(1, 6), 6, 1, 6)]
    return bufs, dense, ids


def test_global_norm_is_the_per_occurrence_expansion():
    bufs, dense, ids = _tiny()
    assert cc.sumsq(bufs, dense) == pytest.approx(cc.brute_force_sumsq(bufs, dense), rel=1e-13)
    for one in bufs:                                                                            # and buffer by buffer
        assert cc.sumsq([one], []) == pytest.approx(cc.brute_force_sumsq([one], []), rel=1e-13), one[3]
    assert np.isfinite(cc.global_norm(bufs, dense))                                             # the 1e30 rows did not count
    # an empty bag adds nothing under every pooling; with a weight it counts that often
    assert [list(cc.row_factors(4, 0.0, ids, m)) for m in ("sum", "mean", "sqrtn")] == [[2, 0, 3, 1], [0.5, 0, 1 / 3, 1], [1, 0, 1, 1]]
    assert list(cc.row_factors(4, 2.0, ids, "mean")) == [2.5, 2, 2 + 1 / 3, 3]
    g = bufs[4][0].astype(np.float64)
    assert cc.sumsq([bufs[4]], []) == pytest.approx(2 * (g ** 2).sum(), rel=1e-14)              # weight 2: every row twice
    # the slabs are summed BEFORE they are squared
    slabs = np.array([[3.0, 1.0], [-3.0, 1.0]], dtype=np.float32)
    assert cc.sumsq([], [(slabs, 2, 2, 2)]) == 4.0
    assert cc.scale_of(8.0, 2.0) == 0.25 and cc.scale_of(1.0, 2.0) == 1.0 and cc.scale_of(2.0, 2.0) == 1.0
    assert np.isnan(cc.scale_of(np.inf, 2.0)) and np.isnan(cc.scale_of(np.nan, 2.0))


@pytest.mark.parametrize("rows,dim", [(r, d) for r in cc.ROWS for d in cc.DIMS])
def test_f32_restatement_of_the_kernels_order_stays_within_the_bar_with_headroom(rows, dim):
    """The GPU test's bar is 1e-5 of the f64 norm: the kernel's summation order in f32 (per-thread sums over a workgroup's chunks,
    butterfly, LDS, f64 over the partials) stays at or below 2.5e-6 on exactly its inputs - 4x headroom at least."""
    bufs, dense = cc.problem(rows, dim)
    ref, got = cc.global_norm(bufs, dense), float(cc.kernel_norm_f32(bufs, dense))
    print(rows, dim, ref, got, f"{abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 2.5e-6 * ref
    modes = [b[3] for b in bufs]
    assert sorted(set(modes)) == sorted(cc.MODES) and len(bufs) == 2 * len(cc.MODES)
    assert [d[1:] for d in dense[:3]] == [(c, n, s) for c, s, n in cc.DENSE]                   # (count, n_slabs, stride) of the issue's three
    assert len(bufs) + len(dense) <= _lib.TT_CLIP_MAX_BUFFERS


# ------------------------------------------------------------------------------------------ 5. the C ABI
def test_c_abi_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    B, E = _lib.ClipBuffer, _lib.TT_ERR_INVALID_ARG
    err = lambda: lib.tt_last_error()
    one = C.c_void_p(4096)                                                    # a non-null, 16-byte aligned address (never dereferenced)
    odd = C.c_void_p(4100)

    def call(bufs, c=1.0, ws=one, ws_bytes=1 << 20, stats=one):
        arr = (B * max(len(bufs), 1))(*bufs)
        return lib.tt_clip_global_norm_f32(arr, len(bufs), c, ws, ws_bytes, stats, None)
    rows = lambda **kw: B(**{**dict(data=4096, rows=8, dim=8, mode=_lib.TT_CLIP_ROWS, weight=1.0), **kw})
    dense = lambda **kw: B(**{**dict(data=4096, count=8, slab_stride=8, n_slabs=1, mode=_lib.TT_CLIP_DENSE), **kw})
    assert C.sizeof(B) == 64 == lib.tt_abi_struct_bytes(23) and _lib.CLIP_STRUCT_INDEX == {"ClipBuffer": 23}
    assert _lib.TT_CLIP_MAX_BUFFERS == 8 + _lib.TT_MAX_DENSE_SEGS == 24
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert call([rows()], c=c) == E and b"clip_norm" in err()
    assert call([rows()], stats=None) == E and b"stats" in err()
    assert call([rows()], ws=None) == E and b"workspace" in err()
    assert call([rows()], ws_bytes=0) == _lib.TT_ERR_WORKSPACE
    assert lib.tt_clip_global_norm_f32(None, 1, 1.0, one, 256, one, None) == E and b"bufs is NULL" in err()
    assert call([rows()] * 25) == E and b"n_bufs" in err()
    assert call([rows(dim=6)]) == E and b"multiple of 4" in err()
    assert call([rows(dim=0)]) == E and b"multiple of 4" in err()
    assert call([rows(data=None)]) == E and b"null pointer (data)" in err()
    assert call([rows(data=4100)]) == E and b"16-byte aligned" in err()
    assert call([rows(rows=-1)]) == E and b"rows" in err()
    assert call([rows(weight=-1.0)]) == E and b"weight" in err()
    assert call([rows(mode=9)]) == E and b"unknown mode" in err()
    for mode in (_lib.TT_CLIP_BAG_SUM, _lib.TT_CLIP_BAG_MEAN, _lib.TT_CLIP_BAG_SQRTN):
        assert call([rows(mode=mode, L=3)]) == E and b"slot_ids" in err()
        assert call([rows(mode=mode, L=0, slot_ids=4096)]) == E and b"L must be" in err()
    assert call([rows(mode=_lib.TT_CLIP_SLOT_MASK)]) == E and b"slot_ids" in err()
    assert call([dense(n_slabs=0)]) == E and b"n_slabs" in err()
    assert call([dense(count=-1)]) == E and b"count" in err()
    assert call([dense(n_slabs=2, slab_stride=7)]) == E and b"slab_stride" in err()
    assert call([dense(data=None)]) == E and b"null pointer (data)" in err()
    assert call([dense(data=4098)]) == E and b"4-byte aligned" in err()
    assert b"tt_clip_global_norm_f32" in err()                                 # the messages name the entry that was called
    # the workspace query: one f32 partial per workgroup of launch 1, a function of the shapes alone
    q = lambda bufs: lib.tt_clip_workspace_bytes((B * max(len(bufs), 1))(*bufs), len(bufs))
    assert q([]) == 256 and q([rows(rows=0), dense(count=0)]) == 256
    assert q([dense(count=4096 * 64, slab_stride=4096 * 64)]) == 1024 and q([dense(count=10 ** 7, slab_stride=10 ** 7)]) == 4096
    assert q([rows(rows=8192, dim=128)] * 2) == 2048                          # 32 rows per chunk: 256 chunks each
    assert q([rows(dim=6)]) == -1 and q([dense()] * 25) == -1
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "twotower_hip.h").read_text()
    assert "#define TT_CLIP_MAX_BUFFERS (8 + TT_MAX_DENSE_SEGS)" in header and lib.tt_abi_version() == _lib.ABI_VERSION


def test_ops_and_the_custom_op_exist():
    import torch
    from two_tower_amazon_recommender_amd import ops, torch_ops
    assert callable(ops.clip_global_norm_) and callable(ops.make_clip_rows) and callable(ops.make_clip_dense)
    assert set(ops.CLIP_MODES) == set(cc.MODES)
    assert "clip_by_global_norm_" in torch_ops.OPS
    schema = str(torch.ops.twotower.clip_by_global_norm_.default._schema)
    assert "Tensor(a0!)[] tensors" in schema and "float clip_norm" in schema and schema.endswith("-> Tensor")
    out = torch.ops.twotower.clip_by_global_norm_([torch.empty(5, 3, device="meta"), torch.empty(7, device="meta")], 1.0)
    assert out.shape == (2,) and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.make_clip_rows(torch.zeros(4, 8))

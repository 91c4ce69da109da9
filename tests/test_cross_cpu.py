"""The cross layers without a GPU: the f64 restatement of tests/cross_check.py against autograd, the configuration (dataclass,
YAML block, CLI flag, checkpoints from before the field), and the C entries' argument validation, which happens before any
launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import cross_check as cc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig


def _layer(rng, n, d):
    x0, x = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (n, d))
    lim = np.sqrt(6.0 / (2 * d))
    return x0, x, rng.uniform(-lim, lim, (d, d)), rng.uniform(-0.2, 0.2, d), rng.standard_normal((n, d))


def test_layer_backward_is_the_f64_autograd_gradient():
    rng = np.random.default_rng(0)
    x0, x, w, b, g = _layer(rng, 9, 8)
    t = [torch.tensor(a, requires_grad=True) for a in (x0, x, w, b)]
    y = t[0] * (t[1] @ t[2] + t[3]) + t[1]
    u, y64 = cc.layer_forward(x0, x, w, b)
    assert np.abs(y.detach().numpy() - y64).max() <= 1e-14
    y.backward(torch.tensor(g))
    got = cc.layer_backward(x0, x, u, w, g)
    for k, ref in (("dx0", t[0].grad), ("dx", t[1].grad), ("dw", t[2].grad), ("db", t[3].grad)):
        assert np.abs(got[k] - ref.numpy()).max() <= 1e-13 * max(np.abs(ref.numpy()).max(), 1.0), k
    prev = rng.standard_normal(x0.shape)
    assert np.array_equal(cc.layer_backward(x0, x, u, w, g, dx0_in=prev)["dx0"], got["dx0"] + prev)
    # layer 0: x IS x0, one gradient
    t0 = torch.tensor(x0, requires_grad=True)
    wt, bt = torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)
    (t0 * (t0 @ wt + bt) + t0).backward(torch.tensor(g))
    u0, _ = cc.layer_forward(x0, x0, w, b)
    got0 = cc.layer_backward(x0, x0, u0, w, g, x_is_x0=True, dx0_in=prev)
    assert np.abs(got0["dx"] - (t0.grad.numpy() + prev)).max() <= 1e-13 * np.abs(t0.grad.numpy()).max() and got0["dx0"] is None
    assert np.abs(got0["dw"] - wt.grad.numpy()).max() <= 1e-13 and np.abs(got0["db"] - bt.grad.numpy()).max() <= 1e-13


def test_f32_evaluation_meets_the_kernel_bars_at_every_gpu_shape():
    """The bars of tests/test_gpu_cross.py (1e-5 of max|ref|) can be met in float32 on its own problems, the widths that are no
    power of two included: the same math as torch-CPU f32 operations against the f64 restatement, both backward forms from the
    restatement's u rounded to f32 (what the GPU test hands the launch)."""
    import test_gpu_cross as tg
    assert set(tg.SHAPES) >= {(77, 96), (130, 160), (45, 192), (65, 224)} and sorted({d for _, d in tg.SHAPES}) == list(range(32, 257, 32))
    f = torch.from_numpy
    for n, d in tg.SHAPES:
        p = tg._problem(n, d)
        x0, x, w, b, g, prev = (f(p[k]) for k in ("x0", "x", "w", "b", "g", "prev"))
        worst = 0.0
        for xx, is0 in ((x, False), (x0, True)):
            want_u, want_y = cc.layer_forward(p["x0"], xx.numpy(), p["w"], p["b"])
            u = torch.addmm(b, xx, w)
            errs = dict(u=tg.rel_err(u.numpy(), want_u), y=tg.rel_err((x0 * u + xx).numpy(), want_y))
            u = f(want_u.astype(np.float32))
            want = cc.layer_backward(p["x0"], xx.numpy(), u.numpy(), p["w"], p["g"], x_is_x0=is0, dx0_in=p["prev"])
            t = g * x0
            dx = g + t @ w.t()
            errs.update(dx=tg.rel_err((dx + g * u + prev if is0 else dx).numpy(), want["dx"]), dw=tg.rel_err((xx.t() @ t).numpy(), want["dw"]),
                        db=tg.rel_err(t.sum(0).numpy(), want["db"]))
            if not is0:
                errs["dx0"] = tg.rel_err((prev + g * u).numpy(), want["dx0"])
            assert max(errs.values()) <= 1e-5, (n, d, is0, errs)
            worst = max(worst, *errs.values())
        print(f"n {n} D {d}: worst f32 error {worst:.2e}")


def test_the_backward_chain_of_the_issue_is_the_stack_gradient():
    """G_l = G_{l+1} + t W_l^T, A += G_{l+1} * u_l, demb = ((G_1 + t W_0^T) + G_1 * u_0) + A - against autograd of the stack."""
    rng = np.random.default_rng(1)
    n, d, L = 7, 8, 3
    x0 = rng.uniform(-1, 1, (n, d))
    ws = [rng.uniform(-0.4, 0.4, (d, d)) for _ in range(L)]
    bs = [rng.uniform(-0.2, 0.2, d) for _ in range(L)]
    gl = rng.standard_normal((n, d))
    xs, us = cc.stack_forward(x0, ws, bs)
    g, acc, dws = gl, None, [None] * L
    for l in range(L - 1, 0, -1):
        r = cc.layer_backward(x0, xs[l - 1], us[l], ws[l], g, dx0_in=acc)
        g, acc, dws[l] = r["dx"], r["dx0"], r["dw"]
    r = cc.layer_backward(x0, x0, us[0], ws[0], g, x_is_x0=True, dx0_in=acc)
    dws[0] = r["dw"]
    t0 = torch.tensor(x0, requires_grad=True)
    tw = [torch.tensor(w, requires_grad=True) for w in ws]
    x = t0
    for w, b in zip(tw, bs):
        x = t0 * (x @ w + torch.tensor(b)) + x
    assert np.abs(x.detach().numpy() - xs[-1]).max() <= 1e-13
    x.backward(torch.tensor(gl))
    assert np.abs(r["dx"] - t0.grad.numpy()).max() <= 1e-12 * np.abs(t0.grad.numpy()).max()
    for l in range(L):
        assert np.abs(dws[l] - tw[l].grad.numpy()).max() <= 1e-12 * np.abs(tw[l].grad.numpy()).max(), l
    assert cc.slab_rows(10, 4) == [(0, 3), (3, 6), (6, 9), (9, 10)] and cc.slab_rows(3, 5)[3:] == [(3, 3), (3, 3)]


def test_step_f64_with_zero_cross_parameters_is_the_plain_step():
    rng = np.random.default_rng(2)
    b, d = 6, 8
    x0u, x0i = rng.standard_normal((b, d)) * 0.1, rng.standard_normal((b, d)) * 0.1
    towers = tuple(([rng.standard_normal((d, 4)) * 0.5], [np.zeros(4)]) for _ in range(2))
    zero = tuple(([np.zeros((d, d))], [np.zeros(d)]) for _ in range(2))
    none = (([], []), ([], []))
    r0, r1 = cc.step_f64(x0u, x0i, none, towers, 0.1, ([], [])), cc.step_f64(x0u, x0i, zero, towers, 0.1, ([], []))
    assert r0["loss"] == r1["loss"] and np.array_equal(r0["dx0"][0], r1["dx0"][0]) and np.array_equal(r0["dw"][1][0], r1["dw"][1][0])
    assert np.abs(r1["dcw"][0][0]).max() > 0                     # the kernel still receives a gradient: x_0^T (G * x_0)


def test_tensor_ids_collide_with_none_of_the_trainers():
    from two_tower_amazon_recommender_amd import trainer
    assert trainer.TID_CROSS_BASE == cc.TID_CROSS_BASE == 48 and trainer.MAX_CROSS_LAYERS == 3
    mine = {48 + 2 * l + t for l in range(3) for t in range(2)}
    others = {v for k, v in vars(trainer).items() if k.startswith("TID_") and "CROSS" not in k and "BASE" not in k}
    dense = {trainer.TID_DENSE_BASE + 2 * l + t for l in range(8) for t in range(2)}
    dropout = {trainer.TID_DROPOUT_BASE + 2 * l + t for l in range(8) for t in range(2)}
    assert not mine & (others | dense | dropout) and (others | dense | dropout) <= cc.TRAINER_TIDS_IN_USE


def test_validate_range_embedding_dim_rule_and_segment_limit():
    TwoTowerConfig(10, 10).validate()
    assert TwoTowerConfig(10, 10).cross_layers == 0
    for L in (1, 2, 3):
        TwoTowerConfig(10, 10, cross_layers=L).validate()
    for bad in (-1, 4, 1.0, True, "2"):
        with pytest.raises(ValueError, match="cross_layers"):
            TwoTowerConfig(10, 10, cross_layers=bad).validate()
    for dim in (36, 16, 48, 288, 512):
        with pytest.raises(ValueError, match="multiple of 32 in 32..256"):
            TwoTowerConfig(10, 10, embedding_dim=dim, cross_layers=1).validate()
        TwoTowerConfig(10, 10, embedding_dim=dim).validate()         # without the layers the dimension is as free as before
    for dim in (32, 96, 256):
        TwoTowerConfig(10, 10, embedding_dim=dim, cross_layers=1).validate()
    # 3-layer towers: 12 segments + 2; with the head 16: full.  4-layer towers: 16 + 2 is over TT_MAX_DENSE_SEGS
    assert TwoTowerConfig(10, 10, cross_layers=2).dense_segment_count() == 14
    TwoTowerConfig(10, 10, cross_layers=2, rating_weight=0.5).validate()
    with pytest.raises(NotImplementedError, match="cross layers add two dense segments"):
        TwoTowerConfig(10, 10, tower_dims=[64, 64, 64, 32], cross_layers=1).validate()
    with pytest.raises(NotImplementedError, match="at most 16"):
        TwoTowerConfig(10, 10, cross_layers=1, rating_weight=0.5, n_user_features=3).validate()
    TwoTowerConfig(10, 10, tower_dims=[64, 64, 64, 32]).validate()


DOC = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "training": {"batch_size": 256},
                 "retrieval": {"temperature": 0.1}}}


def _doc(cross):
    return {"model": {**DOC["model"], "cross": cross}}


def test_config_reads_the_cross_block():
    cfg, _ = cfgmod.model_config_from_dict(DOC, 10, 10)
    assert cfg.cross_layers == 0
    cfg, _ = cfgmod.model_config_from_dict(_doc({"layers": 2}), 10, 10)
    assert cfg.cross_layers == 2
    cfg.validate()
    assert cfgmod.model_config_from_dict(_doc({}), 10, 10)[0].cross_layers == 0
    for bad in ({"layers": 4}, {"layers": -1}, {"layers": 1.5}, {"layers": True}, {"layers": "two"}, 2, {"layers": 1, "projection_dim": 8}):
        with pytest.raises(ValueError, match="model.cross"):
            cfgmod.model_config_from_dict(_doc(bad), 10, 10)


def test_cli_flag_and_refusals(tmp_path):
    import yaml
    from two_tower_amazon_recommender_amd import train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text(yaml.safe_dump(DOC))
    base = ["--config", str(cfgp), "--synthetic", "600"]
    assert train.parse(base).cross_layers is None and train.parse(base + ["--cross-layers", "2"]).cross_layers == 2
    with pytest.raises(SystemExit, match="cross-layers"):
        train.main(base + ["--cross-layers", "4"])
    with pytest.raises(NotImplementedError, match="cross layers"):
        train.main(base + ["--cross-layers", "1", "--distributed"])
    bad = tmp_path / "bad.yaml"
    bad.write_text(yaml.safe_dump(_doc({"layers": 7})))
    with pytest.raises(ValueError, match="model.cross.layers"):
        train.main(["--config", str(bad), "--synthetic", "600"])


def test_a_checkpoint_config_without_the_field_loads_as_zero():
    old = dict(TwoTowerConfig(10, 10).__dict__)
    del old["cross_layers"]
    assert TwoTowerConfig(**old).cross_layers == 0                 # recommend.py rebuilds the config from the checkpoint alone
    new = dict(TwoTowerConfig(10, 10, cross_layers=2).__dict__)
    assert TwoTowerConfig(**new).cross_layers == 2


def test_sharded_trainer_refuses_before_it_touches_a_device():
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    with pytest.raises(NotImplementedError, match="cross layers"):
        ShardedTwoTowerTrainer(TwoTowerConfig(10, 10, cross_layers=1), "cuda:0")


def test_torch_op_is_registered():
    from two_tower_amazon_recommender_amd import torch_ops
    for name in ("cross_layer", "cross_layer_bwd"):
        assert name in torch_ops.OPS and hasattr(torch.ops.twotower, name)


# ------------------------------------------------------------------------------------------ the C entries, before any launch
A = 0x1000                                              # fake, 16-byte aligned device addresses: validation never dereferences


def _fwd(n=64, **kw):
    f = dict(x0=A, x=2 * A, w=3 * A, b=4 * A, u_out=5 * A, y=6 * A, n=n)
    f.update(kw)
    return _lib.CrossFwdArgs(**f)


def _bwd(n=64, **kw):
    f = dict(x0=A, x=2 * A, u=3 * A, w=4 * A, g=5 * A, dx=6 * A, dx0=7 * A, dw_slabs=8 * A, db_slabs=9 * A, n=n, slab_stride=32 * 33,
             n_slabs=2, x_is_x0=0, accumulate_dx0=0)
    f.update(kw)
    return _lib.CrossBwdArgs(**f)


def _refused(rc, lib, word=None):
    msg = lib.tt_last_error()
    assert rc == _lib.TT_ERR_INVALID_ARG and len(msg) > 10, (rc, msg)
    if word:
        assert word in msg, msg


def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    one = lambda a: (type(a) * 1)(a)
    for D in (48, 288, 0, 16):
        _refused(lib.tt_cross_fwd_f32(one(_fwd()), 1, D, None), lib, b"multiple of 32")
        _refused(lib.tt_cross_bwd_f32(one(_bwd()), 1, D, None), lib, b"multiple of 32")
    three = (_lib.CrossFwdArgs * 3)(_fwd(), _fwd(), _fwd())
    _refused(lib.tt_cross_fwd_f32(three, 3, 32, None), lib, b"n_probs")
    _refused(lib.tt_cross_fwd_f32(three, 0, 32, None), lib, b"n_probs")
    three = (_lib.CrossBwdArgs * 3)(_bwd(), _bwd(), _bwd())
    _refused(lib.tt_cross_bwd_f32(three, 3, 32, None), lib, b"n_probs")
    _refused(lib.tt_cross_fwd_f32(None, 1, 32, None), lib)
    _refused(lib.tt_cross_bwd_f32(None, 1, 32, None), lib)
    _refused(lib.tt_cross_bwd_f32(one(_bwd(n_slabs=0)), 1, 32, None), lib, b"n_slabs")
    _refused(lib.tt_cross_bwd_f32(one(_bwd(n_slabs=65536)), 1, 32, None), lib, b"n_slabs")
    _refused(lib.tt_cross_fwd_f32(one(_fwd(n=-1)), 1, 32, None), lib)
    # a NULL pointer
    for k in ("x0", "x", "w", "b", "y"):
        _refused(lib.tt_cross_fwd_f32(one(_fwd(**{k: None})), 1, 32, None), lib, b"null")
    for k in ("x0", "x", "u", "w", "g", "dx", "dx0", "dw_slabs", "db_slabs"):
        _refused(lib.tt_cross_bwd_f32(one(_bwd(**{k: None})), 1, 32, None), lib, b"null")
    # a misaligned pointer
    for k in ("x0", "x", "w", "u_out", "y"):
        _refused(lib.tt_cross_fwd_f32(one(_fwd(**{k: 11 * A + 4})), 1, 32, None), lib, b"aligned")
    for k in ("x0", "x", "u", "w", "g", "dx", "dx0"):
        _refused(lib.tt_cross_bwd_f32(one(_bwd(**{k: 11 * A + 4})), 1, 32, None), lib, b"aligned")
    # aliases: the dW tiles read g, x0, x and u while dx is written
    for k in ("g", "x0", "x", "u"):
        _refused(lib.tt_cross_bwd_f32(one(_bwd(dx=_bwd().__getattribute__(k))), 1, 32, None), lib, b"alias")
    _refused(lib.tt_cross_bwd_f32(one(_bwd(dx0=5 * A)), 1, 32, None), lib, b"alias")
    _refused(lib.tt_cross_fwd_f32(one(_fwd(y=2 * A)), 1, 32, None), lib, b"alias")
    _refused(lib.tt_cross_fwd_f32(one(_fwd(y=A)), 1, 32, None), lib, b"alias")
    _refused(lib.tt_cross_bwd_f32(one(_bwd(x_is_x0=1)), 1, 32, None), lib, b"x_is_x0")
    _refused(lib.tt_cross_bwd_f32(one(_bwd(slab_stride=100)), 1, 32, None), lib, b"slab_stride")
    # the second problem is validated like the first
    two = (_lib.CrossBwdArgs * 2)(_bwd(), _bwd(dx=5 * A))
    _refused(lib.tt_cross_bwd_f32(two, 2, 32, None), lib, b"problem 1")


def test_entries_answer_ok_without_a_launch_when_no_problem_has_rows():
    lib = _lib.load()
    two = (_lib.CrossFwdArgs * 2)(_lib.CrossFwdArgs(n=0), _lib.CrossFwdArgs(n=0))
    assert lib.tt_cross_fwd_f32(two, 2, 64, None) == _lib.TT_OK and lib.tt_cross_fwd_f32(two, 1, 256, None) == _lib.TT_OK
    two = (_lib.CrossBwdArgs * 2)(_lib.CrossBwdArgs(n=0, n_slabs=1), _lib.CrossBwdArgs(n=0, n_slabs=3))
    assert lib.tt_cross_bwd_f32(two, 2, 64, None) == _lib.TT_OK and lib.tt_cross_bwd_f32(two, 1, 32, None) == _lib.TT_OK


def test_num_slabs_is_a_host_query_and_the_mirrors_have_the_library_sizes():
    lib = _lib.load()
    assert lib.tt_cross_num_slabs(8192) == 64 and lib.tt_cross_num_slabs(1) == 1
    assert lib.tt_cross_num_slabs(0) == 1 and lib.tt_cross_num_slabs(129) == 2 and lib.tt_cross_num_slabs(1 << 20) == 64
    assert lib.tt_abi_struct_bytes(17) == C.sizeof(_lib.CrossFwdArgs) == 56
    assert lib.tt_abi_struct_bytes(18) == C.sizeof(_lib.CrossBwdArgs) == 104
    assert _lib.CROSS_STRUCT_INDEX == {"CrossFwdArgs": 17, "CrossBwdArgs": 18}
    assert lib.tt_abi_struct_bytes(16) == -1 and lib.tt_abi_struct_bytes(19) == -1
    assert lib.tt_abi_version() == _lib.ABI_VERSION == 10

"""Lazy Adam, the parts that need no GPU: the restatements of tests/adam_check.py against torch.optim.SparseAdam and
torch.optim.Adam in f64, the f32 restatement against the f64 one, argument validation of tt_adam_step_f32 (before any launch), the
workspace query, the ABI's struct sizes, the config / CLI surface, the sharded trainer's refusal, and the resource usage of
csrc/adam.hip (no kernel may use scratch)."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import adam_check as ac
from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
LR = 0.001
REL = 1e-12                  # f64 against f64: the two sides differ by a few roundings of 2^-53


def _six_steps(rows=40, dim=8, n=64, seed=5):
    """(initial table, [(ids, grads)] * 6): duplicate ids in every batch (n > rows / 2 of them), and rows >= rows - 8 never
    touched."""
    rng = np.random.default_rng(seed)
    w0 = rng.uniform(-0.05, 0.05, (rows, dim))
    return w0, [(rng.integers(0, rows - 8, n), rng.standard_normal((n, dim)) * 0.01) for _ in range(6)]


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_f64_restatement_equals_torch_sparse_adam():
    w0, steps = _six_steps()
    w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.SparseAdam([p], lr=LR, betas=(ac.BETA1, ac.BETA2), eps=ac.EPS)
    for t, (ids, g) in enumerate(steps, start=1):
        uniq = ac.sparse_adam(w, m, v, ids, g, LR, t)
        assert len(uniq) < len(ids)                                        # duplicates were summed
        p.grad = torch.sparse_coo_tensor(torch.from_numpy(ids)[None], torch.from_numpy(g), size=w0.shape)
        opt.step()
        st = opt.state[p]
        for got, want, what in ((w, p.detach().numpy(), "w"), (m, st["exp_avg"].numpy(), "m"), (v, st["exp_avg_sq"].numpy(), "v")):
            print(f"step {t} {what}: relative difference {_rel(got, want):.2e}")
            assert _rel(got, want) <= REL, (t, what)
    touched = np.unique(np.concatenate([ids for ids, _ in steps]))
    rest = np.setdiff1d(np.arange(w0.shape[0]), touched)
    assert len(rest) >= 8
    assert np.array_equal(w[rest], w0[rest]) and np.array_equal(p.detach().numpy()[rest], w0[rest])
    assert not m[rest].any() and not v[rest].any()
    assert not np.array_equal(w[touched], w0[touched])


def test_f64_restatement_equals_torch_adam_with_the_epsilon_moved_inside_the_bias_correction():
    """torch.optim.Adam divides by sqrt(v) / sqrt(1 - beta2^t) + eps; with eps / sqrt(1 - beta2^t) handed to it before each step
    that is (sqrt(v) + eps) / sqrt(1 - beta2^t): the contract's form.  Dense gradients (Adam decays every element on every
    step); the last 8 rows never get one, so they keep m = v = 0 and their parameters."""
    rng = np.random.default_rng(9)
    rows, dim = 40, 8
    w0 = rng.uniform(-0.05, 0.05, (rows, dim))
    w, m, v = w0.copy().reshape(-1), np.zeros(rows * dim), np.zeros(rows * dim)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=LR, betas=(ac.BETA1, ac.BETA2), eps=ac.EPS)
    for t in range(1, 7):
        g = rng.standard_normal((2, rows, dim)) * 0.01                    # two slabs
        g[:, rows - 8:] = 0.0
        ac.dense_adam(w, m, v, g.reshape(2, -1), 0.0, LR, t)
        opt.param_groups[0]["eps"] = ac.EPS / np.sqrt(1.0 - ac.BETA2 ** t)
        p.grad = torch.from_numpy(g[0] + g[1])
        opt.step()
        st = opt.state[p]
        for got, want, what in ((w, p.detach().numpy(), "w"), (m, st["exp_avg"].numpy(), "m"), (v, st["exp_avg_sq"].numpy(), "v")):
            print(f"step {t} {what}: relative difference {_rel(got.reshape(rows, dim), want):.2e}")
            assert _rel(got.reshape(rows, dim), want) <= REL, (t, what)
    assert np.array_equal(w.reshape(rows, dim)[rows - 8:], w0[rows - 8:])
    assert np.array_equal(p.detach().numpy()[rows - 8:], w0[rows - 8:])


def test_f32_restatement_is_within_one_ulp_of_the_f64_one():
    """One step from random state.  |w| in [0.5, 1) (one binade: ulp(w) = 2^-24) and an update of at most ~1e-3 (|m'| / sqrt(v')
    <= ~5 with v >= 1e-4, alpha_7 = 1.6e-4), so the f32 error of the update term - a handful of roundings of 2^-24 RELATIVE to
    1e-3 - is far below the 0.5 ulp of the final subtraction."""
    rng = np.random.default_rng(11)
    n, dim = 4096, 16
    w = (rng.uniform(0.5, 1.0, (n, dim)) * rng.choice([-1.0, 1.0], (n, dim))).astype(np.float32)
    m = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    v = ((rng.standard_normal((n, dim)) * 0.01) ** 2 + 1e-4).astype(np.float32)
    g = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    ids = np.arange(n)
    w32, m32, v32 = w.copy(), m.copy(), v.copy()
    ac.sparse_adam(w32, m32, v32, ids, g, LR, 7)
    w64, m64, v64 = w.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    ac.sparse_adam(w64, m64, v64, ids, g.astype(np.float64), LR, 7)
    assert w32.dtype == m32.dtype == v32.dtype == np.float32
    ulps = np.abs(w32.astype(np.float64) - w64) / np.spacing(np.abs(w32))
    print(f"f32 against f64: {ulps.max():.3f} ulp of w; largest update {np.abs(w64 - w).max():.2e}")
    assert ulps.max() <= 1.0
    assert np.abs(w64 - w).max() > 1e-5                                    # the step did move the parameters


# ------------------------------------------------------------------------------------------ the C ABI on the host
def _hyper(**kw):
    h = dict(lr=LR, beta1=ac.BETA1, beta2=ac.BETA2, eps=ac.EPS, step=1)
    h.update(kw)
    return _lib.AdamHyper(h["lr"], h["beta1"], h["beta2"], h["eps"], h["step"])


def _aligned(buf):
    return (C.addressof(buf) + 255) & ~255


def _host_table(buf, moments=True):
    """A table description whose pointers are (256-byte aligned) HOST memory: enough for the checks, which never dereference
    them."""
    a = _aligned(buf)
    return _lib.AdamTable(a, a if moments else None, a if moments else None, 10, a, a, a, a)


@pytest.mark.parametrize("what,kw,word", [
    ("dim 6", dict(dim=6), b"dim"), ("dim 0", dict(dim=0), b"dim"),
    ("step 0", dict(hyper=dict(step=0)), b"step"), ("step -3", dict(hyper=dict(step=-3)), b"step"),
    ("beta1 1", dict(hyper=dict(beta1=1.0)), b"beta1"), ("beta1 < 0", dict(hyper=dict(beta1=-0.1)), b"beta1"),
    ("beta2 1", dict(hyper=dict(beta2=1.0)), b"beta2"), ("beta2 nan", dict(hyper=dict(beta2=float("nan"))), b"beta2"),
    ("eps 0", dict(hyper=dict(eps=0.0)), b"eps"), ("eps < 0", dict(hyper=dict(eps=-1e-7)), b"eps"),
    ("table without moments", dict(moments=False), b"m and v"),
    ("segment without moments", dict(seg_moments=False), b"m and v"),
    ("n_tables 4", dict(n_tables=4), b"n_tables"), ("n_tables -1", dict(n_tables=-1), b"n_tables"),
    ("n_segs 17", dict(n_segs=17), b"n_segs"), ("n_segs -1", dict(n_segs=-1), b"n_segs"),
    ("no hyper-parameters", dict(no_hyper=True), b"null pointer"),
])
def test_invalid_arguments_are_refused_before_any_launch(what, kw, word):
    """Every check happens on the host: no pointer below is device memory, so a launch would fault."""
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    a = _aligned(buf)
    tables = (_lib.AdamTable * 4)(*[_host_table(buf, kw.get("moments", True)) for _ in range(4)])
    mv = a if kw.get("seg_moments", True) else None
    segs = (_lib.AdamSeg * 17)(*[_lib.AdamSeg(a, mv, mv, a, 8, 8, 1, 0.0) for _ in range(17)])
    h = _hyper(**kw.get("hyper", {}))
    rc = lib.tt_adam_step_f32(tables, kw.get("n_tables", 1), kw.get("dim", 32), 4, segs, kw.get("n_segs", 1),
                              None if kw.get("no_hyper") else C.byref(h), None)
    assert rc == _lib.TT_ERR_INVALID_ARG, what
    msg = lib.tt_last_error()
    assert b"tt_adam_step_f32" in msg and word in msg, (what, msg)


def test_nothing_to_do_is_a_no_op_and_the_workspace_query_answers_on_the_host():
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    h = _hyper()
    assert lib.tt_adam_step_f32(None, 0, 32, 0, None, 0, C.byref(h), None) == _lib.TT_OK
    tables = (_lib.AdamTable * 1)(_host_table(buf))
    assert lib.tt_adam_step_f32(tables, 1, 32, 0, None, 0, C.byref(h), None) == _lib.TT_OK      # no ids, no segments
    assert lib.tt_adam_workspace_bytes(0, 128) == 0
    assert lib.tt_adam_workspace_bytes(8192, 128) == 2 * (8192 // 64) * 128 * 4                   # P and S: a row per 64-slot block
    for n, dim in ((1, 4), (65, 12), (777, 32), (20000, 256)):
        got = lib.tt_adam_workspace_bytes(n, dim)
        assert got % 256 == 0 and got >= 2 * -(-n // 64) * dim * 4, (n, dim, got)


def test_struct_sizes_are_reported_and_the_abi_version_stays_10():
    lib = _lib.load()
    assert lib.tt_abi_version() == 10 == _lib.ABI_VERSION
    for mirror, size in ((_lib.AdamTable, 64), (_lib.AdamSeg, 56), (_lib.AdamHyper, 24)):
        which = _lib.ABI_STRUCT_INDEX[mirror.__name__]
        assert lib.tt_abi_struct_bytes(which) == C.sizeof(mirror) == size, mirror.__name__
    assert sorted(_lib.ABI_STRUCT_INDEX.values()) == [10, 11, 12]
    assert lib.tt_abi_struct_bytes(9) == -1 and lib.tt_abi_struct_bytes(13) == -1


def test_ops_refuses_cpu_tensors_and_mismatched_moments():
    from two_tower_amazon_recommender_amd import ops
    assert ops.adam_workspace_bytes(0, 128) == 0
    t = torch.zeros(10, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step_([(t, t, t, torch.zeros(4, 32), None)], [], ops.AdamHyper(step=1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.make_adam_seg(torch.zeros(8), torch.zeros(8), torch.zeros(8), torch.zeros(8), 1, 0.0)
    h = ops.AdamHyper().struct()
    assert (h.step, h.lr, h.beta1, h.beta2, h.eps) == (1, np.float32(0.001), np.float32(0.9), np.float32(0.999), np.float32(1e-7))


# ------------------------------------------------------------------------------------------ config, CLI, refusals
def test_config_accepts_adam_and_validates_its_hyper_parameters():
    base = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32])
    cfg = TwoTowerConfig(**base)
    assert (cfg.optimizer, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_epsilon) == ("sgd", 0.9, 0.999, 1e-7)
    TwoTowerConfig(optimizer="adam", **base).validate()
    TwoTowerConfig(optimizer="adam", adam_beta1=0.0, adam_beta2=0.5, adam_epsilon=1e-3, **base).validate()
    for field, bad in (("adam_beta1", 1.0), ("adam_beta1", -0.1), ("adam_beta2", 1.0), ("adam_beta2", float("nan")),
                       ("adam_epsilon", 0), ("adam_epsilon", -1e-7)):
        with pytest.raises(ValueError, match=field):
            TwoTowerConfig(optimizer="adam", **{field: bad}, **base).validate()
    with pytest.raises(ValueError, match="optimizer"):
        TwoTowerConfig(optimizer="adamw", **base).validate()
    for opt in ("sgd", "adagrad"):
        TwoTowerConfig(optimizer=opt, **base).validate()


def test_yaml_reader_passes_the_optimizer_through():
    from two_tower_amazon_recommender_amd.config import model_config_from_dict
    model = {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "training": {"learning_rate": 0.001}}
    cfg, _ = model_config_from_dict({"model": model}, 100, 100, optimizer="adam")
    cfg.validate()
    assert cfg.optimizer == "adam" and cfg.learning_rate == 0.001


def test_train_cli_has_the_flags():
    from two_tower_amazon_recommender_amd import train
    a = train.parse(["--config", "c.yaml"])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_epsilon) == ("adagrad", 0.9, 0.999, 1e-7)
    a = train.parse(["--config", "c.yaml", "--optimizer", "adam", "--adam-beta1", "0.8", "--adam-beta2", "0.99", "--adam-epsilon", "1e-8"])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_epsilon) == ("adam", 0.8, 0.99, 1e-8)
    with pytest.raises(SystemExit):
        train.parse(["--config", "c.yaml", "--optimizer", "adamw"])


def test_sharded_trainer_refuses_adam_before_touching_a_device(tmp_path):
    from two_tower_amazon_recommender_amd import train
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    cfg = TwoTowerConfig(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32], optimizer="adam")
    with pytest.raises(NotImplementedError, match="adam"):
        ShardedTwoTowerTrainer(cfg, "cuda:0")
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [32]\n  item_tower_dims: [32]\n")
    with pytest.raises(NotImplementedError, match="adam"):
        train.main(["--config", str(cfgp), "--synthetic", "1024", "--distributed", "--optimizer", "adam"])


def test_custom_op_is_registered_as_mutating_its_three_state_tensors():
    from two_tower_amazon_recommender_amd import torch_ops
    assert "sparse_adam_" in torch_ops.OPS and hasattr(torch.ops.twotower, "sparse_adam_")
    schema = str(torch.ops.twotower.sparse_adam_.default._schema)
    assert "Tensor(a0!) table" in schema and "Tensor(a1!) exp_avg" in schema and "Tensor(a2!) exp_avg_sq" in schema
    assert re.search(r"(SymInt|int) step, float lr, float beta1, float beta2, float eps", schema), schema
    z = torch.zeros(4, 32)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CPU: no kernel
        torch.ops.twotower.sparse_adam_(z, z.clone(), z.clone(), z.clone(), torch.zeros(4, dtype=torch.int64), 1, LR, 0.9, 0.999, 1e-7)


# ------------------------------------------------------------------------------------------ resource usage
def test_no_adam_kernel_uses_scratch(tmp_path):
    """Both launches keep everything a lane holds - gradient, parameter and two moment float4s, four rows (eight slabs) in
    flight - in registers (the recipe of tests/test_l2norm_cpu.py::test_no_normalize_kernel_uses_scratch)."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "adam.o"),
                        str(CSRC / "adam.hip")], check=True, capture_output=True, text=True, timeout=900)
    res, name = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r" ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            res[name] = int(m.group(1))
    assert len(res) == 2 and any("adam_sparse_kernel" in n for n in res) and any("adam_finish_kernel" in n for n in res), sorted(res)
    for n, scr in res.items():
        assert scr == 0, (n, scr)

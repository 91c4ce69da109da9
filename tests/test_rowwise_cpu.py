"""Row-wise Adagrad, the parts that need no GPU: the f32 restatement of tests/rowwise_check.py anchored to the pinned oracle
(oracle.two_tower.sparse_adagrad) and compared with the f64 one, argument validation of tt_rowwise_adagrad_step_f32 (before any
launch), the workspace query, the ABI's struct size, the config / YAML / CLI surface, the sharded trainer's refusal, the custom
op's schema, the table record, and the resource usage of csrc/rowwise.hip (no kernel may use scratch)."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import rowwise_check as rc
from oracle import two_tower as tt
from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, TwoTowerConfig

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
LR = 0.005
ENTRY = b"tt_rowwise_adagrad_step_f32"


# ------------------------------------------------------------------------------------------ the restatements
def test_lane_geometry_and_the_longest_path():
    assert [rc.lanes_per_row(d) for d in (4, 8, 12, 32, 96, 128, 256, 512)] == [1, 2, 4, 8, 32, 32, 32, 32]
    # in-lane adds (4 * chunks - 1) + log2(lpr) butterfly adds
    assert [rc.roundings_on_the_longest_path(d) for d in (4, 32, 96, 128, 256)] == [3, 3 + 3, 3 + 5, 3 + 5, 7 + 5]


@pytest.mark.parametrize("dim", [4, 32, 128, 256])
def test_f32_restatement_equals_the_pinned_oracle_when_every_row_has_one_magnitude(dim):
    """Power-of-two dim, every gradient row +-m in all its elements, distinct ids (a duplicate sum of rows with different signs
    would not have one magnitude), a constant accumulator row: S * inv_dim equals g_j^2 EXACTLY, so the row-wise update is the
    element-wise Keras Adagrad of the oracle with the accumulator broadcast to [rows, dim] - bit for bit.
    m = k / 1024 with k < 1024: q = m^2 has at most 20 significant bits, so the in-lane sums q, 2q, ... 8q (at most 23 bits) and the
    butterfly's doublings are exact, as is the product with inv_dim, a power of two."""
    rng = np.random.default_rng(100 + dim)
    rows, n = 300, 200
    ids = rng.permutation(rows - 20)[:n].astype(np.int64)
    mag = (rng.integers(1, 1024, n) / 1024.0).astype(np.float32)
    grads = (mag[:, None] * rng.choice([-1.0, 1.0], (n, dim))).astype(np.float32)
    table = rng.uniform(-0.05, 0.05, (rows, dim)).astype(np.float32)
    a = rng.uniform(0.1, 0.2, rows).astype(np.float32)
    w_rw, a_rw = table.copy(), a.copy()
    uniq = rc.sparse_rowwise_adagrad(w_rw, a_rw, ids, grads, LR)
    assert len(uniq) == n
    w_or, a_or = tt.sparse_adagrad(table.copy(), np.repeat(a[:, None], dim, axis=1), ids, grads, LR)
    assert np.array_equal(rc.bits(w_rw), rc.bits(w_or))
    assert np.array_equal(rc.bits(np.repeat(a_rw[:, None], dim, axis=1)), rc.bits(a_or))
    rest = np.setdiff1d(np.arange(rows), ids)
    assert len(rest) >= 20 and np.array_equal(rc.bits(w_rw[rest]), rc.bits(table[rest])) and np.array_equal(rc.bits(a_rw[rest]), rc.bits(a[rest]))
    assert not np.array_equal(w_rw[ids], table[ids]) and (a_rw[ids] > a[ids]).all()


@pytest.mark.parametrize("dim", [4, 32, 96, 128, 256, 160, 384, 512])      # (160, 384, 512: the wider instantiations)
def test_f32_restatement_against_the_f64_one(dim):
    """The same already-summed f32 g on both sides (widened for f64).  a' within (R + 2) * 2^-24 relative, R = the additions on
    the longest path of S (every term is >= 0, so each addition's error is relative to a partial sum no larger than S); the + 2
    covers the square and the scale.  All of these act on s, which is ~1e-3 of a' here (a in [0.1, 0.2), |g| ~ 0.01), as does the
    rounding of inv_dim itself (dim = 96); the final a + s costs one more 2^-24 of a' - inside the bound since R >= 3.
    w' within 1 ulp: |w| in [0.5, 1) (one binade) and an update of at most ~1e-3 (|g| <= ~0.06, lr 0.005, sqrt(a') >= 0.31), so
    the update term's few roundings of 2^-24 RELATIVE to 1e-3 are far below the 0.5 ulp of the final subtraction."""
    rng = np.random.default_rng(200 + dim)
    n = 2048
    w = (rng.uniform(0.5, 1.0, (n, dim)) * rng.choice([-1.0, 1.0], (n, dim))).astype(np.float32)
    a = rng.uniform(0.1, 0.2, n).astype(np.float32)
    g = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    w32, a32 = rc.rowwise_update32(w, a, g, LR, 1e-7)
    w64, a64 = rc.rowwise_update64(w.astype(np.float64), a.astype(np.float64), g.astype(np.float64), LR, 1e-7)
    assert w32.dtype == a32.dtype == np.float32 and w64.dtype == a64.dtype == np.float64
    R = rc.roundings_on_the_longest_path(dim)
    rel = np.abs(a32.astype(np.float64) - a64) / a64
    ulps = np.abs(w32.astype(np.float64) - w64) / np.spacing(np.abs(w32))
    print(f"dim {dim}: R = {R}; a' relative error {rel.max():.3e} (bound {(R + 2) * 2.0 ** -24:.3e}); w' {ulps.max():.3f} ulp; "
          f"largest update {np.abs(w64 - w).max():.2e}")
    assert rel.max() <= (R + 2) * 2.0 ** -24
    assert ulps.max() <= 1.0
    assert np.abs(w64 - w).max() > 1e-5 and (a64 > a).all()                # the step did move the state


def test_sum_of_squares_order_is_the_documented_one_and_not_a_plain_sum():
    """dim 96: 32 lanes, 24 chunks, 8 idle lanes.  The restated order equals an independent scalar walk of the contract."""
    rng = np.random.default_rng(9)
    g = rng.standard_normal((64, 96)).astype(np.float32)
    f = np.float32
    want = np.empty(64, dtype=np.float32)
    for r in range(64):
        p = [f(0)] * 32
        for l in range(24):                                  # one chunk per working lane
            q = [g[r, 4 * l + e] * g[r, 4 * l + e] for e in range(4)]
            p[l] = ((q[0] + q[1]) + q[2]) + q[3]
        for off in (1, 2, 4, 8, 16):
            p = [p[l] + p[l ^ off] for l in range(32)]
        assert len({x.tobytes() for x in p}) == 1
        want[r] = p[0]
    got = rc.row_sum_of_squares32(g)
    assert np.array_equal(rc.bits(got), rc.bits(want))
    seq = np.zeros(64, dtype=np.float32)
    for j in range(96):
        seq = seq + g[:, j] * g[:, j]
    assert not np.array_equal(rc.bits(got), rc.bits(seq))    # the order matters in f32


# ------------------------------------------------------------------------------------------ the C ABI on the host
def _aligned(buf):
    return (C.addressof(buf) + 255) & ~255


def _host_table(a, **kw):
    """A table description whose pointers are (256-byte aligned) HOST memory: enough for the checks, which never dereference
    them."""
    f = dict(table=a, row_accum=a, rows=10, grads=a, sorted_ids=a, order=a, workspace=a)
    f.update(kw)
    return _lib.RowwiseTable(f["table"], f["row_accum"], f["rows"], f["grads"], f["sorted_ids"], f["order"], f["workspace"])


@pytest.mark.parametrize("what,kw,word", [
    ("dim 6", dict(dim=6), b"dim"), ("dim 0", dict(dim=0), b"dim"), ("dim -4", dict(dim=-4), b"dim"),
    ("rows 0", dict(table=dict(rows=0)), b"rows"), ("rows -5", dict(table=dict(rows=-5)), b"rows"),
    ("eps 0", dict(eps=0.0), b"eps"), ("eps < 0", dict(eps=-1e-7), b"eps"), ("eps nan", dict(eps=float("nan")), b"eps"),
    ("lr inf", dict(lr=float("inf")), b"lr"), ("lr nan", dict(lr=float("nan")), b"lr"),
    ("null table", dict(table=dict(table=None)), b"null pointer"), ("null row_accum", dict(table=dict(row_accum=None)), b"null pointer"),
    ("null grads", dict(table=dict(grads=None)), b"null pointer"), ("null sorted ids", dict(table=dict(sorted_ids=None)), b"null pointer"),
    ("null order", dict(table=dict(order=None)), b"null pointer"),
    ("null tables", dict(no_tables=True), b"null pointer"), ("null segments", dict(no_segs=True), b"null pointer"),
    ("misaligned table", dict(table=dict(table=8)), b"aligned"), ("misaligned grads", dict(table=dict(grads=4)), b"aligned"),
    ("null workspace", dict(table=dict(workspace=None)), b"workspace"), ("misaligned workspace", dict(table=dict(workspace=128)), b"workspace"),
    ("segment without accumulator", dict(seg=dict(accum=None)), b"accum"), ("segment without parameter", dict(seg=dict(param=None)), b"segment"),
    ("n_tables 4", dict(n_tables=4), b"n_tables"), ("n_tables -1", dict(n_tables=-1), b"n_tables"),
    ("n_segs 17", dict(n_segs=17), b"n_segs"), ("n_segs -1", dict(n_segs=-1), b"n_segs"),
    ("n_ids -1", dict(n_ids=-1), b"n_ids"),
])
def test_invalid_arguments_are_refused_before_any_launch(what, kw, word):
    """Every check happens on the host: no pointer below is device memory, so a launch would fault."""
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    a = _aligned(buf)
    tk = {k: (a + v if isinstance(v, int) and k != "rows" else v) for k, v in kw.get("table", {}).items()}
    tables = (_lib.RowwiseTable * 4)(*[_host_table(a, **tk) for _ in range(4)])
    sk = dict(param=a, accum=a)
    sk.update(kw.get("seg", {}))
    segs = (_lib.DenseSeg * 17)(*[_lib.DenseSeg(sk["param"], sk["accum"], a, None, 8, 8, 1, 0.0) for _ in range(17)])
    rc_ = lib.tt_rowwise_adagrad_step_f32(None if kw.get("no_tables") else tables, kw.get("n_tables", 1), kw.get("dim", 32),
                                          kw.get("n_ids", 4), None if kw.get("no_segs") else segs, kw.get("n_segs", 1),
                                          kw.get("lr", LR), kw.get("eps", 1e-7), None)
    assert rc_ == _lib.TT_ERR_INVALID_ARG, what
    msg = lib.tt_last_error()
    assert ENTRY in msg and word in msg, (what, msg)


def test_rows_wider_than_the_kernels_hold_in_registers_are_unsupported_before_any_launch():
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    tables = (_lib.RowwiseTable * 1)(_host_table(_aligned(buf)))
    assert lib.tt_rowwise_adagrad_step_f32(tables, 1, 516, 4, None, 0, LR, 1e-7, None) == _lib.TT_ERR_UNSUPPORTED
    assert ENTRY in lib.tt_last_error() and b"516" in lib.tt_last_error()


def test_nothing_to_do_is_a_no_op_and_the_workspace_query_answers_on_the_host():
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    assert lib.tt_rowwise_adagrad_step_f32(None, 0, 32, 0, None, 0, LR, 1e-7, None) == _lib.TT_OK
    tables = (_lib.RowwiseTable * 1)(_host_table(_aligned(buf)))
    assert lib.tt_rowwise_adagrad_step_f32(tables, 1, 32, 0, None, 0, LR, 1e-7, None) == _lib.TT_OK      # no ids, no segments
    assert lib.tt_rowwise_adagrad_workspace_bytes(0, 128) == 0
    assert lib.tt_rowwise_adagrad_workspace_bytes(8192, 128) == 2 * (8192 // 64) * 128 * 4    # P and S: a row per 64-slot block
    for n, dim in ((1, 4), (65, 12), (777, 32), (20000, 256)):
        got = lib.tt_rowwise_adagrad_workspace_bytes(n, dim)
        assert got % 256 == 0 and got >= 2 * -(-n // 64) * dim * 4, (n, dim, got)


def test_struct_size_is_reported_at_its_own_index_and_the_abi_version_stays_10():
    lib = _lib.load()
    assert lib.tt_abi_version() == 10 == _lib.ABI_VERSION
    assert _lib.ROWWISE_STRUCT_INDEX == {"RowwiseTable": 24}
    assert lib.tt_abi_struct_bytes(24) == C.sizeof(_lib.RowwiseTable) == 56
    assert lib.tt_abi_struct_bytes(25) == -1
    assert sorted(_lib.ABI_STRUCT_INDEX.values()) == [10, 11, 12]            # the Adam mirrors' dict is left alone


def test_ops_refuses_cpu_tensors():
    from two_tower_amazon_recommender_amd import ops
    assert ops.rowwise_adagrad_workspace_bytes(0, 128) == 0
    t = torch.zeros(10, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10), torch.zeros(4, 32), None)], [], LR, 1e-7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rowwise_adagrad_step_([(t, torch.zeros(10, 32), torch.zeros(4, 32), None)], [], LR, 1e-7)


# ------------------------------------------------------------------------------------------ config, YAML, CLI, refusals
def test_config_accepts_rowwise_adagrad_and_still_refuses_adamw():
    base = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32])
    cfg = TwoTowerConfig(optimizer="rowwise_adagrad", **base)
    cfg.validate()
    assert (cfg.adagrad_initial_accumulator, cfg.adagrad_epsilon) == (0.1, 1e-7)
    with pytest.raises(ValueError, match="optimizer"):
        TwoTowerConfig(optimizer="adamw", **base).validate()
    for opt in ("sgd", "adagrad", "adam"):
        TwoTowerConfig(optimizer=opt, **base).validate()


def test_yaml_reader_passes_the_optimizer_through():
    from two_tower_amazon_recommender_amd.config import model_config_from_dict
    model = {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "training": {"learning_rate": 0.01}}
    cfg, _ = model_config_from_dict({"model": model}, 100, 100, optimizer="rowwise_adagrad")
    cfg.validate()
    assert cfg.optimizer == "rowwise_adagrad" and cfg.learning_rate == 0.01


def test_train_cli_has_the_choice():
    from two_tower_amazon_recommender_amd import train
    assert train.parse(["--config", "c.yaml"]).optimizer == "adagrad"
    assert train.parse(["--config", "c.yaml", "--optimizer", "rowwise_adagrad"]).optimizer == "rowwise_adagrad"
    with pytest.raises(SystemExit):
        train.parse(["--config", "c.yaml", "--optimizer", "adamw"])


def test_sharded_trainer_refuses_rowwise_adagrad_before_touching_a_device(tmp_path):
    from two_tower_amazon_recommender_amd import train
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    cfg = TwoTowerConfig(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32], optimizer="rowwise_adagrad")
    with pytest.raises(NotImplementedError, match="rowwise_adagrad"):
        ShardedTwoTowerTrainer(cfg, "cuda:0")
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [32]\n  item_tower_dims: [32]\n")
    with pytest.raises(NotImplementedError, match="rowwise_adagrad"):
        train.main(["--config", str(cfgp), "--synthetic", "1024", "--distributed", "--optimizer", "rowwise_adagrad"])


def test_custom_op_is_registered_as_mutating_the_table_and_the_row_accumulator():
    from two_tower_amazon_recommender_amd import torch_ops
    assert "sparse_rowwise_adagrad_" in torch_ops.OPS and hasattr(torch.ops.twotower, "sparse_rowwise_adagrad_")
    assert "sparse_rowwise_adagrad_" in torch_ops.__doc__
    schema = str(torch.ops.twotower.sparse_rowwise_adagrad_.default._schema)
    assert "Tensor(a0!) table" in schema and "Tensor(a1!) row_accum" in schema
    assert "Tensor grads, Tensor ids, float lr, float eps" in schema and schema.endswith("-> ()"), schema
    z = torch.zeros(4, 32)
    with pytest.raises((NotImplementedError, RuntimeError)):                # CPU: no kernel
        torch.ops.twotower.sparse_rowwise_adagrad_(z, torch.zeros(4), z.clone(), torch.zeros(4, dtype=torch.int64), LR, 1e-7)
    assert not z.any()


def test_embedding_table_record_keeps_one_float_per_row_and_no_full_accumulator():
    cfg = TwoTowerConfig(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32], optimizer="rowwise_adagrad",
                         adagrad_initial_accumulator=0.25)
    t = EmbeddingTable.new(cfg, torch.device("cpu"), "user", 1, 50, None)
    assert t.accum is None and t.m is None and t.v is None
    assert t.row_accum.shape == (50,) and t.row_accum.dtype == torch.float32 and (t.row_accum == 0.25).all()
    assert sorted(t.state()) == ["user_row_accum", "user_table"]
    for opt in ("sgd", "adagrad", "adam"):
        cfg.optimizer = opt
        assert EmbeddingTable.new(cfg, torch.device("cpu"), "user", 1, 50, None).row_accum is None


# ------------------------------------------------------------------------------------------ resource usage
def test_no_rowwise_kernel_uses_scratch(tmp_path):
    """Both launches keep everything a lane holds - its chunks of the gradient and the parameter row, the rows (piece sums) in
    flight - in registers, in every instantiation (1, 2 and 4 float4 chunks per lane) (the recipe of
    tests/test_adam_cpu.py::test_no_adam_kernel_uses_scratch)."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "rowwise.o"),
                        str(CSRC / "rowwise.hip")], check=True, capture_output=True, text=True, timeout=900)
    res, name = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r" ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            res[name] = int(m.group(1))
    kernels = {re.search(r"rowwise_(sparse|finish)_kernel", n).group(0) if re.search(r"rowwise_(sparse|finish)_kernel", n) else n
               for n in res}
    assert kernels == {"rowwise_sparse_kernel", "rowwise_finish_kernel"}, sorted(res)     # exactly the two kernels
    assert len(res) == 6, sorted(res)                                                     # each for 1, 2, 4 chunks per lane
    for n, scr in res.items():
        assert scr == 0, (n, scr)

"""Int8 top-k without a GPU: argument validation of tt_quantize_rows_i8 / tt_retrieval_topk_i8_f32 (before any launch), the
workspace query, ops / serving refusals, the recommend CLI's --index int8 arguments, the NumPy restatement's self-checks and
recall calibration, and the ISA audit of csrc/topk_i8.hip."""
import ctypes as C
import importlib.util
import pathlib
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from int8_check import (RECALL_CASES, RECALL_MIN, RECALL_SHAPE, exact_topk_ids, np_order, np_quantize, np_stage1, np_topk_i8,
                        recall_at_k, recall_corpus)
from two_tower_amazon_recommender_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parents[1]
SRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc" / "topk_i8.hip"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _buf(n, align=256, offset=0):
    raw = (C.c_uint8 * (n + 2 * align))()
    base = (C.addressof(raw) + align - 1) // align * align + offset
    return raw, base


def test_topk_i8_validates_arguments_before_any_launch():
    lib = _lib.load()
    nq, nc, d = 4, 1000, 64
    bufs = {name: _buf(size) for name, size in [("q", nq * d * 4), ("codes", nc * d), ("scales", nc * 4), ("c", nc * d * 4),
                                                 ("s", nq * 256 * 4), ("i", nq * 256 * 8), ("ex", 64)]}
    ws_bytes = lib.tt_retrieval_topk_i8_workspace_bytes(nq, nc, d, 256, 256)
    assert ws_bytes > 0
    ws = _buf(ws_bytes)
    P = {k: v[1] for k, v in bufs.items()}

    def rc(*, q=P["q"], codes=P["codes"], scales=P["scales"], c=P["c"], nq=nq, nc=nc, dim=d, k=10, k1=40, eo=None, ei=None,
           w=ws[1], wb=ws_bytes, s=P["s"], i=P["i"]):
        got = lib.tt_retrieval_topk_i8_f32(q, codes, scales, c, nq, nc, dim, k, k1, eo, ei, w, wb, s, i, None)
        return got, lib.tt_last_error().decode()

    for kw, word in [(dict(dim=48), "dim 48"),
                     (dict(dim=512), "dim 512"),
                     (dict(k=41), "exceeds k1"),
                     (dict(k=0, k1=0), "k 0"),
                     (dict(k1=257), "k1 257"),
                     (dict(nc=30, k1=31), "exceeds nc"),
                     (dict(c=None, k=10, k1=40), "without c"),
                     (dict(codes=P["codes"] + 8), "16-byte aligned"),
                     (dict(q=P["q"] + 4), "16-byte aligned"),
                     (dict(c=P["c"] + 4), "16-byte aligned"),
                     (dict(scales=P["scales"] + 2), "aligned"),
                     (dict(w=ws[1] + 16), "256-byte aligned"),
                     (dict(i=P["i"] + 4), "aligned"),
                     (dict(eo=P["ex"]), "together"),
                     (dict(eo=P["ex"] + 4, ei=P["ex"]), "8-byte aligned"),
                     (dict(q=None), "null"),
                     (dict(codes=None), "null"),
                     (dict(scales=None), "null"),
                     (dict(w=None), "null"),
                     (dict(nq=0), "positive"),
                     (dict(nc=2**31), "2^31"),
                     (dict(wb=ws_bytes - 1, k=256, k1=256), "workspace"),
                     (dict(wb=0), "workspace")]:
        got, msg = rc(**kw)
        assert got == _lib.TT_ERR_INVALID_ARG, (kw, got, msg)
        assert word in msg and msg.startswith("tt_retrieval_topk_i8_f32"), (kw, msg)


def test_quantize_validates_arguments_before_any_launch():
    lib = _lib.load()
    x, codes, scales = _buf(10 * 64 * 4), _buf(10 * 64), _buf(10 * 4)
    for args, word in [((None, 10, 64, codes[1], scales[1]), "null"),
                       ((x[1], 10, 64, None, scales[1]), "null"),
                       ((x[1], 10, 64, codes[1], None), "null"),
                       ((x[1], 0, 64, codes[1], scales[1]), "n 0"),
                       ((x[1], 10, 48, codes[1], scales[1]), "dim 48"),
                       ((x[1] + 4, 10, 64, codes[1], scales[1]), "16-byte aligned"),
                       ((x[1], 10, 64, codes[1] + 4, scales[1]), "16-byte aligned"),
                       ((x[1], 10, 64, codes[1], scales[1] + 1), "4-byte aligned")]:
        got = lib.tt_quantize_rows_i8(*args, None)
        msg = lib.tt_last_error().decode()
        assert got == _lib.TT_ERR_INVALID_ARG and word in msg and msg.startswith("tt_quantize_rows_i8"), (args, got, msg)


def test_topk_i8_workspace_size_query():
    lib = _lib.load()
    f = lib.tt_retrieval_topk_i8_workspace_bytes
    assert f(1, 1000, 32, 1, 1) > 0 and f(1, 1000, 32, 1, 1) % 256 == 0
    for bad in [(0, 10, 32, 1, 1), (4, 0, 32, 1, 1), (4, 1000, 48, 1, 1), (4, 1000, 32, 0, 1), (4, 1000, 32, 11, 10),
                (4, 1000, 32, 10, 257), (4, 30, 32, 10, 31), (4, 2**31, 32, 1, 1)]:
        assert f(*bad) == 0, bad
    # grows with nq and k1 (the lists are k1 long), not with k
    assert f(16, 10_000_000, 128, 10, 256) > f(16, 10_000_000, 128, 10, 40) > 0
    assert f(16, 10_000_000, 128, 10, 40) == f(16, 10_000_000, 128, 40, 40)
    assert f(64, 10_000_000, 128, 10, 40) > f(16, 10_000_000, 128, 10, 40)
    assert f(8192, 1_000_000, 128, 100, 256) < 2**30
    from two_tower_amazon_recommender_amd import ops
    assert ops.retrieval_topk_i8_workspace_bytes(7, 4097, 64, 10, 40) == f(7, 4097, 64, 10, 40)


def test_ops_and_serving_refuse_bad_arguments():
    from two_tower_amazon_recommender_amd import ops
    from two_tower_amazon_recommender_amd.serving import Int8BruteForce
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.quantize_rows_i8(torch.zeros(2, 32))
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.retrieval_topk_i8(torch.zeros(2, 32), torch.zeros(10, 32, dtype=torch.int8), torch.zeros(10), 3)
    with pytest.raises(TypeError):
        ops.quantize_rows_i8("nope")
    assert ops.default_k1(10, 10_000) == 40 and ops.default_k1(100, 10_000) == 256 and ops.default_k1(1, 10_000) == 32
    assert ops.default_k1(10, 20) == 20 and ops.default_k1(10, 10_000, rerank=False) == 10
    assert ops.default_k1(10, 10_000, factor=8) == 80
    with pytest.raises(ValueError, match="rerank"):
        Int8BruteForce(rerank=0)
    with pytest.raises(RuntimeError, match="index"):
        Int8BruteForce()(torch.zeros(1, 32))
    with pytest.raises(RuntimeError, match="index"):
        Int8BruteForce().state_dict()
    with pytest.raises(ValueError, match="codes"):
        Int8BruteForce().load_state_dict({"codes": torch.zeros(4, 32), "scales": torch.zeros(4)})
    with pytest.raises(ValueError, match="candidates"):
        Int8BruteForce().load_state_dict({"codes": torch.zeros(4, 32, dtype=torch.int8), "scales": torch.zeros(4)})
    with pytest.raises(ValueError, match="do not match"):
        Int8BruteForce().load_state_dict({"codes": torch.zeros(4, 32, dtype=torch.int8), "scales": torch.zeros(4),
                                          "candidates": torch.zeros(5, 32)})


def _recommend(*argv):
    return subprocess.run([sys.executable, "-m", "two_tower_amazon_recommender_amd.recommend", *argv], capture_output=True,
                          text=True, timeout=120, cwd=str(ROOT))


def test_recommend_int8_arguments(tmp_path):
    from two_tower_amazon_recommender_amd import recommend
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"x")
    base = ["--checkpoint", str(ck), "--all-users"]
    a = recommend.parse(base + ["--index", "int8"])
    assert (a.index, a.rerank) == ("int8", 4)
    a = recommend.parse(base + ["--index", "int8", "--rerank", "9"])
    assert a.rerank == 9
    assert recommend.parse(base).rerank is None
    cases = [(["--index", "int8", "--rerank", "0"], "--rerank"),
             (["--index", "int8", "--rerank", "-2"], "--rerank"),
             (["--rerank", "4"], "--index int8"),
             (["--index", "ivf", "--rerank", "4"], "--index int8"),
             (["--index", "int8", "--nprobe", "4"], "--index ivf")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            recommend.parse(base + argv)
        assert e.value.code == 2, argv
    for argv, word in cases:
        r = _recommend(*base, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr[-500:])
    r = _recommend("--help")
    assert r.returncode == 0 and "--rerank" in r.stdout and "int8" in r.stdout


def test_restatement_rounds_half_to_even_and_keeps_a_zero_row_zero():
    x = np.zeros((3, 32), dtype=np.float32)
    x[0, :8] = [127.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5]                # amax 127: scale exactly 1
    x[2, :4] = [-3.0, 1.0, 0.1, 3.0]
    codes, scales = np_quantize(x)
    assert scales[0] == 1.0 and codes[0, :8].tolist() == [127, 0, 0, 2, -2, 2, -2, 4]
    assert scales[1] == 0.0 and not codes[1].any()
    assert scales[2] == np.float32(3.0) / np.float32(127.0) and codes[2, :4].tolist() == [-127, 42, 4, 127]
    assert codes.dtype == np.int8 and scales.dtype == np.float32 and np.abs(codes.astype(int)).max() <= 127


def test_restatement_breaks_ties_by_the_lower_index():
    rng = np.random.default_rng(3)
    base = rng.integers(-127, 128, (5, 32)).astype(np.int8)
    codes = base[np.arange(40) % 5]                                           # every row 8 times: exact ties
    scales = np.ones(40, dtype=np.float32)
    qc = rng.integers(-127, 128, (2, 32)).astype(np.int8)
    S, I = np_stage1(qc, np.ones(2, dtype=np.float32), codes, scales, 12)
    for r in range(2):
        assert (np.diff(S[r]) <= 0).all()
        for a, b in zip(range(11), range(1, 12)):
            assert S[r, a] > S[r, b] or I[r, a] < I[r, b]
        best = I[r, 0] % 5
        assert I[r, :8].tolist() == [best + 5 * j for j in range(8)]          # a whole tie group, ascending
        nxt = I[r, 8] % 5
        assert I[r, 8:].tolist() == [nxt + 5 * j for j in range(4)]           # the cut splits the next group: lowest ids stay
    S2, I2 = np_stage1(qc, np.ones(2, dtype=np.float32), codes, scales, 12, excluded=[[int(I[0, 0]), -1, 99], []])
    assert I2[0, 0] == I[0, 1] and I[0, 0] not in I2[0] and np.array_equal(I2[1], I[1])
    s, i = np_order([1.0, 3.0, 3.0, 2.0, 9.0], [7, 5, 2, 1, -1], 4)
    assert i.tolist() == [2, 5, 1, 7] and s.tolist() == [3.0, 3.0, 2.0, 1.0]
    s, i = np_order([1.0], [4], 3)
    assert i.tolist() == [4, -1, -1] and s[0] == 1.0 and np.isneginf(s[1:]).all()


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_numpy_restatement_recall(kind):
    """The calibration behind RECALL_MIN: the NumPy restatement alone reaches it on the recall corpora."""
    q, x = recall_corpus(kind, **RECALL_SHAPE)
    for k, k1 in RECALL_CASES:
        rec = recall_at_k(np_topk_i8(q, x, k, k1), exact_topk_ids(q, x, k))
        assert rec >= RECALL_MIN, (kind, k, k1, rec)


def _audit_mod():
    spec = importlib.util.spec_from_file_location("audit_barriers", ROOT / "tests" / "isa_audit" / "audit_barriers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_topk_i8_kernels_barrier_loops_close_on_scalar_control_and_use_no_scratch(tmp_path):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "topk_i8.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(SRC)], check=True, capture_output=True, timeout=900)
    lines = out.read_text().split("\n")
    audit = _audit_mod()
    bodies = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\S*_kernel\S*):", lines[i])
        if m:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            bodies[m.group(1)] = lines[i:j]
            i = j
        i += 1
    # quantize, scan and re-rank at 4 dims each, and the scale kernel
    assert len(bodies) == 13 and all("i8_" in name for name in bodies), list(bodies)
    for name, body in bodies.items():
        r = audit.audit(body)
        bad = r["vector"] or r["unknown"] or r["masked"] or (r["in_loop"] and not r["scalar"])
        assert not bad, (name, r)
        assert r["barriers"] == 0, (name, r)                 # one-wave workgroups: __syncthreads orders LDS, no s_barrier
        if "scan" in name:
            assert sum("v_mfma_i32_32x32x32_i8" in l for l in body) >= 1, name
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "topk_i8.o"),
                          str(SRC)], check=True, capture_output=True, text=True, timeout=900).stderr
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res)]
    assert len(scratch) == 13 and all(x == 0 for x in scratch), scratch

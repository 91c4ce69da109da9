"""Int8 IVF without a GPU: argument validation of tt_ivf_search_i8_f32 (before any launch), the workspace query, ops /
serving refusals, the recommend CLI's --index ivf-int8 arguments, the NumPy restatement's recall calibration, and the ISA
audit of csrc/ivf_i8.hip."""
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

import int8_check
import ivf_check
from ivf_check import (RECALL_CORPUS, RECALL_NLIST, RECALL_NPROBE, clustered, exact_topk_ids, np_ivf_build, np_ivf_search,
                       recall_at_k)
from ivf_i8_check import RECALL_CASES, np_ivf_i8_search
from two_tower_amazon_recommender_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parents[1]
SRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc" / "ivf_i8.hip"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _buf(n, align=256, offset=0):
    raw = (C.c_uint8 * (n + 2 * align))()
    base = (C.addressof(raw) + align - 1) // align * align + offset
    return raw, base


def test_ivf_i8_validates_arguments_before_any_launch():
    lib = _lib.load()
    nq, nlist, n, d = 4, 64, 5000, 64
    bufs = {name: _buf(size) for name, size in [("q", nq * d * 4), ("cent", nlist * d * 4), ("off", (nlist + 1) * 8),
                                                 ("codes", n * d), ("scales", n * 4), ("ids", n * 4), ("c", n * d * 4),
                                                 ("s", nq * 256 * 4), ("i", nq * 256 * 8), ("ex", 64)]}
    ws_bytes = lib.tt_ivf_search_i8_workspace_bytes(nq, nlist, n, d, 256, 256, 64)
    assert ws_bytes > 0
    ws = _buf(ws_bytes)
    P = {k: v[1] for k, v in bufs.items()}

    def rc(*, q=P["q"], nq=nq, cent=P["cent"], nlist=nlist, off=P["off"], codes=P["codes"], scales=P["scales"], ids=P["ids"],
           c=P["c"], n=n, dim=d, k=10, k1=40, nprobe=8, eo=None, ei=None, w=ws[1], wb=ws_bytes, s=P["s"], i=P["i"]):
        got = lib.tt_ivf_search_i8_f32(q, nq, cent, nlist, off, codes, scales, ids, c, n, dim, k, k1, nprobe, eo, ei, w, wb, s, i,
                                       None)
        return got, lib.tt_last_error().decode()

    E = _lib.TT_ERR_INVALID_ARG
    for kw, code, word in [(dict(dim=48), E, "dim 48"),
                           (dict(dim=512), E, "dim 512"),
                           (dict(k=0, k1=0), E, "k 0"),
                           (dict(k=41), E, "exceeds k1"),
                           (dict(k1=257), E, "k1 257"),
                           (dict(n=100, k1=101, k=10), E, "exceeds n"),
                           (dict(c=None, k=10, k1=40), E, "without c"),
                           (dict(nprobe=0), E, "nprobe 0"),
                           (dict(nprobe=65), E, "nprobe 65"),
                           (dict(nlist=300, nprobe=257), E, "nprobe 257"),
                           (dict(n=2**31), E, "2^31"),
                           (dict(nq=2**31 - 1, nprobe=2), E, "nq * nprobe"),
                           (dict(q=P["q"] + 4), E, "16-byte aligned"),
                           (dict(cent=P["cent"] + 8), E, "16-byte aligned"),
                           (dict(codes=P["codes"] + 8), E, "16-byte aligned"),
                           (dict(c=P["c"] + 4), E, "16-byte aligned"),
                           (dict(off=P["off"] + 4), E, "aligned"),
                           (dict(scales=P["scales"] + 2), E, "aligned"),
                           (dict(ids=P["ids"] + 2), E, "aligned"),
                           (dict(w=ws[1] + 16), E, "256-byte aligned"),
                           (dict(s=P["s"] + 2), E, "aligned"),
                           (dict(i=P["i"] + 4), E, "aligned"),
                           (dict(eo=P["ex"]), E, "together"),
                           (dict(ei=P["ex"]), E, "together"),
                           (dict(eo=P["ex"] + 4, ei=P["ex"]), E, "8-byte aligned"),
                           (dict(q=None), E, "null"),
                           (dict(cent=None), E, "null"),
                           (dict(off=None), E, "null"),
                           (dict(codes=None), E, "null"),
                           (dict(scales=None), E, "null"),
                           (dict(ids=None), E, "null"),
                           (dict(w=None), E, "null"),
                           (dict(s=None), E, "null"),
                           (dict(nq=0), E, "positive"),
                           (dict(nlist=0), E, "positive"),
                           (dict(n=0), E, "positive"),
                           (dict(wb=ws_bytes - 1, k=256, k1=256, nprobe=64), _lib.TT_ERR_WORKSPACE, "workspace"),
                           (dict(wb=0), _lib.TT_ERR_WORKSPACE, "workspace")]:
        got, msg = rc(**kw)
        assert got == code, (kw, got, msg)
        assert word in msg and msg.startswith("tt_ivf_search_i8_f32"), (kw, msg)


def test_ivf_i8_workspace_size_query():
    lib = _lib.load()
    f = lib.tt_ivf_search_i8_workspace_bytes                                   # (nq, nlist, n, dim, k, k1, nprobe)
    assert f(1, 64, 5000, 32, 1, 1, 1) > 0 and f(1, 64, 5000, 32, 1, 1, 1) % 256 == 0
    for bad in [(0, 64, 5000, 32, 10, 40, 8), (4, 0, 5000, 32, 10, 40, 1), (4, 64, 0, 32, 10, 40, 8), (4, 64, 5000, 48, 10, 40, 8),
                (4, 64, 5000, 32, 0, 40, 8), (4, 64, 5000, 32, 41, 40, 8), (4, 64, 5000, 32, 10, 257, 8),
                (4, 64, 100, 32, 10, 101, 8), (4, 64, 5000, 32, 10, 40, 65), (4, 64, 5000, 32, 10, 40, 0),
                (4, 300, 5000, 32, 10, 40, 257), (4, 64, 2**31, 32, 10, 40, 8), (2**31 - 1, 64, 5000, 32, 10, 40, 2)]:
        assert f(*bad) == 0, bad
    # grows with nq, k1 (the lists are k1 long) and nprobe, not with k; includes the coarse probe's own top-k workspace
    big = (16, 4096, 10_000_000, 128)
    assert f(*big, 10, 256, 32) > f(*big, 10, 40, 32) > 0
    assert f(*big, 10, 40, 32) == f(*big, 40, 40, 32)
    assert f(*big, 10, 40, 128) > f(*big, 10, 40, 32)
    assert f(64, *big[1:], 10, 40, 32) > f(*big, 10, 40, 32)
    assert f(*big, 10, 40, 32) > lib.tt_retrieval_topk_workspace_bytes(16, 4096, 128, 32)
    assert f(*big, 100, 256, 32) >= 16 * 32 * 256 * 8
    from two_tower_amazon_recommender_amd import ops
    assert ops.ivf_search_i8_workspace_bytes(7, 100, 4097, 64, 10, 40, 9) == f(7, 100, 4097, 64, 10, 40, 9)


def test_ops_and_serving_refuse_bad_arguments():
    from two_tower_amazon_recommender_amd import ops, torch_ops
    from two_tower_amazon_recommender_amd.serving import IVF, Int8IVF
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.ivf_search_i8(torch.zeros(2, 32), torch.zeros(4, 32), torch.zeros(5, dtype=torch.int64),
                          torch.zeros(10, 32, dtype=torch.int8), torch.zeros(10), torch.zeros(10, dtype=torch.int32), 3, 2)
    assert "ivf_search_i8" in torch_ops.OPS and hasattr(torch.ops.twotower, "ivf_search_i8")
    m = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="meta")  # noqa: E731
    s, i = torch.ops.twotower.ivf_search_i8(m(8, 32), m(4, 32), m(5, dtype=torch.int64), m(100, 32, dtype=torch.int8), m(100),
                                            m(100, dtype=torch.int32), None, 7, 7, 2, None, None)
    assert s.shape == (8, 7) and s.dtype == torch.float32 and i.shape == (8, 7) and i.dtype == torch.int64
    assert issubclass(Int8IVF, IVF)
    with pytest.raises(ValueError, match="nprobe"):
        Int8IVF(nlist=8, nprobe=9)
    with pytest.raises(ValueError, match="nprobe"):
        Int8IVF(nlist=300, nprobe=257)
    with pytest.raises(ValueError, match="nlist"):
        Int8IVF(nlist=0)
    with pytest.raises(ValueError, match="rerank"):
        Int8IVF(rerank=0)
    with pytest.raises(ValueError, match="iters"):
        Int8IVF(iters=-1)
    with pytest.raises(RuntimeError, match="index"):
        Int8IVF(nlist=8, nprobe=2)(torch.zeros(1, 32))
    with pytest.raises(RuntimeError, match="index"):
        Int8IVF(nlist=8, nprobe=2).state_dict()
    good = {"nlist": 2, "centroids": torch.zeros(2, 32), "list_offsets": torch.tensor([0, 1, 4]),
            "list_codes": torch.zeros(4, 32, dtype=torch.int8), "list_scales": torch.zeros(4),
            "list_ids": torch.arange(4, dtype=torch.int32)}
    with pytest.raises(ValueError, match="list_codes"):
        Int8IVF(nlist=2, nprobe=1).load_state_dict({**good, "list_codes": torch.zeros(4, 32)})
    with pytest.raises(ValueError, match="candidates"):
        Int8IVF(nlist=2, nprobe=1).load_state_dict(good)
    with pytest.raises(ValueError, match="do not match"):
        Int8IVF(nlist=2, nprobe=1).load_state_dict({**good, "candidates": torch.zeros(5, 32)})
    with pytest.raises(ValueError, match="nprobe"):
        Int8IVF(nlist=8, nprobe=3, keep_f32=False).load_state_dict(good)
    with pytest.raises(ValueError, match="nlist"):
        Int8IVF(nlist=2, nprobe=1, keep_f32=False).load_state_dict({**good, "nlist": 3})
    with pytest.raises(ValueError, match="list_offsets"):
        Int8IVF(nlist=2, nprobe=1, keep_f32=False).load_state_dict({**good, "list_offsets": torch.tensor([0, 3, 2])})
    r = Int8IVF(nlist=2, nprobe=1, keep_f32=False).load_state_dict(good)
    assert r.list_vectors is None and r.k1(10) == 10 and Int8IVF(nlist=2, nprobe=1).keep_f32


def _recommend(*argv):
    return subprocess.run([sys.executable, "-m", "two_tower_amazon_recommender_amd.recommend", *argv], capture_output=True,
                          text=True, timeout=120, cwd=str(ROOT))


def test_recommend_ivf_int8_arguments(tmp_path):
    from two_tower_amazon_recommender_amd import recommend
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"x")
    base = ["--checkpoint", str(ck), "--all-users"]
    a = recommend.parse(base + ["--index", "ivf-int8"])
    assert (a.index, a.nlist, a.nprobe, a.seed, a.rerank) == ("ivf-int8", 1024, 32, 0, 4)
    a = recommend.parse(base + ["--index", "ivf-int8", "--nlist", "8"])
    assert (a.nlist, a.nprobe) == (8, 8)
    a = recommend.parse(base + ["--index", "ivf-int8", "--nlist", "64", "--nprobe", "5", "--seed", "3", "--rerank", "9"])
    assert (a.nlist, a.nprobe, a.seed, a.rerank) == (64, 5, 3, 9)
    assert recommend.parse(base).rerank is None
    cases = [(["--index", "ivf-int8", "--nlist", "16", "--nprobe", "17"], "--nprobe"),
             (["--index", "ivf-int8", "--nlist", "1024", "--nprobe", "257"], "--nprobe"),
             (["--index", "ivf-int8", "--nprobe", "0"], "--nprobe"),
             (["--index", "ivf-int8", "--nlist", "0"], "--nlist"),
             (["--index", "ivf-int8", "--rerank", "0"], "--rerank"),
             # the pinned behaviour of the other choices
             (["--nlist", "16"], "--index ivf"),
             (["--index", "brute", "--nprobe", "4"], "--index ivf"),
             (["--index", "int8", "--nprobe", "4"], "--index ivf"),
             (["--rerank", "4"], "--index int8"),
             (["--index", "ivf", "--rerank", "4"], "--index int8"),
             (["--index", "annoy"], "invalid choice")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            recommend.parse(base + argv)
        assert e.value.code == 2, argv
    for argv, word in cases:
        r = _recommend(*base, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr[-500:])
    r = _recommend("--help")
    assert r.returncode == 0 and "ivf-int8" in r.stdout


@pytest.fixture(scope="module")
def recall_data():
    x, q = clustered(**RECALL_CORPUS)
    return x, q, exact_topk_ids(q, x, 10)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_restatement_recall(recall_data, seed):
    """The calibration behind the GPU test's recall condition: the int8 candidates of the probed union, re-ranked exactly,
    agree with the f32 IVF answer and lose no recall against the exact answer.  Measured: agreement 1.000 at every (k, k1);
    recall@10 0.8719 / 0.8715 / 0.8703 at seeds 0 / 1 / 2."""
    x, q, exact = recall_data
    cent, off, order = np_ivf_build(x, RECALL_NLIST, seed)
    for k, k1 in RECALL_CASES:
        got = np_ivf_i8_search(q, x, cent, off, order, k, k1, RECALL_NPROBE)
        agree = recall_at_k(got, np_ivf_search(q, x, cent, off, order, k, RECALL_NPROBE))
        print(f"seed {seed} k {k} k1 {k1}: agreement {agree:.4f}")
        assert agree >= int8_check.RECALL_MIN, (seed, k, k1, agree)
        if k == 10:
            rec = recall_at_k(got, exact)
            print(f"seed {seed} k {k} k1 {k1}: recall@10 {rec:.4f}")
            assert rec >= ivf_check.RECALL_MIN + 0.05, (seed, k, k1, rec)


def _audit_mod():
    spec = importlib.util.spec_from_file_location("audit_barriers", ROOT / "tests" / "isa_audit" / "audit_barriers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ivf_i8_kernels_barrier_loops_close_on_scalar_control_and_use_no_scratch(tmp_path):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "ivf_i8.s"
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
    assert len(bodies) == 4 and all("ivf_i8_" in name for name in bodies), list(bodies)     # the select kernel at 4 dims
    for name, body in bodies.items():
        r = audit.audit(body)
        bad = r["vector"] or r["unknown"] or r["masked"] or (r["in_loop"] and not r["scalar"])
        assert not bad, (name, r)
        assert r["barriers"] == 0, (name, r)                 # one-wave workgroups: __syncthreads orders LDS, no s_barrier
        assert sum("v_mfma_i32_32x32x32_i8" in l for l in body) >= 1, name
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "ivf_i8.o"),
                          str(SRC)], check=True, capture_output=True, text=True, timeout=900).stderr
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res)]
    assert len(scratch) == 4 and all(x == 0 for x in scratch), scratch

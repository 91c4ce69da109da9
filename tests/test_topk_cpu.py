"""Exact top-k retrieval without a GPU: argument validation of tt_retrieval_topk_f32 (before any launch), the workspace
query, the recommend CLI's argument handling, the tie-aware checker itself, and the ISA audit of csrc/topk.hip."""
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

from topk_check import check_topk
from two_tower_amazon_recommender_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parents[1]
TOPK = ROOT / "two_tower_amazon_recommender_amd" / "csrc" / "topk.hip"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _buf(n, align=256, offset=0):
    """A host buffer whose address is `offset` past an `align` boundary (the entry point only checks pointers)."""
    raw = (C.c_uint8 * (n + 2 * align))()
    base = (C.addressof(raw) + align - 1) // align * align + offset
    return raw, base


def _call(lib, q, c, nq, nc, dim, k, ws, ws_bytes, s, i, off=None, idx=None):
    return lib.tt_retrieval_topk_f32(q, c, nq, nc, dim, k, off, idx, ws, ws_bytes, s, i, None)


def test_topk_validates_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.tt_abi_version() == 10 and _lib.TT_TOPK_MAX_K == 256
    nq, nc, d = 4, 1000, 64
    keep = []
    q = _buf(nq * d * 4); c = _buf(nc * d * 4); s = _buf(nq * 256 * 4); i = _buf(nq * 256 * 8)
    ws_bytes = lib.tt_retrieval_topk_workspace_bytes(nq, nc, d, 256)
    ws = _buf(ws_bytes)
    keep += [q, c, s, i, ws]
    Q, Cc, S, I, W = q[1], c[1], s[1], i[1], ws[1]

    def rc(*, nq=nq, nc=nc, dim=d, k=10, q=Q, c=Cc, ws=W, ws_bytes=ws_bytes, s=S, i=I, off=None, idx=None):
        return _call(lib, q, c, nq, nc, dim, k, ws, ws_bytes, s, i, off, idx), lib.tt_last_error().decode()

    for kw, code, word in [(dict(k=0), _lib.TT_ERR_INVALID_ARG, "k 0"),
                           (dict(k=257), _lib.TT_ERR_INVALID_ARG, "k 257"),
                           (dict(nc=100, k=101), _lib.TT_ERR_INVALID_ARG, "exceeds nc"),
                           (dict(dim=48), _lib.TT_ERR_INVALID_ARG, "dim 48"),
                           (dict(q=None), _lib.TT_ERR_INVALID_ARG, "null"),
                           (dict(c=None), _lib.TT_ERR_INVALID_ARG, "null"),
                           (dict(ws=None), _lib.TT_ERR_INVALID_ARG, "null"),
                           (dict(s=None), _lib.TT_ERR_INVALID_ARG, "null"),
                           (dict(i=None), _lib.TT_ERR_INVALID_ARG, "null"),
                           (dict(q=Q + 4), _lib.TT_ERR_INVALID_ARG, "16-byte aligned"),
                           (dict(c=Cc + 8), _lib.TT_ERR_INVALID_ARG, "16-byte aligned"),
                           (dict(ws=W + 16), _lib.TT_ERR_INVALID_ARG, "256-byte aligned"),
                           (dict(i=I + 4), _lib.TT_ERR_INVALID_ARG, "aligned"),
                           (dict(off=W), _lib.TT_ERR_INVALID_ARG, "together"),
                           (dict(nq=0), _lib.TT_ERR_INVALID_ARG, "positive"),
                           (dict(nc=2**31), _lib.TT_ERR_INVALID_ARG, "2^31"),
                           (dict(ws_bytes=ws_bytes - 1, k=256), _lib.TT_ERR_WORKSPACE, "workspace")]:
        got, msg = rc(**kw)
        assert got == code, (kw, got, msg)
        assert word in msg and msg.startswith("tt_retrieval_topk_f32"), (kw, msg)


def test_topk_workspace_size_query():
    lib = _lib.load()
    f = lib.tt_retrieval_topk_workspace_bytes
    assert f(1, 1000, 32, 1) > 0 and f(1, 1000, 32, 1) % 256 == 0
    for bad in [(0, 10, 32, 1), (4, 0, 32, 1), (4, 10, 32, 0), (4, 10, 32, 11), (4, 1000, 32, 257), (4, 2**31, 32, 1)]:
        assert f(*bad) == 0, bad
    # grows with nq and k; a serving batch over 10 M items uses far more than the scorer's 64 splits
    assert f(16, 10_000_000, 128, 100) > f(16, 10_000_000, 128, 10) > 0
    assert f(16, 10_000_000, 128, 100) >= 16 * 1024 * 100 * 8
    assert f(8192, 1_000_000, 128, 100) < 2**28
    from two_tower_amazon_recommender_amd import ops
    assert ops.retrieval_topk_workspace_bytes(7, 4097, 64, 10) == f(7, 4097, 64, 10)


def test_ops_refuses_bad_arguments_as_python_exceptions():
    from two_tower_amazon_recommender_amd import ops
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.retrieval_topk(torch.zeros(2, 32), torch.zeros(10, 32), 3)
    with pytest.raises(TypeError):
        ops.exclusions_csr("nope", 2)


def _recommend(*argv):
    return subprocess.run([sys.executable, "-m", "two_tower_amazon_recommender_amd.recommend", *argv], capture_output=True,
                          text=True, timeout=120, cwd=str(ROOT))


def test_recommend_help_and_argument_errors(tmp_path):
    r = _recommend("--help")
    assert r.returncode == 0
    for flag in ("--checkpoint", "--k", "--users-file", "--all-users", "--data", "--exclude-seen", "--out"):
        assert flag in r.stdout, flag
    from two_tower_amazon_recommender_amd import recommend
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"x")
    cases = [([], "--checkpoint"),
             (["--checkpoint", str(ck)], "--users-file"),
             (["--checkpoint", str(ck), "--all-users", "--users-file", "u.npy"], "not allowed"),
             (["--checkpoint", str(ck), "--all-users", "--k", "0"], "--k"),
             (["--checkpoint", str(ck), "--all-users", "--k", "257"], "--k"),
             (["--checkpoint", str(ck), "--all-users", "--exclude-seen"], "--data"),
             (["--checkpoint", str(tmp_path / "missing.pt"), "--all-users"], "no such file"),
             (["--checkpoint", str(ck) + ".rank0of2", "--all-users"], "rankRofW")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            recommend.parse(argv)
        assert e.value.code == 2, argv
    for argv, word in cases:
        r = _recommend(*argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr[-500:])
    (tmp_path / "sh.pt.rank0of2").write_bytes(b"x")
    r = _recommend("--checkpoint", str(tmp_path / "sh.pt"), "--all-users")
    assert r.returncode == 2 and "sharded" in r.stderr


def test_recommend_builds_each_users_exclusions():
    from two_tower_amazon_recommender_amd import recommend
    u = np.array([2, 0, 2, 1, 2, 0])
    it = np.array([10, 11, 12, 13, 14, 15])
    starts, items = recommend.seen_csr(u, it, 4)
    off, idx = recommend.batch_exclusions(starts, items, np.array([2, 3, 0]))
    assert off.tolist() == [0, 3, 3, 5]
    assert idx.tolist() == [10, 12, 14, 11, 15]


def test_item_categories_helper():
    from two_tower_amazon_recommender_amd import data
    out = data.item_categories(np.array([3, 1, 3, 0]), np.array([7, 8, 9, 5]), 5)
    assert out.tolist() == [5, 8, 0, 7, 0]


def test_checker_accepts_exact_answers_and_rejects_wrong_ones():
    q = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    c = torch.tensor([[3.0, 0.0], [2.0, 5.0], [2.0, 1.0], [3.0, 0.0], [-1.0, 1.0]])
    # query 0 scores 3, 2, 2, 3, -1: a tie at the top and a tie across the cut at k = 3
    good_s = torch.tensor([[3.0, 3.0, 2.0], [5.0, 1.0, 1.0]])
    good_i = torch.tensor([[0, 3, 1], [1, 2, 4]])
    check_topk(q, c, 3, good_s, good_i)
    check_topk(q, c, 3, torch.tensor([[3.0, 3.0, 2.0], [5.0, 1.0, 1.0]]), torch.tensor([[0, 3, 2], [1, 4, 2]]))  # any tie member
    bad = [(good_s, torch.tensor([[0, 3, 4], [1, 2, 4]])),                        # a candidate below the cut returned
           (good_s, torch.tensor([[0, 1, 2], [1, 2, 4]])),                        # a candidate above t missing (index 3)
           (torch.tensor([[3.0, 3.0, 2.5], [5.0, 1.0, 1.0]]), good_i),             # a score off its f64 value
           (torch.tensor([[3.0, 3.0, 2.0], [1.0, 5.0, 1.0]]), torch.tensor([[0, 3, 1], [2, 1, 4]])),   # not descending
           (good_s, torch.tensor([[0, 0, 1], [1, 2, 4]]))]                        # a duplicate
    for s, i in bad:
        with pytest.raises(AssertionError):
            check_topk(q, c, 3, s, i)
    # exclusions: query 0 loses 0 and 3 -> (1, 2) tie at 2, then -1; query 1 loses all but one -> padding
    ex = [[0, 3, 99], [0, 1, 2, 3]]
    s = torch.tensor([[2.0, 2.0, -1.0], [1.0, float("-inf"), float("-inf")]])
    i = torch.tensor([[1, 2, 4], [4, -1, -1]])
    check_topk(q, c, 3, s, i, excluded=ex)
    with pytest.raises(AssertionError):
        check_topk(q, c, 3, torch.tensor([[3.0, 2.0, 2.0], [1.0, float("-inf"), float("-inf")]]), torch.tensor([[0, 1, 2], [4, -1, -1]]),
                   excluded=ex)                                                  # an excluded index returned
    with pytest.raises(AssertionError):
        check_topk(q, c, 3, s, torch.tensor([[1, 2, 4], [4, 0, -1]]), excluded=ex)   # the tail is not padding


def _audit_mod():
    spec = importlib.util.spec_from_file_location("audit_barriers", ROOT / "tests" / "isa_audit" / "audit_barriers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_topk_kernels_barrier_loops_close_on_scalar_control_and_use_no_scratch(tmp_path):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "topk.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(TOPK)], check=True, capture_output=True, timeout=900)
    lines = out.read_text().split("\n")
    audit = _audit_mod()
    bodies = {}
    i = 0
    while i < len(lines):                                    # the audit's kernel splitter, for the top-k kernel names
        m = re.match(r"^(_Z\S*topk_\S*kernel\S*):", lines[i])
        if m:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            bodies[m.group(1)] = lines[i:j]
            i = j
        i += 1
    assert len(bodies) == 5, list(bodies)                    # select at dims 32 / 64 / 128 / 256, merge
    for name, body in bodies.items():
        r = audit.audit(body)
        bad = r["vector"] or r["unknown"] or r["masked"] or (r["in_loop"] and not r["scalar"])
        assert not bad, (name, r)
        if "select" in name:                                 # one-wave workgroups: __syncthreads orders LDS, no s_barrier
            assert r["barriers"] == 0, (name, r)
        else:
            assert r["barriers"] >= 1, (name, r)
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "topk.o"),
                          str(TOPK)], check=True, capture_output=True, text=True, timeout=900).stderr
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res)]
    assert len(scratch) == 5 and all(x == 0 for x in scratch), scratch

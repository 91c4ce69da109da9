"""IVF approximate top-k without a GPU: argument validation of tt_ivf_search_f32 (before any launch), the workspace query,
ops / serving refusals, the recommend CLI's --index ivf arguments, the NumPy restatement's recall calibration, and the ISA
audit of csrc/ivf.hip."""
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

from ivf_check import (RECALL_CORPUS, RECALL_K, RECALL_MIN, RECALL_NLIST, RECALL_NPROBE, clustered, exact_topk_ids,
                       np_ivf_build, np_ivf_search, recall_at_k)
from two_tower_amazon_recommender_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parents[1]
IVF_SRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc" / "ivf.hip"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _buf(n, align=256, offset=0):
    raw = (C.c_uint8 * (n + 2 * align))()
    base = (C.addressof(raw) + align - 1) // align * align + offset
    return raw, base


def test_ivf_validates_arguments_before_any_launch():
    lib = _lib.load()
    nq, nlist, n, d = 4, 64, 5000, 64
    keep = []
    bufs = {name: _buf(size) for name, size in [("q", nq * d * 4), ("c", nlist * d * 4), ("off", (nlist + 1) * 8),
                                                 ("v", n * d * 4), ("ids", n * 4), ("s", nq * 256 * 4), ("i", nq * 256 * 8),
                                                 ("ex", 64)]}
    keep += list(bufs.values())
    ws_bytes = lib.tt_ivf_search_workspace_bytes(nq, nlist, n, d, 256, 64)
    assert ws_bytes > 0
    ws = _buf(ws_bytes)
    keep.append(ws)
    P = {k: v[1] for k, v in bufs.items()}

    def rc(*, q=P["q"], nq=nq, c=P["c"], nlist=nlist, off=P["off"], v=P["v"], ids=P["ids"], n=n, dim=d, k=10, nprobe=8,
           eo=None, ei=None, w=ws[1], wb=ws_bytes, s=P["s"], i=P["i"]):
        got = lib.tt_ivf_search_f32(q, nq, c, nlist, off, v, ids, n, dim, k, nprobe, eo, ei, w, wb, s, i, None)
        return got, lib.tt_last_error().decode()

    E = _lib.TT_ERR_INVALID_ARG
    for kw, code, word in [(dict(nprobe=65), E, "nprobe 65"),
                           (dict(nprobe=0), E, "nprobe 0"),
                           (dict(nlist=300, nprobe=257), E, "nprobe 257"),
                           (dict(k=257), E, "k 257"),
                           (dict(k=0), E, "k 0"),
                           (dict(dim=48), E, "dim 48"),
                           (dict(q=P["q"] + 4), E, "16-byte aligned"),
                           (dict(c=P["c"] + 8), E, "16-byte aligned"),
                           (dict(v=P["v"] + 4), E, "16-byte aligned"),
                           (dict(off=P["off"] + 4), E, "aligned"),
                           (dict(ids=P["ids"] + 2), E, "aligned"),
                           (dict(w=ws[1] + 16), E, "256-byte aligned"),
                           (dict(i=P["i"] + 4), E, "aligned"),
                           (dict(eo=P["ex"]), E, "together"),
                           (dict(ei=P["ex"]), E, "together"),
                           (dict(eo=P["ex"] + 4, ei=P["ex"]), E, "8-byte aligned"),
                           (dict(q=None), E, "null"),
                           (dict(ids=None), E, "null"),
                           (dict(off=None), E, "null"),
                           (dict(nq=0), E, "positive"),
                           (dict(n=0), E, "positive"),
                           (dict(n=2**31), E, "2^31"),
                           (dict(wb=ws_bytes - 1, k=256, nprobe=64), _lib.TT_ERR_WORKSPACE, "workspace")]:
        got, msg = rc(**kw)
        assert got == code, (kw, got, msg)
        assert word in msg and msg.startswith("tt_ivf_search_f32"), (kw, msg)


def test_ivf_workspace_size_query():
    lib = _lib.load()
    f = lib.tt_ivf_search_workspace_bytes
    assert f(1, 64, 5000, 32, 1, 1) > 0 and f(1, 64, 5000, 32, 1, 1) % 256 == 0
    for bad in [(0, 64, 5000, 32, 10, 8), (4, 0, 5000, 32, 10, 1), (4, 64, 0, 32, 10, 8), (4, 64, 5000, 48, 10, 8),
                (4, 64, 5000, 32, 0, 8), (4, 64, 5000, 32, 257, 8), (4, 64, 5000, 32, 10, 65), (4, 64, 5000, 32, 10, 0),
                (4, 300, 5000, 32, 10, 257), (4, 64, 2**31, 32, 10, 8)]:
        assert f(*bad) == 0, bad
    # grows with nq, k and nprobe; includes the coarse probe's own top-k workspace
    assert f(16, 4096, 10_000_000, 128, 100, 32) > f(16, 4096, 10_000_000, 128, 10, 32) > 0
    assert f(16, 4096, 10_000_000, 128, 100, 128) > f(16, 4096, 10_000_000, 128, 100, 32)
    assert f(16, 4096, 10_000_000, 128, 100, 32) > lib.tt_retrieval_topk_workspace_bytes(16, 4096, 128, 32)
    assert f(16, 4096, 10_000_000, 128, 100, 32) >= 16 * 32 * 100 * 8
    from two_tower_amazon_recommender_amd import ops
    assert ops.ivf_search_workspace_bytes(7, 100, 4097, 64, 10, 9) == f(7, 100, 4097, 64, 10, 9)


def test_ops_and_serving_refuse_bad_arguments():
    from two_tower_amazon_recommender_amd import ops
    from two_tower_amazon_recommender_amd.serving import IVF
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.ivf_search(torch.zeros(2, 32), torch.zeros(4, 32), torch.zeros(5, dtype=torch.int64), torch.zeros(10, 32),
                       torch.zeros(10, dtype=torch.int32), 3, 2)
    with pytest.raises(ValueError, match="nprobe"):
        IVF(nlist=8, nprobe=9)
    with pytest.raises(ValueError, match="nprobe"):
        IVF(nlist=300, nprobe=257)
    with pytest.raises(ValueError, match="nlist"):
        IVF(nlist=0)
    with pytest.raises(RuntimeError, match="index"):
        IVF(nlist=8, nprobe=2)(torch.zeros(1, 32))
    with pytest.raises(RuntimeError, match="index"):
        IVF(nlist=8, nprobe=2).state_dict()


def _recommend(*argv):
    return subprocess.run([sys.executable, "-m", "two_tower_amazon_recommender_amd.recommend", *argv], capture_output=True,
                          text=True, timeout=120, cwd=str(ROOT))


def test_recommend_index_arguments(tmp_path):
    from two_tower_amazon_recommender_amd import recommend
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"x")
    base = ["--checkpoint", str(ck), "--all-users"]
    a = recommend.parse(base)
    assert a.index == "brute"
    a = recommend.parse(base + ["--index", "ivf"])
    assert (a.index, a.nlist, a.nprobe) == ("ivf", 1024, 32)
    a = recommend.parse(base + ["--index", "ivf", "--nlist", "8"])
    assert (a.nlist, a.nprobe) == (8, 8)
    cases = [(["--index", "annoy"], "invalid choice"),
             (["--index", "ivf", "--nlist", "0"], "--nlist"),
             (["--index", "ivf", "--nlist", "16", "--nprobe", "17"], "--nprobe"),
             (["--index", "ivf", "--nlist", "1024", "--nprobe", "257"], "--nprobe"),
             (["--index", "ivf", "--nprobe", "0"], "--nprobe"),
             (["--nlist", "16"], "--index ivf"),
             (["--index", "brute", "--nprobe", "4"], "--index ivf")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            recommend.parse(base + argv)
        assert e.value.code == 2, argv
    for argv, word in cases:
        r = _recommend(*base, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr[-500:])
    r = _recommend("--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--index", "--nlist", "--nprobe"))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_numpy_restatement_recall(seed):
    """The calibration behind RECALL_MIN: the NumPy restatement of the index reaches it on the recall corpus."""
    x, q = clustered(**RECALL_CORPUS)
    cent, off, order = np_ivf_build(x, RECALL_NLIST, seed)
    assert np.allclose(np.linalg.norm(cent, axis=1), 1.0)
    assert np.array_equal(np.sort(order), np.arange(x.shape[0]))
    rec = recall_at_k(np_ivf_search(q, x, cent, off, order, RECALL_K, RECALL_NPROBE), exact_topk_ids(q, x, RECALL_K))
    assert RECALL_MIN + 0.05 <= rec <= 0.95, rec                              # a margin above the threshold; not trivial
    full = np_ivf_search(q[:32], x, cent, off, order, RECALL_K, RECALL_NLIST)
    assert recall_at_k(full, exact_topk_ids(q[:32], x, RECALL_K)) == 1.0      # nprobe = nlist is exact


def _audit_mod():
    spec = importlib.util.spec_from_file_location("audit_barriers", ROOT / "tests" / "isa_audit" / "audit_barriers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ivf_kernels_barrier_loops_close_on_scalar_control_and_use_no_scratch(tmp_path):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "ivf.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(IVF_SRC)], check=True, capture_output=True, timeout=900)
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
    assert len(bodies) == 5 and all("ivf_" in name for name in bodies), list(bodies)   # select at 4 dims, bucket
    for name, body in bodies.items():
        r = audit.audit(body)
        bad = r["vector"] or r["unknown"] or r["masked"] or (r["in_loop"] and not r["scalar"])
        assert not bad, (name, r)
        if "select" in name:                                 # one-wave workgroups: __syncthreads orders LDS, no s_barrier
            assert r["barriers"] == 0, (name, r)
        else:
            assert r["barriers"] >= 1, (name, r)
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                          "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "ivf.o"),
                          str(IVF_SRC)], check=True, capture_output=True, text=True, timeout=900).stderr
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", res)]
    assert len(scratch) == 5 and all(x == 0 for x in scratch), scratch

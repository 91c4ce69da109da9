"""MMR diversified re-ranking without a GPU: the NumPy restatement's self-checks (mmr_check.py), every refusal of
tt_mmr_rerank_f32 (arguments are validated before any launch), ops / serving / recommend argument errors and the item-group
helper of data.py."""
import ctypes as C
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmr_check import cluster_corpus, intra_list_cosine, np_dot_all, np_mmr

from two_tower_amazon_recommender_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_dot_is_four_partial_sums():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 12)).astype(np.float32)
    g = np_dot_all(x)
    for j in range(3):
        for p in range(3):
            s = [np.float32(0)] * 4
            for d in range(12):
                s[d % 4] = np.float32(s[d % 4] + np.float32(x[j, d] * x[p, d]))
            assert g[j, p] == np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3]))
    assert g.dtype == np.float32


def test_restatement_lambda_one_is_the_identity():
    c, groups, q, s, i = cluster_corpus()
    for k in (1, 10, 64):
        os_, oi = np_mmr(s, i, c, k, 1.0)
        assert np.array_equal(oi, i[:, :k]) and np.array_equal(os_.view(np.int32), s[:, :k].view(np.int32))
    # ... and skips invalid candidates: the first k valid ones, in order
    s2, i2 = s[:2].copy(), i[:2].copy()
    i2[0, 3] = -1
    i2[1, 0] = c.shape[0]
    s2[1, 5] = np.inf
    _, oi = np_mmr(s2, i2, c, 5, 1.0)
    assert oi[0].tolist() == i2[0, [0, 1, 2, 4, 5]].tolist() and oi[1].tolist() == i2[1, [1, 2, 3, 4, 6]].tolist()


def test_restatement_intra_list_cosine_falls_with_lambda():
    c, groups, q, s, i = cluster_corpus()
    spans = [len(set(groups[row].tolist())) for row in i]
    assert min(spans) >= 4                                       # the pools mix several clusters: there is something to trade
    ils = {lam: intra_list_cosine(c, np_mmr(s, i, c, 10, lam)[1]) for lam in (1.0, 0.5, 0.0)}
    print("pool groups", min(spans), max(spans), "intra-list cosine", ils)
    assert ils[1.0] > ils[0.5] > ils[0.0]


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_restatement_group_caps(cap):
    c, groups, q, s, i = cluster_corpus()
    g = groups.copy()
    g[::7] = -1                                                  # ungrouped rows are never capped
    for lam in (1.0, 0.5):
        for k in (10, 40):
            _, oi = np_mmr(s, i, c, k, lam, g, cap)
            for row, pool in zip(oi, i):
                got = row[row >= 0]
                gg = g[got]
                ids, counts = np.unique(gg[gg >= 0], return_counts=True)
                assert counts.size == 0 or counts.max() <= cap
                assert len(set(got.tolist())) == len(got) and set(got.tolist()) <= set(pool.tolist())
                pg = g[pool]
                _, members = np.unique(pg[pg >= 0], return_counts=True)
                assert len(got) == min(k, int(np.minimum(members, cap).sum() + (pg < 0).sum()))
                assert (row[len(got):] == -1).all()


def test_restatement_ties_zero_rows_and_padding():
    c = np.zeros((6, 4), dtype=np.float32)
    c[0] = c[1] = [1, 2, 3, 4]                                   # duplicates: the twin of a picked row carries the largest penalty
    c[2] = [4, -3, 2, -1]                                        # orthogonal to row 0; row 3 is a zero row (inv = 0, sim = 0)
    c[4] = [-1, -2, -3, -4]                                      # opposite of row 0: no bonus (the penalty is floored at 0)
    s = np.array([[3, 3, 3, 3, 3, -np.inf]], dtype=np.float32)   # all scores equal: rel = 0, ties go to the lower position
    i = np.array([[0, 1, 2, 3, 4, -1]], dtype=np.int64)
    os_, oi = np_mmr(s, i, c, 6, 0.5)
    assert oi[0].tolist() == [0, 2, 3, 4, 1, -1]                 # 2, 3 and 4 tie at penalty 0, in position order; the twin is last
    assert os_[0, 5] == -np.inf and (os_[0, :5] == 3).all()
    os_, oi = np_mmr(np.full((1, 3), -np.inf, np.float32), np.full((1, 3), -1), c, 2, 0.3)
    assert oi.tolist() == [[-1, -1]] and np.isneginf(os_).all()


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def _call(lib, **over):
    raw = (C.c_uint8 * 4096)()
    base = (C.addressof(raw) + 255) // 256 * 256
    a = dict(scores=base, idx=base + 512, nq=2, k1=8, c=base + 1024, nc=100, dim=32, groups=None, max_per_group=0,
             lam=0.5, k=4, out_scores=base + 2048, out_idx=base + 2560, stream=None)
    for name, v in over.items():
        a[name] = (base + 1024 + v[1]) if isinstance(v, tuple) else v
    rc = lib.tt_mmr_rerank_f32(a["scores"], a["idx"], a["nq"], a["k1"], a["c"], a["nc"], a["dim"], a["groups"],
                               a["max_per_group"], a["lam"], a["k"], a["out_scores"], a["out_idx"], a["stream"])
    return rc, lib.tt_last_error().decode()


REFUSALS = [
    (dict(scores=None), "null"), (dict(idx=None), "null"), (dict(c=None), "null"), (dict(out_scores=None), "null"),
    (dict(out_idx=None), "null"),
    (dict(nq=-1), "nq"),
    (dict(k1=0), "k1"), (dict(k1=_lib.TT_TOPK_MAX_K + 1, k=4), "k1"),
    (dict(k=0), ": k "), (dict(k=9), ": k "),
    (dict(dim=0), "dim"), (dict(dim=30), "dim"), (dict(dim=1028), "dim"), (dict(dim=-4), "dim"),
    (dict(nc=0), "nc"), (dict(nc=2 ** 31), "nc"),
    (dict(lam=-0.01), "lambda"), (dict(lam=1.5), "lambda"), (dict(lam=float("nan")), "lambda"),
    (dict(max_per_group=-1), "max_per_group"),
    (dict(max_per_group=2), "groups"),
    (dict(c=("offset", 4)), "16-byte"),
]


@pytest.mark.parametrize("over,word", REFUSALS, ids=[f"{list(o)[0]}={list(o.values())[0]}" for o, _ in REFUSALS])
def test_abi_refuses_bad_arguments_before_any_launch(over, word):
    lib = _lib.load()
    rc, msg = _call(lib, **over)
    assert rc == _lib.TT_ERR_INVALID_ARG, (over, rc, msg)
    assert msg.startswith("tt_mmr_rerank_f32") and word in msg, (over, msg)


def test_abi_empty_batch_launches_nothing():
    rc, _ = _call(_lib.load(), nq=0)
    assert rc == _lib.TT_OK


# ------------------------------------------------------------------------------------------------ Python surface
def test_ops_and_serving_refuse_bad_arguments():
    from two_tower_amazon_recommender_amd import ops, torch_ops
    from two_tower_amazon_recommender_amd.serving import MMR, BruteForce
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.mmr_rerank(torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int64), torch.zeros(10, 32), 4, 0.5)
    with pytest.raises(TypeError):
        ops.mmr_rerank("nope", None, None, 4, 0.5)
    for kw, word in [(dict(lambda_=1.5), "lambda_"), (dict(lambda_=-0.1), "lambda_"), (dict(lambda_=float("nan")), "lambda_"),
                     (dict(pool=0), "pool"), (dict(max_per_group=-1), "max_per_group")]:
        with pytest.raises(ValueError, match=word):
            MMR(BruteForce(), **kw)
    with pytest.raises(RuntimeError, match="index"):
        MMR(BruteForce())(torch.zeros(1, 32))
    with pytest.raises(ValueError, match="groups"):
        MMR(BruteForce(), max_per_group=2).index(torch.zeros(10, 32))
    with pytest.raises(RuntimeError, match="no state"):
        MMR(BruteForce()).state_dict()
    assert MMR(BruteForce(k=7)).k == 7
    assert "mmr_rerank" in torch_ops.OPS and hasattr(torch.ops.twotower, "mmr_rerank")
    m = dict(device="meta")
    s, i = torch.ops.twotower.mmr_rerank(torch.empty(5, 40, **m), torch.empty(5, 40, dtype=torch.int64, **m),
                                         torch.empty(100, 32, **m), 10, 0.7, None, 0)
    assert s.shape == (5, 10) and s.dtype == torch.float32 and i.shape == (5, 10) and i.dtype == torch.int64


def test_item_category_groups_takes_the_first_interaction():
    from two_tower_amazon_recommender_amd import data
    item = np.array([3, 1, 3, 0, 1, 9], dtype=np.int64)
    code = np.array([5, 2, 7, 0, 4, 1], dtype=np.int64)
    g = data.item_category_groups(item, code, 6)
    assert g.dtype == np.int32 and g.tolist() == [0, 2, -1, 5, -1, -1]      # items 2, 4, 5 never seen; item 9 is out of range


def _recommend(*argv):
    return subprocess.run([sys.executable, "-m", "two_tower_amazon_recommender_amd.recommend", *argv], capture_output=True,
                          text=True, timeout=120, cwd=str(ROOT))


def test_recommend_diversify_arguments(tmp_path):
    from two_tower_amazon_recommender_amd import recommend
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"x")
    data = tmp_path / "d.parquet"
    data.write_bytes(b"x")
    base = ["--checkpoint", str(ck), "--all-users"]
    a = recommend.parse(base)
    assert a.diversify is None and a.diversify_pool is None and a.max_per_category is None
    a = recommend.parse(base + ["--diversify", "0.3"])
    assert (a.diversify, a.diversify_pool, a.max_per_category) == (0.3, 4, None)
    a = recommend.parse(base + ["--diversify", "0", "--diversify-pool", "8", "--index", "ivf-int8"])
    assert (a.diversify, a.diversify_pool, a.index) == (0.0, 8, "ivf-int8")
    a = recommend.parse(base + ["--max-per-category", "2", "--data", str(data)])
    assert (a.diversify, a.diversify_pool, a.max_per_category) == (1.0, 4, 2)       # the cap implies --diversify 1.0
    a = recommend.parse(base + ["--max-per-category", "1", "--data", str(data), "--diversify", "0.5"])
    assert (a.diversify, a.max_per_category) == (0.5, 1)
    cases = [(["--diversify", "1.5"], "--diversify must be in [0, 1]"),
             (["--diversify", "-0.1"], "--diversify must be in [0, 1]"),
             (["--diversify", "nan"], "--diversify must be in [0, 1]"),
             (["--max-per-category", "2"], "--max-per-category needs --data"),
             (["--max-per-category", "0", "--data", str(data)], "--max-per-category must be positive"),
             (["--diversify-pool", "4"], "--diversify-pool needs"),
             (["--diversify", "0.5", "--diversify-pool", "0"], "--diversify-pool must be positive")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            recommend.parse(base + argv)
        assert e.value.code == 2, argv
    for argv, word in cases[:4:3]:                                # one subprocess each for the two errors users will meet
        r = _recommend(*base, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.stderr[-500:])

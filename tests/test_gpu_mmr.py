"""MMR diversified re-ranking (tt_mmr_rerank_f32, ops.mmr_rerank, torch.ops.twotower.mmr_rerank, serving.MMR, recommend
--diversify / --max-per-category) on the GPU.  Every step of the contract is one IEEE f32 operation, so the NumPy restatement
(mmr_check.py) is bit-exact: all comparisons are equalities of bits."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmr_check import cluster_corpus, exact_pool, np_mmr

pytestmark = pytest.mark.gpu

# (nq, k1, k, D): one candidate; an odd pool; just past one wave; k = k1 (a permutation); D not a multiple of 32; the largest
# pool whose rows fit LDS; rows that do not fit (the global-memory path)
SHAPES = [(1, 1, 1, 4), (3, 33, 10, 32), (2, 65, 20, 64), (5, 64, 64, 128), (7, 200, 50, 36), (4, 256, 100, 128),
          (2, 256, 256, 256)]
LAMBDAS = [0.0, 0.3, 0.7, 1.0]


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _problem(nq, k1, d):
    """(c f32 [nc, d], groups int32 [nc], pool scores f32 [nq, k1], pool idx int64 [nq, k1]): rows around 8 centroids, so
    that the cosines inside a pool spread from near 0 to near 1; groups in -1..5."""
    rng = np.random.default_rng(1000 * k1 + d)
    nc = max(3 * k1, 5)
    cent = rng.standard_normal((8, d))
    c = (cent[np.arange(nc) % 8] + 0.5 * rng.standard_normal((nc, d))).astype(np.float32)
    q = (cent[rng.integers(0, 8, nq)] + cent[rng.integers(0, 8, nq)] + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    s, i = exact_pool(q, c, k1)
    groups = rng.integers(-1, 6, nc).astype(np.int32)
    for a in (c, groups, s, i):
        a.setflags(write=False)
    return c, groups, s, i


@functools.lru_cache(maxsize=None)
def _reference(nq, k1, k, d, lam, cap):
    c, groups, s, i = _problem(nq, k1, d)
    return np_mmr(s, i, c, k, lam, groups if cap else None, cap)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                   # (a copy: the cached problems are read-only)


def _same(got, ref):
    s, i = got
    assert np.array_equal(i.cpu().numpy(), ref[1])
    assert np.array_equal(s.cpu().numpy().view(np.int32), np.asarray(ref[0], dtype=np.float32).view(np.int32))


def _run(dev, nq, k1, k, d, lam, cap=0):
    c, groups, s, i = _problem(nq, k1, d)
    return _ops().mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), k, lam, groups=_t(groups, dev) if cap else None,
                             max_per_group=cap)


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("nq,k1,k,d", SHAPES)
def test_rerank_is_bit_exact(dev, nq, k1, k, d, lam):
    _same(_run(dev, nq, k1, k, d, lam), _reference(nq, k1, k, d, lam, 0))


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("nq,k1,k,d", [(3, 33, 10, 32), (2, 65, 20, 64), (4, 256, 100, 128), (2, 256, 256, 256)])
def test_group_caps_are_bit_exact(dev, nq, k1, k, d, cap):
    for lam in (0.3, 1.0):
        got = _run(dev, nq, k1, k, d, lam, cap)
        _same(got, _reference(nq, k1, k, d, lam, cap))
        groups = _problem(nq, k1, d)[1]
        for row in got[1].cpu().numpy():
            g = groups[row[row >= 0]]
            assert g.size == 0 or np.bincount(g[g >= 0], minlength=1).max() <= cap


def test_lambda_one_keeps_the_first_k_valid(dev):
    nq, k1, k, d = 7, 200, 50, 36
    c, groups, s, i = _problem(nq, k1, d)
    got_s, got_i = _run(dev, nq, k1, k, d, 1.0)
    assert np.array_equal(got_i.cpu().numpy(), i[:, :k])
    assert np.array_equal(got_s.cpu().numpy().view(np.int32), s[:, :k].view(np.int32))


def test_crafted_rows(dev):
    """Padding with fewer than k valid, a query with nothing valid, indices past the corpus, non-finite scores, equal scores,
    a zero corpus row and duplicated corpus rows."""
    rng = np.random.default_rng(5)
    nc, d, k1, k = 60, 32, 40, 10
    c = rng.standard_normal((nc, d)).astype(np.float32)
    c[7] = 0.0                                                   # a zero row: inv = 0, every cosine with it is 0
    c[11] = c[3]
    c[12] = c[3]                                                 # duplicates: sim 1 with each other, ties to the lower position
    q = rng.standard_normal((7, d)).astype(np.float32)
    s, i = (a.copy() for a in exact_pool(q, c, k1))
    s[0, 5:], i[0, 5:] = -np.inf, -1                             # 5 valid < k: the tail is padding
    s[1, :], i[1, :] = -np.inf, -1                               # nothing valid
    i[2, 1], i[2, 4], i[2, 9] = nc, nc + 7, -5                   # outside the corpus: ignored, never read
    s[3, 2], s[3, 6], s[3, 8] = np.inf, np.nan, -np.inf          # non-finite scores: invalid
    s[4, :] = 0.25                                               # all equal: relevance 0 everywhere
    i[5, :8] = [3, 11, 7, 12, 20, 21, 22, 23]                    # duplicates and the zero row up front
    s[5, :8] = s[5, 0]
    i[6, :] = 7                                                  # only the zero row, k1 times
    ops = _ops()
    ts, ti, tc = _t(s, dev), _t(i, dev), _t(c, dev)
    groups = (np.arange(nc) % 3 - 1).astype(np.int32)
    for lam in (0.0, 0.5, 1.0):
        ref = np_mmr(s, i, c, k, lam)
        _same(ops.mmr_rerank(ts, ti, tc, k, lam), ref)
        assert (ref[1][0, 5:] == -1).all() and (ref[1][1] == -1).all() and not np.isin(ref[1][2], [nc, nc + 7, -5]).any()
        _same(ops.mmr_rerank(ts, ti, tc, k, lam, groups=_t(groups, dev), max_per_group=2), np_mmr(s, i, c, k, lam, groups, 2))
    _same(ops.mmr_rerank(ts, ti, tc, k1, 0.5), np_mmr(s, i, c, k1, 0.5))       # k = k1 over rows with invalid entries


def test_a_query_alone_equals_its_row_in_the_batch_and_runs_repeat(dev):
    ops = _ops()
    for nq, k1, k, d in [(7, 200, 50, 36), (2, 256, 256, 256)]:
        c, groups, s, i = _problem(nq, k1, d)
        ts, ti, tc, tg = _t(s, dev), _t(i, dev), _t(c, dev), _t(groups, dev)
        full = ops.mmr_rerank(ts, ti, tc, k, 0.3, groups=tg, max_per_group=3)
        again = ops.mmr_rerank(ts, ti, tc, k, 0.3, groups=tg, max_per_group=3)
        assert torch.equal(full[1], again[1]) and torch.equal(full[0].view(torch.int32), again[0].view(torch.int32))
        for r in range(nq):
            one = ops.mmr_rerank(ts[r:r + 1].contiguous(), ti[r:r + 1].contiguous(), tc, k, 0.3, groups=tg, max_per_group=3)
            assert torch.equal(one[1][0], full[1][r]) and torch.equal(one[0][0].view(torch.int32), full[0][r].view(torch.int32))


def test_cluster_corpus_on_the_gpu(dev):
    c, groups, q, s, i = cluster_corpus()
    ops = _ops()
    for lam, cap in [(0.5, 0), (0.0, 0), (0.7, 1)]:
        got = ops.mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), 10, lam, groups=_t(groups, dev) if cap else None, max_per_group=cap)
        _same(got, np_mmr(s, i, c, 10, lam, groups if cap else None, cap))


def test_out_tensors_and_empty_batch(dev):
    ops = _ops()
    c, groups, s, i = _problem(3, 33, 32)
    out = (torch.zeros(3, 10, device=dev), torch.zeros(3, 10, dtype=torch.int64, device=dev))
    got = ops.mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), 10, 0.7, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    _same(out, _reference(3, 33, 10, 32, 0.7, 0))
    es, ei = ops.mmr_rerank(torch.empty(0, 33, device=dev), torch.empty(0, 33, dtype=torch.int64, device=dev), _t(c, dev), 10, 0.7)
    assert tuple(es.shape) == (0, 10) and tuple(ei.shape) == (0, 10)
    with pytest.raises(ValueError, match="k ="):
        ops.mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), 34, 0.7)
    with pytest.raises(ValueError, match="lam"):
        ops.mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), 10, 1.5)
    with pytest.raises(ValueError, match="groups"):
        ops.mmr_rerank(_t(s, dev), _t(i, dev), _t(c, dev), 10, 0.5, max_per_group=1)


# ------------------------------------------------------------------------------------------------ 2. public surface
@functools.lru_cache(maxsize=None)
def _serving_problem():
    rng = np.random.default_rng(77)
    n, d, nq = 3000, 64, 19
    cent = rng.standard_normal((30, d))
    x = (cent[np.arange(n) % 30] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, 30, nq)] + cent[rng.integers(0, 30, nq)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    groups = (np.arange(n) % 30).astype(np.int32)
    groups[::11] = -1
    return x, q, groups


def _eq(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_serving_mmr_over_brute_force_and_ivf(dev):
    from two_tower_amazon_recommender_amd.serving import IVF, MMR, BruteForce
    ops = _ops()
    xn, qn, gn = _serving_problem()
    x, q, g = _t(xn, dev), _t(qn, dev), _t(gn, dev)
    pool = ops.retrieval_topk(q, x, ops.default_k1(10, 3000, True, 4))
    assert pool[0].shape[1] == 40
    want = ops.mmr_rerank(pool[0], pool[1], x, 10, 0.7)
    mmr = MMR(BruteForce(k=10), lambda_=0.7).index(x)
    assert _eq(mmr(q), want)
    _same(want, np_mmr(pool[0].cpu().numpy(), pool[1].cpu().numpy(), xn, 10, 0.7))
    assert _eq(mmr(q, k=25), ops.mmr_rerank(*ops.retrieval_topk(q, x, 100), x, 25, 0.7))      # pool = 4 k
    # IVF scanning every list answers what BruteForce answers: the diversified lists agree bit for bit, caps included
    capped = MMR(BruteForce(k=10), lambda_=0.5, pool=6, max_per_group=1).index(x, groups=g)
    ivf = MMR(IVF(k=10, nlist=8, nprobe=8), lambda_=0.5, pool=6, max_per_group=1).index(x, groups=g)
    a, b = capped(q), ivf(q)
    assert _eq(a, b)
    _same(a, np_mmr(*(t.cpu().numpy() for t in ops.retrieval_topk(q, x, 60)), xn, 10, 0.5, gn, 1))
    # the state of an IVF-backed wrapper round-trips (the corpus comes back in original order)
    again = MMR(IVF(k=10, nlist=8, nprobe=8), lambda_=0.5, pool=6, max_per_group=1).load_state_dict(ivf.state_dict())
    assert torch.equal(again._corpus, x) and _eq(again(q), b)
    # lambda = 1 without a cap is the inner index's own top-k
    plain = BruteForce(k=10).index(x)(q)
    assert _eq(MMR(BruteForce(k=10), lambda_=1.0).index(x)(q), plain)
    assert _eq(MMR(IVF(k=10, nlist=8, nprobe=8), lambda_=1.0).index(x)(q), plain)


def test_serving_mmr_identifiers_and_exclusions(dev):
    from two_tower_amazon_recommender_amd.serving import MMR, BruteForce, Int8BruteForce
    ops = _ops()
    xn, qn, gn = _serving_problem()
    x, q = _t(xn, dev), _t(qn, dev)
    ident = torch.arange(3000, device=dev) * 7 + 1000
    first = ops.retrieval_topk(q, x, 12)[1]
    excl = torch.full((19, 16), -1, dtype=torch.int64, device=dev)
    excl[:, :12] = first                                          # every query's 12 best rows are excluded
    mmr = MMR(BruteForce(k=10), lambda_=0.6).index(x, identifiers=ident)
    s, i = mmr.query_with_exclusions(q, excl)
    pool = ops.retrieval_topk(q, x, 40, exclusions=excl)
    rs, ri = ops.mmr_rerank(pool[0], pool[1], x, 10, 0.6)
    assert torch.equal(i, ident[ri]) and torch.equal(s.view(torch.int32), rs.view(torch.int32))
    assert not (ri[:, :, None] == first[:, None, :]).any()
    # padding stays -1 through the identifier map: a pool with fewer valid candidates than k
    few = torch.arange(3000, device=dev)[None, :].expand(19, -1)[:, :2995].contiguous()      # all but 5 rows excluded
    s, i = mmr.query_with_exclusions(q, few, k=10)
    assert (i[:, 5:] == -1).all() and (i[:, :5] >= 1000).all() and torch.isneginf(s[:, 5:]).all()
    # an int8 inner index: its exact re-rank feeds the pool
    i8 = MMR(Int8BruteForce(k=10, rerank=4), lambda_=0.6).index(x)
    inner = Int8BruteForce(k=10, rerank=4).index(x)
    ps, pi = inner(q, k=40)
    assert _eq(i8(q), ops.mmr_rerank(ps, pi, x, 10, 0.6))


def test_torch_op_equals_ops(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    ops = _ops()
    c, groups, s, i = _problem(3, 33, 32)
    ts, ti, tc, tg = _t(s, dev), _t(i, dev), _t(c, dev), _t(groups, dev)
    torch.library.opcheck(torch.ops.twotower.mmr_rerank, (ts, ti, tc, 10, 0.7, None, 0))
    torch.library.opcheck(torch.ops.twotower.mmr_rerank, (ts, ti, tc, 10, 0.3, tg, 2))
    assert _eq(torch.ops.twotower.mmr_rerank(ts, ti, tc, 10, 0.7, None, 0), ops.mmr_rerank(ts, ti, tc, 10, 0.7))
    assert _eq(torch.ops.twotower.mmr_rerank(ts, ti, tc, 10, 0.3, tg, 2), ops.mmr_rerank(ts, ti, tc, 10, 0.3, groups=tg, max_per_group=2))


def _env():
    import os
    import pathlib
    env = dict(os.environ)
    root = str(pathlib.Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def test_recommend_cli_diversifies(dev, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    n_users, n_items, n_cat = 300, 200, 5
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump({"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                                                  "dropout_rate": 0.0, "training": {"batch_size": 256, "epochs": 1},
                                                  "retrieval": {"temperature": 0.1}}}))
    ck = tmp_path / "ck.pt"
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], capture_output=True, text=True, timeout=600,  # noqa: E731
                                    cwd=str(tmp_path.parent), env=_env())
    r = run("two_tower_amazon_recommender_amd.train", "--config", str(cfg_path), "--synthetic", "4096", "--synthetic-users",
            str(n_users), "--synthetic-items", str(n_items), "--save", str(ck))
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(9)
    u = rng.integers(0, n_users, 3000)
    it = rng.integers(0, n_items - 10, 3000)                      # the last 10 items are never seen: group -1, never capped
    u[:n_users] = np.arange(n_users)
    data = tmp_path / "inter.parquet"
    pq.write_table(pa.table({"user_idx": u.astype(np.int64), "item_idx": it.astype(np.int64),
                             "category": [f"cat{v % n_cat}" for v in it]}), data)
    outs = {}
    for name, extra in [("plain", []), ("lam1", ["--diversify", "1.0"]),
                        ("capped", ["--diversify", "0.5", "--max-per-category", "1"])]:
        outs[name] = tmp_path / f"{name}.parquet"
        r = run("two_tower_amazon_recommender_amd.recommend", "--checkpoint", str(ck), "--data", str(data), "--all-users",
                "--exclude-seen", "--k", "10", "--out", str(outs[name]), "--batch-users", "128", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
    plain, lam1, capped = (pq.read_table(outs[n]) for n in ("plain", "lam1", "capped"))
    assert plain.num_rows == n_users * 10 and lam1.equals(plain)
    users, items, rank = (capped.column(n).to_numpy() for n in ("user_idx", "item_idx", "rank"))
    assert 0 < capped.num_rows < n_users * 10
    for usr in range(n_users):
        mine = items[users == usr]
        assert len(mine) >= 1 and rank[users == usr].tolist() == list(range(len(mine)))
        cats = mine[mine < n_items - 10] % n_cat
        assert len(set(cats.tolist())) == len(cats), (usr, mine)

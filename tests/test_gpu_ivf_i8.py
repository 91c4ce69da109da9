"""Int8 IVF (tt_ivf_search_i8_f32, ops.ivf_search_i8, torch.ops.twotower.ivf_search_i8, serving.Int8IVF, recommend --index
ivf-int8) on the GPU.  The yardstick is ops.retrieval_topk_i8 (itself pinned bit for bit to NumPy): over the whole corpus
at nprobe = nlist, and over the union of the probed lists (gathered in ascending original id) otherwise - bit for bit,
scores (compared as int32 patterns) and ids."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

import int8_check
import ivf_check
from ivf_check import RECALL_CORPUS, RECALL_K, RECALL_NLIST, RECALL_NPROBE, clustered, exact_topk_ids, recall_at_k, union_reference

pytestmark = pytest.mark.gpu


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


def _rand(n, d, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n, d, generator=g) * 2.0 - 1.0).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(got, ref):
    s, i = got
    rs, ri = ref
    assert torch.equal(i.cpu(), ri.cpu())
    assert torch.equal(_bits(s.cpu()), _bits(rs.cpu()))


def _csr(ex, dev):
    off = np.zeros(len(ex) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in ex])
    flat = np.concatenate([np.asarray(e, dtype=np.int64) for e in ex]) if off[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev)


def _index_from_assignment(x, assign, nlist, seed, dev):
    """Int8 index arrays (cent, offsets, list_codes, list_scales, list_ids) for an arbitrary list assignment: random unit
    centroids, items stable-sorted by list, the quantised rows permuted into list order."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cent = torch.nn.functional.normalize(torch.randn(nlist, x.shape[1], generator=g), dim=1).to(dev).contiguous()
    a = torch.as_tensor(assign, dtype=torch.int64, device=dev)
    order = torch.argsort(a, stable=True)
    offsets = torch.cat([a.new_zeros(1), torch.cumsum(torch.bincount(a, minlength=nlist), 0)])
    codes, scales = _ops().quantize_rows_i8(x)
    return cent, offsets.contiguous(), codes[order].contiguous(), scales[order].contiguous(), order.to(torch.int32).contiguous()


def _arrays(ivf):
    return ivf.centroids, ivf.list_offsets, ivf.list_codes, ivf.list_scales, ivf.list_ids


def _search(index, q, k, k1, nprobe, c=None, exclusions=None):
    return _ops().ivf_search_i8(q, *index, k, nprobe, c=c, k1=k1, exclusions=exclusions)


def _union_reference(x, index, q, k, k1, nprobe, with_c, excluded=None):
    """ops.retrieval_topk_i8 over each query's probed lists gathered in ascending original id (codes, scales and, with_c, f32
    rows), k and k1 clipped to the union size, exclusions mapped to union positions, ids mapped back."""
    ops = _ops()
    cent, off, _, _, ids = index
    codes, scales = ops.quantize_rows_i8(x)                       # original order
    probes = ops.retrieval_topk(q, cent, nprobe)[1].cpu().numpy()
    lid, offs = ids.cpu().numpy(), off.cpu().numpy()
    nq = q.shape[0]
    S = torch.full((nq, k), float("-inf"))
    I = torch.full((nq, k), -1, dtype=torch.int64)
    for r in range(nq):
        u = union_reference(lid, offs, probes[r])
        if len(u) == 0:
            continue
        kk, kk1 = min(k, len(u)), min(k1, len(u))
        ex = None
        if excluded is not None and len(excluded[r]):
            e = np.asarray(excluded[r], dtype=np.int64)
            pos = np.searchsorted(u, e)
            hit = pos < len(u)
            hit[hit] = u[pos[hit]] == e[hit]
            pos = pos[hit]
            if len(pos):
                ex = (torch.tensor([0, len(pos)], device=q.device), torch.from_numpy(pos.astype(np.int64)).to(q.device))
        ut = torch.from_numpy(u).to(x.device)
        s, i = ops.retrieval_topk_i8(q[r:r + 1].contiguous(), codes[ut].contiguous(), scales[ut].contiguous(), kk,
                                     c=x[ut].contiguous() if with_c else None, k1=kk1, exclusions=ex)
        s, i = s[0].cpu(), i[0].cpu().numpy()
        S[r, :kk] = s
        I[r, :kk] = torch.from_numpy(np.where(i >= 0, u[np.maximum(i, 0)], -1))
    return S, I


# ------------------------------------------------------------------------------------------------ 1. full probe
@pytest.mark.parametrize("d,k,k1,nq,with_c", [(32, 1, 1, 1, False), (64, 10, 40, 33, True), (128, 64, 256, 70, True),
                                              (256, 10, 32, 33, True), (128, 10, 10, 1000, False)])
def test_full_probe_is_the_exhaustive_int8_path_bit_for_bit(dev, d, k, k1, nq, with_c):
    from two_tower_amazon_recommender_amd.serving import Int8IVF
    ops = _ops()
    x, q = _rand(6000, d, 100 + d, dev), _rand(nq, d, 200 + nq, dev)
    idx = Int8IVF(k=k, nlist=40, nprobe=40, iters=3, keep_f32=with_c).index(x)
    counts = idx.list_offsets.diff().cpu().numpy()
    assert (counts % 32 != 0).any()
    codes, scales = ops.quantize_rows_i8(x)
    c = x if with_c else None
    got = _search(_arrays(idx), q, k, k1, 40, c=c)
    ref = ops.retrieval_topk_i8(q, codes, scales, k, c=c, k1=k1)
    _assert_same(got, ref)
    # with exclusions (original ids): empty, the whole answer, and random ids with out-of-range values
    rng = np.random.default_rng(d + k + nq)
    ri_np = ref[1].cpu().numpy()
    ex = [[] if r % 3 == 0 else list(ri_np[r]) if r % 3 == 1 else [int(v) for v in rng.integers(0, 6000, 300)] + [-3, 6000, 2**40]
          for r in range(nq)]
    csr = _csr(ex, dev)
    _assert_same(_search(_arrays(idx), q, k, k1, 40, c=c, exclusions=csr),
                 ops.retrieval_topk_i8(q, codes, scales, k, c=c, k1=k1, exclusions=csr))


# ------------------------------------------------------------------------------------------------ 2. ties across lists
def test_ties_across_lists_go_to_the_lower_id(dev):
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(5)
    base = torch.randint(-4, 5, (37, 64), generator=g).float() / 8.0           # few distinct rows: many exact ties
    x = base[torch.randint(0, 37, (4000,), generator=g)].to(dev).contiguous()
    q = (torch.randint(-4, 5, (9, 64), generator=g).float() / 8.0).to(dev)
    # duplicates of one row sit in different lists: a random assignment, not k-means
    index = _index_from_assignment(x, torch.randint(0, 24, (4000,), generator=g), 24, 6, dev)
    codes, scales = ops.quantize_rows_i8(x)
    ref = ops.retrieval_topk_i8(q, codes, scales, 50, k1=50)
    _assert_same(_search(index, q, 50, 50, 24), ref)
    assert any(len(np.unique(row)) < 50 for row in ref[0].cpu().numpy()), "the corpus must plant ties"
    ref = ops.retrieval_topk_i8(q, codes, scales, 50, c=x, k1=200)
    _assert_same(_search(index, q, 50, 200, 24, c=x), ref)
    assert any(len(np.unique(row)) < 50 for row in ref[0].cpu().numpy()), "the corpus must plant ties"


# ------------------------------------------------------------------------------------------------ 3. partial probe
@pytest.mark.parametrize("d,k,k1,nprobe,nq", [(64, 10, 40, 1, 37), (64, 100, 256, 3, 37), (128, 10, 40, 7, 70),
                                              (32, 256, 256, 5, 9), (256, 20, 80, 12, 33)])
def test_partial_probe_is_the_int8_path_over_the_probed_lists(dev, d, k, k1, nprobe, nq):
    from two_tower_amazon_recommender_amd.serving import Int8IVF
    xn, qn = clustered(8000, d, 60, nq, seed=d + nprobe)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    idx = Int8IVF(k=k, nlist=50, nprobe=nprobe, iters=5).index(x)
    index = _arrays(idx)
    got = _search(index, q, k, k1, nprobe, c=x)
    _assert_same(got, _union_reference(x, index, q, k, k1, nprobe, True))
    rng = np.random.default_rng(nq)
    got_i = got[1].cpu().numpy()
    ex = [list(got_i[r][: k // 2 + 1]) + [int(v) for v in rng.integers(0, 8000, 200)] if r % 2 else [] for r in range(nq)]
    _assert_same(_search(index, q, k, k1, nprobe, c=x, exclusions=_csr(ex, dev)),
                 _union_reference(x, index, q, k, k1, nprobe, True, excluded=ex))
    if d == 128:
        # without c: also against the NumPy stage 1 on the restricted arrays
        s, i = _search(index, q, k, k, nprobe)
        _assert_same((s, i), _union_reference(x, index, q, k, k, nprobe, False))
        ops = _ops()
        codes, scales = (t.cpu().numpy() for t in ops.quantize_rows_i8(x))
        qc, qs = int8_check.np_quantize(qn)
        probes = ops.retrieval_topk(q, idx.centroids, nprobe)[1].cpu().numpy()
        lid, offs = idx.list_ids.cpu().numpy(), idx.list_offsets.cpu().numpy()
        for r in range(nq):
            u = union_reference(lid, offs, probes[r])
            S, I = int8_check.np_stage1(qc[r:r + 1], qs[r:r + 1], codes[u], scales[u], k)
            assert np.array_equal(i[r].cpu().numpy(), np.where(I[0] >= 0, u[np.maximum(I[0], 0)], -1)), r
            assert np.array_equal(s[r].cpu().numpy().view(np.int32), S[0].view(np.int32)), r


# ------------------------------------------------------------------------------------------------ 4. awkward lists
def test_awkward_lists(dev):
    """Empty lists, one list holding most of the corpus, lists shorter than k, probes with fewer than k candidates in
    total (-inf, -1 padding), and nq * nprobe not a multiple of 32."""
    n, d, nlist, k, k1 = 5000, 64, 20, 30, 120
    x = _rand(n, d, 71, dev)
    rng = np.random.default_rng(72)
    assign = np.full(n, 3)                                                   # list 3 holds most of the corpus
    small = rng.choice(n, 400, replace=False)
    assign[small] = rng.choice([0, 5, 6, 9, 11, 12, 17], 400)                # lists 1, 2, 4, 7, ... stay empty
    for j, l in enumerate([13, 14, 15, 16]):                                 # lists shorter than k: 1..4 items
        assign[small[:j + 1]] = l
        small = small[j + 1:]
    index = _index_from_assignment(x, assign, nlist, 73, dev)
    counts = np.bincount(assign, minlength=nlist)
    assert (counts == 0).sum() >= 5 and counts.max() > n // 2 and ((counts > 0) & (counts < k)).sum() >= 4
    for nq, nprobe in [(7, 3), (1, 1), (5, 20), (33, 7), (13, 5)]:
        q = _rand(nq, d, 80 + nq, dev)
        _assert_same(_search(index, q, k, k1, nprobe, c=x), _union_reference(x, index, q, k, k1, nprobe, True))
    # probing only empty and short lists: centroids aimed at the query's own direction
    cent = index[0]
    q = _rand(6, d, 90, dev)[:1].contiguous()
    c2 = cent.clone()
    c2[[1, 2, 13, 14]] = torch.nn.functional.normalize(q.repeat(4, 1), dim=1) * torch.tensor([[1.0], [0.999], [0.998], [0.997]], device=dev)
    index2 = (c2.contiguous(), *index[1:])
    for with_c in (True, False):
        kk1 = k1 if with_c else k
        s, i = _search(index2, q, k, kk1, 4, c=x if with_c else None)
        _assert_same((s, i), _union_reference(x, index2, q, k, kk1, 4, with_c))
        assert (i[0, 3:] == -1).all() and torch.isneginf(s[0, 3:]).all() and (i[0, :3] >= 0).all()   # lists 13 + 14: 1 + 2 items


# ------------------------------------------------------------------------------------------------ 5. batch independence
def test_rows_do_not_depend_on_the_batch_or_the_run(dev):
    from two_tower_amazon_recommender_amd.serving import Int8IVF
    xn, qn = clustered(30_000, 128, 100, 2000, seed=11)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    idx = Int8IVF(k=100, nlist=64, nprobe=8, iters=4).index(x)
    assert idx.k1(100) == 256
    s_all, i_all = idx(q)
    a, b = 1000, 1037
    s37, i37 = idx(q[a:b].contiguous())
    assert torch.equal(i37, i_all[a:b]) and torch.equal(_bits(s37), _bits(s_all[a:b]))
    for r in (a, a + 17, b - 1):
        s1, i1 = idx(q[r:r + 1].contiguous())
        assert torch.equal(i1[0], i_all[r]) and torch.equal(_bits(s1[0]), _bits(s_all[r]))
    s2, i2 = idx(q)
    assert torch.equal(i2, i_all) and torch.equal(_bits(s2), _bits(s_all))


# ------------------------------------------------------------------------------------------------ 6. many lists
def test_many_lists_keep_their_counters_in_the_workspace(dev):
    """nlist above the bucketing kernel's LDS counter capacity (8192): the counters live in the workspace."""
    n, d, nlist = 40_000, 32, 10_000
    x = _rand(n, d, 75, dev)
    assign = np.random.default_rng(76).integers(0, nlist, n)
    index = _index_from_assignment(x, assign, nlist, 77, dev)
    for nq, nprobe, k in [(1, 256, 10), (300, 40, 50)]:
        q = _rand(nq, d, 78 + nq, dev)
        k1 = _ops().default_k1(k, n)
        _assert_same(_search(index, q, k, k1, nprobe, c=x), _union_reference(x, index, q, k, k1, nprobe, True))


# ------------------------------------------------------------------------------------------------ 7. offsets past 2^31
def test_byte_offsets_past_two_to_the_31(dev):
    ops = _ops()
    n, d, tail, k = 8_400_000, 256, 3000, 20
    assert n * d > 2**31
    g = torch.Generator(device=dev).manual_seed(31)
    codes = torch.randint(-127, 128, (n, d), dtype=torch.int8, device=dev, generator=g)
    scales = torch.ones(n, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    off = torch.tensor([0, n - tail, n], device=dev)
    q = _rand(1, d, 32, dev)
    cent = torch.cat([-q, q]).contiguous()
    cent = torch.nn.functional.normalize(cent, dim=1).contiguous()
    s, i = ops.ivf_search_i8(q, cent, off, codes, scales, ids, k, 1, k1=k)
    rs, ri = ops.retrieval_topk_i8(q, codes[n - tail:], scales[n - tail:], k, k1=k)
    _assert_same((s, i), (rs, ri + (n - tail)))
    assert (i >= n - tail).all()


# ------------------------------------------------------------------------------------------------ 8. build and state
def test_build_matches_ivf_and_the_quantiser_and_state_round_trips(dev):
    from two_tower_amazon_recommender_amd.serving import IVF, Int8IVF
    ops = _ops()
    xn, qn = clustered(9000, 64, 40, 50, seed=3)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    a = IVF(k=10, nlist=32, nprobe=6, seed=4, iters=4).index(x)
    b = Int8IVF(k=10, nlist=32, nprobe=6, seed=4, iters=4).index(x)
    b2 = Int8IVF(k=10, nlist=32, nprobe=6, seed=4, iters=4)
    b2.QUANT_BATCH = 1000                                                    # several row batches
    b2.index(x)
    for name in ("centroids", "list_offsets", "list_ids"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    codes, scales = ops.quantize_rows_i8(x)
    order = b.list_ids.long()
    for idx in (b, b2):
        assert torch.equal(idx.list_codes, codes[order]) and torch.equal(_bits(idx.list_scales), _bits(scales[order]))
        assert idx.list_vectors is None
    assert torch.equal(b._candidates, x)                                     # the f32 corpus in original order
    r = Int8IVF(k=10, nlist=1, nprobe=1).load_state_dict(b.state_dict())
    r.nprobe = 6
    _assert_same(r(q), b(q))
    _assert_same(b(q), _union_reference(x, _arrays(b), q, 10, b.k1(10), 6, True))
    # keep_f32=False: no f32 rows, the stage-1 order
    lean = Int8IVF(k=10, nlist=32, nprobe=32, seed=4, iters=4, keep_f32=False).index(x)
    assert lean._candidates is None and lean.k1(10) == 10 and "candidates" not in lean.state_dict()
    _assert_same(lean(q), ops.retrieval_topk_i8(q, codes, scales, 10, k1=10))
    r = Int8IVF(k=10, nlist=1, nprobe=1, keep_f32=False).load_state_dict(lean.state_dict())
    r.nprobe = 32
    _assert_same(r(q), lean(q))
    # identifiers map, padding stays -1
    ident = torch.arange(9000, device=dev) * 7 + 1000
    named = Int8IVF(k=10, nlist=32, nprobe=6, seed=4, iters=4).index(x, identifiers=ident)
    s0, i0 = b(q)
    s1, i1 = named(q)
    assert torch.equal(i1, ident[i0]) and torch.equal(_bits(s1), _bits(s0))
    ex = torch.arange(9000, device=dev)[None].repeat(2, 1)[:, :8995].contiguous()      # at most 5 items left per query
    s2, i2 = named.query_with_exclusions(q[:2].contiguous(), ex, k=10)
    assert (i2[:, 5:] == -1).all() and torch.isneginf(s2[:, 5:]).all()
    assert (i2[i2 >= 0] >= 1000 + 7 * 8995).all() and torch.equal(i2 >= 0, torch.isfinite(s2))


# ------------------------------------------------------------------------------------------------ 9. recall
def test_recall_on_the_clustered_corpus(dev):
    from two_tower_amazon_recommender_amd.serving import IVF, Int8IVF
    xn, qn = clustered(**RECALL_CORPUS)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    i8 = Int8IVF(k=RECALL_K, nlist=RECALL_NLIST, nprobe=RECALL_NPROBE, rerank=4).index(x)
    f32 = IVF(k=RECALL_K, nlist=RECALL_NLIST, nprobe=RECALL_NPROBE).index(x)
    got = i8(q)[1].cpu().numpy()
    agree = recall_at_k(got, f32(q)[1].cpu().numpy())
    rec = recall_at_k(got, exact_topk_ids(qn, xn, RECALL_K))
    print(f"agreement with IVF {agree:.4f}, recall@{RECALL_K} {rec:.4f}")
    assert agree >= int8_check.RECALL_MIN, agree
    assert rec >= ivf_check.RECALL_MIN, rec


# ------------------------------------------------------------------------------------------------ 10. public surface
def test_custom_op_equals_ops(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    from two_tower_amazon_recommender_amd.serving import Int8IVF
    ops = _ops()
    xn, qn = clustered(3000, 64, 30, 19, seed=41)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    idx = Int8IVF(k=10, nlist=16, nprobe=4, iters=3).index(x)
    arrays = _arrays(idx)
    off = torch.tensor([0] + [3] * 19, device=dev)
    flat = torch.tensor([5, 1, 7], device=dev)
    torch.library.opcheck(torch.ops.twotower.ivf_search_i8, (q, *arrays, x, 10, 40, 4, None, None))
    torch.library.opcheck(torch.ops.twotower.ivf_search_i8, (q, *arrays, None, 10, 10, 4, off, flat))
    _assert_same(torch.ops.twotower.ivf_search_i8(q, *arrays, x, 10, 40, 4, None, None),
                 ops.ivf_search_i8(q, *arrays, 10, 4, c=x, k1=40))
    _assert_same(torch.ops.twotower.ivf_search_i8(q, *arrays, None, 10, 10, 4, off, flat),
                 ops.ivf_search_i8(q, *arrays, 10, 4, exclusions=(off, flat)))
    _assert_same(idx(q), ops.ivf_search_i8(q, *arrays, 10, 4, c=x))           # k1 defaults to default_k1(k, n, True)
    ws = idx._ws
    idx(q[:3].contiguous())
    assert idx._ws is ws                                                      # the workspace is kept across calls


def _env():
    env = dict(os.environ)
    root = str(pathlib.Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def test_index_from_trainer_and_recommend_cli(dev, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    from two_tower_amazon_recommender_amd.serving import Int8BruteForce, Int8IVF
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    n_users, n_items = 300, 500
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
    it = rng.integers(0, n_items, 3000)
    u[:n_users] = np.arange(n_users)
    data = tmp_path / "inter.parquet"
    pq.write_table(pa.table({"user_idx": u.astype(np.int64), "item_idx": it.astype(np.int64)}), data)
    out = tmp_path / "ivf_int8.parquet"
    r = run("two_tower_amazon_recommender_amd.recommend", "--checkpoint", str(ck), "--data", str(data), "--all-users",
            "--exclude-seen", "--k", "10", "--out", str(out), "--batch-users", "128", "--index", "ivf-int8", "--nlist", "20",
            "--nprobe", "20", "--rerank", "5", "--seed", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    t = pq.read_table(out)
    assert t.num_rows == n_users * 10
    seen = set(zip(u.tolist(), it.tolist()))
    assert not any((a, b) in seen for a, b in zip(t["user_idx"].to_pylist(), t["item_idx"].to_pylist()))
    # index_from_trainer: the user tower as the query model; full probe = Int8BruteForce of the same trainer
    sd = torch.load(ck, map_location=dev, weights_only=True)
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev)
    tr.load_state_dict(sd)
    users = torch.arange(n_users, device=dev)
    _assert_same(Int8IVF(k=10, nlist=20, nprobe=20, rerank=5).index_from_trainer(tr)(users),
                 Int8BruteForce(k=10, rerank=5).index_from_trainer(tr)(users))

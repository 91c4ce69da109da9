"""IVF approximate top-k (tt_ivf_search_f32, ops.ivf_search, torch.ops.twotower.ivf_search, serving.IVF, recommend --index
ivf) on the GPU.  The yardstick is tt_retrieval_topk_f32 itself: over the whole corpus at nprobe = nlist, and over the
union of the probed lists (gathered in ascending original id) otherwise - bit for bit, scores and ids."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from ivf_check import (RECALL_CORPUS, RECALL_K, RECALL_MIN, RECALL_NLIST, RECALL_NPROBE, clustered, exact_topk_ids,
                       recall_at_k, union_reference)

pytestmark = pytest.mark.gpu


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


def _rand(n, d, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n, d, generator=g) * 2.0 - 1.0).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _index_from_assignment(x, assign, nlist, seed, dev):
    """Index arrays for an arbitrary list assignment (the search does not need argmax placement): random unit centroids,
    items stable-sorted by list."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cent = torch.nn.functional.normalize(torch.randn(nlist, x.shape[1], generator=g), dim=1).to(dev).contiguous()
    a = torch.as_tensor(assign, dtype=torch.int64, device=dev)
    order = torch.argsort(a, stable=True)
    offsets = torch.cat([a.new_zeros(1), torch.cumsum(torch.bincount(a, minlength=nlist), 0)])
    return cent, offsets.contiguous(), x[order].contiguous(), order.to(torch.int32).contiguous()


def _search(index, q, k, nprobe, exclusions=None):
    cent, off, vec, ids = index
    return _ops().ivf_search(q, cent, off, vec, ids, k, nprobe, exclusions=exclusions)


def _union_reference(x, index, q, k, nprobe, excluded=None):
    """tt_retrieval_topk_f32 over each query's probed lists, gathered in ascending original id, ids mapped back."""
    ops = _ops()
    cent, off, _, ids = index
    probes = ops.retrieval_topk(q, cent, nprobe)[1].cpu().numpy()
    lid, offs = ids.cpu().numpy(), off.cpu().numpy()
    nq = q.shape[0]
    S = torch.full((nq, k), float("-inf"))
    I = torch.full((nq, k), -1, dtype=torch.int64)
    for r in range(nq):
        u = union_reference(lid, offs, probes[r])
        if len(u) == 0:
            continue
        kk = min(k, len(u))
        ex = None
        if excluded is not None and len(excluded[r]):
            e = np.asarray(excluded[r], dtype=np.int64)
            pos = np.searchsorted(u, e)
            hit = pos < len(u)
            hit[hit] = u[pos[hit]] == e[hit]
            pos = pos[hit]
            if len(pos):
                ex = (torch.tensor([0, len(pos)], device=q.device), torch.from_numpy(pos.astype(np.int64)).to(q.device))
        s, i = ops.retrieval_topk(q[r:r + 1].contiguous(), x[torch.from_numpy(u).to(x.device)].contiguous(), kk, exclusions=ex)
        s, i = s[0].cpu(), i[0].cpu().numpy()
        S[r, :kk] = s
        I[r, :kk] = torch.from_numpy(np.where(i >= 0, u[np.maximum(i, 0)], -1))
    return S, I


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


# ------------------------------------------------------------------------------------------------ 1. full probe = exact
@pytest.mark.parametrize("d,k,nq", [(32, 1, 1), (64, 10, 33), (128, 256, 1000), (256, 10, 33), (128, 1, 1000),
                                    (64, 256, 1), (32, 10, 1000), (256, 256, 33), (128, 10, 1), (256, 1, 1000)])
def test_full_probe_is_brute_force_bit_for_bit(dev, d, k, nq):
    from two_tower_amazon_recommender_amd.serving import IVF
    ops = _ops()
    x, q = _rand(6000, d, 100 + d, dev), _rand(nq, d, 200 + nq, dev)
    ivf = IVF(k=k, nlist=40, nprobe=40, iters=3).index(x)
    s, i = ivf(q)
    rs, ri = ops.retrieval_topk(q, x, k)
    assert torch.equal(i, ri) and torch.equal(_bits(s), _bits(rs))
    # with exclusions (original ids): empty, the whole exact top-k, and random ids with out-of-range values
    rng = np.random.default_rng(d + k + nq)
    ri_np = ri.cpu().numpy()
    ex = [[] if r % 3 == 0 else list(ri_np[r]) if r % 3 == 1 else [int(v) for v in rng.integers(0, 6000, 300)] + [-3, 6000, 2**40]
          for r in range(nq)]
    csr = _csr(ex, dev)
    s, i = ivf.query_with_exclusions(q, csr)
    rs, ri = ops.retrieval_topk(q, x, k, exclusions=csr)
    assert torch.equal(i, ri) and torch.equal(_bits(s), _bits(rs))


def test_full_probe_ties_across_lists_go_to_the_lower_id(dev):
    from two_tower_amazon_recommender_amd.serving import IVF
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(5)
    base = torch.randint(-4, 5, (37, 64), generator=g).float() / 8.0           # few distinct rows: many exact ties
    x = base[torch.randint(0, 37, (4000,), generator=g)].to(dev).contiguous()
    q = (torch.randint(-4, 5, (9, 64), generator=g).float() / 8.0).to(dev)
    # duplicates of one row sit in different lists: a random assignment, not k-means
    index = _index_from_assignment(x, torch.randint(0, 24, (4000,), generator=g), 24, 6, dev)
    ivf_s, ivf_i = _search(index, q, 50, 24)
    rs, ri = ops.retrieval_topk(q, x, 50)
    assert torch.equal(ivf_i, ri) and torch.equal(_bits(ivf_s), _bits(rs))
    s_np = rs.cpu().numpy()
    assert any(len(np.unique(row)) < 50 for row in s_np), "the corpus must plant ties"
    assert IVF(k=50, nlist=24, nprobe=24, iters=2).index(x)(q)[1].equal(ri)


# ------------------------------------------------------------------------------------------------ 2. partial probe
@pytest.mark.parametrize("d,k,nprobe,nq", [(64, 10, 1, 37), (64, 100, 3, 37), (128, 10, 7, 70), (32, 256, 5, 9),
                                           (256, 20, 12, 33)])
def test_partial_probe_is_brute_force_over_the_probed_lists(dev, d, k, nprobe, nq):
    from two_tower_amazon_recommender_amd.serving import IVF
    xn, qn = clustered(8000, d, 60, nq, seed=d + nprobe)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    ivf = IVF(k=k, nlist=50, nprobe=nprobe, iters=5).index(x)
    index = (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids)
    _assert_same(ivf(q), _union_reference(x, index, q, k, nprobe))
    rng = np.random.default_rng(nq)
    got_i = ivf(q)[1].cpu().numpy()
    ex = [list(got_i[r][: k // 2 + 1]) + [int(v) for v in rng.integers(0, 8000, 200)] if r % 2 else [] for r in range(nq)]
    _assert_same(ivf.query_with_exclusions(q, _csr(ex, dev)), _union_reference(x, index, q, k, nprobe, excluded=ex))


# ------------------------------------------------------------------------------------------------ 3. batch independence
def test_rows_do_not_depend_on_the_batch_or_the_run(dev):
    from two_tower_amazon_recommender_amd.serving import IVF
    xn, qn = clustered(30_000, 128, 100, 2000, seed=11)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    ivf = IVF(k=100, nlist=64, nprobe=8, iters=4).index(x)
    s_all, i_all = ivf(q)
    a, b = 1000, 1037
    s37, i37 = ivf(q[a:b].contiguous())
    assert torch.equal(i37, i_all[a:b]) and torch.equal(_bits(s37), _bits(s_all[a:b]))
    for r in (a, a + 17, b - 1):
        s1, i1 = ivf(q[r:r + 1].contiguous())
        assert torch.equal(i1[0], i_all[r]) and torch.equal(_bits(s1[0]), _bits(s_all[r]))
    s2, i2 = ivf(q)
    assert torch.equal(i2, i_all) and torch.equal(_bits(s2), _bits(s_all))


# ------------------------------------------------------------------------------------------------ 4. awkward lists
def test_awkward_lists(dev):
    """Empty lists, one list holding most of the corpus, lists shorter than k, probes with fewer than k candidates in
    total (-inf, -1 padding), and nq * nprobe not a multiple of 32."""
    n, d, nlist, k = 5000, 64, 20, 30
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
        _assert_same(_search(index, q, k, nprobe), _union_reference(x, index, q, k, nprobe))
    # probing only empty and short lists: centroids aimed at the queries' own direction
    cent, off, vec, ids = index
    q = _rand(6, d, 90, dev)
    c2 = cent.clone()
    c2[[1, 2, 13, 14]] = torch.nn.functional.normalize(q[:1].repeat(4, 1), dim=1) * torch.tensor([[1.0], [0.999], [0.998], [0.997]], device=dev)
    index2 = (c2.contiguous(), off, vec, ids)
    s, i = _search(index2, q[:1].contiguous(), k, 4)
    _assert_same((s, i), _union_reference(x, index2, q[:1].contiguous(), k, 4))
    assert (i[0, 3:] == -1).all() and torch.isneginf(s[0, 3:]).all() and (i[0, :3] >= 0).all()   # lists 13 + 14: 1 + 2 items


def test_many_lists_keep_their_counters_in_the_workspace(dev):
    """nlist above the bucketing kernel's LDS counter capacity (8192): the counters live in the workspace."""
    n, d, nlist = 40_000, 32, 10_000
    x = _rand(n, d, 75, dev)
    assign = np.random.default_rng(76).integers(0, nlist, n)
    index = _index_from_assignment(x, assign, nlist, 77, dev)
    for nq, nprobe, k in [(1, 256, 10), (300, 40, 50)]:
        q = _rand(nq, d, 78 + nq, dev)
        _assert_same(_search(index, q, k, nprobe), _union_reference(x, index, q, k, nprobe))


# ------------------------------------------------------------------------------------------------ 5. build invariants
def test_build_is_deterministic_and_places_every_item_in_its_best_list(dev):
    from two_tower_amazon_recommender_amd.serving import IVF
    xn, _ = clustered(50_000, 64, 300, 1, seed=3)
    x = torch.from_numpy(xn).to(dev)
    a = IVF(nlist=256, nprobe=8, seed=4).index(x)
    b = IVF(nlist=256, nprobe=8, seed=4).index(x)
    for name in ("centroids", "list_offsets", "list_vectors", "list_ids"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    off, ids = a.list_offsets.cpu().numpy(), a.list_ids.cpu().numpy().astype(np.int64)
    assert off[0] == 0 and off[-1] == 50_000 and (np.diff(off) >= 0).all()
    assert np.array_equal(np.sort(ids), np.arange(50_000))                    # every item exactly once
    for l in range(256):
        assert (np.diff(ids[off[l]:off[l + 1]]) > 0).all(), l                 # ascending within a list
    assert torch.equal(a.list_vectors, x[a.list_ids.long()])
    cent = a.centroids.double()
    assert torch.allclose(cent.norm(dim=1), torch.ones(256, dtype=torch.float64, device=dev), atol=1e-6)
    s = x.double() @ cent.T                                                   # f64 scores of every item against every list
    lists = torch.from_numpy(np.repeat(np.arange(256), np.diff(off))).to(dev)
    own = s[a.list_ids.long(), lists]
    best = s[a.list_ids.long()].amax(dim=1)
    tol = 1e-5 * (x.abs().double() @ cent.abs().T).amax(dim=1)[a.list_ids.long()]
    assert bool((own >= best - tol).all())                                    # argmax centroid, up to f32 ties
    c = IVF(nlist=256, nprobe=8, seed=5).index(x)
    assert not torch.equal(c.centroids, a.centroids)                          # the seed matters
    r = IVF(k=10, nlist=1, nprobe=1).load_state_dict(a.state_dict())
    r.nprobe = 8
    for name in ("centroids", "list_offsets", "list_vectors", "list_ids"):
        assert torch.equal(getattr(r, name), getattr(a, name)), name
    q = x[:50].contiguous()
    sa, ia = a(q)
    sr, ir = r(q)
    assert torch.equal(ia, ir) and torch.equal(_bits(sa), _bits(sr))


# ------------------------------------------------------------------------------------------------ 6. usefulness
def test_recall_on_the_clustered_corpus(dev):
    from two_tower_amazon_recommender_amd.serving import IVF
    xn, qn = clustered(**RECALL_CORPUS)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    ivf = IVF(k=RECALL_K, nlist=RECALL_NLIST, nprobe=RECALL_NPROBE).index(x)
    got = ivf(q)[1].cpu().numpy()
    rec = recall_at_k(got, exact_topk_ids(qn, xn, RECALL_K))
    assert rec >= RECALL_MIN, rec


# ------------------------------------------------------------------------------------------------ 7. public surface
def test_custom_op_and_serving_surface(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    from two_tower_amazon_recommender_amd.serving import IVF
    ops = _ops()
    xn, qn = clustered(3000, 64, 30, 19, seed=41)
    x, q = torch.from_numpy(xn).to(dev), torch.from_numpy(qn).to(dev)
    ivf = IVF(k=10, nlist=16, nprobe=4, iters=3).index(x)
    arrays = (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids)
    off = torch.tensor([0] + [3] * 19, device=dev)
    flat = torch.tensor([5, 1, 7], device=dev)
    torch.library.opcheck(torch.ops.twotower.ivf_search, (q, *arrays, 10, 4, None, None))
    torch.library.opcheck(torch.ops.twotower.ivf_search, (q, *arrays, 10, 4, off, flat))
    s, i = torch.ops.twotower.ivf_search(q, *arrays, 10, 4, None, None)
    s0, i0 = ops.ivf_search(q, *arrays, 10, 4)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    ident = torch.arange(3000, device=dev) * 7 + 1000
    ivf2 = IVF(k=10, nlist=16, nprobe=4, iters=3).index(x, identifiers=ident)
    bs, bi = ivf2(q)
    assert torch.equal(bi, ident[i0]) and torch.equal(bs, s0)
    pad = torch.full((19, 4), -1, dtype=torch.int64, device=dev)
    pad[:, 0] = i0[:, 0]
    es, ei = ivf.query_with_exclusions(q, pad)
    rs, ri = ops.ivf_search(q, *arrays, 10, 4, exclusions=pad)
    assert torch.equal(ei, ri) and torch.equal(es, rs) and not (ei == i0[:, :1]).any()
    ws = ivf._ws
    ivf(q[:3].contiguous())
    assert ivf._ws is ws                                                      # the workspace is kept across calls


def test_index_from_trainer_and_recommend_cli(dev, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    from two_tower_amazon_recommender_amd.serving import IVF, BruteForce
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
    outs = {}
    for name, extra in [("brute", []), ("ivf", ["--index", "ivf", "--nlist", "20", "--nprobe", "20"])]:
        outs[name] = tmp_path / f"{name}.parquet"
        r = run("two_tower_amazon_recommender_amd.recommend", "--checkpoint", str(ck), "--data", str(data), "--all-users",
                "--exclude-seen", "--k", "10", "--out", str(outs[name]), "--batch-users", "128", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
    tb, ti = pq.read_table(outs["brute"]), pq.read_table(outs["ivf"])
    assert tb.num_rows == n_users * 10 and tb.equals(ti)
    # index_from_trainer: the user tower as the query model; full probe = BruteForce, partial probe = its union reference
    sd = torch.load(ck, map_location=dev, weights_only=True)
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev)
    tr.load_state_dict(sd)
    users = torch.arange(n_users, device=dev)
    s0, i0 = BruteForce(k=10).index_from_trainer(tr)(users)
    s1, i1 = IVF(k=10, nlist=20, nprobe=20).index_from_trainer(tr)(users)
    assert torch.equal(i0, i1) and torch.equal(_bits(s0), _bits(s1))
    ivf = IVF(k=10, nlist=20, nprobe=4).index_from_trainer(tr)
    x = tr.item_corpus_embeddings(None).contiguous()
    qe = tr.user_embeddings(users).contiguous()
    _assert_same(ivf(users), _union_reference(x, (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids), qe, 10, 4))


def _env():
    import os
    import pathlib
    env = dict(os.environ)
    root = str(pathlib.Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


# ------------------------------------------------------------------------------------------------ 8. full size
def test_full_size_index(dev):
    """10 M x 128 clustered corpus made on the device, nlist 4096: nq = 16, k = 100, nprobe = 32, four queries checked
    against tt_retrieval_topk_f32 over the union of their probed lists."""
    from two_tower_amazon_recommender_amd.serving import IVF
    n, d, nq = 10_000_000, 128, 16
    g = torch.Generator(device=dev).manual_seed(2024)
    dirs = torch.nn.functional.normalize(torch.randn(20_000, d, device=dev, generator=g), dim=1)
    x = torch.empty(n, d, device=dev)
    for s in range(0, n, 1 << 21):
        e = min(n, s + (1 << 21))
        lab = torch.randint(0, 20_000, (e - s,), device=dev, generator=g)
        x[s:e] = dirs[lab] + 1.5 / d ** 0.5 * torch.randn(e - s, d, device=dev, generator=g)
    q = (x[torch.randint(0, n, (nq,), device=dev, generator=g)] + 0.75 / d ** 0.5 * torch.randn(nq, d, device=dev, generator=g)).contiguous()
    ivf = IVF(k=100, nlist=4096, nprobe=32).index(x)
    s, i = ivf(q)
    rows = torch.tensor([0, 5, 10, 15], device=dev)
    ref = _union_reference(x, (ivf.centroids, ivf.list_offsets, ivf.list_vectors, ivf.list_ids), q[rows].contiguous(), 100, 32)
    _assert_same((s[rows], i[rows]), ref)
    assert (i >= 0).all()

"""Exact top-k retrieval (tt_retrieval_topk_f32, ops.retrieval_topk, torch.ops.twotower.retrieval_topk, serving.BruteForce,
the recommend CLI) on the GPU against f64 scores."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from topk_check import check_topk

pytestmark = pytest.mark.gpu


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


def _rand(n, d, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n, d, generator=g) * 2.0 - 1.0).to(dev)


@pytest.mark.parametrize("nq,nc,d,k", [(1, 1000, 32, 1), (7, 4097, 64, 10), (33, 5000, 256, 256), (300, 70_001, 128, 100),
                                       (1024, 262_144, 128, 100), (5, 200, 128, 200), (40, 33, 64, 33)])
def test_topk_matches_f64(dev, nq, nc, d, k):
    q, c = _rand(nq, d, 1 + nq, dev), _rand(nc, d, 2 + nc, dev)
    s, i = _ops().retrieval_topk(q, c, k)
    torch.cuda.synchronize()
    assert s.shape == (nq, k) and i.shape == (nq, k) and i.dtype == torch.int64
    check_topk(q, c, k, s, i)


def _all_scores(q, c):
    """The kernel's own f32 score of every pair: top-k with k = the chunk's size over corpus chunks of <= 256 rows."""
    ops = _ops()
    out = torch.empty(q.shape[0], c.shape[0], device=q.device)
    for j in range(0, c.shape[0], 256):
        cc = c[j:j + 256].contiguous()
        s, i = ops.retrieval_topk(q, cc, cc.shape[0])
        out[:, j:j + cc.shape[0]].scatter_(1, i, s)
    return out


def test_ties_go_to_the_lower_index_including_the_cut(dev):
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(5)
    base = torch.randint(-4, 5, (37, 64), generator=g).float() / 8.0          # few distinct rows: many exact ties
    c = base[torch.randint(0, 37, (3000,), generator=g)].to(dev).contiguous()
    q = (torch.randint(-4, 5, (9, 64), generator=g).float() / 8.0).to(dev)
    k = 50
    s, i = ops.retrieval_topk(q, c, k)
    full = _all_scores(q, c).cpu().numpy()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    cut_tie = False
    for r in range(q.shape[0]):
        order = np.lexsort((np.arange(c.shape[0]), -full[r]))[:k]
        assert np.array_equal(i[r], order), r
        assert np.array_equal(s[r].view(np.uint32), full[r][order].view(np.uint32)), r
        cut_tie |= bool((full[r] == s[r, -1]).sum() > (s[r] == s[r, -1]).sum())
    assert cut_tie, "the corpus must put a tie group across the cut at position k"


def test_rows_do_not_depend_on_the_batch_or_the_run(dev):
    ops = _ops()
    q, c = _rand(8192, 128, 11, dev), _rand(20_000, 128, 12, dev)
    s_all, i_all = ops.retrieval_topk(q, c, 100)
    a, b = 4000, 4037
    s37, i37 = ops.retrieval_topk(q[a:b].contiguous(), c, 100)
    assert torch.equal(i37, i_all[a:b]) and torch.equal(s37.view(torch.int32), s_all[a:b].view(torch.int32))
    for r in (a, a + 17, b - 1):
        s1, i1 = ops.retrieval_topk(q[r:r + 1].contiguous(), c, 100)
        assert torch.equal(i1[0], i_all[r]) and torch.equal(s1[0].view(torch.int32), s_all[r].view(torch.int32))
    s2, i2 = ops.retrieval_topk(q, c, 100)
    assert torch.equal(i2, i_all) and torch.equal(s2.view(torch.int32), s_all.view(torch.int32))


def test_exclusions(dev):
    ops = _ops()
    nq, nc, d, k = 12, 9000, 64, 20
    q, c = _rand(nq, d, 21, dev), _rand(nc, d, 22, dev)
    rng = np.random.default_rng(3)
    s0, i0 = ops.retrieval_topk(q, c, k)
    i0 = i0.cpu().numpy()
    ex = []
    for r in range(nq):
        if r % 4 == 0:
            ex.append([])                                                           # empty segment
        elif r % 4 == 1:
            ex.append(list(i0[r]) + [int(x) for x in rng.integers(0, nc, 30)])       # the whole unexcluded top-k
        else:
            e = [int(x) for x in rng.integers(0, nc, 1000)]
            e += e[:50] + [-5, nc, nc + 100, 2**40]                                 # duplicates, out-of-range ids
            ex.append(e)
    off = np.zeros(nq + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in ex])
    flat = np.concatenate([np.asarray(e, dtype=np.int64) for e in ex])
    csr = (torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev))          # unsorted: ops sorts on the device
    s, i = ops.retrieval_topk(q, c, k, exclusions=csr)
    check_topk(q, c, k, s, i, excluded=ex)
    width = max(len(e) for e in ex)
    pad = np.full((nq, width), -1, dtype=np.int64)
    for r, e in enumerate(ex):
        pad[r, :len(e)] = e
    sp, ip = ops.retrieval_topk(q, c, k, exclusions=torch.from_numpy(pad).to(dev))
    assert torch.equal(ip, i) and torch.equal(sp.view(torch.int32), s.view(torch.int32))


def test_exclusions_leaving_fewer_than_k_pad_the_tail(dev):
    ops = _ops()
    nq, nc, d, k = 3, 600, 32, 10
    q, c = _rand(nq, d, 31, dev), _rand(nc, d, 32, dev)
    ex = [list(range(0, nc - (k - 3))), list(range(3, nc)), []]                     # k - 3 and 3 left; the third unrestricted
    off = torch.tensor([0, len(ex[0]), len(ex[0]) + len(ex[1]), len(ex[0]) + len(ex[1])], device=dev)
    flat = torch.tensor(ex[0] + ex[1], device=dev)
    s, i = ops.retrieval_topk(q, c, k, exclusions=(off, flat))
    check_topk(q, c, k, s, i, excluded=ex)
    assert (i[0, k - 3:] == -1).all() and torch.isneginf(s[0, k - 3:]).all() and (i[0, :k - 3] >= 0).all()
    assert (i[1, 3:] == -1).all() and (i[1, :3] >= 0).all() and (i[2] >= 0).all()


def test_full_size_corpus(dev):
    """cfg3's corpus (10 M items x 128) made on the device; 1024 queries, k = 100; 16 queries checked against f64."""
    ops = _ops()
    nc, d, nq, k = 10_000_000, 128, 1024, 100
    c = torch.empty(nc, d, device=dev)
    ops.fill_uniform_(c, 77, 1, -1.0, 2.0)
    q = torch.empty(nq, d, device=dev)
    ops.fill_uniform_(q, 77, 2, -1.0, 2.0)
    s, i = ops.retrieval_topk(q, c, k)
    rows = torch.arange(0, nq, nq // 16, device=dev)
    check_topk(q[rows], c, k, s[rows], i[rows], chunk=4)
    del c


def test_custom_op_and_brute_force(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    from two_tower_amazon_recommender_amd.serving import BruteForce
    ops = _ops()
    q, c = _rand(19, 64, 41, dev), _rand(3000, 64, 42, dev)
    off = torch.tensor([0] + [3] * 19, device=dev)
    flat = torch.tensor([5, 1, 7], device=dev)
    torch.library.opcheck(torch.ops.twotower.retrieval_topk, (q, c, 10, None, None))
    torch.library.opcheck(torch.ops.twotower.retrieval_topk, (q, c, 10, off, flat))
    s, i = torch.ops.twotower.retrieval_topk(q, c, 10, None, None)
    s0, i0 = ops.retrieval_topk(q, c, 10)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    ident = torch.arange(3000, device=dev) * 7 + 1000
    bf = BruteForce(k=10).index(c, identifiers=ident)
    bs, bi = bf(q)
    assert torch.equal(bi, ident[i0]) and torch.equal(bs, s0)
    pad = torch.full((19, 4), -1, dtype=torch.int64, device=dev)
    pad[:, 0] = i0[:, 0]
    pad[:, 1] = i0[:, 3]
    es, ei = BruteForce(k=12).index(c).query_with_exclusions(q, pad)
    rs, ri = ops.retrieval_topk(q, c, 12, exclusions=pad)
    assert torch.equal(ei, ri) and torch.equal(es, rs)
    assert not (ei == i0[:, :1]).any()
    assert BruteForce(query_model=lambda x: x * 1.0, k=3).index(c)(q)[1].shape == (19, 3)


def test_recommend_cli_end_to_end(dev, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    from two_tower_amazon_recommender_amd.serving import BruteForce
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
    u[:n_users] = np.arange(n_users)                     # every user has seen something
    data = tmp_path / "inter.parquet"
    pq.write_table(pa.table({"user_idx": u.astype(np.int64), "item_idx": it.astype(np.int64)}), data)
    out = tmp_path / "recs.parquet"
    r = run("two_tower_amazon_recommender_amd.recommend", "--checkpoint", str(ck), "--data", str(data), "--all-users",
            "--exclude-seen", "--k", "10", "--out", str(out), "--batch-users", "512")
    assert r.returncode == 0, r.stderr[-3000:]
    tbl = pq.read_table(out)
    cols = {n: tbl.column(n).to_numpy() for n in ("user_idx", "rank", "item_idx", "score")}
    assert len(cols["user_idx"]) == n_users * 10
    seen = set(zip(u.tolist(), it.tolist()))
    assert not any((a, b) in seen for a, b in zip(cols["user_idx"].tolist(), cols["item_idx"].tolist()))
    # the same answer in process from the loaded checkpoint
    sd = torch.load(ck, map_location=dev, weights_only=True)
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev)
    tr.load_state_dict(sd)
    order = np.argsort(u, kind="stable")
    starts = np.searchsorted(u[order], np.arange(n_users + 1))
    off = torch.from_numpy(starts.astype(np.int64)).to(dev)
    flat = torch.from_numpy(it[order].astype(np.int64)).to(dev)
    s, i = BruteForce(k=10).index_from_trainer(tr).query_with_exclusions(torch.arange(n_users, device=dev), (off, flat))
    assert np.array_equal(cols["item_idx"].reshape(n_users, 10), i.cpu().numpy())
    assert np.array_equal(cols["score"].reshape(n_users, 10), s.cpu().numpy())
    assert np.array_equal(cols["rank"].reshape(n_users, 10), np.tile(np.arange(10), (n_users, 1)))


def _env():
    import os
    import pathlib
    env = dict(os.environ)
    root = str(pathlib.Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env

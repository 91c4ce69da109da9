"""Int8 top-k (tt_quantize_rows_i8, tt_retrieval_topk_i8_f32, ops, torch.ops.twotower, serving.Int8BruteForce, recommend
--index int8) on the GPU.  Stage 1 is integer arithmetic and one f32 multiply, so the NumPy restatement (int8_check.py) is
bit-exact; the re-rank's yardstick is tt_retrieval_topk_f32 itself over each query's candidate rows."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

from int8_check import (RECALL_CASES, RECALL_MIN, RECALL_SHAPE, exact_topk_ids, np_keys, np_quantize, np_stage1, recall_at_k,
                        recall_corpus)

pytestmark = pytest.mark.gpu


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, ref_s, ref_i):
    s, i = got
    assert np.array_equal(i.cpu().numpy(), np.asarray(ref_i))
    assert np.array_equal(s.cpu().numpy().view(np.int32), np.asarray(ref_s, dtype=np.float32).view(np.int32))


def _csr(ex, dev):
    off = np.zeros(len(ex) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in ex])
    flat = np.concatenate([np.asarray(e, dtype=np.int64) for e in ex]) if off[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev)


def _queries_with_codes(qc, rng):
    """f32 query rows whose quantisation is exactly the integer rows qc (each must hold a +-127): q = qc * scale with a
    power-of-two scale per row, so amax / 127 is that scale exactly and q / scale = qc."""
    scale = (2.0 ** rng.integers(-6, 3, qc.shape[0])).astype(np.float32)
    return (qc.astype(np.float32) * scale[:, None]).astype(np.float32), scale


def _int_problem(nq, nc, d, seed):
    """Codes / scales / query codes over the full -127..127 range, built in NumPy; every query row holds a 127."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(-127, 128, (nc, d)).astype(np.int8)
    scales = (rng.random(nc, dtype=np.float32) * 0.02 + 0.001).astype(np.float32)
    qc = rng.integers(-127, 128, (nq, d)).astype(np.int8)
    qc[np.arange(nq), rng.integers(0, d, nq)] = 127
    return codes, scales, qc, rng


# ------------------------------------------------------------------------------------------------ 1. quantiser
@pytest.mark.parametrize("n,d", [(1, 32), (33, 64), (1000, 128), (257, 256)])
def test_quantiser_is_bit_exact(dev, n, d):
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, d)) * rng.random((n, 1)) * 3).astype(np.float32)
    x[n // 2] = 0.0                                                           # an all-zero row
    r = n - 1 if n > 1 else None
    if r is not None:                                                         # amax exactly 127: scale 1, halves to even
        x[r] = 0.0
        x[r, :8] = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 127.0, 3.5]
    codes, scales = _ops().quantize_rows_i8(torch.from_numpy(x).to(dev))
    rc, rs = np_quantize(x)
    assert codes.dtype == torch.int8 and scales.dtype == torch.float32
    assert np.array_equal(codes.cpu().numpy(), rc)
    assert np.array_equal(scales.cpu().numpy().view(np.int32), rs.view(np.int32))
    assert scales[n // 2].item() == 0.0 and not codes[n // 2].any()
    if r is not None:
        assert scales[r].item() == 1.0 and codes[r, :8].tolist() == [0, 0, 2, -2, 2, -2, 127, 4]


# ------------------------------------------------------------------------------------------------ 2. stage 1 alone
@pytest.mark.parametrize("nq,nc,d,k", [(1, 1000, 32, 1), (7, 4097, 64, 10), (33, 5000, 256, 256), (300, 70001, 128, 100),
                                       (40, 33, 64, 33), (5, 200, 128, 200)])
def test_stage1_equals_the_restatement_bit_for_bit(dev, nq, nc, d, k):
    codes, scales, qc, rng = _int_problem(nq, nc, d, 1000 + nc)
    if d == 256:                                                              # the largest iscore: 256 * 127^2
        codes[nc // 3] = 127
        qc[nq // 2] = 127
    q, qscale = _queries_with_codes(qc, rng)
    got_qc, got_qs = np_quantize(q)
    assert np.array_equal(got_qc, qc) and np.array_equal(got_qs, qscale)      # the kernel quantises q to exactly qc
    S, I = np_stage1(qc, qscale, codes, scales, k)
    if d == 256:
        assert np_keys(qc[nq // 2:nq // 2 + 1], codes[nc // 3:nc // 3 + 1], np.ones(1, np.float32))[0, 0] == 256 * 127 * 127
    got = _ops().retrieval_topk_i8(torch.from_numpy(q).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), k)
    _same(got, S, I)


def test_asymmetric_integer_data_pairs_a_and_b_consistently(dev):
    """One-hot queries against rows that differ in a single position: any k <-> element mismatch between the two MFMA
    operands changes the winner."""
    d, nc = 128, 256
    codes = np.zeros((nc, d), dtype=np.int8)
    codes[np.arange(nc), np.arange(nc) % d] = np.where(np.arange(nc) < d, 100, -100)   # row j: +-100 at position j % d
    codes[:, 0] += 1
    qc = np.zeros((d, d), dtype=np.int8)
    qc[np.arange(d), np.arange(d)] = 127                                      # query i: one-hot at position i
    q = qc.astype(np.float32)
    scales = np.ones(nc, dtype=np.float32)
    S, I = np_stage1(qc, np.ones(d, np.float32), codes, scales, 2)
    assert I[5, 0] == 5 and I[77, 0] == 77
    got = _ops().retrieval_topk_i8(torch.from_numpy(q).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), 2)
    _same(got, S, I)


# ------------------------------------------------------------------------------------------------ 3. ties
def test_ties_go_to_the_lower_index_also_at_the_cut(dev):
    rng = np.random.default_rng(5)
    base = rng.integers(-127, 128, (37, 64)).astype(np.int8)
    codes = base[np.arange(3000) % 37]                                        # 37 distinct rows, each ~81 times
    scales = np.full(3000, 0.25, dtype=np.float32)
    qc = rng.integers(-127, 128, (9, 64)).astype(np.int8)
    qc[:, 0] = 127
    q, qscale = _queries_with_codes(qc, rng)
    S, I = np_stage1(qc, qscale, codes, scales, 50)
    keys = np_keys(qc, codes, scales)
    for r in range(9):
        cut = keys[r, I[r, -1]]
        assert (keys[r] == cut).sum() > (S[r] == cut * qscale[r]).sum() >= 1  # a tie group straddles the cut
        order = list(zip((-S[r]).tolist(), I[r].tolist()))
        assert order == sorted(order)                                         # lexicographic (key desc, index asc)
    got = _ops().retrieval_topk_i8(torch.from_numpy(q).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev), 50)
    _same(got, S, I)


# ------------------------------------------------------------------------------------------------ 4. re-rank
def _float_problem(nq, nc, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((nc, d)).astype(np.float32)


def test_rerank_of_the_whole_corpus_is_exact_topk_bit_for_bit(dev):
    ops = _ops()
    qn, xn = _float_problem(9, 200, 64, 21)
    q, x = torch.from_numpy(qn).to(dev), torch.from_numpy(xn).to(dev)
    codes, scales = ops.quantize_rows_i8(x)
    s, i = ops.retrieval_topk_i8(q, codes, scales, 50, c=x, k1=200)
    rs, ri = ops.retrieval_topk(q, x, 50)
    assert torch.equal(i, ri) and torch.equal(_bits(s), _bits(rs))


@pytest.mark.parametrize("nq,nc,d,k,k1", [(7, 4097, 64, 10, 40), (300, 70001, 128, 100, 256), (33, 5000, 256, 20, 256),
                                          (5, 3000, 32, 10, 32)])
def test_rerank_equals_exact_topk_over_the_candidate_rows(dev, nq, nc, d, k, k1):
    ops = _ops()
    qn, xn = _float_problem(nq, nc, d, 31 + nc)
    q, x = torch.from_numpy(qn).to(dev), torch.from_numpy(xn).to(dev)
    codes, scales = ops.quantize_rows_i8(x)
    cn, sn = np_quantize(xn)
    assert np.array_equal(codes.cpu().numpy(), cn) and np.array_equal(scales.cpu().numpy(), sn)
    qc, qs = np_quantize(qn)
    _, cand = np_stage1(qc, qs, cn, sn, k1)
    s, i = ops.retrieval_topk_i8(q, codes, scales, k, c=x, k1=k1)
    s, i = s.cpu(), i.cpu()
    ws = torch.empty(max(ops.retrieval_topk_workspace_bytes(1, k1, d, k), 1), dtype=torch.uint8, device=dev)
    for r in range(nq):
        rows = np.sort(cand[r])
        rs, ri = ops.retrieval_topk(q[r:r + 1].contiguous(), x[torch.from_numpy(rows).to(dev)].contiguous(), k, workspace=ws)
        assert np.array_equal(i[r].numpy(), rows[ri[0].cpu().numpy()]), r
        assert torch.equal(_bits(s[r]), _bits(rs[0].cpu())), r


# ------------------------------------------------------------------------------------------------ 5. batch independence
def test_rows_do_not_depend_on_the_batch_or_the_run(dev):
    ops = _ops()
    qn, xn = _float_problem(200, 20_000, 128, 41)
    q, x = torch.from_numpy(qn).to(dev), torch.from_numpy(xn).to(dev)
    codes, scales = ops.quantize_rows_i8(x)
    for kw in (dict(c=x, k1=40), dict()):
        s_all, i_all = ops.retrieval_topk_i8(q, codes, scales, 10, **kw)
        a, b = 100, 137
        s37, i37 = ops.retrieval_topk_i8(q[a:b].contiguous(), codes, scales, 10, **kw)
        assert torch.equal(i37, i_all[a:b]) and torch.equal(_bits(s37), _bits(s_all[a:b]))
        for r in (0, a + 17, 199):
            s1, i1 = ops.retrieval_topk_i8(q[r:r + 1].contiguous(), codes, scales, 10, **kw)
            assert torch.equal(i1[0], i_all[r]) and torch.equal(_bits(s1[0]), _bits(s_all[r]))
        s2, i2 = ops.retrieval_topk_i8(q, codes, scales, 10, **kw)
        assert torch.equal(i2, i_all) and torch.equal(_bits(s2), _bits(s_all))


# ------------------------------------------------------------------------------------------------ 6. exclusions
def test_exclusions_free_their_candidate_slots(dev):
    ops = _ops()
    nq, nc, d, k = 12, 3000, 64, 10
    codes, scales, qc, rng = _int_problem(nq, nc, d, 51)
    q, qscale = _queries_with_codes(qc, rng)
    _, I0 = np_stage1(qc, qscale, codes, scales, k)
    ex = []
    for r in range(nq):
        if r % 4 == 0:
            ex.append([])                                                     # empty segment
        elif r % 4 == 1:
            ex.append(sorted(I0[r].tolist()))                                 # the whole unexcluded stage-1 set
        elif r % 4 == 2:
            e = I0[r, :5].tolist()
            ex.append(sorted(e + e + [-7, nc, nc + 5, 2**40]))                # duplicates and out-of-range ids
        else:
            ex.append(sorted(set(range(nc)) - set(I0[r, 2:6].tolist()) - {7}))    # leaves 4 or 5 candidates: fewer than k
    S, I = np_stage1(qc, qscale, codes, scales, k, excluded=ex)
    tq, tc, ts = torch.from_numpy(q).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev)
    got = ops.retrieval_topk_i8(tq, tc, ts, k, exclusions=_csr(ex, dev))
    _same(got, S, I)
    gi = got[1].cpu().numpy()
    for r in range(nq):
        assert not set(gi[r][gi[r] >= 0].tolist()) & set(ex[r]), r
    assert np.array_equal(gi[1], np_stage1(qc[1:2], qscale[1:2], codes, scales, 2 * k)[1][0, k:])   # the next-best keys
    assert (gi[3, 5:] == -1).all() and torch.isneginf(got[0][3, 5:]).all() and (gi[3, :4] >= 0).all()
    # with the re-rank: the candidates are the unexcluded stage-1 set, re-ordered by the exact score
    xf = (codes.astype(np.float32) * scales[:, None]).astype(np.float32)
    x = torch.from_numpy(xf).to(dev)
    s2, i2 = ops.retrieval_topk_i8(tq, tc, ts, 6, c=x, k1=k, exclusions=_csr(ex, dev))
    for r in range(nq):
        rows = np.sort(I[r][I[r] >= 0])
        kk = min(6, len(rows))                                                # 4 or 5 at r % 4 == 3: a padded tail
        rs, ri = ops.retrieval_topk(tq[r:r + 1].contiguous(), x[torch.from_numpy(rows).to(dev)].contiguous(), kk)
        assert np.array_equal(i2[r, :kk].cpu().numpy(), rows[ri[0].cpu().numpy()]), r
        assert torch.equal(_bits(s2[r, :kk]), _bits(rs[0])), r
        assert (i2[r, kk:] == -1).all() and torch.isneginf(s2[r, kk:]).all()


# ------------------------------------------------------------------------------------------------ 7. offsets past 2^31
def test_code_offsets_past_two_to_the_31_bytes(dev):
    nc, d, nq, k = 9_000_000, 256, 4, 8
    g = torch.Generator(device=dev).manual_seed(7)
    codes = torch.randint(-16, 17, (nc, d), device=dev, generator=g, dtype=torch.int8)
    scales = torch.ones(nc, device=dev)
    rng = np.random.default_rng(8)
    qn = rng.standard_normal((nq, d)).astype(np.float32)
    qc, qs = np_quantize(qn)
    rows = np.zeros((nq, k), dtype=np.int64)
    for r in range(nq):
        for j in range(k):                                                    # half in the first 1,000 rows, half in the last
            rows[r, j] = 10 + 8 * r + j if j % 2 == 0 else nc - 1 - (8 * r + j)
    planted = (127 * np.sign(qc)).astype(np.int8)
    flat = torch.from_numpy(rows.reshape(-1)).to(dev)
    codes[flat] = torch.from_numpy(np.repeat(planted, k, axis=0)).to(dev)
    scales[flat] = torch.from_numpy(np.tile(2.0 - np.arange(k, dtype=np.float32) / 8, nq)).to(dev)   # fixes the order
    # the planted rows of query r beat everything else for it: 127 sum|qc| * 1.125 against 16 sum|qc| (ordinary rows) and
    # the other queries' planted rows (checked here on the 32 planted rows)
    pc, ps = codes[flat].cpu().numpy(), scales[flat].cpu().numpy()
    S, I = np_stage1(qc, qs, pc, ps, k)
    assert np.array_equal(I, np.arange(nq * k).reshape(nq, k))
    assert (127 * 1.125 * np.abs(qc.astype(np.int64)).sum(1) > 16 * np.abs(qc.astype(np.int64)).sum(1)).all()
    got = _ops().retrieval_topk_i8(torch.from_numpy(qn).to(dev), codes, scales, k)
    _same(got, S, rows)


# ------------------------------------------------------------------------------------------------ 8. recall
@functools.lru_cache(maxsize=None)
def _recall_problem(kind):
    q, x = recall_corpus(kind, **RECALL_SHAPE)
    return q, x, {k: exact_topk_ids(q, x, k) for k, _ in RECALL_CASES}


@pytest.mark.parametrize("kind", ["uniform", "normal"])
def test_recall_against_the_exact_answer(dev, kind):
    ops = _ops()
    qn, xn, exact = _recall_problem(kind)
    q, x = torch.from_numpy(qn).to(dev), torch.from_numpy(xn).to(dev)
    codes, scales = ops.quantize_rows_i8(x)
    for k, k1 in RECALL_CASES:
        got = ops.retrieval_topk_i8(q, codes, scales, k, c=x, k1=k1)[1].cpu().numpy()
        rec = recall_at_k(got, exact[k])
        print(f"recall@{k} (k1 {k1}, {kind}): {rec:.4f}")
        assert rec >= RECALL_MIN, (kind, k, k1, rec)


# ------------------------------------------------------------------------------------------------ 9. public surface
def test_custom_ops_and_serving_surface(dev):
    from two_tower_amazon_recommender_amd import torch_ops  # noqa: F401
    from two_tower_amazon_recommender_amd.serving import Int8BruteForce
    ops = _ops()
    qn, xn = _float_problem(19, 3000, 64, 61)
    q, x = torch.from_numpy(qn).to(dev), torch.from_numpy(xn).to(dev)
    codes, scales = ops.quantize_rows_i8(x)
    off = torch.tensor([0] + [3] * 19, device=dev)
    flat = torch.tensor([5, 1, 7], device=dev)
    torch.library.opcheck(torch.ops.twotower.quantize_rows_i8, (x,))
    torch.library.opcheck(torch.ops.twotower.retrieval_topk_i8, (q, codes, scales, x, 10, 40, None, None))
    torch.library.opcheck(torch.ops.twotower.retrieval_topk_i8, (q, codes, scales, None, 10, 10, off, flat))
    c2, s2 = torch.ops.twotower.quantize_rows_i8(x)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    s0, i0 = ops.retrieval_topk_i8(q, codes, scales, 10, c=x)                 # default k1 = 40
    s, i = torch.ops.twotower.retrieval_topk_i8(q, codes, scales, x, 10, 40, None, None)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    with pytest.raises(ValueError, match="k1"):
        ops.retrieval_topk_i8(q, codes, scales, 10, k1=40)                    # no c: k1 must equal k
    with pytest.raises(ValueError, match="k1"):
        ops.retrieval_topk_i8(q, codes, scales, 10, c=x, k1=5)

    ident = torch.arange(3000, device=dev) * 7 + 1000
    bf = Int8BruteForce(k=10).index(x, identifiers=ident)
    bs, bi = bf(q)
    assert torch.equal(bi, ident[i0]) and torch.equal(bs, s0)
    bf = Int8BruteForce(k=10).index(x)
    pad = torch.full((19, 4), -1, dtype=torch.int64, device=dev)
    pad[:, 0] = i0[:, 0]
    es, ei = bf.query_with_exclusions(q, pad)
    rs, ri = ops.retrieval_topk_i8(q, codes, scales, 10, c=x, k1=40, exclusions=pad)
    assert torch.equal(ei, ri) and torch.equal(es, rs) and not (ei == i0[:, :1]).any()
    ws = bf._ws
    bf(q[:3].contiguous())
    assert bf._ws is ws                                                       # the workspace is kept across calls
    s8, i8 = Int8BruteForce(k=10, rerank=8).index(x)(q)
    r8 = ops.retrieval_topk_i8(q, codes, scales, 10, c=x, k1=80)
    assert torch.equal(i8, r8[1]) and torch.equal(s8, r8[0])
    # state_dict round trips, with and without the f32 rows
    again = Int8BruteForce(k=10).load_state_dict(bf.state_dict())
    sa, ia = again(q)
    assert torch.equal(ia, i0) and torch.equal(_bits(sa), _bits(s0))
    lean = Int8BruteForce(k=10, keep_f32=False).index(x)
    assert lean._candidates is None and "candidates" not in lean.state_dict()
    sl, il = lean(q)
    rl = ops.retrieval_topk_i8(q, codes, scales, 10)
    assert torch.equal(il, rl[1]) and torch.equal(_bits(sl), _bits(rl[0]))
    lean2 = Int8BruteForce(k=10, keep_f32=False).load_state_dict(lean.state_dict())
    assert torch.equal(lean2(q)[1], il)


def _env():
    import os
    import pathlib
    env = dict(os.environ)
    root = str(pathlib.Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def test_recommend_cli_with_the_int8_index(dev, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    from two_tower_amazon_recommender_amd import recommend
    from two_tower_amazon_recommender_amd.serving import Int8BruteForce
    from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, TwoTowerTrainer
    n_users, n_items = 300, 200
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
    for name, extra in [("brute", []), ("int8", ["--index", "int8"]), ("int8_all", ["--index", "int8", "--rerank", "100"])]:
        outs[name] = tmp_path / f"{name}.parquet"
        r = run("two_tower_amazon_recommender_amd.recommend", "--checkpoint", str(ck), "--data", str(data), "--all-users",
                "--exclude-seen", "--k", "10", "--out", str(outs[name]), "--batch-users", "128", *extra)
        assert r.returncode == 0, r.stderr[-3000:]
    tb, t8, tall = (pq.read_table(outs[n]) for n in ("brute", "int8", "int8_all"))
    assert tb.num_rows == n_users * 10 and tall.equals(tb)                    # k1 = every item: the re-rank is exact top-k
    # the default --rerank equals the in-process index, exclusions included
    sd = torch.load(ck, map_location=dev, weights_only=True)
    tr = TwoTowerTrainer(TwoTowerConfig(**sd["config"]), dev)
    tr.load_state_dict(sd)
    bf = Int8BruteForce(k=10, rerank=4).index_from_trainer(tr)
    users = np.arange(n_users, dtype=np.int64)
    off, idx = recommend.batch_exclusions(*recommend.seen_csr(u, it, n_users), users)
    s, i = bf.query_with_exclusions(torch.from_numpy(users).to(dev), (torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev)))
    assert t8.num_rows == n_users * 10
    assert np.array_equal(t8.column("item_idx").to_numpy().reshape(n_users, 10), i.cpu().numpy())
    assert np.array_equal(t8.column("score").to_numpy().astype(np.float32).reshape(n_users, 10).view(np.int32),
                          s.cpu().numpy().view(np.int32))

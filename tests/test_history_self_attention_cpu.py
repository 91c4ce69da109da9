"""The multi-head self-attention encoder of the user history without a GPU: the restatements of tests/selfattn_check.py against
f64 torch autograd, the float32 restatements against the bars on every problem the GPU sweep uses, the dense layout with the new
blocks, config / YAML / CLI parsing, the refusals, the C entries' argument validation (before any launch), the ctypes signatures
against the header, the custom ops' registration, and the new translation unit's register report (no kernel uses scratch)."""
import ctypes as C
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import selfattn_check as sc
from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, dense_layout

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------ 1. the restatements
@pytest.mark.parametrize("heads,L", [(1, 7), (2, 7), (4, 1), (8, 3)])
def test_closed_form_backward_equals_f64_autograd(heads, L):
    """37 bags, dim 8, with padding, leave-one-out bags, an emptied bag, a single-slot bag, a duplicate token inside a bag (one
    of the two the newest slot) and indirect rows: every result of the closed form within 1e-10 of torch autograd (f64) of the
    forward restatement; skipped slots get zero rows."""
    rng = np.random.default_rng([1, heads, L])
    d, n = 8, 37
    tok, bag_rows, exclude = sc.problem(rng, 50, n, L, 97, True)
    tok[12, 0] = tok[12, L - 1] = 40                                                 # a duplicate, one of them the newest slot
    bag_rows[12], exclude[12] = 12, 96
    tok[13] = -1
    tok[13, L // 2] = 41                                                              # a single kept slot
    bag_rows[13], exclude[13] = 13, 96
    table = rng.standard_normal((97, d)).astype(np.float32)
    Wqk, Wvo, p = rng.standard_normal((d, heads * d)), rng.standard_normal((heads * d, d)) * 0.5, rng.standard_normal((heads, L))
    dy = rng.standard_normal((n, d))
    base = (rng.standard_normal((20, d)).astype(np.float32), rng.integers(0, 20, n))
    out, ids, flag, saved = sc.forward(table, tok, Wqk, Wvo, p, bag_rows, exclude, base)
    got = sc.backward(saved, dy, Wqk, Wvo)
    valid = saved["valid"]
    assert not valid[1].any() and (~valid).any() and saved["newest"][1] == -1 and flag == 0
    if L > 1:
        assert valid[12, 0] and valid[12, L - 1] and saved["newest"][12] == L - 1
    assert np.array_equal(out[1], base[0][base[1][1]].astype(np.float64))           # the emptied bag: the base row itself
    one = valid.sum(1) == 1
    assert one.any() and np.array_equal(saved["w"][one].sum(2), np.ones((one.sum(), heads)))
    assert np.abs(got["de"][one]).max() < 1e-13            # w = 1 and P = x: t = G but for the two sums' own rounding
    tt, Wq, Wv, pt = (torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True) for x in (table, Wqk, Wvo, p))
    o = sc.forward_torch(tt, torch.from_numpy(ids.reshape(n, L)), Wq, Wv, pt, torch.from_numpy(base[0].astype(np.float64))[base[1]])
    assert np.abs(o.detach().numpy() - out).max() < 1e-10
    (o * torch.from_numpy(dy)).sum().backward()
    sg = got["slot_grads"]
    dense = np.zeros((97, d))
    np.add.at(dense, ids[ids >= 0], sg[ids >= 0])
    assert np.abs(dense - tt.grad.numpy()).max() < 1e-10
    assert not sg[ids < 0].any()
    for k, want in (("dWqk", Wq.grad), ("dWvo", Wv.grad), ("dp", pt.grad)):
        assert np.abs(got[k] - want.numpy()).max() < 1e-10, k
    dp_bag, dT_bag = sc.per_bag_terms(saved, dy, Wvo)
    assert np.abs(dp_bag.sum(0) - got["dp"]).max() < 1e-12 and np.abs(dT_bag - got["dT"]).max() < 1e-12


def restatement_errors(dim, nb, L, heads, scale):
    """{name: (float32 result, f64 reference, zero_scale or None)} of one problem of the GPU sweep."""
    q = sc.forward_problem(dim, nb, L, heads, scale)
    args = (q["table"], q["tokens"], q["Wqk"], q["Wvo"], q["p"], q["bag_rows"], q["exclude"], q["base"])
    out64, ids, flag, s64 = sc.forward(*args)
    out32, ids32, flag32, s32 = sc.forward_f32(*args)
    want = sc.backward(s64, q["dy"], q["Wqk"], q["Wvo"])
    got = sc.backward_f32(s32, q["dy"], q["Wqk"], q["Wvo"])
    zs = sc.uncancelled_scales(s64, q["dy"], q["Wqk"], q["Wvo"])
    assert np.array_equal(ids, ids32) and flag == flag32 == 0 and out32.dtype == np.float32
    res = dict(out=(out32, out64, None), weights=(s32["w"], s64["w"], None), P=(s32["P"], s64["P"], None))
    for k in ("slot_grads", "dWqk", "dWvo", "dp", "dT"):
        res[k] = (got[k], want[k], zs.get(k))
    return res


@pytest.mark.parametrize("scale", sc.SCALES, ids=["soft", "sharp"])
@pytest.mark.parametrize("dim", sc.DIMS)
def test_float32_restatements_stay_within_the_bars_on_every_gpu_problem(dim, scale):
    """The bars the GPU tests hold the kernels to (1e-4 in the 2-norm and in max-abs / max|ref|, against f64) are reachable by
    the formulas themselves in float32 on every problem of the GPU sweep, at both logit scales - so no scale is dropped."""
    worst = {}
    for nb in sc.BAGS:
        for L in sc.LS:
            for heads in sc.HEADS:
                for k, (g, w, z) in restatement_errors(dim, nb, L, heads, scale).items():
                    worst[k] = max(worst.get(k, 0.0), max(sc.within_bars(g, w, (k, dim, nb, L, heads, scale), z)))
    print(dim, scale, worst)


def test_the_sharp_scale_spreads_the_logits_and_the_special_bags_are_in_place():
    q = sc.forward_problem(128, 300, 64, 4, 4.0)
    valid, tok, newest, flag = sc.resolve(q["table"], q["tokens"], q["bag_rows"], q["exclude"])
    assert valid[8].all() and valid[9, :8].all() and not valid[9, 8:].any() and valid[10, -8:].all() and not valid[10, :-8].any()
    assert valid[11].sum() == 1 and newest[11] == 32 and not valid[1].any() and not valid[7].any() and newest[1] == newest[7] == -1
    assert tok[12, 0] == tok[12, 63] and newest[12] == 63 and q["base"][1][3] == -1 and flag == 0
    _, _, _, s = sc.forward(q["table"], q["tokens"], q["Wqk"], q["Wvo"], q["p"], q["bag_rows"], q["exclude"], q["base"])
    e = np.einsum("bld,bhd->bhl", s["x"], s["T"]) / np.sqrt(128.0)
    e = e[np.broadcast_to(valid[:, None, :], e.shape)]
    assert 3.0 < e.std() < 5.0 and np.abs(e).max() > 10.0                            # roughly +-10
    assert s["w"].max(2)[valid.sum(1) > 8].mean() > 0.5                               # a few slots carry a head


# ------------------------------------------------------------------------------------------ 2. config and layout
BASE = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[64, 32])
SA = dict(user_history_len=5, history_pooling="self_attention", history_heads=2)


def test_config_validation_yaml_and_cli(tmp_path):
    TwoTowerConfig(**BASE, **SA).validate()
    for h in (1, 2, 4, 8):
        TwoTowerConfig(**BASE, user_history_len=64, history_pooling="self_attention", history_heads=h).validate()
    cfg = TwoTowerConfig(**BASE, **SA)
    assert cfg.history_self_attention and not cfg.history_attention and not cfg.history_gru
    assert TwoTowerConfig(**BASE).history_heads == 1
    assert not TwoTowerConfig(**BASE, history_pooling="self_attention").history_self_attention      # (no feature: not used)
    TwoTowerConfig(n_users=10, n_items=10, embedding_dim=36, tower_dims=[64, 32], history_pooling="self_attention").validate()
    for dim in (36, 288, 16):
        with pytest.raises(ValueError, match="multiple of 32"):
            TwoTowerConfig(n_users=10, n_items=10, embedding_dim=dim, tower_dims=[64, 32], **SA).validate()
    for h in (0, 3, 16, True, 2.5):
        with pytest.raises(ValueError, match="history_heads"):
            TwoTowerConfig(**BASE, user_history_len=5, history_pooling="self_attention", history_heads=h).validate()
    with pytest.raises(ValueError, match="user_history_len"):
        TwoTowerConfig(**BASE, user_history_len=65, history_pooling="self_attention").validate()
    with pytest.raises(ValueError, match="history_pooling"):
        TwoTowerConfig(**BASE, user_history_len=5, history_pooling="selfattention").validate()
    with pytest.raises(ValueError, match="title_pooling"):
        TwoTowerConfig(**BASE, n_title_buckets=20, title_pooling="self_attention").validate()
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerConfig(**BASE, **SA, candidate_sampling="mixed", n_sampled_negatives=8).validate()
    from two_tower_amazon_recommender_amd import config, ops, train
    from two_tower_amazon_recommender_amd.trainer import HISTORY_ENCODERS, HISTORY_POOLINGS
    assert HISTORY_POOLINGS == ("sum", "mean", "sqrtn", "attention", "gru")           # still five values
    assert HISTORY_ENCODERS == HISTORY_POOLINGS + ("self_attention",) and ops.SELF_ATTENTION_HEADS == (1, 2, 4, 8)
    doc = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                     "features": {"history": {"max_items": 12, "pooling": "self_attention", "heads": 4}}}}
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.user_history_len, cfg.history_pooling, cfg.history_heads, cfg.history_self_attention) == (12, "self_attention", 4, True)
    cfg.validate()
    del doc["model"]["features"]["history"]["heads"]
    assert config.model_config_from_dict(doc, 10, 10)[0].history_heads == 1
    args = train.parse(["--config", "x.yaml", "--history-len", "7", "--history-pooling", "self_attention", "--history-heads", "8"])
    assert (args.history_len, args.history_pooling, args.history_heads) == (7, "self_attention", 8)
    assert train.parse(["--config", "x.yaml"]).history_heads is None
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--history-heads", "3"])
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--title-pooling", "self_attention"])
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n")
    with pytest.raises(NotImplementedError, match="history"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--history-len", "4", "--history-pooling", "self_attention",
                    "--distributed"])


def test_graph_capture_and_the_sharded_trainer_refuse_the_feature():
    from two_tower_amazon_recommender_amd import trainer
    cfg = TwoTowerConfig(**BASE, **SA)
    assert any(refused(cfg) for refused, _ in trainer._GRAPH_REFUSALS)
    assert not any(refused(TwoTowerConfig(**BASE)) for refused, _ in trainer._GRAPH_REFUSALS)


def test_layout_blocks_are_last_from_a_16_byte_boundary_and_carry_no_l2():
    d, L = 32, 5
    everything = dict(BASE, n_user_features=3, rating_weight=0.5, rating_hidden=32, cross_layers=1, layer_norm=True,
                      time_fields=("hour", "period"), time_buckets=5, time_max=100)
    for extra in (BASE, everything):
        for h in (1, 2, 8):
            off = dense_layout(TwoTowerConfig(**extra, user_history_len=L))         # (pooled by the mean: no dense block)
            on = dense_layout(TwoTowerConfig(**extra, user_history_len=L, history_pooling="self_attention", history_heads=h))
            names = list(on.blocks)
            assert names[-3:] == ["history_sa.Wqk", "history_sa.Wvo", "history_sa.p"]
            assert names[:-3] == list(off.blocks) and all(on.blocks[k] == off.blocks[k] for k in off.blocks)     # no offset moved
            assert on.segments[:len(off.segments)] == off.segments
            wqk, wvo, p = (on.blocks[k] for k in names[-3:])
            assert wqk.offset % 4 == 0 and 0 <= wqk.offset - off.total < 4 and wvo.offset == wqk.end and p.offset == wvo.end
            assert on.total == p.end and wvo.offset % 4 == 0 and p.offset % 4 == 0
            assert wqk.shape == (d, h * d) and wvo.shape == (h * d, d) and p.shape == (h, L)
            assert wqk.glorot == (44, d + d) and wvo.glorot == (45, h * d + d) and p.glorot is None and p.fill == 0.0
            segs = on.segments[len(off.segments):]
            assert [s.name for s in segs] == names[-3:] and all(s.group == "self_attention" and not s.l2 for s in segs)
            assert [(s.lo, s.hi, s.stride) for s in segs] == [(b.offset, b.end, b.end - b.offset) for b in (wqk, wvo, p)]


def test_layout_with_the_option_off_is_unchanged():
    """The offsets of the configs tests/test_history_gru_cpu.py lists, stated: nothing of the encoder leaks into a config without
    it, and the earlier keywords of dense_segment_count keep their meaning."""
    for kw in (dict(BASE), dict(BASE, user_history_len=5), dict(BASE, user_history_len=5, history_pooling="attention"),
               dict(BASE, history_pooling="gru"), dict(BASE, user_history_len=5, history_pooling="gru"),
               dict(BASE, history_pooling="self_attention", history_heads=4)):
        lay = dense_layout(TwoTowerConfig(**kw))
        assert not any(k.startswith("history_sa") for k in lay.blocks) and not any(s.group == "self_attention" for s in lay.segments)
    lay = dense_layout(TwoTowerConfig(**BASE))
    assert lay.total == 2 * (32 * 64 + 64 + 64 * 32 + 32) and len(lay.segments) == 8
    assert dense_layout(TwoTowerConfig(**BASE, history_heads=8)) == lay
    gru = TwoTowerConfig(**BASE, user_history_len=5, history_pooling="gru")
    assert gru.dense_segment_count() == 12 and gru.dense_segment_count(gru=False) == 8 and gru.dense_segment_count(True, True, False) == 8
    assert dense_layout(gru).total == lay.total + 2 * 32 * 96 + 2 * 96
    attn = TwoTowerConfig(**BASE, user_history_len=5, history_pooling="attention")
    assert attn.dense_segment_count() == 9 and attn.dense_segment_count(attention=False) == 8 and dense_layout(attn).total == lay.total + 37
    cfg = TwoTowerConfig(**BASE, **SA)
    assert cfg.dense_segment_count() == 11 and cfg.dense_segment_count(self_attention=False) == 8
    assert cfg.dense_segment_count(True, True) == 11 and cfg.dense_segment_count(cross=False, attention=False, gru=False) == 11
    assert TwoTowerConfig(**BASE, history_pooling="self_attention").dense_segment_count() == 8


def test_segment_limit_blames_the_right_block():
    full = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[128, 64, 32], user_history_len=3, history_pooling="self_attention")
    cfg = TwoTowerConfig(**full)
    cfg.validate()                                                                    # 12 + 3 = 15: fits
    assert cfg.dense_segment_count() == 15
    TwoTowerConfig(**full, n_user_features=3).validate()                              # 16: one more feature still fits
    with pytest.raises(NotImplementedError, match="self-attention adds three"):
        TwoTowerConfig(**full, n_user_features=3, n_item_features=3).validate()       # 17: the last block over the limit is blamed


def test_checkpoint_keys_do_not_change():
    from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, TwoTowerTrainer

    class Stub:
        pass
    keys = {}
    for pooling in ("mean", "self_attention"):
        s = Stub()
        s.cfg = TwoTowerConfig(**BASE, optimizer="adam", user_history_len=3, history_pooling=pooling, history_heads=2)
        for name in ("dense_flat", "dense_accum", "dense_m", "dense_v"):
            setattr(s, name, name)
        s.tables = {p: EmbeddingTable.new(s.cfg, "cpu", p, 0, 10, None, {"user_history": "user_history"} if p == "history" else None)
                    for p in ("user", "item", "history")}
        s.step_index, s.dropout_seed, s.adam_step = 0, 0, 1
        sd = TwoTowerTrainer.state_dict(s)
        keys[pooling] = set(sd)
        assert sd["config"]["history_pooling"] == pooling and sd["config"]["history_heads"] == 2
    assert keys["mean"] == keys["self_attention"]


# ------------------------------------------------------------------------------------------ 3. the C entries and the ops
def test_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    res, fwd, comb = (lib.tt_history_self_attention_resolve_f32, lib.tt_history_self_attention_pool_fwd_f32,
                      lib.tt_history_self_attention_combine_f32)
    bwd, qg = lib.tt_history_self_attention_pool_bwd_f32, lib.tt_history_self_attention_query_grad_f32
    one, odd = C.c_void_p(16), C.c_void_p(20)                        # never dereferenced: every call fails first
    err = lib.tt_last_error
    #   table rows dim tokens n_token_rows L bag_rows n_bags exclude base_ids base_rows ids newest xn flag stream
    r = lambda dim, L, n_rows, n_bags, *ptrs: res(ptrs[0], 10, dim, ptrs[1], n_rows, L, None, n_bags, None, None, 0, ptrs[2], ptrs[3],
                                                  ptrs[4], None, None)
    N5 = (None,) * 5
    assert r(36, 3, 4, 4, *N5) == E and b"multiple of 32" in err()
    assert r(288, 3, 4, 4, *N5) == E and b"32..256" in err()
    assert r(32, 0, 4, 4, *N5) == E and b"L must be" in err()
    assert r(32, 65, 4, 4, *N5) == E and b"L must be" in err()
    assert r(32, 3, 2 ** 30, 2 ** 30, *N5) == E and b"31 bits" in err()
    assert r(32, 3, 4, 5, *N5) == E and b"identity" in err()
    assert res(None, 10, 32, None, 4, 3, None, 4, None, one, 0, None, None, None, None, None) == E and b"base_rows" in err()
    assert r(32, 3, 4, 4, one, one, one, one, None) == E and b"null" in err()
    assert r(32, 3, 4, 4, one, one, one, one, odd) == E and b"aligned" in err()
    assert b"tt_history_self_attention_resolve_f32" in err()
    assert r(32, 3, 0, 0, *N5) == _lib.TT_OK
    #   table rows dim L heads ids n_bags t p pooled weights stream
    f = lambda dim, L, h, n, *ptrs: fwd(ptrs[0], 10, dim, L, h, ptrs[1], n, ptrs[2], ptrs[3], ptrs[4], ptrs[5], None)
    N6 = (None,) * 6
    assert f(48, 3, 2, 4, *N6) == E and b"multiple of 32" in err()
    assert f(32, 0, 2, 4, *N6) == E and b"L must be" in err()
    for h in (0, 3, 16, -1):
        assert f(32, 3, h, 4, *N6) == E and b"heads must be" in err()
    assert f(32, 3, 2, 2 ** 30, *N6) == E and b"31 bits" in err()
    assert f(32, 3, 2, 4, one, one, one, one, one, None) == E and b"null" in err()
    assert f(32, 3, 2, 4, one, one, odd, one, one, one) == E and b"aligned" in err()
    assert b"tt_history_self_attention_pool_fwd_f32" in err()
    assert f(32, 3, 2, 0, *N6) == _lib.TT_OK
    #   out newest n_bags dim base_table base_rows base_ids stream
    assert comb(None, None, 4, 40, None, 5, None, None) == E and b"multiple of 32" in err()
    assert comb(None, None, 4, 32, None, 0, None, None) == E and b"base_rows" in err()
    assert comb(one, one, 4, 32, one, 5, None, None) == E and b"null" in err()
    assert comb(odd, one, 4, 32, one, 5, one, None) == E and b"aligned" in err()
    assert b"tt_history_self_attention_combine_f32" in err()
    assert comb(None, None, 0, 32, None, 5, None, None) == _lib.TT_OK
    #   table rows dim L heads ids weights pooled dpooled t n_bags slot_grads dt dp_slabs n_slabs stream
    b = lambda dim, L, h, n, ns, *ptrs: bwd(ptrs[0], 10, dim, L, h, *ptrs[1:6], n, *ptrs[6:9], ns, None)
    N9 = (None,) * 9
    assert b(24, 3, 2, 4, 1, *N9) == E and b"multiple of 32" in err()
    assert b(32, 65, 2, 4, 1, *N9) == E and b"L must be" in err()
    assert b(32, 3, 5, 4, 1, *N9) == E and b"heads must be" in err()
    assert b(32, 3, 2, 4, 0, *N9) == E and b"n_slabs" in err()
    assert b(32, 3, 2, 2 ** 30, 1, *N9) == E and b"31 bits" in err()
    assert b(32, 3, 2, 4, 1, *((one,) * 8), None) == E and b"null" in err()
    assert b(32, 3, 2, 4, 1, *((one,) * 6), odd, one, one) == E and b"aligned" in err()
    assert b"tt_history_self_attention_pool_bwd_f32" in err()
    assert b(32, 3, 2, 0, 1, *N9) == _lib.TT_OK
    #   newest dxn n_bags L dim slot_grads stream
    assert qg(None, None, 4, 3, 36, None, None) == E and b"multiple of 32" in err()
    assert qg(None, None, 4, 0, 32, None, None) == E and b"L must be" in err()
    assert qg(one, one, 4, 3, 32, None, None) == E and b"null" in err()
    assert qg(one, odd, 4, 3, 32, one, None) == E and b"aligned" in err()
    assert b"tt_history_self_attention_query_grad_f32" in err()
    assert qg(None, None, 0, 3, 32, None, None) == _lib.TT_OK
    assert lib.tt_history_self_attention_num_slabs(0) == 1 and lib.tt_history_self_attention_num_slabs(33) == 5
    assert lib.tt_history_self_attention_num_slabs(300) == 38 and lib.tt_history_self_attention_num_slabs(10 ** 6) == 1024
    assert lib.tt_abi_version() == 10


def test_header_signatures_and_the_custom_ops_exist():
    header = (ROOT / "include" / "twotower_hip.h").read_text()
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "tt_stream_t": C.c_void_p}
    for name in ("resolve", "pool_fwd", "combine", "pool_bwd", "query_grad"):
        name = f"tt_history_self_attention_{name}_f32"
        restype, argtypes = _lib.SIGNATURES[name]
        m = re.search(r"int " + name + r"\((.*?)\);", header, re.S)
        params = [p.strip() for p in m.group(1).split(",")]
        assert [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in params] == argtypes, name
        assert restype is C.c_int
    assert "int32_t tt_history_self_attention_num_slabs(int64_t n_bags);" in header
    from two_tower_amazon_recommender_amd import ops, torch_ops
    assert callable(ops.history_self_attention) and callable(ops.history_self_attention_bwd) and "self_attention" not in ops.POOLINGS
    for name in ("history_self_attention", "history_self_attention_bwd"):
        assert name in torch_ops.OPS and hasattr(torch.ops.twotower, name)
    d, L, h = 32, 5, 4
    table, tokens = torch.empty(100, d, device="meta"), torch.empty(7, L, dtype=torch.int32, device="meta")
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="meta")
    Wqk, Wvo, p = torch.empty(d, h * d, device="meta"), torch.empty(h * d, d, device="meta"), torch.empty(h, L, device="meta")
    out, ids, newest, xn, T, P, w = torch.ops.twotower.history_self_attention(table, tokens, None, None, None, None, Wqk, Wvo, p)
    assert out.shape == xn.shape == (7, d) and ids.shape == (35,) and ids.dtype == torch.int64 and newest.shape == (7,)
    assert newest.dtype == torch.int32 and T.shape == P.shape == (7, h * d) and w.shape == (7, h, L)
    out, ids, newest, xn, T, P, w = torch.ops.twotower.history_self_attention(table, tokens, i64(3), i64(3),
                                                                              torch.empty(9, d, device="meta"), i64(3), Wqk, Wvo, p)
    assert out.shape == (3, d) and ids.shape == (15,) and w.shape == (3, h, L)
    sg, dWqk, dWvo, dp = torch.ops.twotower.history_self_attention_bwd(table, ids, newest, xn, T, P, w, out, Wqk, Wvo)
    assert sg.shape == (15, d) and dWqk.shape == (d, h * d) and dWvo.shape == (h * d, d) and dp.shape == (h, L)
    z = torch.zeros
    with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel, no fallback
        torch.ops.twotower.history_self_attention(z(10, d), z(2, 3, dtype=torch.int32), None, None, None, None, z(d, d), z(d, d), z(1, 3))
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        ops.history_self_attention(z(10, d), z(2, 3, dtype=torch.int32), z(d, d), z(d, d), z(1, 3))


# ------------------------------------------------------------------------------------------ 4. registers
def test_no_kernel_of_the_translation_unit_uses_scratch(tmp_path):
    """csrc/history_selfattn.hip compiles for gfx950; the resolve, combine and query-gradient kernels and the four head counts
    of both pool kernels report 0 bytes of scratch."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / "history_selfattn.o"),
                        str(CSRC / "history_selfattn.hip")], check=True, capture_output=True, text=True, timeout=900)
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 11, names
    assert sum("sa_pool_fwd_kernel" in n for n in names) == 4 and sum("sa_pool_bwd_kernel" in n for n in names) == 4
    assert not any(scratch), dict(zip(names, scratch))

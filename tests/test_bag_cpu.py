"""The pooled item-title feature without a GPU: the restatement of tests/bag_check.py against torch's embedding_bag, the title
tokenizer, config validation, the C entries' argument validation (before any launch), the ctypes signatures, and that a model
without the feature keeps its configuration defaults and checkpoint keys."""
import dataclasses

import numpy as np
import pytest
import torch

import bag_check as bc
from two_tower_amazon_recommender_amd import _lib, data
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig


def _problem(rng, rows=40, dim=12, n=37, L=7):
    table = rng.standard_normal((rows, dim))
    tokens = rng.integers(0, rows, (n, L)).astype(np.int32)
    tokens[rng.random((n, L)) < 0.35] = -1                  # padding anywhere in a row
    tokens[3] = -1                                          # an all-padding row
    tokens[5, :3] = tokens[5, 3]                            # a repeated token
    return table, tokens


@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_restatement_agrees_with_torch_embedding_bag_in_f64(pooling):
    rng = np.random.default_rng(1)
    table, tokens = _problem(rng)
    rows = table.shape[0]
    got, batch_ids, inv, flag = bc.bag_forward(table, tokens, pooling=pooling)
    assert flag == 0 and np.array_equal(batch_ids, tokens.reshape(-1).astype(np.int64))
    # torch: the padding id is an extra (zero) row at index `rows`
    w = torch.from_numpy(np.concatenate([table, np.zeros((1, table.shape[1]))]))
    idx = torch.from_numpy(np.where(tokens < 0, rows, tokens).astype(np.int64))
    want = torch.nn.functional.embedding_bag(idx, w, mode=pooling, padding_idx=rows).numpy()
    assert np.isfinite(want).all() and not want[3].any()
    assert np.abs(got - want).max() <= 1e-13
    cnt = (tokens >= 0).sum(1)
    assert np.array_equal(inv, np.where(cnt > 0, 1.0 / np.maximum(cnt, 1) if pooling == "mean" else 1.0, 0.0))
    # indirect bags, accumulate: out + pooled, an empty bag's row untouched
    br = np.array([5, 3, -1, 0, 5, 36], dtype=np.int64)
    base = rng.standard_normal((len(br), table.shape[1]))
    acc, ids2, inv2, flag2 = bc.bag_forward(table, tokens, br, pooling, accumulate=True, out=base)
    assert flag2 == 0 and np.abs(acc - (base + np.where((br >= 0)[:, None], want[np.maximum(br, 0)], 0.0))).max() <= 1e-13
    assert np.array_equal(acc[1], base[1]) and np.array_equal(acc[2], base[2]) and inv2[1] == 0 and inv2[2] == 0
    assert (ids2.reshape(len(br), -1)[2] == -1).all()


def test_restatement_sqrtn_flags_and_the_first_row_rule():
    rng = np.random.default_rng(2)
    table, tokens = _problem(rng)
    table = table.astype(np.float32)
    got, _, inv, _ = bc.bag_forward(table, tokens, pooling="sqrtn")
    cnt = (tokens >= 0).sum(1)
    s, _, _, _ = bc.bag_forward(table, tokens, pooling="sum")
    want_inv = np.where(cnt > 0, np.float32(1) / np.sqrt(np.maximum(cnt, 1).astype(np.float32)), np.float32(0))
    assert np.array_equal(bc.bits(inv), bc.bits(want_inv)) and np.array_equal(bc.bits(got), bc.bits(s * want_inv[:, None]))
    # a token out of range is skipped and flagged; a bag row out of range is an empty bag and flagged; -1 is neither
    bad = tokens.copy()
    bad[0, 0] = table.shape[0]
    out, ids, _, flag = bc.bag_forward(table, bad, pooling="sum")
    assert flag == 1 and ids[0] == -1
    clean = bad.copy()
    clean[0, 0] = -1
    assert np.array_equal(bc.bits(out), bc.bits(bc.bag_forward(table, clean, pooling="sum")[0]))
    _, _, inv3, flag3 = bc.bag_forward(table, tokens, np.array([0, len(tokens)]), "mean")
    assert flag3 == 1 and inv3[1] == 0
    assert bc.bag_forward(table, tokens, np.array([0, -1]), "mean")[3] == 0
    # the sum starts AT the first valid row: a bag of one -0.0 row stays -0.0 (0 + -0.0 would be +0.0); an empty bag is +0.0
    t2 = np.array([[-0.0, 1.0], [2.0, 3.0]], dtype=np.float32)
    o2 = bc.bag_forward(t2, np.array([[-1, 0], [-1, -1]], dtype=np.int32), pooling="mean")[0]
    assert np.signbit(o2[0, 0]) and not np.signbit(o2[1]).any() and not o2[1].any()


def test_title_tokenizer():
    rows, valid = data.title_token_rows(["The QUICK brown-fox, 2nd ed.!", "", "a b c d e f", "x" * 40 + " Y"], 4, width=8)
    assert rows.shape == (4, 4, 8) and rows.dtype == np.uint8 and valid.dtype == bool
    word = lambda i, k: bytes(rows[i, k]).rstrip(b"\0").decode()
    assert [word(0, k) for k in range(4)] == ["the", "quick", "brown", "fox"]       # case, punctuation, truncation at max_tokens
    assert valid[0].all()
    assert not valid[1].any() and not rows[1].any()                                  # empty title: an all-padding row
    assert [word(2, k) for k in range(4)] == ["a", "b", "c", "d"]
    assert word(3, 0) == "x" * 8 and word(3, 1) == "y" and valid[3].tolist() == [True, True, False, False]   # truncation at width
    r2, v2 = data.title_token_rows(["Café déjà-vu 10%"], 8)
    assert [bytes(r2[0, k]).rstrip(b"\0").decode() for k in range(int(v2.sum()))] == ["caf", "d", "j", "vu", "10"]
    assert r2.shape == (1, 8, 32)


def test_read_item_titles_takes_the_first_interaction_and_fills_missing(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    item_idx = np.array([2, 0, 2, 4, 0], dtype=np.int64)
    p = tmp_path / "x.parquet"
    pq.write_table(pa.table({"user_idx": np.arange(5), "item_idx": item_idx,
                             "title": ["Red Shoe", None, "other", "Blue Hat", "Zero"]}), p)
    assert data.read_item_titles(p, item_idx, 6) == ["", "", "Red Shoe", "", "Blue Hat", ""]
    pq.write_table(pa.table({"user_idx": np.arange(5), "item_idx": item_idx}), p)
    with pytest.raises(KeyError, match="title"):
        data.read_item_titles(p, item_idx, 6)


def test_config_validation():
    base = dict(n_users=10, n_items=10)
    TwoTowerConfig(**base, n_title_buckets=100, title_max_tokens=64, title_pooling="sqrtn").validate()
    TwoTowerConfig(**base, n_title_buckets=0, title_max_tokens=1, title_pooling="sum").validate()
    for bad in (dict(n_title_buckets=-1), dict(title_max_tokens=0), dict(title_max_tokens=65), dict(title_pooling="max")):
        with pytest.raises(ValueError, match="title"):
            TwoTowerConfig(**base, **bad).validate()
    from two_tower_amazon_recommender_amd import config
    doc = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                     "features": {"title": {"buckets": 5000, "max_tokens": 12, "pooling": "sqrtn"}}}}
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.n_title_buckets, cfg.title_max_tokens, cfg.title_pooling) == (5000, 12, "sqrtn")
    del doc["model"]["features"]
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.n_title_buckets, cfg.title_max_tokens, cfg.title_pooling) == (0, 16, "mean")


def test_feature_off_keeps_the_config_defaults_and_the_checkpoint_keys():
    cfg = TwoTowerConfig(n_users=10, n_items=10)
    assert (cfg.n_title_buckets, cfg.title_max_tokens, cfg.title_pooling) == (0, 16, "mean")
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]
    assert names[-3:] == ["n_title_buckets", "title_max_tokens", "title_pooling"]         # appended: every earlier field as it was
    assert cfg.embedding_dim == 128 and cfg.n_category_buckets == 0 and cfg.normalize_embeddings is False
    # state_dict reads nothing but attributes: a stand-in without a device shows the keys of a model without the feature
    from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, TwoTowerTrainer

    class Stub:
        pass
    for opt, extra in (("sgd", set()), ("adagrad", {"user_accum", "item_accum", "dense_accum"}),
                       ("adam", {"user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "adam_step"})):
        s = Stub()
        s.cfg = TwoTowerConfig(n_users=10, n_items=10, optimizer=opt)
        for k in ("dense_flat", "dense_accum", "dense_m", "dense_v"):
            setattr(s, k, k)
        s.tables = {p: EmbeddingTable.new(s.cfg, "cpu", p, 0, 10, None) for p in ("user", "item")}     # (the records: CPU tensors)
        s.step_index, s.dropout_seed, s.adam_step = 0, 0, 1
        sd = TwoTowerTrainer.state_dict(s)
        assert set(sd) == {"config", "user_table", "item_table", "dense", "step_index", "dropout_seed"} | extra, opt
        assert sd["config"]["n_title_buckets"] == 0


def test_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    fwd = lib.tt_embedding_bag_fwd_f32
    #            table rows dim tokens n_token_rows L bag_rows n_bags pooling acc out ids inv flag stream
    assert fwd(None, 10, 6, None, 4, 3, None, 4, 1, 0, None, None, None, None, None) == E and b"multiple of 4" in lib.tt_last_error()
    assert fwd(None, 10, 2048, None, 4, 3, None, 4, 1, 0, None, None, None, None, None) == E
    assert fwd(None, 10, 8, None, 4, 0, None, 4, 1, 0, None, None, None, None, None) == E and b"L must be" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, -2, None, 4, 1, 0, None, None, None, None, None) == E
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 3, 0, None, None, None, None, None) == E and b"pooling" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, -1, 0, None, None, None, None, None) == E
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 2, None, None, None, None, None) == E and b"accumulate" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 5, 1, 0, None, None, None, None, None) == E and b"identity" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 0, None, None, None, None, None) == E and b"null" in lib.tt_last_error()
    assert fwd(None, 0, 8, None, 4, 3, None, 4, 1, 0, None, None, None, None, None) == E
    assert fwd(None, 10, 8, None, 2 ** 30, 3, None, 2 ** 30, 1, 0, None, None, None, None, None) == E and b"31 bits" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 0, 3, None, 0, 1, 0, None, None, None, None, None) == _lib.TT_OK       # no bags: nothing launched
    bwd = lib.tt_embedding_bag_bwd_f32
    #            dy inv n_bags dim L order n_ids gs order_bags stream
    assert bwd(None, None, 4, 6, 3, None, 12, None, None, None) == E and b"multiple of 4" in lib.tt_last_error()
    assert bwd(None, None, 4, 8, 0, None, 0, None, None, None) == E and b"L must be" in lib.tt_last_error()
    assert bwd(None, None, 4, 8, 3, None, 11, None, None, None) == E and b"n_ids" in lib.tt_last_error()
    assert bwd(None, None, 4, 8, 3, None, 12, None, None, None) == E and b"null" in lib.tt_last_error()
    assert bwd(None, None, 0, 8, 3, None, 0, None, None, None) == _lib.TT_OK


def test_ctypes_signatures_and_the_custom_op_exist():
    import ctypes as C
    assert len(_lib.SIGNATURES["tt_embedding_bag_fwd_f32"][1]) == 15 and len(_lib.SIGNATURES["tt_embedding_bag_bwd_f32"][1]) == 10
    assert _lib.SIGNATURES["tt_embedding_bag_fwd_f32"][0] is C.c_int
    lib = _lib.load()
    assert lib.tt_embedding_bag_fwd_f32.argtypes[5] is C.c_int32 and lib.tt_embedding_bag_bwd_f32.argtypes[6] is C.c_int64
    from two_tower_amazon_recommender_amd import ops, torch_ops
    assert ops.POOLINGS == {"sum": 0, "mean": 1, "sqrtn": 2}
    assert "embedding_bag" in torch_ops.OPS and hasattr(torch.ops.twotower, "embedding_bag")
    table, tokens = torch.empty(100, 32, device="meta"), torch.empty(7, 5, dtype=torch.int32, device="meta")
    assert torch.ops.twotower.embedding_bag(table, tokens, None, "mean").shape == (7, 32)
    assert torch.ops.twotower.embedding_bag(table, tokens, torch.empty(3, dtype=torch.int64, device="meta"), "sum").shape == (3, 32)
    with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel, no fallback
        torch.ops.twotower.embedding_bag(torch.zeros(10, 8), torch.zeros(2, 3, dtype=torch.int32), None, "mean")

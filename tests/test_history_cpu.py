"""The pooled user-history feature without a GPU: the restatement of tests/history_check.py against torch's embedding_bag, the
history builder of data.py, config validation (YAML block, CLI overrides, field order), the C entry's argument validation
(before any launch), the ctypes signature against the header, and that a model without the feature keeps its checkpoint keys."""
import ctypes as C
import dataclasses
import pathlib
import re

import numpy as np
import pytest
import torch

import history_check as hc
from two_tower_amazon_recommender_amd import _lib, data
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _problem(rng, rows=40, dim=12, n=37, L=7):
    table = rng.standard_normal((rows, dim))
    tokens = rng.integers(0, rows, (n, L)).astype(np.int32)
    tokens[rng.random((n, L)) < 0.3] = -1
    tokens[3] = -1                                          # an all-padding row
    tokens[5, :3] = tokens[5, 3] = 9                        # a repeated token (excluded below: every occurrence goes)
    tokens[6] = [4, -1, 4, -1, -1, -1, 4]                   # all valid slots match: an empty bag after the exclusion
    exclude = rng.integers(0, rows, n).astype(np.int64)
    exclude[5], exclude[6], exclude[7], exclude[8] = 9, 4, -1, rows + 3
    exclude[10] = tokens[10, 0] = 17                        # a match in the first slot
    return table, tokens, exclude


@pytest.mark.parametrize("pooling", ["sum", "mean"])
def test_restatement_agrees_with_torch_embedding_bag_in_f64(pooling):
    rng = np.random.default_rng(1)
    table, tokens, exclude = _problem(rng)
    rows, dim = table.shape
    base_table = rng.standard_normal((20, dim))
    base_ids = rng.integers(0, 20, len(tokens)).astype(np.int64)
    got, batch_ids, inv, flag = hc.history_forward(table, tokens, None, exclude, (base_table, base_ids), pooling)
    assert flag == 0
    skipped = (tokens < 0) | (tokens == exclude[:, None])
    assert (tokens == exclude[:, None]).any() and np.array_equal(batch_ids.reshape(tokens.shape), np.where(skipped, -1, tokens))
    # torch: the sum with per-sample weight 0 on every skipped slot; mean = that sum over the corrected count
    w = torch.from_numpy(table)
    idx = torch.from_numpy(np.where(tokens < 0, 0, tokens).astype(np.int64))
    psw = torch.from_numpy((~skipped).astype(np.float64))
    s = torch.nn.functional.embedding_bag(idx, w, mode="sum", per_sample_weights=psw).numpy()
    cnt = (~skipped).sum(1)
    pooled = s if pooling == "sum" else s / np.maximum(cnt, 1)[:, None]
    assert np.abs(got - (base_table[base_ids] + pooled)).max() <= 1e-13
    assert cnt[6] == 0 and cnt[3] == 0 and inv[6] == 0 and np.array_equal(got[6], base_table[base_ids[6]])
    assert np.array_equal(inv, np.where(cnt > 0, 1.0 / np.maximum(cnt, 1) if pooling == "mean" else 1.0, 0.0))
    # without a base and without exclusion it is bag_forward itself; exclusion alone = bag_forward on the masked matrix
    import bag_check as bc
    a, b = hc.history_forward(table, tokens, pooling=pooling), bc.bag_forward(table, tokens, pooling=pooling)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    masked = np.where(skipped, -1, tokens).astype(np.int32)
    a, b = hc.history_forward(table, tokens, None, exclude, None, pooling), bc.bag_forward(table, masked, pooling=pooling)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    # indirect bags; an out-of-range base id is a zero row and the flag, -1 a zero row and no flag
    br = np.array([5, 3, -1, 0, 6], dtype=np.int64)
    ex = np.array([9, 1, 2, -5, 4], dtype=np.int64)
    out, ids, inv2, f2 = hc.history_forward(table, tokens, br, ex, (base_table, np.array([0, 1, -1, 20, 3])), pooling)
    assert f2 == 1 and not out[2].any() and inv2[1] == 0 and inv2[2] == 0 and inv2[4] == 0 and np.array_equal(out[4], base_table[3])
    assert hc.history_forward(table, tokens, br, ex, (base_table, np.array([0, 1, -1, 19, 3])), pooling)[3] == 0
    assert (ids.reshape(5, -1)[0] != 9).all() and np.abs(out[3] - pooled_row(table, tokens[0], pooling)).max() <= 1e-13


def pooled_row(table, tok, pooling):
    v = tok[tok >= 0]
    s = table[v].sum(0)
    return s if pooling == "sum" else s / max(len(v), 1)


def test_user_histories():
    #            position: 0  1  2  3  4  5  6  7  8  9 10
    u = np.array([0, 1, 0, 0, 2, 0, 1, 0, 2, 2, 2])
    i = np.array([5, 7, 6, 5, 1, 8, 7, 9, 2, 3, 1])
    t = np.array([9, 3, 1, 1, 4, 5, 3, 0, 2, 2, 7])
    h = data.user_histories(u, i, 5, 3, timestamp=t)
    assert h.dtype == np.int32 and h.shape == (5, 3)
    # user 0: by time 9(t0) 6(t1, pos 2) 5(t1, pos 3) 8(t5) 5(t9) -> the last three, oldest first; the tie goes by file position
    assert h[0].tolist() == [5, 8, 5]                       # more than L; item 5 is kept twice
    assert h[1].tolist() == [7, 7, -1]                      # fewer than L, a repeated item kept twice, a tie by position
    assert h[2].tolist() == [3, 1, 1] and h[3].tolist() == [-1, -1, -1] and h[4].tolist() == [-1, -1, -1]
    assert data.user_histories(u, i, 5, 4, timestamp=t)[2].tolist() == [2, 3, 1, 1]       # exactly L, ties 2 (pos 8) before 3 (pos 9)
    assert data.user_histories(u, i, 5, 5, timestamp=t)[0].tolist() == [9, 6, 5, 8, 5]
    # no timestamps: file position alone
    h2 = data.user_histories(u, i, 5, 3)
    assert h2[0].tolist() == [5, 8, 9] and h2[1].tolist() == [7, 7, -1] and h2[2].tolist() == [2, 3, 1]
    assert data.user_histories(u[:0], i[:0], 2, 3).tolist() == [[-1] * 3] * 2
    # against a plain loop on a random problem
    rng = np.random.default_rng(0)
    u, i, t = rng.integers(0, 30, 400), rng.integers(0, 50, 400), rng.integers(0, 40, 400).astype(np.float64)
    got = data.user_histories(u, i, 31, 6, timestamp=t)
    for user in range(31):
        pos = np.flatnonzero(u == user)
        pos = pos[np.argsort(t[pos], kind="stable")][-6:]
        assert got[user].tolist() == i[pos].tolist() + [-1] * (6 - len(pos))
    with pytest.raises(ValueError):
        data.user_histories(u, i, 10, 6)
    with pytest.raises(ValueError):
        data.user_histories(u, i[:-1], 31, 6)


def test_read_timestamps(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    p = tmp_path / "x.parquet"
    pq.write_table(pa.table({"user_idx": np.arange(4), "item_idx": np.arange(4), "timestamp": pa.array([3, None, 1, 2], pa.int64())}), p)
    ts = data.read_timestamps(p)
    assert ts.dtype == np.float64 and ts.tolist() == [3.0, -np.inf, 1.0, 2.0]
    pq.write_table(pa.table({"user_idx": np.arange(4), "item_idx": np.arange(4), "timestamp": np.array([0.5, np.nan, 2.0, 1.0])}), p)
    assert data.read_timestamps(p).tolist() == [0.5, -np.inf, 2.0, 1.0]
    pq.write_table(pa.table({"user_idx": np.arange(4), "item_idx": np.arange(4)}), p)
    assert data.read_timestamps(p) is None


def test_config_validation_yaml_and_cli():
    base = dict(n_users=10, n_items=10)
    TwoTowerConfig(**base, user_history_len=64, history_pooling="sqrtn").validate()
    TwoTowerConfig(**base, user_history_len=1, history_pooling="sum").validate()
    for bad in (dict(user_history_len=-1), dict(user_history_len=65), dict(user_history_len=4, history_pooling="max"),
                dict(history_pooling="max")):
        with pytest.raises(ValueError, match="history"):
            TwoTowerConfig(**base, **bad).validate()
    with pytest.raises(ValueError, match="2\\^31"):
        TwoTowerConfig(n_users=10, n_items=2 ** 31, user_history_len=4).validate()
    TwoTowerConfig(n_users=10, n_items=2 ** 31).validate()                  # the limit belongs to the feature
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerConfig(**base, user_history_len=4, candidate_sampling="mixed", n_sampled_negatives=8).validate()
    from two_tower_amazon_recommender_amd import config, train
    doc = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                     "features": {"history": {"max_items": 12, "pooling": "sqrtn"}, "title": {"buckets": 50}}}}
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.user_history_len, cfg.history_pooling, cfg.n_title_buckets) == (12, "sqrtn", 50)
    del doc["model"]["features"]
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.user_history_len, cfg.history_pooling) == (0, "mean")
    args = train.parse(["--config", "x.yaml", "--history-len", "7", "--history-pooling", "sum"])
    assert (args.history_len, args.history_pooling) == (7, "sum")
    args = train.parse(["--config", "x.yaml"])
    assert args.history_len is None and args.history_pooling is None
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--history-pooling", "max"])


def test_distributed_cli_refuses_the_feature(tmp_path):
    from two_tower_amazon_recommender_amd import train
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n")
    with pytest.raises(NotImplementedError, match="history"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--history-len", "4", "--distributed"])


def test_feature_off_keeps_the_field_order_and_the_checkpoint_keys():
    cfg = TwoTowerConfig(n_users=10, n_items=10)
    assert (cfg.user_history_len, cfg.history_pooling) == (0, "mean")
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]
    k = names.index("n_title_buckets")
    assert names[k - 2:k] == ["user_history_len", "history_pooling"] and names[-3:] == ["n_title_buckets", "title_max_tokens", "title_pooling"]
    from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, TwoTowerTrainer

    class Stub:
        pass
    for opt, extra in (("sgd", set()), ("adagrad", {"user_accum", "item_accum", "dense_accum"}),
                       ("adam", {"user_m", "user_v", "item_m", "item_v", "dense_m", "dense_v", "adam_step"})):
        for hist in (False, True):
            s = Stub()
            s.cfg = TwoTowerConfig(n_users=10, n_items=10, optimizer=opt, user_history_len=3 if hist else 0)
            for name in ("dense_flat", "dense_accum", "dense_m", "dense_v"):
                setattr(s, name, name)
            s.tables = {p: EmbeddingTable.new(s.cfg, "cpu", p, 0, 10, None) for p in ("user", "item")}     # (the records: CPU tensors)
            if hist:
                s.tables["history"] = EmbeddingTable.new(s.cfg, "cpu", "history", 0, 10, None, {"user_history": "user_history"})
            s.step_index, s.dropout_seed, s.adam_step = 0, 0, 1
            sd = TwoTowerTrainer.state_dict(s)
            more = set()
            if hist:
                more = {"history_table", "user_history"} | {"sgd": set(), "adagrad": {"history_accum"}, "adam": {"history_m", "history_v"}}[opt]
            assert set(sd) == {"config", "user_table", "item_table", "dense", "step_index", "dropout_seed"} | extra | more, (opt, hist)
            assert sd["config"]["user_history_len"] == (3 if hist else 0)


def test_c_entry_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    fwd = lib.tt_history_bag_fwd_f32
    one = C.c_void_p(16)                                    # a non-null, aligned pointer that is never dereferenced: every call fails first
    #         table rows dim tokens n_token_rows L bag_rows n_bags pooling acc out ids inv flag exclude base_table base_rows base_ids stream
    assert fwd(None, 10, 6, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, None, 0, None, None) == E and b"multiple of 4" in lib.tt_last_error()
    assert fwd(None, 10, 2048, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, None, 0, None, None) == E
    assert fwd(None, 10, 0, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, None, 0, None, None) == E
    assert fwd(None, 10, 8, None, 4, 0, None, 4, 1, 0, None, None, None, None, None, None, 0, None, None) == E and b"L must be" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 2 ** 30, 3, None, 2 ** 30, 1, 0, None, None, None, None, None, None, 0, None, None) == E and b"31 bits" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, one, 5, None, None) == E and b"go together" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, None, 5, one, None) == E and b"go together" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 1, None, None, None, None, None, one, 5, one, None) == E and b"accumulate must be 0" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 0, None, None, None, None, None, one, 0, one, None) == E and b"base_rows" in lib.tt_last_error()
    assert fwd(one, 10, 8, one, 4, 3, None, 4, 1, 0, None, None, None, None, one, one, 5, one, None) == E and b"null" in lib.tt_last_error()
    assert fwd(one, 10, 8, one, 4, 3, None, 4, 1, 0, one, None, None, None, None, C.c_void_p(20), 5, one, None) == E and b"aligned" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 3, 0, None, None, None, None, None, None, 0, None, None) == E and b"pooling" in lib.tt_last_error()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, 1, 2, None, None, None, None, None, None, 0, None, None) == E
    assert fwd(None, 10, 8, None, 4, 3, None, 5, 1, 0, None, None, None, None, None, None, 0, None, None) == E and b"identity" in lib.tt_last_error()
    assert b"tt_history_bag_fwd_f32" in lib.tt_last_error()                  # the messages name the entry that was called
    assert fwd(None, 10, 8, None, 0, 3, None, 0, 1, 0, None, None, None, None, one, one, 5, one, None) == _lib.TT_OK   # no bags: nothing launched
    assert lib.tt_abi_version() == 10


def test_header_signature_and_the_custom_op_exist():
    restype, argtypes = _lib.SIGNATURES["tt_history_bag_fwd_f32"]
    assert restype is C.c_int
    bag = _lib.SIGNATURES["tt_embedding_bag_fwd_f32"][1]
    assert argtypes[:14] == bag[:14] and argtypes[14:] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    header = (ROOT / "include" / "twotower_hip.h").read_text()
    m = re.search(r"int tt_history_bag_fwd_f32\((.*?)\);", header, re.S)
    params = [p.strip() for p in m.group(1).split(",")]
    kinds = {"*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "tt_stream_t": C.c_void_p}
    want = [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in params]
    assert want == argtypes
    assert [p.split()[-1].lstrip("*") for p in params][14:18] == ["exclude", "base_table", "base_rows", "base_ids"]
    from two_tower_amazon_recommender_amd import ops, torch_ops
    assert callable(ops.history_bag)
    assert "history_bag" in torch_ops.OPS and hasattr(torch.ops.twotower, "history_bag")
    table, tokens = torch.empty(100, 32, device="meta"), torch.empty(7, 5, dtype=torch.int32, device="meta")
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="meta")
    assert torch.ops.twotower.history_bag(table, tokens, None, None, None, None, "mean").shape == (7, 32)
    assert torch.ops.twotower.history_bag(table, tokens, i64(3), i64(3), torch.empty(9, 32, device="meta"), i64(3), "sum").shape == (3, 32)
    with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel, no fallback
        torch.ops.twotower.history_bag(torch.zeros(10, 8), torch.zeros(2, 3, dtype=torch.int32), None, None, None, None, "mean")

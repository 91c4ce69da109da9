"""The time-of-interaction context features without a GPU: the restatement's index arithmetic against numpy.datetime64, the period
edges, the table layout, the dense layout, the config / YAML refusals, data.timestamps_to_int64, and the C entries' argument
checks (which run before any launch)."""
import ctypes as C

import numpy as np
import pytest

import time_check as tc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod, data as datamod, ops
from two_tower_amazon_recommender_amd.trainer import TIME_MISSING, TwoTowerConfig, TwoTowerTrainer, dense_layout

ALL = ("hour", "day_of_week", "month", "period")


def _numpy_calendar(t):
    dt = np.asarray(t, dtype=np.int64).astype("datetime64[s]")
    day = dt.astype("datetime64[D]")
    hour = (dt - day).astype(np.int64) // 3600
    dow = (day.astype(np.int64) + 3) % 7                                    # numpy's day 0 is 1970-01-01, a Thursday; Monday = 0
    month = dt.astype("datetime64[M]").astype(np.int64) % 12
    return hour, dow, month


def _secs(date):
    return int(np.datetime64(date, "s").astype(np.int64))


def test_calendar_fields_equal_numpy_datetime64():
    rng = np.random.default_rng(0)
    t = rng.integers(_secs("1900-01-01"), _secs("2100-12-31"), 150_000)
    edges = [0, -1, 86399, 86400, _secs("2000-02-29"), _secs("2000-02-29T23:59:59"), _secs("2100-02-28T23:59:59"), _secs("2100-03-01"),
             _secs("2024-02-29"), _secs("1900-02-28T23:59:59"), _secs("1900-03-01"), _secs("1969-12-31T23:59:59")]
    t = np.concatenate([t, np.array(edges, dtype=np.int64)])
    for got, want, name in zip(tc.calendar(t), _numpy_calendar(t), ("hour", "day_of_week", "month")):
        assert np.array_equal(got, want), name
    h, d, m = tc.calendar(np.array([0, -1, _secs("2000-02-29"), _secs("2100-03-01"), _secs("2024-02-29T13:00")]))
    assert h.tolist() == [0, 23, 0, 0, 13] and d.tolist() == [3, 2, 1, 0, 3] and m.tolist() == [0, 11, 1, 2, 1]
    assert (tc.calendar(t)[0] < 24).all() and (tc.calendar(t)[1] < 7).all() and (tc.calendar(t)[2] < 12).all()
    assert min(x.min() for x in tc.calendar(t)) == 0


def test_period_edges():
    lo, hi = 1_000_000_000, 1_000_086_399
    for n in (1, 5, 4096):
        p = tc.period([lo - 10 ** 12, lo - 1, lo, hi, hi + 1, hi + 10 ** 15], n, lo, hi)
        assert p.tolist() == [0, 0, 0, n - 1, n - 1, n - 1]
        inside = tc.period(np.arange(lo, hi + 1, 997), n, lo, hi)
        assert (np.diff(inside) >= 0).all() and inside.min() == 0 and inside.max() <= n - 1
    assert tc.period([lo, lo + 43199, lo + 43200, hi], 2, lo, hi).tolist() == [0, 0, 1, 1]            # equal halves of the range
    assert tc.period([5, 6, 7], 3, 6, 6).tolist() == [0, 0, 0]                                       # span 0: one second, bucket 0
    assert tc.period([-2 ** 62, 2 ** 62], 4096, -2 ** 39, 2 ** 39 - 2).tolist() == [0, 4095]          # the widest span allowed
    idx = tc.time_indices([TIME_MISSING, lo, TIME_MISSING + 1], ALL, 5, lo, hi)
    assert idx.dtype == np.int32 and idx[0].tolist() == [-1] * 4 and (idx[1:] >= 0).all()
    assert tc.time_indices([lo], ("period", "hour"), 5, lo, hi).shape == (1, 2)                       # the fixed order, whatever is passed
    assert tc.time_indices([lo + 3600], ("period", "hour"), 5, lo, hi)[0].tolist() == [tc.calendar([lo + 3600])[0][0], 0]


def test_restated_backward_is_the_sum_and_depends_on_the_order_only():
    rng = np.random.default_rng(3)
    n, dim = 300, 8
    idx = tc.time_indices(rng.integers(0, 10 ** 9, n), ALL, 5, 0, 10 ** 9)
    idx[7] = -1
    dy = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    g, g64 = tc.time_backward(idx, dy, ALL, 5), tc.time_backward_f64(idx, dy, ALL, 5)
    assert g.dtype == np.float32 and g.shape == (48, dim) and np.abs(g - g64).max() <= 1e-5 * np.abs(g64).max()
    one = np.zeros((40, 1), dtype=np.int32)                                   # positions 0..39 on row 0: sub-sums 0..7 hold two rows
    d1 = np.arange(40, dtype=np.float32)[:, None] + np.float32(0.1)
    want = np.float32(0)
    subs = [np.float32(np.float32(0) + d1[g_, 0]) + (d1[g_ + 32, 0] if g_ < 8 else np.float32(0)) for g_ in range(32)]
    want = subs[0]
    for s in subs[1:]:
        want = np.float32(want + s)
    assert tc.time_backward(one, d1, ("hour",))[0, 0] == want


def test_time_field_layout_offsets_and_rows():
    assert ops.time_field_layout(ALL, 16) == ({"hour": 0, "day_of_week": 24, "month": 31, "period": 43}, 59)
    assert ops.time_field_layout(("period",), 4096) == ({"period": 0}, 4096)
    assert ops.time_field_layout(("month", "hour")) == ({"hour": 0, "month": 24}, 36)                 # the fixed order
    assert ops.time_field_layout(("day_of_week",)) == ({"day_of_week": 0}, 7)
    assert tc.layout(ALL, 16) == ops.time_field_layout(ALL, 16) and ops.TIME_MISSING == tc.TIME_MISSING == -2 ** 63
    for fields, buckets in (((), 0), (("week",), 0), (("hour", "hour"), 0), (("period",), 0), (("period",), 4097), (("hour",), 3)):
        with pytest.raises(ValueError):
            ops.time_field_layout(fields, buckets)


def _cfg(**kw):
    return TwoTowerConfig(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32], **kw)


def test_dense_layout_puts_the_table_last_and_moves_nothing():
    every = dict(n_user_features=5, n_item_features=3, rating_weight=0.5, rating_hidden=32, cross_layers=2, layer_norm=True,
                 user_history_len=6, history_pooling="attention")
    for base in ({}, every, dict(rating_weight=0.5, rating_hidden=32)):          # (the head's parameter count is odd: a pad in front)
        off, on = dense_layout(_cfg(**base)), dense_layout(_cfg(**base, time_fields=ALL, time_buckets=16, time_min=0, time_max=99))
        assert list(on.blocks)[:-1] == list(off.blocks) and list(on.blocks)[-1] == "time_table"
        assert all(on.blocks[k] == off.blocks[k] for k in off.blocks) and on.segments[:-1] == off.segments
        blk, seg = on.blocks["time_table"], on.segments[-1]
        assert blk.shape == (59, 32) and blk.offset % 4 == 0 and 0 <= blk.offset - off.total < 4 and on.total == blk.end
        assert (seg.name, seg.lo, seg.hi, seg.l2, seg.stride, seg.group) == ("time_table", blk.offset, blk.end, False, 59 * 32, "time")
    cfg = _cfg(time_fields=["period", "hour"], time_buckets=7)
    assert cfg.time_fields == ("hour", "period") and cfg.time_rows == 31 and _cfg().time_rows == 0     # lists are put in order


def test_config_validate_and_yaml_refusals():
    _cfg(time_fields=ALL, time_buckets=1, time_min=-5, time_max=-5).validate()
    _cfg(time_fields=("hour",), time_min=0, time_max=2 ** 40 - 1).validate()
    for kw, what in ((dict(time_fields=("hour", "weekday")), "time_fields"), (dict(time_fields=("period",)), "time_buckets"),
                     (dict(time_fields=("hour",), time_buckets=4), "time_buckets"), (dict(time_buckets=4), "time_buckets"),
                     (dict(time_fields=("period",), time_buckets=4097), "time_buckets"),
                     (dict(time_fields=("hour",), time_min=5, time_max=4), "time_min <= time_max"),
                     (dict(time_fields=("hour",), time_min=0, time_max=2 ** 40), "2\\^40"),
                     (dict(time_fields=("hour",), time_min=0.5, time_max=4), "int64")):
        with pytest.raises(ValueError, match=what):
            _cfg(**kw).validate()
    doc = lambda block: {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "features": {"time": block}}}
    assert cfgmod.time_features_from_dict({"model": {}}) == {"fields": (), "buckets": 0}
    assert cfgmod.time_features_from_dict(doc({"fields": ["period", "hour"], "buckets": 9})) == {"fields": ("hour", "period"), "buckets": 9}
    cfg, _ = cfgmod.model_config_from_dict(doc({"fields": ["month", "period"], "buckets": 12}), 300, 200)
    assert cfg.time_fields == ("month", "period") and cfg.time_buckets == 12 and cfg.time_rows == 24
    for block, what in (({"fields": ["hour", "minute"]}, "minute"), ({"fields": ["period"]}, "needs buckets"),
                        ({"fields": ["hour"], "buckets": 8}, "without the 'period'"), ({"fields": ["hour"], "step": 3}, "unknown keys"),
                        ({"fields": "hour"}, "must be a list"), (["hour"], "mapping")):
        with pytest.raises(ValueError, match=what):
            cfgmod.time_features_from_dict(doc(block))


def test_graph_capture_refuses_and_checkpoint_defaults():
    class Stub:
        mixed = False
    s = Stub()
    s.cfg = _cfg(time_fields=("hour",))
    with pytest.raises(NotImplementedError, match="time context"):
        TwoTowerTrainer.capture_graph(s)
    from two_tower_amazon_recommender_amd import trainer
    keys = {k: default for k, default, _, _ in trainer._CHECKPOINT_CHECKS}
    assert keys["time_fields"] == () and keys["time_buckets"] == 0                 # a checkpoint from before the feature: off
    assert 60 <= trainer.TID_TIME_BASE <= 62


def test_timestamps_to_int64():
    got = datamod.timestamps_to_int64(np.array([0.0, 1.9, -0.5, np.nan, -np.inf, np.inf, 1.5e9, -86400.0]))
    assert got.dtype == np.int64
    assert got.tolist() == [0, 1, -1, TIME_MISSING, TIME_MISSING, TIME_MISSING, 1_500_000_000, -86400]
    assert datamod.TIME_MISSING == TIME_MISSING


def test_c_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    fwd = lambda n=4, rows=59, dim=32, mask=15, buckets=16, lo=0, hi=99, acc=0, base=None, base_rows=0, ids=None: \
        lib.tt_time_context_fwd_f32(p, n, p, rows, dim, mask, buckets, lo, hi, p, acc, base, base_rows, ids, None, None, None)
    bad = [fwd(mask=0), fwd(mask=16), fwd(buckets=0), fwd(buckets=4097), fwd(mask=7, rows=43, buckets=3), fwd(dim=30), fwd(dim=516),
           fwd(rows=58), fwd(lo=5, hi=4), fwd(lo=0, hi=2 ** 40), fwd(n=-1), fwd(base=p), fwd(ids=p), fwd(base=p, ids=p, base_rows=0),
           fwd(base=p, ids=p, base_rows=10, acc=1)]
    assert bad == [_lib.TT_ERR_INVALID_ARG] * len(bad)
    assert fwd(n=0) == _lib.TT_OK                                                # nothing to do, nothing launched
    assert lib.tt_time_context_fwd_f32(None, 4, p, 59, 32, 15, 16, 0, 99, p, 0, None, 0, None, None, None, None) == _lib.TT_ERR_INVALID_ARG
    assert b"null pointer" in lib.tt_last_error()
    odd = C.c_void_p(p.value + 4)
    assert lib.tt_time_context_fwd_f32(p, 4, odd, 59, 32, 15, 16, 0, 99, p, 0, None, 0, None, None, None, None) == _lib.TT_ERR_INVALID_ARG
    assert b"aligned" in lib.tt_last_error()
    bwd = lambda n=4, dim=32, mask=15, buckets=16, rows=59, idx=p, dy=p, grad=p: \
        lib.tt_time_context_bwd_f32(idx, dy, n, dim, mask, buckets, rows, grad, None)
    bad = [bwd(mask=0), bwd(buckets=0), bwd(mask=8, buckets=0, rows=0), bwd(dim=6), bwd(dim=1024), bwd(rows=60), bwd(n=-1), bwd(grad=None),
           bwd(idx=None), bwd(dy=None), bwd(grad=odd)]
    assert bad == [_lib.TT_ERR_INVALID_ARG] * len(bad)
    assert b"aligned" in lib.tt_last_error()

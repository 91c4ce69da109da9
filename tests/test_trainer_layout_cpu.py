"""``dense_layout(cfg)``: where every dense parameter sits in ``dense_flat`` and which optimizer segment covers it - checked against
an independent restatement of the layout (plain offset arithmetic, written out below) over a matrix of configurations that reaches
every branch, and ``validate``'s segment-limit refusals.  No GPU, no library call: plain integers."""
import pytest

from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, dense_layout

BASE = dict(n_users=300, n_items=200, embedding_dim=32, tower_dims=[64, 32])
HEAD = dict(rating_weight=0.5, rating_hidden=32)
ATTN = dict(user_history_len=5, history_pooling="attention")
FEATS = dict(n_user_features=3, n_item_features=2)

CONFIGS = {
    "plain": {},
    "asymmetric": dict(tower_dims=[128, 64, 32], item_tower_dims=[48, 32]),
    "user features": dict(n_user_features=3),
    "item features": dict(n_item_features=2),
    "both features": FEATS,
    "head": HEAD,                                            # 2 * 32 * 32 + 32 + 32 + 1 floats: odd
    "cross 1": dict(cross_layers=1),
    "cross 2": dict(cross_layers=2),
    "cross 3": dict(cross_layers=3),
    "head + cross 1": dict(cross_layers=1, **HEAD),          # a non-zero pad in front of the cross block
    "head + cross 2": dict(cross_layers=2, **HEAD),
    "head + cross 3": dict(cross_layers=3, **HEAD),
    "attention": ATTN,                                       # [a | p]: 32 + 5 floats, no multiple of 4
    "attention + cross": dict(cross_layers=2, **ATTN),
    "head + attention": dict(**HEAD, **ATTN),                # a non-zero pad in front of the attention vector
    "everything": dict(cross_layers=2, **FEATS, **HEAD, **ATTN),
    "everything, asymmetric": dict(tower_dims=[128, 64, 32], item_tower_dims=[48, 32], cross_layers=3, n_item_features=4, **HEAD, **ATTN),
    "attention without a history": dict(history_pooling="attention"),      # user_history_len = 0: no block, no segment
    "mean-pooled history": dict(user_history_len=5),                       # a table, but nothing in dense_flat
}


def restated(cfg):
    """(blocks [(offset, size)], segments [(lo, hi, l2, stride)], pads [(lo, hi)], total, cross start, attention start)."""
    d = cfg.embedding_dim
    blocks, segs, pads, off = [], [], [], 0
    for dims in (cfg.user_dims, cfg.item_dims):
        k = d
        for n in dims:
            blocks += [(off, k * n), (off + k * n, n)]
            segs += [(off, off + k * n, True, k * n), (off + k * n, off + k * n + n, False, n)]
            off += k * n + n
            k = n
    for f in (cfg.n_user_features, cfg.n_item_features):
        if f:
            blocks.append((off, f * d))
            segs.append((off, off + f * d, True, f * d))
            off += f * d
    if cfg.rating_weight > 0:
        s, h = cfg.tower_dims[-1], cfg.rating_hidden
        blocks += [(off, 2 * s * h), (off + 2 * s * h, h), (off + 2 * s * h + h, h), (off + 2 * s * h + 2 * h, 1)]
        segs += [(off, off + 2 * s * h + h, True, 2 * s * h + h), (off + 2 * s * h + h, off + 2 * s * h + 2 * h + 1, False, h + 1)]
        off += 2 * s * h + 2 * h + 1
    cross_at = attn_at = None
    if cfg.cross_layers:
        L = cfg.cross_layers
        cross_at = -(-off // 4) * 4
        pads.append((off, cross_at))
        n_w, n_b = 2 * L * d * d, 2 * L * d
        blocks += [(cross_at + i * d * d, d * d) for i in range(2 * L)] + [(cross_at + n_w + i * d, d) for i in range(2 * L)]
        segs += [(cross_at, cross_at + n_w, True, n_w + n_b), (cross_at + n_w, cross_at + n_w + n_b, False, n_w + n_b)]
        off = cross_at + n_w + n_b
    if cfg.user_history_len > 0 and cfg.history_pooling == "attention":
        attn_at = -(-off // 4) * 4
        pads.append((off, attn_at))
        n = d + cfg.user_history_len
        blocks.append((attn_at, n))
        segs.append((attn_at, attn_at + n, False, n))
        off = attn_at + n
    return blocks, segs, pads, off, cross_at, attn_at


def old_segment_count(cfg, cross=True, attention=True):
    """The count as the config computed it before the layout existed."""
    return (2 * (len(cfg.user_dims) + len(cfg.item_dims)) + (cfg.n_user_features > 0) + (cfg.n_item_features > 0)
            + 2 * (cfg.rating_weight > 0) + 2 * (bool(cross) and cfg.cross_layers > 0)
            + (bool(attention) and cfg.user_history_len > 0 and cfg.history_pooling == "attention"))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_layout_matches_the_restatement(name):
    cfg = TwoTowerConfig(**{**BASE, **CONFIGS[name]})
    cfg.validate()
    lay = dense_layout(cfg)
    blocks, segs, pads, total, cross_at, attn_at = restated(cfg)
    got_blocks = list(lay.blocks.values())
    assert [(b.offset, b.end - b.offset) for b in got_blocks] == blocks
    assert lay.total == total
    assert [(s.lo, s.hi, s.l2, s.stride) for s in lay.segments] == segs               # order, ranges, l2 flags, slab strides
    # the cross block and the attention vector start at 16-byte boundaries, behind pads of at most 3 floats
    assert (cross_at is not None) == bool(cfg.cross_layers) and (attn_at is not None) == cfg.history_attention
    if cross_at is not None:
        assert lay.blocks["cross.user.W0"].offset == cross_at and cross_at % 4 == 0
    if attn_at is not None:
        assert lay.blocks["history_attn"].offset == attn_at and attn_at % 4 == 0
    assert "history_attn" in lay.blocks or not cfg.history_attention
    assert all(0 <= hi - lo <= 3 for lo, hi in pads)
    if name in ("head + cross 1", "head + attention", "everything"):
        assert any(hi > lo for lo, hi in pads), "an odd head must leave a pad"
    # the segments are pairwise disjoint and, with the pads, cover [0, total) exactly - and so do the blocks
    for ranges in ([(s.lo, s.hi) for s in lay.segments], [(b.offset, b.end) for b in got_blocks]):
        pieces = sorted(ranges + [p for p in pads if p[1] > p[0]])
        assert pieces[0][0] == 0 and pieces[-1][1] == lay.total
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])), pieces
        assert all(hi > lo for lo, hi in pieces)
    # the order of the groups, and which carry l2: kernels do, biases and the attention vector do not
    groups = [s.group for s in lay.segments]
    order = ["towers", "features", "head", "cross", "attention"]
    assert groups == sorted(groups, key=order.index)
    n_towers = 2 * (len(cfg.user_dims) + len(cfg.item_dims))
    assert groups.count("towers") == n_towers and [s.l2 for s in lay.segments[:n_towers]] == [True, False] * (n_towers // 2)
    assert [s.l2 for s in lay.segments if s.group == "features"] == [True] * ((cfg.n_user_features > 0) + (cfg.n_item_features > 0))
    assert [s.l2 for s in lay.segments if s.group == "head"] == ([True, False] if cfg.rating_weight > 0 else [])
    assert [s.l2 for s in lay.segments if s.group == "cross"] == ([True, False] if cfg.cross_layers else [])
    assert [s.l2 for s in lay.segments if s.group == "attention"] == ([False] if cfg.history_attention else [])
    # the count, in all the forms the config offers
    assert len(lay.segments) == cfg.dense_segment_count() == old_segment_count(cfg)
    for kw in (dict(cross=False), dict(attention=False), dict(cross=False, attention=False)):
        assert cfg.dense_segment_count(**kw) == old_segment_count(cfg, **kw), kw
    assert cfg.dense_segment_count(False) == old_segment_count(cfg, False)           # (positional, as the callers pass it)
    # views: a block's view has its shape and starts at its offset
    import torch
    flat = torch.arange(lay.total, dtype=torch.float32)
    for b in got_blocks:
        v = b.view(flat)
        assert tuple(v.shape) == b.shape and v.reshape(-1)[0].item() == b.offset and v.numel() == b.end - b.offset
    # kernels are initialised (tensor id, fan_in + fan_out), biases and the attention vector start at zero
    for b in got_blocks:
        assert (b.glorot is not None) == (len(b.shape) == 2 or b.name == "head.w2"), b.name
    ids = [b.glorot[0] for b in got_blocks if b.glorot is not None]
    assert len(set(ids)) == len(ids)


DEEP3, DEEP4 = [128, 64, 32], [256, 128, 64, 32]


def test_the_segment_limit_is_checked_in_validate_as_before():
    M = _lib.TT_MAX_DENSE_SEGS
    assert M == 16

    def cfg(dims, **kw):
        return TwoTowerConfig(n_users=10, n_items=10, embedding_dim=32, tower_dims=dims, **kw)
    # plain towers are never refused here, at any depth
    for dims in (DEEP3, DEEP4, [512] + DEEP4, [512, 512] + DEEP4):
        cfg(dims).validate()
    assert cfg(DEEP4).dense_segment_count() == 16
    # 3-layer towers: 12 + cross 2 + head 2 = 16 fits; so does 12 + 2 features + head
    full = cfg(DEEP3, cross_layers=2, **HEAD)
    full.validate()
    assert full.dense_segment_count() == 16
    cfg(DEEP3, **FEATS, **HEAD).validate()
    cfg(DEEP3, user_history_len=3, **FEATS, **HEAD).validate()                        # a mean-pooled history adds no segment
    # one more block is refused, and blamed on the block that crosses the limit
    for kw, blame in ((dict(cross_layers=2, **HEAD, **ATTN), "attention"),
                      (dict(**FEATS, **HEAD, **ATTN), "attention"),
                      (dict(cross_layers=1, **FEATS, **HEAD), "cross layers add two dense segments"),
                      (dict(cross_layers=1, **FEATS, **HEAD, **ATTN), "cross layers add two dense segments")):
        with pytest.raises(NotImplementedError, match=blame) as e:
            cfg(DEEP3, **kw).validate()
        assert "dense segment" in str(e.value) and "16" in str(e.value)
    # 4-layer towers hold 16 segments already: any optional block is refused
    for kw, blame in ((dict(n_user_features=3), "numeric side features"), (dict(n_item_features=2), "numeric side features"),
                      (HEAD, "rating head"), (dict(cross_layers=1), "cross layers add two dense segments"), (ATTN, "attention"),
                      (dict(**FEATS, **HEAD), "numeric side features"), (dict(cross_layers=2, **HEAD), "rating head"),
                      (dict(cross_layers=2, **FEATS), "numeric side features")):
        with pytest.raises(NotImplementedError, match=blame) as e:
            cfg(DEEP4, **kw).validate()
        assert "dense segment" in str(e.value)
    # deeper towers with an optional block: refused as well
    with pytest.raises(NotImplementedError, match="rating head"):
        cfg([512] + DEEP4, **HEAD).validate()

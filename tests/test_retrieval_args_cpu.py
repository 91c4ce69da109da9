"""The argument contract of the scorer's launching entries (csrc/score.hip), without a GPU: every call here violates exactly one
requirement, so each returns from validation before anything is launched; host buffers stand in for device memory (the entries
only look at the pointers' values).  Also pins the three workspace-size queries."""
import ctypes as C

import pytest

from two_tower_amazon_recommender_amd import _lib

INVALID, UNSUPPORTED, WORKSPACE = _lib.TT_ERR_INVALID_ARG, _lib.TT_ERR_UNSUPPORTED, _lib.TT_ERR_WORKSPACE

_LOSS = "q c nq nc dim diag_offset inv_temperature sample_weight cand_prob cand_ids hard_thr".split()
_FWD = _LOSS + "ws ws_bytes lse per_row loss stream".split()
_BWD = _LOSS + "lse grad_scale ws ws_bytes dq dc stream".split()
_FWD_BWD = _LOSS + "grad_scale ws ws_bytes lse per_row loss dq dc stream".split()
_RANK = "q c nq nc dim inv_temperature cand_prob pos_index ws ws_bytes rank stream".split()
_BATCH_RANK = "q c nq nc dim diag_offset inv_temperature cand_prob cand_ids ws ws_bytes rank stream".split()
_HARD_NEG = ("q c nq nc dim diag_offset inv_temperature cand_prob cand_ids num_hard_negatives ws ws_bytes scratch scratch_bytes "
             "thr stream").split()

# entry -> (parameters in ABI order, the workspace query that sizes it, the pointers of its own that must not be null)
ENTRIES = {
    "tt_retrieval_fwd_f32": (_FWD, "tt_retrieval_fwd_workspace_bytes", ["lse", "per_row", "loss"]),
    "tt_retrieval_fwd_bf16x3_f32": (_FWD, "tt_retrieval_fwd_workspace_bytes", ["lse", "per_row", "loss"]),
    "tt_retrieval_bwd_f32": (_BWD, "tt_retrieval_fwd_workspace_bytes", ["lse", "dq", "dc"]),
    "tt_retrieval_fwd_bwd_f32": (_FWD_BWD, "tt_retrieval_workspace_bytes", ["lse", "per_row", "loss", "dq", "dc"]),
    "tt_retrieval_fwd_bwd_bf16x3_f32": (_FWD_BWD, "tt_retrieval_workspace_bytes", ["lse", "per_row", "loss", "dq", "dc"]),
    "tt_retrieval_rank_f32": (_RANK, "tt_retrieval_rank_workspace_bytes", ["pos_index", "rank"]),
    "tt_retrieval_rank_bf16x3_f32": (_RANK, "tt_retrieval_rank_workspace_bytes", ["pos_index", "rank"]),
    "tt_retrieval_batch_rank_f32": (_BATCH_RANK, "tt_retrieval_rank_workspace_bytes", ["rank"]),
    "tt_retrieval_hard_negative_thresholds_f32": (_HARD_NEG, "tt_retrieval_fwd_workspace_bytes", ["scratch", "thr"]),
}
NQ, NC, DIM, OFF = 100, 131, 128, 31


def _buf(n, align=256):
    raw = (C.c_uint8 * (n + align))()
    return raw, (C.addressof(raw) + align - 1) // align * align


@pytest.fixture(scope="module")
def base():
    """Valid arguments for every entry at (NQ, NC, DIM, OFF): 256-byte aligned host buffers, the optional inputs absent."""
    lib = _lib.load()
    big = max(NQ, NC)
    sizes = dict(q=big * 256 * 4, c=big * 256 * 4, dq=NQ * DIM * 4, dc=NC * DIM * 4, lse=NQ * 4, per_row=NQ * 4, loss=4,
                 pos_index=big * 8, rank=big * 4, thr=NQ * 4, scratch=NQ * NC * 4,
                 ws=max(lib.tt_retrieval_workspace_bytes(a, b, d) for a, b in ((NQ, NC), (NC, NQ)) for d in (32, 64, 128, 256)))
    keep = {k: _buf(n) for k, n in sizes.items()}
    vals = {k: v[1] for k, v in keep.items()}
    vals.update(nq=NQ, nc=NC, dim=DIM, diag_offset=OFF, inv_temperature=10.0, grad_scale=1.0, num_hard_negatives=3,
                scratch_bytes=NQ * NC * 4, sample_weight=None, cand_prob=None, cand_ids=None, hard_thr=None, stream=None)
    return lib, vals, keep


def _cases(name, params, own, vals):
    """(overrides, return code, a word of the message) - each violates one requirement of entry `name`."""
    bx3 = "bf16x3" in name
    out = [({p: None}, INVALID, "null") for p in ["q", "c", "ws"] + own]
    out += [(dict(nq=0), INVALID, "positive"),
            (dict(dim=48), UNSUPPORTED if bx3 else INVALID, "dim 48"),
            (dict(q=vals["q"] + 4), INVALID, "q/c must be 16-byte aligned"),
            (dict(c=vals["c"] + 4), INVALID, "q/c must be 16-byte aligned"),
            (dict(ws=vals["ws"] + 16), INVALID, "256-byte aligned")]
    if bx3:
        out.append((dict(dim=64), UNSUPPORTED, "dim 64"))
    if "dq" in params:
        out += [(dict(dq=vals["dq"] + 4), INVALID, "dq/dc must be 16-byte aligned"),
                (dict(dc=vals["dc"] + 4), INVALID, "dq/dc must be 16-byte aligned")]
    if "diag_offset" in params:
        out += [(dict(diag_offset=-1), INVALID, "diag_offset"), (dict(diag_offset=NC - NQ + 1), INVALID, "diag_offset"),
                (dict(nq=NC, nc=NQ, diag_offset=0), INVALID, "diag_offset")]
    if "num_hard_negatives" in params:
        out += [(dict(num_hard_negatives=0), INVALID, "num_hard_negatives"),
                (dict(scratch_bytes=NQ * NC * 4 - 1), WORKSPACE, f"scratch {NQ * NC * 4 - 1} < {NQ * NC * 4} bytes")]
    return out


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_validates_arguments_before_any_launch(name, base):
    lib, vals, _ = base
    params, ws_query, own = ENTRIES[name]
    fn = getattr(lib, name)

    def call(**kw):
        v = dict(vals, **kw)
        if "ws_bytes" not in v:                        # the entry's own size for the shape of this call
            v["ws_bytes"] = getattr(lib, ws_query)(v["nq"], v["nc"], v["dim"]) if v["nq"] > 0 else 1 << 20
        return fn(*[v[p] for p in params]), lib.tt_last_error().decode()

    for kw, code, word in _cases(name, params, own, vals):
        got, msg = call(**kw)
        assert got == code, (name, kw, got, msg)
        assert word in msg and msg.startswith(name + ":"), (name, kw, msg)
    # one byte short of the entry's own workspace size, and the message names that size: exactly that many bytes are enough
    shapes = [(NQ, NC)] + ([(NC, NQ)] if name == "tt_retrieval_rank_f32" else [])   # explicit positives: no diagonal, nq > nc is legal
    for nq, nc in shapes:
        need = getattr(lib, ws_query)(nq, nc, DIM)
        got, msg = call(nq=nq, nc=nc, ws_bytes=need - 1)
        assert got == WORKSPACE, (name, nq, nc, got, msg)
        assert f"workspace {need - 1} < {need} bytes" in msg and msg.startswith(name + ":"), (name, msg)


def test_workspace_size_queries():
    lib = _lib.load()
    full, fwd, rank = lib.tt_retrieval_workspace_bytes, lib.tt_retrieval_fwd_workspace_bytes, lib.tt_retrieval_rank_workspace_bytes
    # (workspace_bytes, fwd_workspace_bytes, rank_workspace_bytes) as recorded before the host side's validation was shared
    pinned = {(129, 1000, 128): (1702400, 1047040, 14336), (100, 131, 64): (137984, 56064, 3328),
              (257, 300, 256): (1612544, 1243904, 9472)}
    for shape, want in pinned.items():
        got = (full(*shape), fwd(*shape), rank(*shape))
        assert got == want, (shape, got)
        assert got[0] > got[1] > got[2] > 0 and all(x % 256 == 0 for x in got), (shape, got)
    for f in (full, fwd, rank):
        for bad in [(0, 10, 32), (10, 0, 32), (10, 10, 0)]:
            assert f(*bad) == 0, bad
    from two_tower_amazon_recommender_amd import ops
    assert (ops.retrieval_workspace_bytes(129, 1000, 128), ops.retrieval_fwd_workspace_bytes(129, 1000, 128),
            ops.retrieval_rank_workspace_bytes(129, 1000, 128)) == pinned[(129, 1000, 128)]

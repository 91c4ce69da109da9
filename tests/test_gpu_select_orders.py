"""The four copies of the retrieval selection scheme on the GPU against the designed arrival orders of select_orders_check.py:
every scenario through every entry point that can express it - ops.retrieval_topk, ops.ivf_search, ops.retrieval_topk_i8 and
ops.ivf_search_i8, the int8 ones with and without the f32 corpus - compared with the NumPy reference BIT FOR BIT (ids equal, score
bits equal to np.float32 of the exact score; the scores are exact by construction, so there is no tolerance).  Every call runs
twice on the same workspace, which starts out filled with a byte pattern: the second call shows that nothing was left behind.  No GPU
call is ever the reference."""
import numpy as np
import pytest
import torch

import select_orders_check as so

pytestmark = pytest.mark.gpu


def _ops():
    from two_tower_amazon_recommender_amd import ops
    return ops


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)              # (a copy: the scenario arrays are read-only)


def _csr(s, dev):
    if s.excl is None:
        return None
    off = np.zeros(s.nq + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(e) for e in s.excl])
    flat = np.concatenate([np.asarray(e, dtype=np.int64) for e in s.excl])
    return T(off, dev), T(flat, dev)


def _call(s, entry, dev):
    """(function of (workspace, out), workspace bytes) of one entry point on scenario ``s``."""
    ops = _ops()
    q, ex, k, d = T(s.queries(), dev), _csr(s, dev), s.k, s.dim
    with_c = entry.endswith("_c")
    k1 = s.k1 if with_c else k
    if entry == "topk":
        c = T(s.c_original(), dev)
        return (lambda ws, out: ops.retrieval_topk(q, c, k, exclusions=ex, workspace=ws, out=out),
                ops.retrieval_topk_workspace_bytes(s.nq, s.n, d, k))
    if entry in ("topk_i8", "topk_i8_c"):
        codes, scales = T(s.codes(), dev), T(s.scales(), dev)
        c = T(s.c_original(), dev) if with_c else None
        return (lambda ws, out: ops.retrieval_topk_i8(q, codes, scales, k, c=c, k1=k1, exclusions=ex, workspace=ws, out=out),
                ops.retrieval_topk_i8_workspace_bytes(s.nq, s.n, d, k, k1))
    L = s.ivf
    cent, off, ids = T(L["centroids"], dev), T(L["list_offsets"], dev), T(L["list_ids"], dev)
    if entry == "ivf":
        vec = T(L["list_vectors"], dev)
        return (lambda ws, out: ops.ivf_search(q, cent, off, vec, ids, k, L["nprobe"], exclusions=ex, workspace=ws, out=out),
                ops.ivf_search_workspace_bytes(s.nq, L["nlist"], L["n"], d, k, L["nprobe"]))
    codes, scales = T(L["list_codes"], dev), T(L["list_scales"], dev)
    c = T(L["c"], dev) if with_c else None
    return (lambda ws, out: ops.ivf_search_i8(q, cent, off, codes, scales, ids, k, L["nprobe"], c=c, k1=k1, exclusions=ex,
                                              workspace=ws, out=out),
            ops.ivf_search_i8_workspace_bytes(s.nq, L["nlist"], L["n"], d, k, k1, L["nprobe"]))


def _first_difference(got_s, got_i, S, I):
    bad = np.argwhere((got_i != I) | (got_s.view(np.int32) != S.view(np.int32)))
    r, e = (int(v) for v in bad[0])
    return (f"{len(bad)} of {I.size} entries differ; first at query {r}, position {e}: got ({got_s[r, e]!r}, {got_i[r, e]}), "
            f"expected ({S[r, e]!r}, {I[r, e]})")


@pytest.mark.parametrize("s,entry", so.cases(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_designed_order(dev, s, entry):
    S, I = so.expected(s, entry)
    run, need = _call(s, entry, dev)
    assert need > 0, f"{s.name} / {entry}: the entry point refuses the shape"
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    for attempt in ("first call", "second call on the same workspace"):
        out = (torch.full((s.nq, s.k), float("nan"), dtype=torch.float32, device=dev),
               torch.full((s.nq, s.k), -7, dtype=torch.int64, device=dev))
        try:
            got_s, got_i = run(ws, out)
            got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
        except RuntimeError as e:                            # a device error: nothing more may run on this device
            pytest.exit(f"{s.name} / {entry}, {attempt}: {e}", returncode=3)
        same = np.array_equal(got_i, I) and np.array_equal(got_s.view(np.int32), S.view(np.int32))
        assert same, f"{s.name} ({s.doc}) / {entry}, {attempt}: {_first_difference(got_s, got_i, S, I)}"

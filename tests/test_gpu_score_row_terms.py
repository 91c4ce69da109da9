"""Pass 2 of the plain train step with its row terms in LDS, against the general kernels, bit for bit (MI355X).

`tt_retrieval_fwd_bwd_f32` without a sampling probability runs pass 2 as `score_kernel<D, 7, ...>` (csrc/score.hip,
MODE_BWD_S_NR).  At dim <= 128 that kernel stages `a_c` / `s_c` of ALL the streamed rows of its split into one LDS array in its
prologue (at most kRowTermRows = 4096 rows per split) and its tile loops read them from there; a split longer than the array takes
`score_kernel<D, 8, ...>` (MODE_BWD_S_NR_T), which stages them per tile.  Both fast forms address their per-tile loads from scalar
bases and test for the positive's tile on the scalar unit.  With an all-ones probability the same call runs the general kernels
(bias -0.0, which changes no sum).  All five outputs must agree in every bit, and a second run must repeat the first:

  * 96 x 96, dim 32: one split of three tiles, shorter than the prefetch distance (tail loop only);
  * 200 x 328, dim 64: ragged in both directions, three splits of 96 / 96 / 8 streamed rows;
  * 64 x 512, dim 128, the positives on the diagonal and shifted to the far end (diag_offset = 0 / 448);
  * 1024 x 1024, dim 128, with and without `sample_weight`: 16 splits, two tiles each;
  * 4096 x 4096, dim 64, weighted: 16 splits of eight tiles - the main loop over full tiles, the positive's tile inside it;
  * dim 256 (per-tile staging: the array is a dim <= 128 form), three-tile splits;
  * 4128 x 65536, dim 32: ONE split of 4128 streamed rows, more than the LDS array holds - asserted below through
    `tt_retrieval_num_splits` - so pass 2 runs the per-tile form.

(nq > nc is not a legal call of the entry - it requires nq + diag_offset <= nc - so there is no 512 x 64 case.)
"""
import numpy as np
import pytest
import torch

from oracle import synth
from test_gpu_parity import T
from two_tower_amazon_recommender_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROW_TERM_ROWS = 4096          # csrc/score.hip kRowTermRows
KEYS = ("loss", "lse", "per_row", "dq", "dc")


def _rows_per_split(nq, nc, d):
    ns = int(_lib.load().tt_retrieval_num_splits(nq, nc, d, 2))        # pass 2 streams the nq query rows in ns pieces
    return (-(-nq // ns) + 31) // 32 * 32


def _run(dev, q, c, off, prob, w):
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    ws = torch.empty(ops.retrieval_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=dev)
    lse = torch.empty(nq, device=dev); per_row = torch.empty(nq, device=dev); loss = torch.empty(1, device=dev)
    dq, dc = torch.full((nq, d), float("nan"), device=dev), torch.full((nc, d), float("nan"), device=dev)
    ops.retrieval_fwd_bwd(q, c, 10.0, ws, lse, per_row, loss, dq, dc, sample_weight=w, cand_prob=prob, diag_offset=off)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32) for k, v in zip(KEYS, (loss, lse, per_row, dq, dc))}


def _check(dev, nq, nc, d, off=0, weighted=False, seed=53):
    q = T(synth.uniform_f32(seed, 1, nq * d, -0.3, 0.6).reshape(nq, d), dev)
    c = T(synth.uniform_f32(seed, 2, nc * d, -0.3, 0.6).reshape(nc, d), dev)
    w = T(synth.uniform_f32(seed, 3, nq, 0.5, 1.0), dev) if weighted else None
    fast = _run(dev, q, c, off, None, w)
    again = _run(dev, q, c, off, None, w)
    general = _run(dev, q, c, off, torch.ones(nc, device=dev), w)
    for k in KEYS:
        d_gen, d_rep = int((fast[k] != general[k]).sum()), int((fast[k] != again[k]).sum())
        print(f"nq {nq} nc {nc} dim {d} off {off} w {weighted}: {k}: {d_gen} of {fast[k].size} words differ from the general "
              f"kernels, {d_rep} from the second run")
        assert d_gen == 0, (k, d_gen, fast[k].size)
        assert d_rep == 0, (k, d_rep, fast[k].size)
    for k in ("dq", "dc", "lse"):
        assert np.isfinite(fast[k].view(np.float32)).all(), k


@pytest.mark.parametrize("nq,nc,d,off,weighted", [
    (96, 96, 32, 0, False),
    (200, 328, 64, 0, False),
    (200, 328, 64, 128, False),
    (64, 512, 128, 0, False),
    (64, 512, 128, 448, False),
    (1024, 1024, 128, 0, False),
    (1024, 1024, 128, 0, True),
    (4096, 4096, 64, 0, True),
    (1056, 1056, 256, 0, False),
])
def test_row_terms_in_lds_match_the_general_kernels(dev, nq, nc, d, off, weighted):
    if d <= 128:
        assert _rows_per_split(nq, nc, d) <= ROW_TERM_ROWS
    _check(dev, nq, nc, d, off, weighted)


def test_a_split_longer_than_the_lds_array_takes_the_per_tile_form(dev):
    nq, nc, d = 4128, 65536, 32
    assert _rows_per_split(nq, nc, d) > ROW_TERM_ROWS, _rows_per_split(nq, nc, d)
    _check(dev, nq, nc, d, off=nc - nq)

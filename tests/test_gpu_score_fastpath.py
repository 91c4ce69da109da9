"""The plain train step's scorer instantiations against the general kernels, bit for bit (MI355X).

`tt_retrieval_fwd_bwd_f32` without a candidate sampling probability dispatches the fast forms (csrc/score.hip: MODE_FUSED_S_NC /
MODE_BWD_S_NR - no bias arithmetic, full tiles in a main loop without clamps, selects or masks, the ragged end in a tail loop).
With an all-ones probability the bias is -log2(1) = -0.0, which changes no sum it is added to, and the same call runs the general
kernels.  Both must give the same bits in `loss`, `lse`, the per-row loss, `dq` and `dc`:

  * dims 32 / 64 / 128 / 256 (at 32 and 256 only pass 2 has a fast form);
  * batches of full tiles only (1024, 8192) and with a ragged last tile (33, 1000, 4100, 8200);
  * the shapes of test_retrieval_odd_and_short_tile_counts whose splits are 2, 3 or 33 tiles long or empty (1056 = 33 tiles).

Every case also goes through test_gpu_parity.check_retrieval: the f64 oracle at the suite's usual bars.
"""
import numpy as np
import pytest
import torch

from oracle import synth
from test_gpu_parity import T, check_retrieval
from two_tower_amazon_recommender_amd import ops

pytestmark = pytest.mark.gpu

DIMS = (32, 64, 128, 256)
FULL_TILES = (1024, 8192)
RAGGED = (33, 1000, 4100, 8200)
ODD_AND_EMPTY_SPLITS = [(160, 160, 128), (1056, 1056, 128), (96, 96, 256), (1056, 1056, 256), (1120, 1184, 64)]


def _run(dev, q, c, off, prob):
    nq, nc, d = q.shape[0], c.shape[0], q.shape[1]
    ws = torch.empty(ops.retrieval_workspace_bytes(nq, nc, d), dtype=torch.uint8, device=dev)
    lse = torch.empty(nq, device=dev); per_row = torch.empty(nq, device=dev); loss = torch.empty(1, device=dev)
    dq, dc = torch.full((nq, d), float("nan"), device=dev), torch.full((nc, d), float("nan"), device=dev)
    ops.retrieval_fwd_bwd(q, c, 10.0, ws, lse, per_row, loss, dq, dc, cand_prob=prob, diag_offset=off)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32) for k, v in (("loss", loss), ("lse", lse), ("per_row", per_row), ("dq", dq), ("dc", dc))}


def _bit_identical(dev, nq, nc, d, off=0, seed=47):
    q = T(synth.uniform_f32(seed, 1, nq * d, -0.3, 0.6).reshape(nq, d), dev)
    c = T(synth.uniform_f32(seed, 2, nc * d, -0.3, 0.6).reshape(nc, d), dev)
    fast = _run(dev, q, c, off, None)
    general = _run(dev, q, c, off, torch.ones(nc, device=dev))
    for k in fast:
        diff = int((fast[k] != general[k]).sum())
        print(f"nq {nq} nc {nc} dim {d} off {off}: {k}: {diff} of {fast[k].size} words differ")
        assert diff == 0, (k, diff, fast[k].size)
    assert not np.isnan(fast["dq"].view(np.float32)).any() and not np.isnan(fast["dc"].view(np.float32)).any()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", FULL_TILES + RAGGED)
def test_fast_forms_match_the_general_kernels_bit_for_bit(dev, n, d):
    _bit_identical(dev, n, n, d)
    check_retrieval(dev, n, n, d)


@pytest.mark.parametrize("nq,nc,d", ODD_AND_EMPTY_SPLITS)
def test_fast_forms_match_on_odd_short_and_empty_splits(dev, nq, nc, d):
    _bit_identical(dev, nq, nc, d, off=nc - nq)
    check_retrieval(dev, nq, nc, d, off=nc - nq)

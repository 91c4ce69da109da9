"""Pass 1 of the plain train step with its column splits inside the workgroup, against the slab path, bit for bit (MI355X).

`tt_retrieval_fwd_bwd_f32` at dim 128 without a sampling probability, ids or hard negatives, where pass 1 cuts the candidates 8
ways (`tt_retrieval_num_splits(nq, nc, 128, 0) == 8`), runs pass 1 as `score_rowfrag_kernel<128>` (csrc/score.hip,
MODE_FUSED_S_WG): one 32-row fragment per workgroup, wave w = split w on a private LDS tile, the 8 partial results combined in
LDS by the kernel itself - no slab, no `fused_combine_kernel` launch.  With an all-ones probability the same call runs the general
slab kernels and the combine launch (bias -0.0, which changes no sum).  All five outputs must agree in every bit and a second run
must repeat the first; dq is pre-filled with NaN, so a row or column the new form leaves unwritten shows.

That the new form really ran is asserted per call through the library's own launch tags: under `score_aux` the slab path records
two launches (the combine and the dc slab reduction), the new form one.

  * 32 x 512: one fragment, splits of two tiles (tail loop only);
  * 33 x 575: ragged rows, a ragged last split of three tiles and two EMPTY splits; also with the positives at the far end;
  * 64 x 512, diag_offset 0 / 448: the positive's tile in the first and in the last wave;
  * 250 x 560: 8 fragments, the last ragged, weighted;
  * 7700 x 7712: splits of 31 tiles (the last 24) - the main loop over full tiles with the positive's tile inside it, a ragged
    last fragment and a ragged last split; with and without `sample_weight`.  (A long split and 8 splits only coincide from
    7681 rows up.)
"""
import numpy as np
import pytest
import torch

from oracle import synth, two_tower as tt
from test_gpu_parity import T
from two_tower_amazon_recommender_amd import _lib, ops

pytestmark = pytest.mark.gpu

D = 128
KEYS = ("loss", "lse", "per_row", "dq", "dc")


def _run(dev, q, c, off, prob, w):
    """(the five outputs as 32-bit words, launches recorded under `score_aux`)"""
    nq, nc = q.shape[0], c.shape[0]
    ws = torch.empty(ops.retrieval_workspace_bytes(nq, nc, D), dtype=torch.uint8, device=dev)
    lse = torch.empty(nq, device=dev); per_row = torch.empty(nq, device=dev); loss = torch.empty(1, device=dev)
    dq, dc = torch.full((nq, D), float("nan"), device=dev), torch.full((nc, D), float("nan"), device=dev)
    _lib.profile_enable("score_aux", 16)
    try:
        ops.retrieval_fwd_bwd(q, c, 10.0, ws, lse, per_row, loss, dq, dc, sample_weight=w, cand_prob=prob, diag_offset=off)
        torch.cuda.synchronize()
        aux = _lib.profile_read("score_aux", 16)[1]
    finally:
        _lib.profile_enable("")
    return {k: v.cpu().numpy().view(np.uint32) for k, v in zip(KEYS, (loss, lse, per_row, dq, dc))}, aux


def _check(dev, q, c, off=0, w=None):
    nq, nc = q.shape[0], c.shape[0]
    assert int(_lib.load().tt_retrieval_num_splits(nq, nc, D, 0)) == 8
    new, aux_new = _run(dev, q, c, off, None, w)
    again, aux_again = _run(dev, q, c, off, None, w)
    slab, aux_slab = _run(dev, q, c, off, torch.ones(nc, device=dev), w)
    print(f"nq {nq} nc {nc} off {off} w {w is not None}: score_aux launches {aux_new} / {aux_again} (in-workgroup), {aux_slab} (slab path)")
    assert aux_new == 1 and aux_again == 1, (aux_new, aux_again)     # the dc slab reduction alone: no combine launch
    assert aux_slab == 2, aux_slab                                    # fused_combine_kernel + the dc slab reduction
    for k in KEYS:
        d_slab, d_rep = int((new[k] != slab[k]).sum()), int((new[k] != again[k]).sum())
        print(f"    {k}: {d_slab} of {new[k].size} words differ from the slab path, {d_rep} from the second run")
        assert d_slab == 0, (k, d_slab, new[k].size)
        assert d_rep == 0, (k, d_rep, new[k].size)
    for k in ("dq", "dc", "lse"):
        assert np.isfinite(new[k].view(np.float32)).all(), k
    return new


def _inputs(dev, nq, nc, weighted, seed=59):
    q = T(synth.uniform_f32(seed, 1, nq * D, -0.3, 0.6).reshape(nq, D), dev)
    c = T(synth.uniform_f32(seed, 2, nc * D, -0.3, 0.6).reshape(nc, D), dev)
    w = T(synth.uniform_f32(seed, 3, nq, 0.5, 1.0), dev) if weighted else None
    return q, c, w


@pytest.mark.parametrize("nq,nc,off,weighted", [
    (32, 512, 0, False),
    (33, 575, 0, False),
    (33, 575, 542, False),
    (64, 512, 0, False),
    (64, 512, 448, False),
    (250, 560, 0, True),
    (7700, 7712, 0, False),
    (7700, 7712, 0, True),
])
def test_splits_inside_the_workgroup_match_the_slab_path(dev, nq, nc, off, weighted):
    q, c, w = _inputs(dev, nq, nc, weighted)
    _check(dev, q, c, off, w)


def test_lazy_rescale_branch_is_exercised_in_the_workgroup_form(dev):
    """The online softmax rescales its accumulators only when a row maximum grows by more than 2^8.  Every split's first tile does
    that trivially (from -1e30); here a candidate in the SECOND tile of a split has a logit ~75 (log2 units: ~108) above everything
    before it, for one query each in the first, a middle and the last split's wave (wave-uniform branch, per-lane factors).
    Bit for bit against the slab path, and against the f64 oracle at the 1e-4 of test_fused_online_rescale_branch_is_exercised."""
    nq, nc = 64, 512                                      # 8 splits of 64 candidates = two tiles each
    q = synth.uniform_f32(46, 1, nq * D, -0.3, 0.6).reshape(nq, D)
    c = synth.uniform_f32(46, 2, nc * D, -0.3, 0.6).reshape(nc, D)
    for row, col in ((5, 40), (37, 300), (63, 511)):     # second tiles of splits 0, 4 and 7
        c[col] = 3.0 * q[row] / np.linalg.norm(q[row]) ** 2 * 2.5      # q_row . c_col = 7.5 -> logit 75
    out = _check(dev, T(q, dev), T(c, dev))
    f = {k: v.view(np.float32) for k, v in out.items()}
    rl, _, rlse = tt.retrieval_loss(q, c, temperature=0.1)
    rdq, rdc = tt.retrieval_grad(q, c, temperature=0.1)
    assert abs(float(f["loss"][0]) - rl) <= 1e-4 * abs(rl)
    assert np.abs(f["lse"] - rlse).max() <= 1e-4 * np.abs(rlse).max()
    assert np.abs(f["dq"].reshape(nq, D) - rdq).max() <= 1e-4 * np.abs(rdq).max()
    assert np.abs(f["dc"].reshape(nc, D) - rdc).max() <= 1e-4 * np.abs(rdc).max()

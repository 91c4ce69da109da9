"""Pass 2 (dc) of the plain train step with its 8 query splits inside the workgroup, against the slab path, bit for bit (MI355X).

`tt_retrieval_fwd_bwd_f32` at dim 128 without a sampling probability, ids or hard negatives, where the dc pass cuts the queries 8
ways (`tt_retrieval_num_splits(nq, nc, 128, 2) == 8`) into splits of whole tiles (`nq == 8 * c_per_split`), runs the dc pass as
`score_colfrag_kernel<128>` (csrc/score.hip, MODE_BWD_S_WG): one 32-candidate fragment per workgroup, wave w = split w on a private
LDS tile, the 8 partial blocks summed in LDS in split order by the kernel itself, which also sums the per-row losses - no slab, no
`reduce_slabs_kernel` launch.  With an all-ones probability the same call runs the general slab kernels and both small launches
(bias -0.0, which changes no sum).  All five outputs must agree in every bit and a second run must repeat the first; dq and dc
are pre-filled with NaN, so a row or column the new form leaves unwritten shows.

Which form ran is asserted per call through the library's own launch tags, under `score_aux`: the slab path records two launches
(pass 1's combine and the dc slab reduction), the new form none - or one, where pass 1 itself is on the slab path.

  * 512 x 512: 16 fragments, splits of two tiles; the positive's tile lands in every wave (fragment f's in wave f / 2);
  * 512 x 545, diag_offset 0 / 33: a ragged last fragment of c (one valid candidate), with and without a positive;
  * 512 x 1000, weighted: pass 1 cuts the candidates 15 ways (slab path + combine launch) while pass 2 takes the new form;
  * 7936 x 7936: splits of 31 tiles - an odd count, the prefetch at its full depth;
  * 8192 x 8192, weighted: splits of 32 tiles (the benchmark's shape);
  * 7700 x 7712: 8 splits, but 7700 rows are no whole tiles - not eligible, the reduction launch must be recorded.
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
    lse = torch.empty(nq, device=dev); per_row = torch.empty(nq, device=dev); loss = torch.full((1,), float("nan"), device=dev)
    dq, dc = torch.full((nq, D), float("nan"), device=dev), torch.full((nc, D), float("nan"), device=dev)
    _lib.profile_enable("score_aux", 16)
    try:
        ops.retrieval_fwd_bwd(q, c, 10.0, ws, lse, per_row, loss, dq, dc, sample_weight=w, cand_prob=prob, diag_offset=off)
        torch.cuda.synchronize()
        aux = _lib.profile_read("score_aux", 16)[1]
    finally:
        _lib.profile_enable("")
    return {k: v.cpu().numpy().view(np.uint32) for k, v in zip(KEYS, (loss, lse, per_row, dq, dc))}, aux


def _inputs(dev, nq, nc, weighted, seed=61):
    q = T(synth.uniform_f32(seed, 1, nq * D, -0.3, 0.6).reshape(nq, D), dev)
    c = T(synth.uniform_f32(seed, 2, nc * D, -0.3, 0.6).reshape(nc, D), dev)
    w = T(synth.uniform_f32(seed, 3, nq, 0.5, 1.0), dev) if weighted else None
    return q, c, w


def _check(dev, q, c, off, w, aux_expected):
    nq, nc = q.shape[0], c.shape[0]
    assert int(_lib.load().tt_retrieval_num_splits(nq, nc, D, 2)) == 8
    new, aux_new = _run(dev, q, c, off, None, w)
    again, aux_again = _run(dev, q, c, off, None, w)
    slab, aux_slab = _run(dev, q, c, off, torch.ones(nc, device=dev), w)
    print(f"nq {nq} nc {nc} off {off} w {w is not None}: score_aux launches {aux_new} / {aux_again} (no probability), {aux_slab} (slab path)")
    assert aux_new == aux_expected and aux_again == aux_expected, (aux_new, aux_again, aux_expected)
    assert aux_slab == 2, aux_slab                                    # fused_combine_kernel + the dc slab reduction
    for k in KEYS:
        d_slab, d_rep = int((new[k] != slab[k]).sum()), int((new[k] != again[k]).sum())
        print(f"    {k}: {d_slab} of {new[k].size} words differ from the slab path, {d_rep} from the second run")
        assert d_slab == 0, (k, d_slab, new[k].size)
        assert d_rep == 0, (k, d_rep, new[k].size)
    assert np.isfinite(new["dc"].view(np.float32)).all()
    return new


@pytest.mark.parametrize("nq,nc,off,weighted,aux_new", [
    (512, 512, 0, False, 0),
    (512, 545, 0, False, 0),
    (512, 545, 33, False, 0),
    (512, 1000, 0, True, 1),            # pass 1: 15 splits, the slab path and its combine launch
    (7936, 7936, 0, False, 0),
    (8192, 8192, 0, True, 0),
])
def test_query_splits_inside_the_workgroup_match_the_slab_path(dev, nq, nc, off, weighted, aux_new):
    q, c, w = _inputs(dev, nq, nc, weighted)
    _check(dev, q, c, off, w, aux_new)


def test_in_workgroup_form_against_the_f64_oracle(dev):
    """dc and the loss of the new form at 512 x 512 against the f64 restatement, at the project's 1e-4 bars."""
    nq = nc = 512
    q = synth.uniform_f32(62, 1, nq * D, -0.3, 0.6).reshape(nq, D)
    c = synth.uniform_f32(62, 2, nc * D, -0.3, 0.6).reshape(nc, D)
    out, aux = _run(dev, T(q, dev), T(c, dev), 0, None, None)
    assert aux == 0, aux
    f = {k: v.view(np.float32) for k, v in out.items()}
    rl, _, _ = tt.retrieval_loss(q, c, temperature=0.1)
    _, rdc = tt.retrieval_grad(q, c, temperature=0.1)
    err_loss, err_dc = abs(float(f["loss"][0]) - rl) / abs(rl), np.abs(f["dc"].reshape(nc, D) - rdc).max() / np.abs(rdc).max()
    print(f"loss {float(f['loss'][0])} (oracle {rl}, relative error {err_loss:.3g}); dc: {err_dc:.3g} of its maximum")
    assert err_loss <= 1e-4
    assert err_dc <= 1e-4


def test_splits_of_ragged_tiles_keep_the_slab_path_and_its_reduction(dev):
    """7700 x 7712 has 8 dc splits, but 7700 query rows do not cut into 8 splits of whole tiles: the dc pass stays on the slab path,
    so the reduction launch is recorded (pass 1 takes its in-workgroup form there: no combine launch)."""
    nq, nc = 7700, 7712
    assert int(_lib.load().tt_retrieval_num_splits(nq, nc, D, 2)) == 8
    q, c, _ = _inputs(dev, nq, nc, False)
    _, aux = _run(dev, q, c, 0, None, None)
    assert aux == 1, aux

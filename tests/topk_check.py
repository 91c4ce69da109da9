"""Tie-aware checker of a top-k answer against f64 scores (shared by test_topk_cpu.py and test_gpu_topk.py).

With t the f64 k-th best score of a query (over the candidates that are not excluded) and eps = 1e-5 * max_j sum_d |q_d c_jd|:
every candidate scoring above t + eps must be returned, none scoring below t - eps may be, returned scores lie within eps
of their f64 value and never increase along the list, no index repeats, and no excluded index appears.  When fewer than k
candidates remain the tail must be (-inf, -1).  Works on torch tensors on any device (f64 on the device for big shapes).
"""
import torch


def check_topk(q, c, k, scores, idx, excluded=None, chunk=256):
    """q [nq, D], c [nc, D] (f32), scores [nq, k] f32, idx [nq, k] int64; excluded: optional list of per-query iterables of
    candidate indices.  Raises AssertionError with the first violation."""
    dev = c.device
    c64 = c.to(dev, torch.float64)
    ca = c64.abs()
    nq = q.shape[0]
    scores, idx = scores.to(dev), idx.to(dev)
    for s in range(0, nq, chunk):
        e = min(s + chunk, nq)
        q64 = q[s:e].to(dev, torch.float64)
        S = q64 @ c64.T
        eps = 1e-5 * (q64.abs() @ ca.T).amax(dim=1)
        for r in range(e - s):
            row = S[r].clone()
            ex = excluded[s + r] if excluded is not None else ()
            ex = torch.as_tensor([x for x in ex if 0 <= x < c.shape[0]], dtype=torch.int64, device=dev)
            if ex.numel():
                row[ex] = float("-inf")
            avail = int(torch.isfinite(row).sum())
            got_i, got_s = idx[s + r], scores[s + r]
            nreal = min(k, avail)
            assert bool((got_i[nreal:] == -1).all()) and bool(torch.isneginf(got_s[nreal:]).all()), \
                f"query {s + r}: tail past {nreal} is not (-inf, -1)"
            gi, gs = got_i[:nreal], got_s[:nreal].to(torch.float64)
            assert bool((gi >= 0).all()) and bool((gi < c.shape[0]).all()), f"query {s + r}: index out of range"
            assert torch.unique(gi).numel() == nreal, f"query {s + r}: duplicate indices"
            if ex.numel():
                assert not bool(torch.isin(gi, ex).any()), f"query {s + r}: an excluded index was returned"
            if nreal == 0:
                continue
            t = torch.topk(row, nreal).values[-1]
            ep = float(eps[r])
            must = torch.nonzero(row > t + ep).flatten()
            assert bool(torch.isin(must, gi).all()), f"query {s + r}: a candidate above t + eps is missing"
            ref = row[gi]
            assert bool((ref >= t - ep).all()), f"query {s + r}: a candidate below t - eps was returned"
            assert bool(((gs - ref).abs() <= ep).all()), f"query {s + r}: returned scores differ from f64 by more than eps"
            assert bool((gs[1:] <= gs[:-1]).all()), f"query {s + r}: scores increase along the list"

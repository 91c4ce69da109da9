"""The pairwise retrieval losses without a GPU: the f64 restatement of tests/pairwise_check.py against an f64 torch-autograd
matrix form, its edge cases, the C ABI's symbols and argument contract (host buffers stand in for device memory: every call
returns from validation before anything is launched), the workspace query, and config / YAML / CLI parsing."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import pairwise_check as pc
from two_tower_amazon_recommender_amd import _lib, config as cfgmod, ops, tasks, train
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig, _GRAPH_REFUSALS

INVALID, WORKSPACE = _lib.TT_ERR_INVALID_ARG, _lib.TT_ERR_WORKSPACE
# the shapes the margin search was checked on (the issue): q, c ~ U(-1, 1) / sqrt(D) in f32, inv_t = 10, p ~ U(1e-4, 0.2)
SHAPES = [(33, 33, 32, 0), (100, 131, 128, 31), (257, 300, 256, 0), (64, 64, 64, 0), (96, 160, 64, 64), (130, 515, 128, 7),
          (300, 557, 256, 257)]


def _inputs(shape, seed=0):
    nq, nc, d, _ = shape
    rng = np.random.default_rng(seed)
    q = (rng.uniform(-1, 1, (nq, d)) / np.sqrt(d)).astype(np.float32)
    c = (rng.uniform(-1, 1, (nc, d)) / np.sqrt(d)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, nq)
    w[::7] = 0.0
    p = rng.uniform(1e-4, 0.2, nc).astype(np.float32)
    ids = rng.integers(0, max(nc * 5, 2), nc).astype(np.int64)
    ids[(shape[3] + 1) % nc] = ids[shape[3]]
    return q, c, w, p, ids


def _autograd(q, c, kind, margin, reduction, inv_t, w, p, ids, thr, off, grad_scale):
    """The matrix form in f64 torch autograd: the mask is data, the loss a function of q and c."""
    tq, tc = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (q, c))
    nq = q.shape[0]
    s = tq @ tc.t() * inv_t
    if p is not None:
        s = s - torch.log(torch.clamp(torch.tensor(p.astype(np.float64)), 1e-6, 1.0))[None, :]
    rows = torch.arange(nq)
    x = s[rows, rows + off][:, None] - s
    valid = torch.from_numpy(pc.pairs(q, c, inv_t, p, ids, thr, off)[2])
    phi = torch.nn.functional.softplus(-x) if kind == "logistic" else torch.clamp(margin - x, min=0.0)
    n = valid.sum(1).to(torch.float64)
    r = 1.0 / torch.clamp(n, min=1.0) if reduction == "mean" else torch.ones(nq, dtype=torch.float64)
    wt = torch.ones(nq, dtype=torch.float64) if w is None else torch.tensor(w)
    per_row = wt * r * torch.where(valid, phi, torch.zeros_like(phi)).sum(1)
    (grad_scale * per_row.sum()).backward()
    return float(per_row.sum().detach()), per_row.detach().numpy(), tq.grad.numpy(), tc.grad.numpy()


@pytest.mark.parametrize("kind", ["logistic", "hinge"])
@pytest.mark.parametrize("shape", SHAPES[:4] + [SHAPES[5]], ids=str)
def test_restatement_equals_the_autograd_matrix_form(shape, kind):
    q, c, w, p, ids = _inputs(shape)
    off = shape[3]
    s, _, cand, _ = pc.pairs(q, c, 10.0, p, ids, None, off)
    thr = np.sort(np.where(cand, s, -np.inf), axis=1)[:, -3:-1].mean(1)       # between the 2nd and 3rd highest negative
    for reduction in ("mean", "sum"):
        for kw in (dict(w=None, p=None, ids=None, thr=None), dict(w=w, p=p, ids=ids, thr=thr)):
            margin = pc.pick_margin(*pc.pairs(q, c, 10.0, kw["p"], kw["ids"], kw["thr"], off)[3:1:-1])
            want = _autograd(q, c, kind, margin, reduction, 10.0, off=off, grad_scale=2.0, **kw)
            loss, per_row, n = pc.loss(q, c, kind, margin, reduction, 10.0, off=off, **kw)
            dq, dc = pc.grads(q, c, kind, margin, reduction, 10.0, off=off, grad_scale=2.0, **kw)
            assert abs(loss - want[0]) <= 1e-12 * abs(want[0]) and np.allclose(per_row, want[1], rtol=1e-12, atol=1e-14)
            assert np.allclose(dq, want[2], rtol=1e-10, atol=1e-13) and np.allclose(dc, want[3], rtol=1e-10, atol=1e-13)
            if kw["thr"] is not None:
                assert n.max() <= 2


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_margin_clear_of_every_pair_exists(shape):
    q, c, _, p, _ = _inputs(shape, seed=3)
    for prob in (None, p):
        _, _, valid, x = pc.pairs(q, c, 10.0, prob, None, None, shape[3])
        m = pc.pick_margin(x, valid)
        assert 0.5 <= m < 0.6 and np.abs(m - x[valid]).min() >= pc.GAP
        # the f32 logits' error on these inputs is far inside the gap
        s32 = (q @ c.T * np.float32(10.0)).astype(np.float64)
        s64 = q.astype(np.float64) @ c.astype(np.float64).T * 10.0
        assert np.abs(s32 - s64).max() <= 2e-6
    with pytest.raises(AssertionError):
        pc.pick_margin(np.arange(0.5, 0.6, 1e-5))


def test_rows_without_negatives_zero_weights_and_the_two_reductions():
    q, c, w, p, ids = _inputs((33, 33, 32, 0))
    for kind in ("logistic", "hinge"):
        # nc == 1, and every negative masked: n_i = 0, no loss, no gradient
        loss, per_row, n = pc.loss(q[:1], c[:1], kind, 0.5)
        assert loss == 0.0 and n[0] == 0 and not np.any(pc.grads(q[:1], c[:1], kind, 0.5)[0])
        same = np.zeros(33, dtype=np.int64)
        loss, per_row, n = pc.loss(q, c, kind, 0.5, ids=same)
        dq, dc = pc.grads(q, c, kind, 0.5, ids=same)
        assert loss == 0.0 and not n.any() and not dq.any() and not dc.any()
        # w_i = 0: the row has no loss and q_i no gradient; the other rows are as without it
        loss_w, rows_w, _ = pc.loss(q, c, kind, 0.5, w=w, inv_t=10.0)
        _, rows_1, n = pc.loss(q, c, kind, 0.5, inv_t=10.0)
        dq, _ = pc.grads(q, c, kind, 0.5, w=w, inv_t=10.0)
        assert not rows_w[::7].any() and not dq[::7].any() and np.allclose(rows_w, w * rows_1)
        # sum = mean times the row's number of negatives
        _, rows_s, _ = pc.loss(q, c, kind, 0.5, "sum", inv_t=10.0)
        assert (n == 32).all() and np.allclose(rows_s, 32 * rows_1)
        gs, gm = pc.grads(q, c, kind, 0.5, "sum", inv_t=10.0), pc.grads(q, c, kind, 0.5, "mean", inv_t=10.0)
        assert np.allclose(gs[0], 32 * gm[0]) and np.allclose(gs[1], 32 * gm[1])
    with pytest.raises(ValueError):
        pc.loss(q, c, "triplet")
    with pytest.raises(ValueError):
        pc.loss(q, c, "hinge", reduction="batch")


# ------------------------------------------------------------------------------------------------- the C ABI
_P, _I64, _I32, _F = C.c_void_p, C.c_int64, C.c_int32, C.c_float
_LOSS = "q c nq nc dim diag_offset inv_temperature sample_weight cand_prob cand_ids hard_thr".split()
_TAIL = "kind margin reduction stream".split()
ENTRIES = {"tt_retrieval_pairwise_fwd_f32": (_LOSS + "ws ws_bytes per_row loss".split() + _TAIL, ["per_row", "loss"]),
           "tt_retrieval_pairwise_fwd_bwd_f32": (_LOSS + "grad_scale ws ws_bytes per_row loss dq dc".split() + _TAIL,
                                                 ["per_row", "loss", "dq", "dc"])}
NQ, NC, DIM, OFF = 100, 131, 128, 31


def test_symbols_and_signatures_are_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.tt_abi_version() == 10
    base = [_P, _P, _I64, _I64, _I32, _I64, _F, _P, _P, _P, _P]
    tail = [_I32, _F, _I32, _P]
    assert _lib.SIGNATURES["tt_retrieval_pairwise_workspace_bytes"] == (_I64, [_I64, _I64, _I32])
    assert _lib.SIGNATURES["tt_retrieval_pairwise_fwd_f32"] == (C.c_int, base + [_P, _I64, _P, _P] + tail)
    assert _lib.SIGNATURES["tt_retrieval_pairwise_fwd_bwd_f32"] == (C.c_int, base + [_F, _P, _I64, _P, _P, _P, _P] + tail)
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ops.PAIRWISE_KINDS == {"logistic": 0, "hinge": 1} and ops.PAIRWISE_REDUCTIONS == {"mean": 0, "sum": 1}
    header = (_lib._PKG.parent / "include" / "twotower_hip.h").read_text()
    for name in list(ENTRIES) + ["tt_retrieval_pairwise_workspace_bytes", "#define TT_PAIRWISE_HINGE 1", "#define TT_PAIRWISE_SUM 1"]:
        assert name in header, name


def _buf(n, align=256):
    raw = (C.c_uint8 * (n + align))()
    return raw, (C.addressof(raw) + align - 1) // align * align


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_validates_arguments_before_any_launch(name):
    lib = _lib.load()
    params, own = ENTRIES[name]
    big = max(NQ, NC)
    keep = {k: _buf(n) for k, n in dict(q=big * 256 * 4, c=big * 256 * 4, dq=NQ * DIM * 4, dc=NC * DIM * 4, per_row=NQ * 4, loss=4,
                                        ws=max(lib.tt_retrieval_pairwise_workspace_bytes(a, b, d) for a, b in ((NQ, NC), (NC, NQ))
                                               for d in (32, 64, 128, 256))).items()}
    vals = {k: v[1] for k, v in keep.items()}
    vals.update(nq=NQ, nc=NC, dim=DIM, diag_offset=OFF, inv_temperature=10.0, grad_scale=1.0, sample_weight=None, cand_prob=None,
                cand_ids=None, hard_thr=None, stream=None, kind=1, margin=0.5, reduction=0)
    fn = getattr(lib, name)

    def call(**kw):
        v = dict(vals, **kw)
        if "ws_bytes" not in v:
            v["ws_bytes"] = lib.tt_retrieval_pairwise_workspace_bytes(v["nq"], v["nc"], v["dim"]) if v["nq"] > 0 else 1 << 20
        return fn(*[v[p] for p in params]), lib.tt_last_error().decode()

    cases = [({p: None}, INVALID, "null") for p in ["q", "c", "ws"] + own]
    cases += [(dict(nq=0), INVALID, "positive"), (dict(dim=48), INVALID, "dim 48"),
              (dict(q=vals["q"] + 4), INVALID, "q/c must be 16-byte aligned"), (dict(c=vals["c"] + 4), INVALID, "q/c must be 16-byte aligned"),
              (dict(ws=vals["ws"] + 16), INVALID, "256-byte aligned"),
              (dict(diag_offset=-1), INVALID, "diag_offset"), (dict(diag_offset=NC - NQ + 1), INVALID, "diag_offset"),
              (dict(nq=NC, nc=NQ, diag_offset=0), INVALID, "diag_offset"),
              (dict(kind=2), INVALID, "kind 2"), (dict(kind=-1), INVALID, "kind -1"),
              (dict(margin=float("nan")), INVALID, "margin must be finite"), (dict(margin=float("inf")), INVALID, "margin must be finite"),
              (dict(reduction=2), INVALID, "reduction 2")]
    if "dq" in params:
        cases += [(dict(dq=vals["dq"] + 4), INVALID, "dq/dc must be 16-byte aligned"), (dict(dc=vals["dc"] + 4), INVALID, "dq/dc must be 16-byte aligned")]
    for kw, code, word in cases:
        got, msg = call(**kw)
        assert got == code, (name, kw, got, msg)
        assert word in msg and msg.startswith(name + ":"), (name, kw, msg)
    need = lib.tt_retrieval_pairwise_workspace_bytes(NQ, NC, DIM)
    got, msg = call(ws_bytes=need - 1)
    assert got == WORKSPACE and f"workspace {need - 1} < {need} bytes" in msg and msg.startswith(name + ":"), msg


def test_workspace_query():
    f, full = ops.retrieval_pairwise_workspace_bytes, ops.retrieval_workspace_bytes
    for bad in [(0, 10, 32), (10, 0, 32), (10, 10, 0), (-1, 5, 32)]:
        assert f(*bad) == 0, bad
    for nq, nc, d, _ in SHAPES + [(1, 1, 32, 0), (32, 64, 32, 32), (8192, 8192, 64, 0), (8192, 8192, 128, 0), (8192, 8192, 256, 0),
                                  (2048, 65536, 128, 0), (8200, 8200, 128, 0)]:
        n = f(nq, nc, d)
        # no [nq, nc] array: below the scorer's workspace, which keeps one (the issue's bound, without the row-term allowance)
        assert n > 0 and n % 256 == 0 and n <= full(nq, nc, d), (nq, nc, d, n)
    assert f(8192, 8192, 128) < 4 * 8192 * 8192 // 4


# ------------------------------------------------------------------------------------------------- config, YAML, CLI, task
def _doc(loss=None):
    rt = {"temperature": 0.1}
    if loss is not None:
        rt["loss"] = loss
    return {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32], "retrieval": rt}}


def test_config_and_yaml():
    cfg = TwoTowerConfig(n_users=10, n_items=10)
    assert (cfg.retrieval_loss, cfg.pairwise_margin, cfg.pairwise_reduction) == ("softmax", 1.0, "mean")
    TwoTowerConfig(n_users=10, n_items=10, retrieval_loss="hinge", pairwise_margin=0.3, pairwise_reduction="sum").validate()
    for kw, word in ((dict(retrieval_loss="triplet"), "retrieval_loss"), (dict(pairwise_margin=float("nan")), "pairwise_margin"),
                     (dict(pairwise_margin="1"), "pairwise_margin"), (dict(pairwise_reduction="batch"), "pairwise_reduction"),
                     (dict(retrieval_loss="bpr", scorer_precision="bf16x3", tower_dims=[64, 128]), "scorer_precision='f32'")):
        with pytest.raises(ValueError, match=word):
            TwoTowerConfig(n_users=10, n_items=10, **kw).validate()
    assert cfgmod.retrieval_loss_from_dict(_doc()) == {"kind": "softmax", "margin": 1.0, "reduction": "mean"}
    assert cfgmod.retrieval_loss_from_dict(_doc({"kind": "hinge", "margin": 0.25})) == {"kind": "hinge", "margin": 0.25, "reduction": "mean"}
    cfg, _ = cfgmod.model_config_from_dict(_doc({"kind": "bpr", "reduction": "sum"}), 10, 10)
    assert (cfg.retrieval_loss, cfg.pairwise_margin, cfg.pairwise_reduction) == ("bpr", 1.0, "sum")
    assert cfgmod.model_config_from_dict(_doc(), 10, 10)[0].retrieval_loss == "softmax"
    for block, word in (({"kind": "bpr", "gamma": 1}, "unknown keys"), ({"kind": "mse"}, "kind"), ({"margin": "x"}, "margin"),
                        ({"margin": float("inf")}, "margin"), ({"reduction": "batch"}, "reduction"), ("bpr", "mapping")):
        with pytest.raises(ValueError, match=word):
            cfgmod.retrieval_loss_from_dict(_doc(block))
    # graph replay refuses the option through the table; the checkpoint's config carries it, one without the keys is softmax
    hits = [what for refused, what in _GRAPH_REFUSALS if refused(TwoTowerConfig(n_users=10, n_items=10, retrieval_loss="bpr"))]
    assert len(hits) == 1 and "pairwise retrieval loss" in hits[0]
    assert not any(refused(TwoTowerConfig(n_users=10, n_items=10)) for refused, _ in _GRAPH_REFUSALS)
    saved = dict(TwoTowerConfig(n_users=10, n_items=10, retrieval_loss="hinge", pairwise_margin=0.3).__dict__)
    back = TwoTowerConfig(**saved)
    assert (back.retrieval_loss, back.pairwise_margin) == ("hinge", 0.3)
    old = {k: v for k, v in saved.items() if k not in ("retrieval_loss", "pairwise_margin", "pairwise_reduction")}
    assert TwoTowerConfig(**old).retrieval_loss == "softmax"


def test_cli_options_and_refusals():
    base = ["--config", "x.yaml", "--synthetic", "600"]
    a = train.parse(base)
    assert (a.retrieval_loss, a.pairwise_margin, a.pairwise_reduction) == (None, None, None)
    assert train.retrieval_loss_settings(a, _doc(), False) == {"kind": "softmax", "margin": 1.0, "reduction": "mean"}
    a = train.parse(base + ["--retrieval-loss", "hinge", "--pairwise-margin", "0.25", "--pairwise-reduction", "sum"])
    assert train.retrieval_loss_settings(a, _doc({"kind": "bpr"}), False) == {"kind": "hinge", "margin": 0.25, "reduction": "sum"}
    a = train.parse(base + ["--pairwise-margin", "0.25"])                      # the YAML's kind, the CLI's margin
    assert train.retrieval_loss_settings(a, _doc({"kind": "hinge"}), False)["margin"] == 0.25
    with pytest.raises(SystemExit, match="need a pairwise loss"):
        train.retrieval_loss_settings(a, _doc(), False)
    with pytest.raises(SystemExit, match="finite"):
        train.retrieval_loss_settings(train.parse(base + ["--retrieval-loss", "hinge", "--pairwise-margin", "nan"]), _doc(), False)
    with pytest.raises(SystemExit, match="f32"):
        train.retrieval_loss_settings(train.parse(base + ["--retrieval-loss", "bpr", "--scorer-precision", "bf16x3"]), _doc(), False)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        train.retrieval_loss_settings(train.parse(base + ["--retrieval-loss", "bpr"]), _doc(), True)
    train.retrieval_loss_settings(train.parse(base), _doc(), True)              # softmax: the sharded trainer as ever
    with pytest.raises(SystemExit):
        train.parse(base + ["--retrieval-loss", "mse"])
    assert isinstance(a, argparse.Namespace)


def test_task_loss_objects():
    assert tasks.BPRLoss is tasks.PairwiseLogisticLoss
    lo = tasks.PairwiseHingeLoss()
    assert (lo.kind, lo.margin, lo.reduction) == ("hinge", 1.0, "mean")
    assert (tasks.BPRLoss(reduction="SUM").kind, tasks.BPRLoss(reduction="SUM").reduction) == ("logistic", "sum")
    for bad in (lambda: tasks.PairwiseHingeLoss(float("nan")), lambda: tasks.PairwiseHingeLoss(reduction="batch"),
                lambda: tasks.BPRLoss(reduction="none")):
        with pytest.raises(ValueError):
            bad()
    tasks.Retrieval(loss=tasks.BPRLoss(), temperature=0.1, remove_accidental_hits=True, num_hard_negatives=5)
    tasks.Retrieval(loss=tasks.PairwiseHingeLoss(0.2, reduction="sum"))
    with pytest.raises(NotImplementedError, match="exact f32 only"):
        tasks.Retrieval(loss=tasks.BPRLoss(), precision="bf16x3")
    with pytest.raises(NotImplementedError):
        tasks.Retrieval(loss=object())
    with pytest.raises(NotImplementedError):
        tasks.Retrieval(loss=tasks.CategoricalCrossentropy(from_logits=False))
    with pytest.raises(NotImplementedError):
        tasks.Retrieval(loss=tasks.MeanSquaredError())
    assert "pairwise" not in tasks.__doc__.split("Differences from TFRS")[1].split("* ``metrics``")[0].replace("pairwise losses above", "")

"""The tower drivers' launch lists (``towers_forward`` / ``towers_backward`` in trainer.py) against a recorded trace: no GPU, no
library load.  The launchers are replaced by recorders, the towers are built on CPU tensors from ``dense_layout``, and every
case's launch sequence - projected onto each tower - must be the one in ``tests/golden/tower_driver_traces.json``, element for
element: the kernel entry and its problem count, the shape of every tensor argument, which optional arguments are None, the
scalars, the dropout tuple; plus the total number of launches and the callback's position in the split backward.

The golden file was recorded with this recorder from the six drivers these two replaced, driven the way their call sites
dispatched them.  It is a record of that behaviour and is never regenerated from the code under test.  It differs from what
those drivers did in the places the file itself marks: asymmetric towers WITHOUT layer normalisation now share the launch of a
layer on which they coincide - the count-2 form of the same kernel entry (``_intended_difference``) - and the dx-only launch of
layer 0 in the split backward takes no lookup, as the asymmetric sequence never did (``_dx_pass_without_lookup``)."""
import inspect
import json
import os

import pytest
import torch

from two_tower_amazon_recommender_amd import ops, trainer
from two_tower_amazon_recommender_amd.trainer import Tower, TwoTowerConfig, dense_layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_driver_traces.json")
EMB, BATCH, SEED, STEP = 32, 64, 7, 3

# launcher -> (kernel entry, the arguments that hold one element per tower and the name each goes by in the projection)
_PAIRED = {
    "dense_fwd2": ("dense_fwd", dict(xs="x", ws="w", bs="b", ys="out", lookups="lookup", relu_bits="relu_bits")),
    "dense_bwd2": ("dense_bwd", dict(xs="x", ws="w", dzs="dz", dxs="dx", dx_relu_srcs="dx_relu_src", dw_slabs="dw_slabs",
                                      db_slabs="db_slabs", lookups="lookup", dx_relu_bits="dx_relu_bits")),
    "tower_fwd2": ("tower_fwd2", {k: k for k in ("xs", "w0s", "b0s", "hs", "h_bits", "w1s", "b1s", "ys", "lookups")}),
    "tower_bwd2": ("tower_bwd2", dict(upper="upper", lower="lower")),
}
_PROBLEMS = ("cross_layer", "cross_layer_bwd", "layer_norm2", "layer_norm_bwd2")
LAUNCHERS = ("dense_fwd", "dense_bwd") + tuple(_PAIRED) + _PROBLEMS


class FakeLookup:
    """What the drivers pass through to layer 0 (ops.make_lookup's struct needs device tensors)."""

    def __init__(self, rows, width):
        self._mk = (rows, width)


def _desc(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.Tensor):
        return ["T"] + list(v.shape)
    if isinstance(v, FakeLookup):
        return ["lookup"] + list(v._mk)
    if isinstance(v, dict):
        return {k: _desc(x) for k, x in sorted(v.items())}
    return [_desc(x) for x in v]


class Recorder:
    """Replaces the ten launchers (and the three shape queries) on ``ops``; ``towers`` tells which tower a buffer belongs to."""

    def __init__(self, monkeypatch, fwd2=True, bwd2=True):
        self.launches = 0
        self.per_tower = ([], [])
        self.owner = {}
        for name in LAUNCHERS:
            monkeypatch.setattr(ops, name, self._wrap(name, inspect.signature(getattr(ops, name))))
        monkeypatch.setattr(ops, "dense_bwd_num_slabs", lambda m: 2)
        monkeypatch.setattr(ops, "tower_fwd2_supported", lambda m, k0, h, n1: fwd2)
        monkeypatch.setattr(ops, "tower_bwd2_supported", lambda m, k0, k1, n: bwd2)

    def own(self, towers):
        for i, t in enumerate(towers):
            for x in t.acts + t.dz + t.pre + t.xc + t.cu + t.cg + [t.demb]:
                self.owner[x.untyped_storage().data_ptr()] = i

    def _tower(self, x):
        return self.owner[x.untyped_storage().data_ptr()]

    def callback(self):
        for p in self.per_tower:
            p.append(["callback", 0, {}])

    def _wrap(self, name, sig):
        def launch(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            assert a.pop("riders", None) is None
            self.launches += 1
            if name in _PAIRED:
                entry, names = _PAIRED[name]
                pick = lambda v, i: v if v is None else ({k: pick(x, i) for k, x in v.items()} if isinstance(v, dict) else v[i])
                probs = [{new: pick(a[old], i) for old, new in names.items()} for i in range(2)]
                shared = {k: v for k, v in a.items() if k not in names}
                drop = shared.pop("dropout", None)
                for i, p in enumerate(probs):
                    if "dropout" in sig.parameters:
                        p["dropout"] = None if drop is None else (drop[0], drop[1], drop[2][i], drop[3])
                    key = p["upper"]["dzs"] if name == "tower_bwd2" else p.get("out", p.get("dz", p.get("ys")))
                    self._emit(self._tower(key), entry, 2, {**shared, **p})
            elif name in _PROBLEMS:
                probs = a.pop("problems")
                us, drop = a.pop("u", None), a.pop("dropout", None)
                for i, p in enumerate(probs):
                    q = dict(a, problem=p)
                    if "u" in sig.parameters:
                        q["u"] = None if us is None else us[i]
                    if "dropout" in sig.parameters:
                        tid = None if drop is None else (drop[2][i] if isinstance(drop[2], (tuple, list)) else drop[2])
                        q["dropout"] = None if drop is None else (drop[0], drop[1], tid, drop[3])
                    key = {"cross_layer": 4, "cross_layer_bwd": 2, "layer_norm2": 3, "layer_norm_bwd2": 2}[name]   # a buffer of the tower's own
                    self._emit(self._tower(p[key]), name, len(probs), q)
            else:
                self._emit(self._tower(a["out"] if name == "dense_fwd" else a["dz"]), name, 1, a)
        return launch

    def _emit(self, tower, entry, count, args):
        self.per_tower[tower].append([entry, count, _desc(args)])

    def result(self):
        return json.loads(json.dumps({"launches": self.launches, "towers": list(self.per_tower)}))


def build_towers(case):
    """Both towers of ``case`` on CPU tensors, wired like TwoTowerTrainer.__init__ wires them (ops.dense_bwd_num_slabs stubbed)."""
    cfg = TwoTowerConfig(n_users=100, n_items=100, embedding_dim=EMB, tower_dims=case["user"], item_tower_dims=case.get("item"),
                         batch_size=BATCH, dropout_rate=case.get("dropout", 0.0), cross_layers=case.get("cross", 0),
                         layer_norm=case.get("ln", False), **({"candidate_sampling": "mixed", "n_sampled_negatives": case["neg"]}
                                                             if case.get("neg") else {}))
    cfg.validate()
    lay = dense_layout(cfg)
    flat = torch.zeros(lay.total)
    dev = torch.device("cpu")
    ut = Tower(cfg, cfg.user_dims, flat, None, lay.blocks["user.W0"].offset, dev)
    it = Tower(cfg, cfg.item_dims, flat, None, lay.blocks["item.W0"].offset, dev, rows=BATCH + case.get("neg", 0))
    for side, t in (("user", ut), ("item", it)):
        if cfg.cross_layers:
            seg = lay.segment("cross.kernels")
            slabs = torch.zeros(2 * seg.stride)
            ws = [lay.blocks[f"cross.{side}.W{l}"] for l in range(cfg.cross_layers)]
            bs = [lay.blocks[f"cross.{side}.b{l}"] for l in range(cfg.cross_layers)]
            t.set_cross([w.view(flat) for w in ws], [b.view(flat) for b in bs], [slabs[w.offset - seg.lo:] for w in ws],
                        [slabs[b.offset - seg.lo:] for b in bs], 2, seg.stride)
        if cfg.layer_norm:
            seg = lay.segment("norm")
            slabs = torch.zeros(2 * seg.stride)
            gs = [lay.blocks[f"norm.{side}.g{l}"] for l in range(t.n_layers - 1)]
            bs = [lay.blocks[f"norm.{side}.b{l}"] for l in range(t.n_layers - 1)]
            t.set_layer_norm([g.view(flat) for g in gs], [b.view(flat) for b in bs], [slabs[g.offset - seg.lo:] for g in gs],
                             [slabs[b.offset - seg.lo:] for b in bs], 2, seg.stride)
    return cfg, ut, it


def lookups_of(towers):
    return tuple(FakeLookup(t.rows, EMB) for t in towers)


# A pass of a case:
#   ("F", train, lookups, rows)       both towers forward; rows: None or the per-tower row counts of an inference pass
#   ("B", lookups, split, workspace)  both towers backward; split: with on_embedding_grads; workspace: with bwd2_ws
#   ("TF", tower, train, lookup, rows) / ("TB", tower, dx, dw, lookup)   one tower through Tower.forward / Tower.backward
# ``step``: the step index the dropout streams' first rows are taken at (default STEP).
def _both(look):
    return [("F", True, look, None), ("B", look, False, False), ("F", False, look, None)]


SYM, ASYM_FAR, ASYM_L0 = dict(user=[64, 32, 32]), dict(user=[128, 64], item=[96, 80, 64]), dict(user=[64, 32], item=[64, 64, 32])
CASES = {
    **{f"sym_drop{d}_fwd2{int(f)}": dict(SYM, dropout=d, fwd2=f, passes=_both(False) + _both(True)) for d in (0.0, 0.1) for f in (True, False)},
    "sym_one_layer": dict(user=[32], passes=_both(False) + _both(True)),
    "sym_mask_from_acts": dict(user=[48, 32], dropout=0.1, passes=_both(False) + _both(True)),
    **{f"cross{n}": dict(SYM, cross=n, dropout=0.1, passes=_both(False)) for n in (1, 2, 3)},
    "layer_norm": dict(SYM, ln=True, dropout=0.1, passes=_both(False) + _both(True)),
    "layer_norm_cross2": dict(SYM, ln=True, cross=2, dropout=0.1, passes=_both(False)),
    "asym_far": dict(ASYM_FAR, dropout=0.1, passes=_both(False) + _both(True)),
    # (layer normalisation takes hidden widths that are multiples of 32: 160 where the plain case has 80)
    "asym_far_layer_norm": dict(user=[128, 64], item=[96, 160, 64], ln=True, dropout=0.1, passes=_both(False) + _both(True)),
    "asym_l0": dict(ASYM_L0, dropout=0.1, passes=_both(False) + _both(True)),
    "asym_l0_layer_norm": dict(ASYM_L0, ln=True, dropout=0.1, passes=_both(False) + _both(True)),
    "mixed": dict(SYM, neg=16, dropout=0.1, passes=_both(False) + _both(True) + [("F", False, False, (64, 64))]),
    "mixed_layer_norm": dict(SYM, neg=16, ln=True, dropout=0.1, passes=_both(False) + _both(True) + [("F", False, False, (64, 64))]),
    "mixed_layer_norm_step0": dict(SYM, neg=16, ln=True, dropout=0.1, step=0, passes=[("F", True, False, None)]),
    "split_sym": dict(SYM, dropout=0.1, passes=[("B", False, True, False), ("B", True, True, False)]),
    "split_asym_far": dict(ASYM_FAR, dropout=0.1, passes=[("B", False, True, False), ("B", True, True, False)]),
    "split_asym_l0": dict(ASYM_L0, dropout=0.1, passes=[("B", False, True, False), ("B", True, True, False)]),
    "bwd2_l2": dict(user=[64, 32], dropout=0.1, passes=[("B", False, False, True), ("B", True, False, True)]),
    "bwd2_l3": dict(SYM, dropout=0.1, passes=[("B", False, False, True), ("B", True, False, True)]),
    "bwd2_unsupported": dict(SYM, dropout=0.1, bwd2=False, passes=[("B", False, False, True)]),
    "single": dict(SYM, dropout=0.1, passes=[("TF", 0, False, False, None), ("TF", 0, False, False, 40), ("TF", 0, False, True, None),
                                             ("TF", 1, True, True, None), ("TB", 0, True, False, False), ("TB", 0, False, True, False),
                                             ("TB", 1, True, True, True)]),
    "single_layer_norm_cross": dict(SYM, ln=True, cross=2, dropout=0.1, passes=[("TF", 0, True, False, None), ("TF", 0, False, False, 40),
                                                                               ("TB", 0, True, True, False)]),
}


def run_case(case, rec):
    """The passes of ``case`` through the two drivers and the Tower wrappers."""
    cfg, ut, it = build_towers(case)
    rec.own((ut, it))
    towers, step, ws = (ut, it), case.get("step", STEP), torch.zeros(8)
    drops = tuple((cfg.dropout_rate, SEED, i, step * t.rows) for i, t in enumerate(towers))
    for p in case["passes"]:
        if p[0] == "F":
            trainer.towers_forward(towers, dropouts=drops if p[1] else None, lookups=lookups_of(towers) if p[2] else None, rows=p[3])
        elif p[0] == "B":
            trainer.towers_backward(towers, cfg.dropout_rate, lookups=lookups_of(towers) if p[1] else None,
                                    on_embedding_grads=rec.callback if p[2] else None, bwd2_ws=ws if p[3] else None)
        elif p[0] == "TF":
            t = towers[p[1]]
            t.forward(drops[p[1]] if p[2] else None, lookup=lookups_of((t,))[0] if p[3] else None, rows=p[4])
        else:
            t = towers[p[1]]
            t.backward(cfg.dropout_rate, dx=p[2], dw=p[3], lookup=lookups_of((t,))[0] if p[4] else None)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_list(name, golden, monkeypatch):
    case = CASES[name]
    rec = Recorder(monkeypatch, fwd2=case.get("fwd2", True), bwd2=case.get("bwd2", True))
    run_case(case, rec)
    got, want = rec.result(), golden[name]
    assert got["launches"] == want["launches"]
    for t in range(2):
        assert len(got["towers"][t]) == len(want["towers"][t])
        for i, (g, w) in enumerate(zip(got["towers"][t], want["towers"][t])):
            assert g == w, f"{name}: launch {i} of tower {t}"


def test_golden_has_no_stale_case(golden):
    assert sorted(k for k in golden if not k.startswith("_")) == sorted(CASES)
    assert golden["_intended_difference"] == ["asym_l0", "split_asym_l0"]


def test_a_plan_is_built_once(monkeypatch):
    """The second pass of a kind launches from the cached plan: the same tensors, not views cut again."""
    rec = Recorder(monkeypatch)
    _, ut, it = build_towers(dict(SYM, ln=True))
    rec.own((ut, it))
    seen = []
    monkeypatch.setattr(ops, "layer_norm2", lambda *problems, **kw: seen.append(problems))
    for _ in range(2):
        trainer.towers_forward((ut, it), rows=(40, 40))
    first, second = seen[:len(seen) // 2], seen[len(seen) // 2:]
    assert first and all(a is b for x, y in zip(first, second) for p, q in zip(x, y) for a, b in zip(p, q))


def test_refusals(monkeypatch):
    rec = Recorder(monkeypatch)
    drop = (0.1, SEED, 0, 0)

    def towers(**case):
        cfg, ut, it = build_towers(dict(SYM, **case))
        rec.own((ut, it))
        return ut, it

    ut, it = towers(cross=1)
    lks = lookups_of((ut, it))
    with pytest.raises(ValueError, match="lookup"):                     # a fused lookup together with cross layers
        trainer.towers_forward((ut, it), lookups=lks)
    with pytest.raises(ValueError, match="lookup"):
        ut.forward(lookup=lks[0])
    with pytest.raises(NotImplementedError):                            # the dx-first split with cross layers
        trainer.towers_backward((ut, it), on_embedding_grads=rec.callback)
    with pytest.raises(NotImplementedError):
        ut.backward(dx=True, dw=False)
    ut, it = towers(ln=True)
    with pytest.raises(NotImplementedError):                            # ... and with layer normalisation
        trainer.towers_backward((ut, it), on_embedding_grads=rec.callback)
    with pytest.raises(NotImplementedError):
        ut.backward(dx=False, dw=True)
    for ut, it in (towers(), towers(ln=True)):                          # a partial pass is an inference pass
        with pytest.raises(ValueError, match="inference"):
            trainer.towers_forward((ut, it), dropouts=(drop, drop), rows=(40, 64))
        with pytest.raises(ValueError, match="inference"):
            ut.forward(drop, rows=40)
    assert rec.launches == 0

"""Attention pooling of the user history without a GPU: the closed-form backward of tests/attention_check.py against f64 torch
autograd of the forward restatement, config validation (YAML, CLI, field order, checkpoint keys, the segment count), the C
entries' argument validation (before any launch), the ctypes signatures against the header, the custom ops' registration, and
the new translation unit's register report (no kernel uses scratch)."""
import ctypes as C
import dataclasses
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import attention_check as atc
import history_check as hc
from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------ 1. the closed form
def test_closed_form_backward_equals_f64_autograd():
    """37 bags, L 7, dim 16, with padding, an empty bag, a single-slot bag and leave-one-out: every result of the closed form
    within 1e-12 of torch autograd (f64) of the forward restatement; the logit gradients of a bag sum to zero."""
    rng = np.random.default_rng(0)
    n, L, dim, rows = 37, 7, 16, 40
    table = rng.standard_normal((rows, dim))
    tokens = rng.integers(0, rows, (n, L)).astype(np.int32)
    tokens[rng.random((n, L)) < 0.3] = -1
    tokens[3] = -1                                          # an empty bag
    tokens[4] = [-1, -1, 5, -1, -1, -1, -1]                 # a single-slot bag
    tokens[6] = [4, -1, 4, -1, -1, -1, 4]                   # emptied by the exclusion
    exclude = rng.integers(0, rows, n).astype(np.int64)
    exclude[6] = 4
    exclude[10] = tokens[10, 0] = 17
    attn = rng.standard_normal(dim + L)
    base_table = rng.standard_normal((20, dim))
    base_ids = rng.integers(0, 20, n)
    dy = rng.standard_normal((n, dim))

    out, w, pooled, ids, flag = atc.attention_forward(table, tokens, attn, None, exclude, (base_table, base_ids))
    assert flag == 0 and (w[3] == 0).all() and (w[6] == 0).all() and w[4, 2] == 1.0 and np.array_equal(out[3], base_table[base_ids[3]])
    per, _ = hc.mask_tokens(tokens, None, exclude)
    assert np.array_equal(ids.reshape(n, L), per)
    some = (per >= 0).any(1)
    assert np.allclose(w.sum(1)[some], 1.0, atol=1e-14)

    tb = torch.tensor(table, requires_grad=True)
    at = torch.tensor(attn, requires_grad=True)
    bt = torch.tensor(base_table, requires_grad=True)
    o_t, w_t, p_t = atc.attention_forward_torch(tb, torch.from_numpy(per.astype(np.int64)), at, bt[torch.from_numpy(base_ids)])
    assert np.abs(o_t.detach().numpy() - out).max() <= 1e-12 and np.abs(w_t.detach().numpy() - w).max() <= 1e-12
    assert np.abs(p_t.detach().numpy() - pooled).max() <= 1e-12
    (o_t * torch.from_numpy(dy)).sum().backward()

    dh, da, dp, de = atc.attention_backward(table, ids, w, pooled, dy, attn, L)
    g_table = np.zeros_like(table)
    valid = ids >= 0
    np.add.at(g_table, ids[valid], dh[valid])
    errs = {"table": np.abs(g_table - tb.grad.numpy()).max(), "da": np.abs(da - at.grad.numpy()[:dim]).max(),
            "dp": np.abs(dp - at.grad.numpy()[dim:]).max()}
    g_base = np.zeros_like(base_table)
    np.add.at(g_base, base_ids, dy)
    errs["base"] = np.abs(g_base - bt.grad.numpy()).max()
    print(errs)
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert np.abs(de.sum(1)).max() <= 1e-12 and np.abs(dp.sum()) <= 1e-12
    assert not dh[~valid].any()


def _f32_closed_form_errors(dim, shapes):
    """The worst errors of the float32 closed form against the f64 one over ``shapes`` = ((L, n_bags), ...), each held to BAR / 10."""
    worst = {}
    for L, n_bags in shapes:
        p = atc.backward_problem(dim, L, n_bags)
        _, w, pooled, ids, flag = atc.attention_forward(p["table"], p["tokens"], p["attn"], p["bag_rows"], p["exclude"], None)
        assert flag == 0 and len(ids) == n_bags * L
        valid = ids >= 0
        want = atc.attention_backward(p["table"], ids, w, pooled, p["dy"], p["attn"], L)
        got = atc.attention_backward_f32(p["table"], ids, w, pooled, p["dy"], p["attn"], L)
        za, zp = atc.uncancelled_scales(p["table"], ids, w, pooled, p["dy"], L)
        zero = np.abs(want[1]).max() <= 1e-9 * za and np.abs(want[2]).max() <= 1e-9 * zp
        assert zero == (L == 1)                                                # one slot per bag: da = dp = 0, and only then
        for name, g, r, z in (("slot_grads", got[0][valid], want[0][valid], None), ("da", got[1], want[1], za), ("dp", got[2], want[2], zp)):
            e = atc.errs(g, r, z)
            worst[name] = max(worst.get(name, 0.0), *e)
            assert e[0] <= atc.BAR / 10 and e[1] <= atc.BAR / 10, (dim, L, n_bags, name, e)
        assert abs(float(want[2].sum())) <= 1e-12 * zp
    return worst


@pytest.mark.parametrize("dim", atc.SWEEP_DIMS)
def test_f32_closed_form_meets_a_tenth_of_the_bar_at_every_sweep_shape(dim):
    """The GPU sweep of the backward (tests/test_gpu_history_attention.py) holds a float32 kernel to BAR = 1e-4 of the f64 closed
    form on the problems of ``attention_check.backward_problem``.  That the problems allow it: at every (dim, L, n_bags) of the
    sweep the closed form evaluated in float32 - both from the f64 forward's weights and pooled rows - stays within BAR / 10 of
    the f64 one under both error measures, for the slot rows of the kept slots, da and dp."""
    worst = _f32_closed_form_errors(dim, [(L, n_bags) for L in atc.SWEEP_LS for n_bags in atc.SWEEP_BAGS])
    print(f"dim {dim}: worst f32 errors {({k: f'{v:.2e}' for k, v in worst.items()})}")


@pytest.mark.parametrize("dim,L,n_bags", atc.NV2_SHAPES)
def test_f32_closed_form_meets_a_tenth_of_the_bar_with_two_float4_per_lane(dim, L, n_bags):
    print(f"dim {dim}: worst f32 errors {({k: f'{v:.2e}' for k, v in _f32_closed_form_errors(dim, [(L, n_bags)]).items()})}")


def test_backward_launch_shapes_of_the_sweep():
    """The forms of the backward launch the sweep reaches, as (lpr, NV, KF, threads, chunks)."""
    got = {(dim, L): atc.backward_launch_shape(dim, L) for dim in atc.SWEEP_DIMS for L in atc.SWEEP_LS}
    assert got[(4, 37)] == (1, 1, 4, 256, 37) and got[(4, 64)] == (1, 1, 4, 128, 64)          # just under the LDS limit; halved
    assert got[(36, 37)] == (16, 1, 4, 256, 3) and got[(36, 64)] == (16, 1, 4, 256, 4)
    assert got[(128, 37)] == got[(128, 64)] == (32, 1, 4, 256, 2) and got[(128, 7)] == (32, 1, 4, 256, 1)
    assert got[(256, 64)] == (64, 1, 4, 256, 1) and got[(516, 64)] == (64, 3, 2, 256, 1) and got[(1024, 64)] == (64, 4, 2, 256, 1)
    assert atc.backward_launch_shape(32, 20) == (8, 1, 4, 256, 3) and atc.backward_launch_shape(32, 5)[4] == 1   # the trainer tests
    assert all(atc.backward_launch_shape(d, L) == (64, 2, 4, 256, 1) for d, L, _ in atc.NV2_SHAPES) and not any(v[1] == 2 for v in got.values())
    assert atc.backward_launch_shape(4, 44)[3] == 256 and atc.backward_launch_shape(4, 45)[3] == 128


# ------------------------------------------------------------------------------------------ 2. config
def test_config_validation_yaml_and_cli(tmp_path):
    base = dict(n_users=10, n_items=10)
    TwoTowerConfig(**base, user_history_len=64, history_pooling="attention").validate()
    TwoTowerConfig(**base, history_pooling="attention").validate()          # (no feature: the pooling is not used)
    with pytest.raises(ValueError, match="history"):
        TwoTowerConfig(**base, user_history_len=4, history_pooling="max").validate()
    with pytest.raises(ValueError, match="title_pooling"):
        TwoTowerConfig(**base, n_title_buckets=20, title_pooling="attention").validate()
    with pytest.raises(ValueError, match="mixed"):
        TwoTowerConfig(**base, user_history_len=4, history_pooling="attention", candidate_sampling="mixed",
                       n_sampled_negatives=8).validate()
    from two_tower_amazon_recommender_amd import config, ops, train
    assert tuple(ops.POOLINGS) == ("sum", "mean", "sqrtn")
    doc = {"model": {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
                     "features": {"history": {"max_items": 12, "pooling": "attention"}}}}
    cfg, _ = config.model_config_from_dict(doc, 10, 10)
    assert (cfg.user_history_len, cfg.history_pooling, cfg.history_attention) == (12, "attention", True)
    doc["model"]["features"] = {"title": {"buckets": 50, "pooling": "attention"}}
    with pytest.raises(ValueError, match="title_pooling"):
        config.model_config_from_dict(doc, 10, 10)[0].validate()
    args = train.parse(["--config", "x.yaml", "--history-len", "7", "--history-pooling", "attention"])
    assert (args.history_len, args.history_pooling) == (7, "attention")
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--history-pooling", "max"])
    with pytest.raises(SystemExit):
        train.parse(["--config", "x.yaml", "--title-pooling", "attention"])
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [64, 32]\n  item_tower_dims: [64, 32]\n")
    with pytest.raises(NotImplementedError, match="history"):
        train.main(["--config", str(cfgp), "--synthetic", "600", "--history-len", "4", "--history-pooling", "attention", "--distributed"])


# ------------------------------------------------------------------------------------------ 3. field order, keys, segments
def test_field_order_checkpoint_keys_and_segment_count():
    names = [f.name for f in dataclasses.fields(TwoTowerConfig)]
    k = names.index("n_title_buckets")
    assert names[k - 2:k] == ["user_history_len", "history_pooling"] and names[-3:] == ["n_title_buckets", "title_max_tokens", "title_pooling"]
    k = names.index("n_user_features")
    assert names[k - 1] == "cross_layers" and names[k:k + 3] == ["n_user_features", "n_item_features", "feature_clip"]
    from two_tower_amazon_recommender_amd.trainer import EmbeddingTable, TwoTowerTrainer

    class Stub:
        pass
    keys = {}
    for pooling in ("mean", "attention"):
        s = Stub()
        s.cfg = TwoTowerConfig(n_users=10, n_items=10, optimizer="adam", user_history_len=3, history_pooling=pooling)
        for name in ("dense_flat", "dense_accum", "dense_m", "dense_v"):
            setattr(s, name, name)
        s.tables = {p: EmbeddingTable.new(s.cfg, "cpu", p, 0, 10, None, {"user_history": "user_history"} if p == "history" else None)
                    for p in ("user", "item", "history")}                                              # (the records: CPU tensors)
        s.step_index, s.dropout_seed, s.adam_step = 0, 0, 1
        sd = TwoTowerTrainer.state_dict(s)
        keys[pooling] = set(sd)
        assert sd["config"]["history_pooling"] == pooling
    assert keys["mean"] == keys["attention"]
    base = dict(n_users=10, n_items=10, tower_dims=[64, 32])
    mean = TwoTowerConfig(**base, user_history_len=3)
    attn = TwoTowerConfig(**base, user_history_len=3, history_pooling="attention")
    assert attn.dense_segment_count() == mean.dense_segment_count() + 1 == 9
    assert attn.dense_segment_count(attention=False) == mean.dense_segment_count()
    assert TwoTowerConfig(**base, history_pooling="attention").dense_segment_count() == 8     # no feature, no segment
    # 16 segments without the attention vector: refused because of it, and only then
    full = dict(n_users=10, n_items=10, tower_dims=[128, 64, 32], n_user_features=3, n_item_features=3, rating_weight=0.5,
                user_history_len=3)
    TwoTowerConfig(**full).validate()
    with pytest.raises(NotImplementedError, match="attention"):
        TwoTowerConfig(**full, history_pooling="attention").validate()


# ------------------------------------------------------------------------------------------ 4. the C entries
def test_c_entries_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.TT_ERR_INVALID_ARG
    fwd, bwd = lib.tt_history_attention_fwd_f32, lib.tt_history_attention_bwd_f32
    one, odd = C.c_void_p(16), C.c_void_p(20)               # non-null pointers that are never dereferenced: every call fails first
    err = lib.tt_last_error
    #   table rows dim tokens n_token_rows L bag_rows n_bags attn out ids weights pooled flag exclude base_table base_rows base_ids stream
    assert fwd(None, 10, 6, None, 4, 3, None, 4, None, None, None, None, None, None, None, None, 0, None, None) == E and b"multiple of 4" in err()
    assert fwd(None, 10, 2048, None, 4, 3, None, 4, None, None, None, None, None, None, None, None, 0, None, None) == E and b"1024" in err()
    assert fwd(None, 10, 8, None, 4, 0, None, 4, None, None, None, None, None, None, None, None, 0, None, None) == E and b"L must be" in err()
    assert fwd(None, 10, 8, None, 4, 65, None, 4, None, None, None, None, None, None, None, None, 0, None, None) == E and b"L must be" in err()
    assert fwd(None, 10, 8, None, 2 ** 30, 3, None, 2 ** 30, None, None, None, None, None, None, None, None, 0, None, None) == E and b"31 bits" in err()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, None, None, None, None, None, None, None, one, 5, None, None) == E and b"go together" in err()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, None, None, None, None, None, None, None, None, 5, one, None) == E and b"go together" in err()
    assert fwd(None, 10, 8, None, 4, 3, None, 4, None, None, None, None, None, None, None, one, 0, one, None) == E and b"base_rows" in err()
    assert fwd(None, 10, 8, None, 4, 3, None, 5, None, None, None, None, None, None, None, None, 0, None, None) == E and b"identity" in err()
    assert fwd(one, 10, 8, one, 4, 3, None, 4, None, one, None, None, None, None, None, None, 0, None, None) == E and b"null" in err()      # attn
    assert fwd(one, 10, 8, one, 4, 3, None, 4, one, None, None, None, None, None, None, None, 0, None, None) == E and b"null" in err()      # out
    assert fwd(one, 10, 8, one, 4, 3, None, 4, odd, one, None, None, None, None, None, None, 0, None, None) == E and b"aligned" in err()
    assert fwd(one, 10, 8, one, 4, 3, None, 4, one, one, None, None, odd, None, None, None, 0, None, None) == E and b"pooled" in err()
    assert fwd(one, 10, 8, one, 4, 3, None, 4, one, one, None, None, None, None, None, odd, 5, one, None) == E and b"base_table" in err()
    assert b"tt_history_attention_fwd_f32" in err()                          # the messages name the entry that was called
    assert fwd(None, 10, 8, None, 0, 3, None, 0, None, None, None, None, None, None, one, one, 5, one, None) == _lib.TT_OK   # no bags
    #   table rows dim L ids weights pooled dy n_bags attn slot_grads slabs n_slabs stream
    assert bwd(None, 10, 6, 3, None, None, None, None, 4, None, None, None, 1, None) == E and b"multiple of 4" in err()
    assert bwd(None, 10, 1028, 3, None, None, None, None, 4, None, None, None, 1, None) == E and b"1024" in err()
    assert bwd(None, 10, 8, 0, None, None, None, None, 4, None, None, None, 1, None) == E and b"L must be" in err()
    assert bwd(None, 10, 8, 65, None, None, None, None, 4, None, None, None, 1, None) == E and b"L must be" in err()
    assert bwd(None, 10, 8, 3, None, None, None, None, 2 ** 30, None, None, None, 1, None) == E and b"31 bits" in err()
    assert bwd(None, 10, 8, 3, None, None, None, None, 4, None, None, None, 0, None) == E and b"n_slabs" in err()
    assert bwd(one, 10, 8, 3, one, one, one, one, 4, one, one, None, 1, None) == E and b"null" in err()
    assert bwd(one, 10, 8, 3, one, one, one, one, 4, one, odd, one, 1, None) == E and b"aligned" in err()
    assert bwd(one, 10, 8, 3, one, one, one, odd, 4, one, one, one, 1, None) == E and b"aligned" in err()
    assert b"tt_history_attention_bwd_f32" in err()
    assert bwd(None, 10, 8, 3, None, None, None, None, 0, None, None, None, 1, None) == _lib.TT_OK
    assert lib.tt_history_attention_num_slabs(8192) == 1024 and lib.tt_history_attention_num_slabs(37) == 5
    assert lib.tt_history_attention_num_slabs(0) == 1 and lib.tt_history_attention_num_slabs(10 ** 6) == 1024
    assert lib.tt_abi_version() == 10
    for which in (9, 13, 16, 19, 20):                                        # no argument struct was added
        assert lib.tt_abi_struct_bytes(which) == -1, which


def test_header_signatures_and_the_custom_ops_exist():
    header = (ROOT / "include" / "twotower_hip.h").read_text()
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "tt_stream_t": C.c_void_p}
    for name, ret in (("tt_history_attention_fwd_f32", "int"), ("tt_history_attention_bwd_f32", "int"),
                      ("tt_history_attention_num_slabs", "int32_t")):
        restype, argtypes = _lib.SIGNATURES[name]
        m = re.search(ret + r" " + name + r"\((.*?)\);", header, re.S)
        params = [p.strip() for p in m.group(1).split(",")]
        assert [C.c_void_p if "*" in p else kinds[p.split()[0]] for p in params] == argtypes, name
        assert restype is (C.c_int if ret == "int" else C.c_int32)
    bag = _lib.SIGNATURES["tt_history_bag_fwd_f32"][1]
    assert len(_lib.SIGNATURES["tt_history_attention_fwd_f32"][1]) == len(bag)
    from two_tower_amazon_recommender_amd import ops, torch_ops
    assert callable(ops.history_attention) and callable(ops.history_attention_bwd) and ops.history_attention_num_slabs(64) == 8
    for name in ("history_attention", "history_attention_bwd"):
        assert name in torch_ops.OPS and hasattr(torch.ops.twotower, name)
    table, tokens = torch.empty(100, 32, device="meta"), torch.empty(7, 5, dtype=torch.int32, device="meta")
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device="meta")
    attn = torch.empty(37, device="meta")
    out, w, pooled, ids = torch.ops.twotower.history_attention(table, tokens, None, None, None, None, attn)
    assert out.shape == (7, 32) and w.shape == (7, 5) and pooled.shape == (7, 32) and ids.shape == (35,) and ids.dtype == torch.int64
    out, w, pooled, ids = torch.ops.twotower.history_attention(table, tokens, i64(3), i64(3), torch.empty(9, 32, device="meta"), i64(3), attn)
    assert out.shape == (3, 32) and w.shape == (3, 5) and ids.shape == (15,)
    sg, da = torch.ops.twotower.history_attention_bwd(table, ids, w, pooled, out, attn)
    assert sg.shape == (15, 32) and da.shape == (37,)
    with pytest.raises((NotImplementedError, RuntimeError)):                 # no CPU kernel, no fallback
        torch.ops.twotower.history_attention(torch.zeros(10, 8), torch.zeros(2, 3, dtype=torch.int32), None, None, None, None,
                                             torch.zeros(11))
    assert "attention" not in ops.POOLINGS                                   # the bag ops keep their three poolings


# ------------------------------------------------------------------------------------------ 5. registers
def _resources(tmp_path, name):
    """{demangled kernel: (vgprs, agprs, scratch bytes per lane, occupancy)} from hipcc's kernel-resource-usage remarks."""
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", "-o", str(tmp_path / f"{name}.o"),
                        str(CSRC / f"{name}.hip")], check=True, capture_output=True, text=True, timeout=900)
    rows, cur = [], {}
    for line in r.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            if cur:
                rows.append(cur)
            cur = {"name": m.group(1)}
        for key, tag in (("VGPRs", "v"), ("AGPRs", "a"), (r"ScratchSize \[bytes/lane\]", "scr"), (r"Occupancy \[waves/SIMD\]", "occ")):
            m = re.search(r" " + key + r": (\d+)", line)
            if m and cur:
                cur[tag] = int(m.group(1))
    if cur:
        rows.append(cur)
    names = subprocess.run(["c++filt"], input="\n".join(x["name"] for x in rows), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for x, n in zip(rows, names):
        n = re.sub(r"\(anonymous namespace\)::", "", n)
        out[re.sub(r"\(.*", "", n).replace("void ", "")] = (x.get("v"), x.get("a"), x.get("scr"), x.get("occ"))
    return out


def test_no_kernel_of_the_translation_unit_uses_scratch(tmp_path):
    """csrc/history_attn.hip compiles for gfx950; all 16 forward and 4 backward instantiations report 0 bytes of scratch, and the
    ones the flagship shape runs (dim 128: NV 1) keep at least 4 waves per SIMD."""
    res = _resources(tmp_path, "history_attn")
    for k, v in sorted(res.items()):
        print(k, v)
    fwd = {k: v for k, v in res.items() if k.startswith("attn_fwd_kernel")}
    bwd = {k: v for k, v in res.items() if k.startswith("attn_bwd_kernel")}
    assert len(fwd) == 16 and len(bwd) == 4 and len(res) == 20, sorted(res)
    assert all(v[2] == 0 for v in res.values()), {k: v for k, v in res.items() if v[2] != 0}
    assert res["attn_fwd_kernel<1, true, true>"][3] >= 4 and res["attn_bwd_kernel<1, 4>"][3] >= 4

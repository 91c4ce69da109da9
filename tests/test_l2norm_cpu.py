"""L2-normalised tower outputs, the parts that need no GPU: argument validation of tt_l2_normalize_fwd_f32 / _bwd_f32 (before
any launch), the ABI's struct sizes, the config switch from TwoTowerConfig to the YAML reader, the sharded trainer's refusal,
and the resource usage of csrc/normalize.hip (no kernel may use scratch)."""
import ctypes as C
import pathlib
import re
import subprocess

import pytest

from two_tower_amazon_recommender_amd import _lib
from two_tower_amazon_recommender_amd.trainer import TwoTowerConfig

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "two_tower_amazon_recommender_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"


def _entries():
    lib = _lib.load()
    return ((lib.tt_l2_normalize_fwd_f32, _lib.L2NormFwdArgs, b"tt_l2_normalize_fwd_f32"),
            (lib.tt_l2_normalize_bwd_f32, _lib.L2NormBwdArgs, b"tt_l2_normalize_bwd_f32"))


@pytest.mark.parametrize("what,n_probs,rows,dim,eps,word", [
    ("dim 6", 2, 4, 6, 1e-12, b"dim"), ("dim 1028", 2, 4, 1028, 1e-12, b"dim"), ("dim 0", 2, 4, 0, 1e-12, b"dim"),
    ("n_probs 0", 0, 4, 32, 1e-12, b"n_probs"), ("n_probs 3", 3, 4, 32, 1e-12, b"n_probs"),
    ("rows -1", 2, -1, 32, 1e-12, b"rows"), ("eps 0", 2, 4, 32, 0.0, b"eps"), ("eps < 0", 2, 4, 32, -1.0, b"eps"),
    ("null tensors", 2, 4, 32, 1e-12, b"null pointer"),
])
def test_invalid_arguments_are_refused_before_any_launch(what, n_probs, rows, dim, eps, word):
    """Every check happens on the host: the pointers inside `probs` are NULL throughout, so a launch would fault."""
    lib = _lib.load()
    for fn, struct, name in _entries():
        probs = (struct * 3)()
        assert fn(probs, n_probs, rows, dim, eps, None) == _lib.TT_ERR_INVALID_ARG, what
        msg = lib.tt_last_error()
        assert name in msg and word in msg, (what, msg)


def test_null_problem_array_is_refused_and_zero_rows_is_a_no_op():
    lib = _lib.load()
    for fn, struct, name in _entries():
        assert fn(None, 1, 4, 32, 1e-12, None) == _lib.TT_ERR_INVALID_ARG
        assert b"null pointer" in lib.tt_last_error()
        assert fn((struct * 2)(), 2, 0, 32, 1e-12, None) == _lib.TT_OK


def test_struct_sizes_are_reported_and_the_abi_version_stays_10():
    lib = _lib.load()
    assert lib.tt_abi_version() == 10 == _lib.ABI_VERSION
    assert lib.tt_abi_struct_bytes(7) == C.sizeof(_lib.L2NormFwdArgs) == 16
    assert lib.tt_abi_struct_bytes(8) == C.sizeof(_lib.L2NormBwdArgs) == 24
    assert lib.tt_abi_struct_bytes(9) == -1


def test_config_switch_is_validated():
    base = dict(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32])
    cfg = TwoTowerConfig(**base)
    assert cfg.normalize_embeddings is False and cfg.normalize_eps == 1e-12
    cfg.validate()
    TwoTowerConfig(normalize_embeddings=True, **base).validate()
    with pytest.raises(ValueError, match="normalize_eps"):
        TwoTowerConfig(normalize_embeddings=True, normalize_eps=0, **base).validate()
    with pytest.raises(ValueError, match="normalize_eps"):
        TwoTowerConfig(normalize_eps=-1e-12, **base).validate()
    with pytest.raises(ValueError, match="normalize_eps"):
        TwoTowerConfig(normalize_eps=float("nan"), **base).validate()


def test_yaml_reader_takes_the_optional_key_and_defaults_it_to_false():
    from two_tower_amazon_recommender_amd.config import model_config_from_dict
    model = {"embedding_dim": 32, "user_tower_dims": [64, 32], "item_tower_dims": [64, 32],
             "retrieval": {"candidate_sampling": "in_batch", "temperature": 0.1}}
    cfg, _ = model_config_from_dict({"model": model}, 100, 100)
    assert cfg.normalize_embeddings is False                        # the reference's schema, unchanged
    model["retrieval"]["normalize_embeddings"] = True
    cfg, _ = model_config_from_dict({"model": model}, 100, 100)
    assert cfg.normalize_embeddings is True and cfg.temperature == 0.1
    model["retrieval"]["normalize_embeddings"] = False
    assert model_config_from_dict({"model": model}, 100, 100)[0].normalize_embeddings is False


def test_train_cli_has_the_flag():
    from two_tower_amazon_recommender_amd import train
    assert train.parse(["--config", "c.yaml"]).normalize_embeddings is False
    assert train.parse(["--config", "c.yaml", "--normalize-embeddings"]).normalize_embeddings is True


def test_sharded_trainer_refuses_the_switch_before_touching_a_device(tmp_path):
    from two_tower_amazon_recommender_amd import train
    from two_tower_amazon_recommender_amd.sharded import ShardedTwoTowerTrainer
    cfg = TwoTowerConfig(n_users=10, n_items=10, embedding_dim=32, tower_dims=[32], normalize_embeddings=True)
    with pytest.raises(NotImplementedError, match="normalize_embeddings"):
        ShardedTwoTowerTrainer(cfg, "cuda:0")
    cfgp = tmp_path / "cfg.yaml"
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [32]\n  item_tower_dims: [32]\n")
    with pytest.raises(NotImplementedError, match="normalize_embeddings"):
        train.main(["--config", str(cfgp), "--synthetic", "1024", "--distributed", "--normalize-embeddings"])
    cfgp.write_text("model:\n  embedding_dim: 32\n  user_tower_dims: [32]\n  item_tower_dims: [32]\n"
                    "  retrieval:\n    normalize_embeddings: true\n")
    with pytest.raises(NotImplementedError, match="normalize_embeddings"):
        train.main(["--config", str(cfgp), "--synthetic", "1024", "--distributed"])


def _resources(tmp_path, name):
    """{demangled kernel: (vgprs, agprs, scratch bytes per lane, occupancy)} from hipcc's kernel-resource-usage remarks
    (the recipe of tests/test_isa_audit.py)."""
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


def test_no_normalize_kernel_uses_scratch(tmp_path):
    """Forward and backward, each in the one-float4-per-lane form (two rows per lane group) and the looped forms (2..4 float4
    per lane: dims above 256): everything a lane holds stays in registers, at an occupancy that keeps the loads in flight."""
    res = _resources(tmp_path, "normalize")
    want = {f"l2norm_{d}_kernel<{r}, {nv}>" for d in ("fwd", "bwd") for r, nv in ((2, 1), (1, 2), (1, 3), (1, 4))}
    assert set(res) == want, sorted(res)
    for name, (v, a, scr, occ) in res.items():
        assert scr == 0, (name, scr)
        assert occ >= 4, (name, occ)

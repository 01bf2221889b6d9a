"""CPU: magcache_amd/lora.py -- LoRA state dicts in the PEFT / diffusers spellings -> the weight names the MM-DiT engine takes
adapters on (mc_mmdit_lora_set).  No GPU, no library."""
import os
import re

import pytest
import torch

from magcache_amd import _lib
from magcache_amd.lora import lora_factor, lora_target_names, parse_lora_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair(out_f, in_f, rank, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rank, in_f, generator=g), torch.randn(out_f, rank, generator=g)


def test_peft_spelling_with_and_without_adapter_name():
    a, b = pair(8, 16, 4)
    for infix in ("", ".default", ".my_style"):
        sd = {f"transformer_blocks.0.attn.to_q.lora_A{infix}.weight": a, f"transformer_blocks.0.attn.to_q.lora_B{infix}.weight": b}
        out = parse_lora_state_dict(sd)
        assert list(out) == ["transformer_blocks.0.attn.to_q.weight"]
        down, up, alpha = out["transformer_blocks.0.attn.to_q.weight"]
        assert down is a and up is b and alpha is None
        assert lora_factor(down, alpha) == 1.0


def test_older_diffusers_spelling_and_alpha():
    a, b = pair(8, 16, 4)
    sd = {"single_transformer_blocks.1.proj_mlp.lora.down.weight": a, "single_transformer_blocks.1.proj_mlp.lora.up.weight": b,
          "single_transformer_blocks.1.proj_mlp.alpha": torch.tensor(8.0)}
    out = parse_lora_state_dict(sd)
    down, up, alpha = out["single_transformer_blocks.1.proj_mlp.weight"]
    assert down is a and up is b and alpha == 8.0
    assert lora_factor(down, alpha) == 2.0                     # alpha / rank
    # a plain float alpha, on the PEFT spelling
    sd = {"x.lora_A.weight": a, "x.lora_B.weight": b, "x.alpha": 2}
    assert parse_lora_state_dict(sd)["x.weight"][2] == 2.0 and lora_factor(a, 2) == 0.5


def test_transformer_prefix():
    a, b = pair(8, 16, 2)
    sd = {"transformer.transformer_blocks.0.ff.net.2.lora_A.weight": a, "transformer.transformer_blocks.0.ff.net.2.lora_B.weight": b,
          "text_encoder.layers.0.q_proj.lora_A.weight": a, "text_encoder.layers.0.q_proj.lora_B.weight": b}
    # with the prefix present, its keys are the adapter and the other component's are not ours
    assert list(parse_lora_state_dict(sd)) == ["transformer_blocks.0.ff.net.2.weight"]
    # no key carries the prefix: every key is taken as it is
    bare = {k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")}
    assert list(parse_lora_state_dict(bare)) == ["transformer_blocks.0.ff.net.2.weight"]
    # another prefix, and none
    assert list(parse_lora_state_dict({"unet." + k: v for k, v in bare.items()}, prefix="unet.")) == ["transformer_blocks.0.ff.net.2.weight"]
    assert list(parse_lora_state_dict(sd, prefix="")) == ["transformer.transformer_blocks.0.ff.net.2.weight",
                                                          "text_encoder.layers.0.q_proj.weight"]


def test_orphans_and_mismatched_pairs_raise():
    a, b = pair(8, 16, 4)
    with pytest.raises(ValueError, match="down without up"):
        parse_lora_state_dict({"m.lora_A.weight": a})
    with pytest.raises(ValueError, match="up without down"):
        parse_lora_state_dict({"m.lora.up.weight": b})
    with pytest.raises(ValueError, match="no pair"):
        parse_lora_state_dict({"m.lora_A.weight": a, "m.lora_B.weight": b, "n.alpha": torch.tensor(1.0)})
    with pytest.raises(ValueError, match="belong to no"):
        parse_lora_state_dict({"m.lora_A.weight": a, "m.lora_B.weight": b, "m.weight": torch.zeros(8, 16)})
    with pytest.raises(ValueError, match="belong to no"):
        parse_lora_state_dict({"transformer.m.lora_A.weight": a, "transformer.m.lora_B.weight": b, "transformer.m.lora_magnitude_vector": a})
    with pytest.raises(ValueError, match="share no rank"):
        parse_lora_state_dict({"m.lora_A.weight": a, "m.lora_B.weight": torch.zeros(8, 5)})
    with pytest.raises(ValueError, match="repeats"):
        parse_lora_state_dict({"m.lora_A.one.weight": a, "m.lora_A.two.weight": a, "m.lora_B.one.weight": b})


def test_targets_are_engine_weight_names_flux_and_qwen():
    """A module of an adapter file maps to `<module>.weight`, the upstream name the engine registers -- also for the parts of
    a fused q | k | v and for the AdaLN Linear inside the stacked modulation matrix."""
    a, b = pair(8, 16, 4)
    flux_modules = ["transformer_blocks.1.attn.to_q", "transformer_blocks.1.attn.to_k", "transformer_blocks.1.attn.to_v",
                    "transformer_blocks.1.attn.add_q_proj", "transformer_blocks.1.attn.to_out.0", "transformer_blocks.1.attn.to_add_out",
                    "transformer_blocks.1.ff.net.0.proj", "transformer_blocks.1.ff_context.net.2", "transformer_blocks.1.norm1.linear",
                    "transformer_blocks.0.norm1_context.linear", "single_transformer_blocks.2.proj_mlp",
                    "single_transformer_blocks.2.proj_out", "single_transformer_blocks.2.attn.to_k",
                    "single_transformer_blocks.0.norm.linear", "context_embedder", "norm_out.linear",
                    "time_text_embed.timestep_embedder.linear_1"]
    sd = {}
    for m in flux_modules:
        sd[f"transformer.{m}.lora_A.weight"], sd[f"transformer.{m}.lora_B.weight"] = a, b
    targets = parse_lora_state_dict(sd)
    assert sorted(targets) == sorted(m + ".weight" for m in flux_modules)
    names = set(lora_target_names("flux", n_double=2, n_single=3))
    assert set(targets) <= names
    assert "proj_out.weight" not in names and "x_embedder.weight" not in names          # the fp32 head; the (padded) image embedder
    assert not any(n.endswith(".bias") or "norm_q" in n for n in names)

    qwen_modules = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.add_v_proj", "transformer_blocks.0.attn.to_out.0",
                    "transformer_blocks.1.img_mlp.net.0.proj", "transformer_blocks.1.txt_mlp.net.2", "transformer_blocks.1.img_mod.1",
                    "transformer_blocks.1.txt_mod.1", "txt_in", "norm_out.linear"]
    sd = {}
    for m in qwen_modules:
        sd[f"transformer.{m}.lora.down.weight"], sd[f"transformer.{m}.lora.up.weight"] = a, b
    targets = parse_lora_state_dict(sd)
    names = set(lora_target_names("qwen", n_double=2))
    assert set(targets) == {m + ".weight" for m in qwen_modules} and set(targets) <= names
    assert "img_in.weight" not in names and not any("single" in n for n in names)
    hy = set(lora_target_names("hunyuan", n_double=1, n_single=1, refiner_depth=1))
    assert {"single_blocks.0.linear1.weight", "double_blocks.0.img_attn_qkv.weight",
            "txt_in.individual_token_refiner.blocks.0.mlp.fc1.weight"} <= hy and "final_layer.linear.weight" not in hy
    with pytest.raises(ValueError):
        lora_target_names("wan", 1)


def test_every_target_name_is_a_name_the_engine_registers():
    """lora_target_names restates the engine's naming: every name must be a string mmdit_engine.cpp can build (its prefixes
    and part names appear there literally)."""
    src = open(os.path.join(ROOT, "magcache_amd", "csrc", "mmdit_engine.cpp")).read()
    literals = set(re.findall(r'"([^"\n]*)"', src))
    for family, kw in (("flux", dict(n_double=1, n_single=1)), ("qwen", dict(n_double=1)),
                       ("hunyuan", dict(n_double=1, n_single=1, refiner_depth=1))):
        for name in lora_target_names(family, **kw):
            stem = re.sub(r"\.weight$", "", name)
            stem = re.sub(r"^(transformer_blocks|single_transformer_blocks|double_blocks|single_blocks|"
                          r"txt_in\.individual_token_refiner\.blocks)\.\d+\.", "", stem)
            stem = re.sub(r"^(img|txt)(_mod\.linear|_attn_qkv|_attn_proj|_mlp\.fc1|_mlp\.fc2)$", r"\2", stem)      # HunyuanVideo: q + part
            stem = re.sub(r"^(ff|ff_context|img_mlp|txt_mlp)(\.net\.)", r"\2", stem)
            assert stem in literals, (family, name, stem)


def test_lora_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read()
    lib = _lib.load()
    for n in ("mc_mmdit_lora_set", "mc_mmdit_lora_scale", "mc_mmdit_lora_remove", "mc_mmdit_lora_apply", "mc_mmdit_lora_info"):
        assert n + "(" in hdr and n in _lib.SIGNATURES and hasattr(lib, n)
    hip = open(os.path.join(ROOT, "include", "magcache_hip.h")).read()
    assert "mc_op_lora_merge(" in hip and "mc_op_lora_merge" in _lib.SIGNATURES and hasattr(lib, "mc_op_lora_merge")
    assert _lib.MC_LORA_MAX_TERMS == int(re.search(r"#define MC_LORA_MAX_TERMS (\d+)", hip).group(1))
    # scratch arithmetic is host only: both operands of every term, rank padded to 16, rows to 32, 256-byte granules
    t = (_lib.McLoraTerm * 2)(_lib.McLoraTerm(None, None, 4, 1.0), _lib.McLoraTerm(None, None, 130, 1.0))
    assert lib.mc_op_lora_merge_scratch(200, 520, t, 2) == (224 + 544) * 16 * 2 + (224 + 544) * 144 * 2
    # the shims ignore the per-call scale without adapters: no engine call is made
    from types import SimpleNamespace
    from magcache_amd import mmdit as MM
    MM._lora_call_scale(SimpleNamespace(engine=SimpleNamespace(_lora={})), {"scale": 0.5})
    MM._lora_call_scale(SimpleNamespace(engine=SimpleNamespace()), {"scale": 0.5})

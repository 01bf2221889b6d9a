"""CPU: the Wan adapter reader (magcache_amd/lora.py: parse_wan_lora_state_dict, wan_lora_target_names), the C declarations of
the Wan engine's adapter calls and the Python surface that carries them.  No GPU, no engine."""
import inspect
import os
import re

import pytest
import torch

from magcache_amd import _lib
from magcache_amd import engine as E
from magcache_amd import generate as G
from magcache_amd import mmdit as MM
from magcache_amd import model as M
from magcache_amd.adapters import LoraHost
from magcache_amd.lora import lora_factor, parse_wan_lora_state_dict, wan_lora_target_names
from oracle import wan_dit_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, R = 8, 2


def pair(module, down_key, up_key, rank=R, rows=D, k=D):
    return {module + down_key: torch.full((rank, k), 1.0), module + up_key: torch.full((rows, rank), 2.0)}


@pytest.mark.parametrize("down_key,up_key", [(".lora_A.weight", ".lora_B.weight"), (".lora_A.default.weight", ".lora_B.default.weight"),
                                             (".lora.down.weight", ".lora.up.weight"), (".lora_down.weight", ".lora_up.weight")])
@pytest.mark.parametrize("prefix", ["", "diffusion_model.", "model.diffusion_model.", "transformer."])
def test_every_pair_spelling_under_every_prefix(down_key, up_key, prefix):
    sd = {prefix + k: v for k, v in pair("blocks.3.self_attn.q", down_key, up_key, rows=12).items()}
    sd[prefix + "blocks.3.self_attn.q.alpha"] = torch.tensor(4.0)
    if prefix:
        sd["text_encoder.layers.0.lora_A.weight"] = torch.zeros(2, 2)        # another component's: not the adapter
    out = parse_wan_lora_state_dict(sd)
    assert list(out) == ["blocks.3.self_attn.q.weight"]
    kind, down, up, alpha = out["blocks.3.self_attn.q.weight"]
    assert kind == "pair" and tuple(down.shape) == (R, D) and tuple(up.shape) == (12, R) and alpha == 4.0
    assert float(down[0, 0]) == 1.0 and float(up[0, 0]) == 2.0
    assert lora_factor(down, alpha) == 2.0 and lora_factor(down, None) == 1.0       # alpha -> factor


def test_the_three_delta_spellings():
    sd = {"diffusion_model.blocks.0.self_attn.norm_q.diff": torch.zeros(D),
          "diffusion_model.blocks.0.self_attn.q.diff_b": torch.ones(D),
          "diffusion_model.blocks.1.diff_m": torch.zeros(1, 6, D),
          "diffusion_model.head.diff_m": torch.zeros(1, 2, D),
          "diffusion_model.time_embedding.0.diff": torch.zeros(D, 4)}
    out = parse_wan_lora_state_dict(sd)
    assert {k: v[0] for k, v in out.items()} == {
        "blocks.0.self_attn.norm_q.weight": "delta", "blocks.0.self_attn.q.bias": "delta", "blocks.1.modulation": "delta",
        "head.modulation": "delta", "time_embedding.0.weight": "delta"}
    assert float(out["blocks.0.self_attn.q.bias"][1][0]) == 1.0


DIFFUSERS = {"blocks.2.attn1.to_q": "blocks.2.self_attn.q", "blocks.2.attn1.to_k": "blocks.2.self_attn.k",
             "blocks.2.attn1.to_v": "blocks.2.self_attn.v", "blocks.2.attn1.to_out.0": "blocks.2.self_attn.o",
             "blocks.2.attn2.to_q": "blocks.2.cross_attn.q", "blocks.2.attn2.to_k": "blocks.2.cross_attn.k",
             "blocks.2.attn2.to_v": "blocks.2.cross_attn.v", "blocks.2.attn2.to_out.0": "blocks.2.cross_attn.o",
             "blocks.2.attn2.add_k_proj": "blocks.2.cross_attn.k_img", "blocks.2.attn2.add_v_proj": "blocks.2.cross_attn.v_img",
             "blocks.2.ffn.net.0.proj": "blocks.2.ffn.0", "blocks.2.ffn.net.2": "blocks.2.ffn.2",
             "condition_embedder.time_embedder.linear_1": "time_embedding.0",
             "condition_embedder.time_embedder.linear_2": "time_embedding.2",
             "condition_embedder.time_proj": "time_projection.1",
             "condition_embedder.text_embedder.linear_1": "text_embedding.0",
             "condition_embedder.text_embedder.linear_2": "text_embedding.2",
             "proj_out": "head.head"}


def test_the_diffusers_table():
    sd = {}
    for module in DIFFUSERS:
        sd.update({"transformer." + k: v for k, v in pair(module, ".lora_A.weight", ".lora_B.weight").items()})
    sd["transformer.blocks.2.norm2.diff"] = torch.zeros(D)
    sd["transformer.blocks.2.norm2.diff_b"] = torch.zeros(D)
    sd["transformer.blocks.2.scale_shift_table.diff"] = torch.zeros(1, 6, D)
    sd["transformer.scale_shift_table.diff"] = torch.zeros(1, 2, D)
    out = parse_wan_lora_state_dict(sd)
    want = {v + ".weight": "pair" for v in DIFFUSERS.values()}
    want.update({"blocks.2.norm3.weight": "delta", "blocks.2.norm3.bias": "delta", "blocks.2.modulation": "delta",
                 "head.modulation": "delta"})
    assert {k: v[0] for k, v in out.items()} == want


def test_orphans_mismatched_ranks_and_repeats_raise():
    good = pair("blocks.0.ffn.0", ".lora_A.weight", ".lora_B.weight")
    for extra in ({"blocks.0.ffn.0.weight": torch.zeros(2)},                       # a plain weight: a checkpoint key, no adapter's
                  {"blocks.0.ffn.2.lora_A.weight": torch.zeros(R, D)},             # down without up
                  {"blocks.0.ffn.2.lora_up.weight": torch.zeros(D, R)},            # up without down
                  {"blocks.0.ffn.2.alpha": torch.tensor(1.0)}):                    # alpha without a pair
        with pytest.raises(ValueError, match="belong to no"):
            parse_wan_lora_state_dict(dict(good, **extra))
    with pytest.raises(ValueError, match="share no rank"):
        parse_wan_lora_state_dict({"m.lora_A.weight": torch.zeros(2, D), "m.lora_B.weight": torch.zeros(D, 3)})
    with pytest.raises(ValueError, match="repeats"):                               # two spellings of the same matrix
        parse_wan_lora_state_dict(dict(good, **{"blocks.0.ffn.0.lora_down.weight": torch.zeros(R, D)}))
    with pytest.raises(ValueError, match="repeats"):                               # two names of one parameter
        parse_wan_lora_state_dict({"head.diff_m": torch.zeros(2), "scale_shift_table.diff": torch.zeros(2)})
    with pytest.raises(ValueError, match="a low-rank pair and a delta"):
        parse_wan_lora_state_dict(dict(good, **{"blocks.0.ffn.0.diff": torch.zeros(D, D)}))
    assert parse_wan_lora_state_dict({}) == {}


@pytest.mark.parametrize("kind", ["t2v", "i2v", "vace"])
def test_target_names_are_the_state_dict_minus_the_patch_embedders(kind):
    cfg = W.tiny_config(num_layers=2, num_heads=2, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64, i2v=kind == "i2v")
    if kind == "vace":
        vace = dict(vace_layers=[0], vace_in_dim=16)
        oracle, cfg = W.VaceWanModel(**cfg, **vace), dict(cfg, model_type="vace", **vace)
    else:
        oracle = W.WanModel(**cfg)
    names = wan_lora_target_names(cfg)
    assert len(names) == len(set(names))
    padded = {"patch_embedding.weight", "vace_patch_embedding.weight"}
    assert set(names) == set(oracle.state_dict()) - padded
    assert set(names) == {n for n, _ in E.weight_names(cfg)} - padded              # what a tiny engine registers
    for n in ("blocks.1.self_attn.q.weight", "blocks.0.modulation", "head.modulation", "time_embedding.0.weight", "head.head.weight",
              "blocks.0.self_attn.q.bias", "blocks.1.cross_attn.norm_k.weight"):
        assert n in names


C_TYPES = {"mc_engine*": _lib._vp, "const mc_engine*": _lib._vp, "const char*": _lib.C.c_char_p, "const void*": _lib._vp,
           "const int64_t*": _lib.C.POINTER(_lib.C.c_int64), "mc_dtype": _lib._i, "float": _lib._f, "mc_stream": _lib._vp,
           "size_t": _lib._sz, "int*": _lib.C.POINTER(_lib._i), "size_t*": _lib.C.POINTER(_lib._sz), "const float*": _lib._vp,
           "float*": _lib._vp, "long": _lib._l, "int": _lib._i, "const mc_lora_term*": _lib._vp, "void*": _lib._vp,
           "const float* const*": _lib.C.POINTER(_lib._vp)}


def test_the_new_calls_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "magcache_hip.h")).read()
    lib = _lib.load()
    for name in ("mc_lora_set", "mc_lora_set_delta", "mc_lora_scale", "mc_lora_remove", "mc_lora_apply", "mc_lora_info",
                 "mc_op_lora_merge_f32", "mc_op_param_delta"):
        m = re.search(r"mc_status\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in magcache_hip.h"
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        want = [C_TYPES[t] for t in types]
        if name == "mc_op_param_delta":
            want[4] = _lib.C.POINTER(_lib._f)           # the scales are a HOST array of floats
        assert res is _lib._i and args == want, (name, types)
    assert b"0.7.1" in lib.mc_version()
    # null engines and null arguments are refused before anything is touched
    assert lib.mc_lora_apply(None, None) == _lib.MC_EINVAL and lib.mc_lora_info(None, None, None, None) == _lib.MC_EINVAL
    assert lib.mc_lora_set_delta(None, b"a", b"w", None, 0, 0, None) == _lib.MC_EINVAL
    assert lib.mc_op_param_delta(None, None, 0, None, None, 1, None) == _lib.MC_EINVAL
    assert lib.mc_op_lora_merge_f32(None, 4, None, 4, 1, 4, None, 0, None, 0, None) == _lib.MC_EINVAL


def test_python_surface_and_shared_bookkeeping():
    methods = ("load_lora", "set_adapters", "set_lora_call_scale", "unload_lora", "apply_lora", "lora_info")
    for name in methods:
        # ONE implementation behind both engines
        assert getattr(E.Engine, name) is getattr(LoraHost, name) and getattr(MM.MMDiTEngine, name) is getattr(LoraHost, name)
        assert callable(getattr(M.WanModelHIP, name))
    assert E.Engine._lora_abi == "mc_lora_" and MM.MMDiTEngine._lora_abi == "mc_mmdit_lora_"
    assert list(inspect.signature(M.WanModelHIP.load_lora).parameters) == ["self", "sd", "adapter", "scale", "strict"]
    # every WanModelHIP method that applies forgets the identity keys of the cached contexts, also when the engine raises
    calls = []

    class Boom:
        def __getattr__(self, name):
            def f(*a, **k):
                calls.append(name)
                if name == "unload_lora":
                    raise RuntimeError("boom")
            return f
    m = M.WanModelHIP.__new__(M.WanModelHIP)
    m.engine = Boom()
    for name, args in (("load_lora", ({},)), ("set_adapters", ("a",)), ("set_lora_call_scale", (0.5,)), ("apply_lora", ()),
                       ("unload_lora", ())):
        m._ctx_keys, m._clip_key, m._vace_key = ["k0", "k1"], "c", "v"
        if name == "unload_lora":
            with pytest.raises(RuntimeError):
                getattr(m, name)(*args)
        else:
            getattr(m, name)(*args)
        assert m._ctx_keys == [None, None] and m._clip_key is None and m._vace_key is None, name
    assert calls == ["load_lora", "set_adapters", "set_lora_call_scale", "apply_lora", "unload_lora"]


def test_generate_lora_file_flag_parses():
    a = G._parse_args(["--task", "t2v-1.3B", "--size", "832*480", "--lora_file", "a.safetensors", "--lora_file", "b.safetensors:0.25"])
    assert a.lora_file == ["a.safetensors", "b.safetensors:0.25"]
    assert [G._lora_spec(s) for s in a.lora_file] == [("a.safetensors", 1.0), ("b.safetensors", 0.25)]
    assert G._lora_spec("C:/x/y.safetensors") == ("C:/x/y.safetensors", 1.0)       # a colon that is no scale's
    assert G._parse_args(["--task", "t2v-1.3B", "--size", "832*480"]).lora_file == []

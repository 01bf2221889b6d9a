"""CPU: the readers of DoRA, LoKr and LoHa adapter files (magcache_amd/lora.py: parse_adapter_state_dict,
parse_wan_adapter_state_dict), their factor rules, the C declarations of the new calls and the refusals the single-op call makes
before it touches the device.  No GPU, no engine."""
import ctypes as C
import os
import re

import pytest
import torch

import adapter_kinds_ref as AR
from magcache_amd import _lib
from magcache_amd import engine as E
from magcache_amd import mmdit as MM
from magcache_amd.adapters import LoraHost
from magcache_amd.lora import (dora_magnitude, loha_factor, lokr_factor, lora_factor, parse_adapter_state_dict,
                               parse_lora_state_dict, parse_wan_adapter_state_dict, parse_wan_lora_state_dict)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, IN, R = 12, 16, 2
MOD = "transformer_blocks.0.attn.to_q"
WAN_MOD = "blocks.3.self_attn.q"


def t(*shape, v=1.0):
    return torch.full(shape, float(v))


def readers():
    """(reader, prefix of the file's keys, module as the file spells it, target) of both engines; the Wan case goes through
    diffusers' module names"""
    return [(parse_adapter_state_dict, "transformer.", MOD, MOD + ".weight"),
            (parse_adapter_state_dict, "", MOD, MOD + ".weight"),
            (parse_wan_adapter_state_dict, "diffusion_model.", WAN_MOD, WAN_MOD + ".weight"),
            (parse_wan_adapter_state_dict, "transformer.", "blocks.3.attn1.to_q", WAN_MOD + ".weight")]


def pre(prefix, sd):
    out = {prefix + k: v for k, v in sd.items()}
    if prefix:
        out["text_encoder.layers.0.q_proj.lora_A.weight"] = t(2, 2)     # another component's
    return out


# ---------------------------------------------------------------------------------------------------- DoRA
@pytest.mark.parametrize("spelling", AR.MAGNITUDE_SPELLINGS + (".lora_magnitude_vector.my_style", ".dora_scale.default"))
@pytest.mark.parametrize("column", [False, True], ids=["[out]", "[out,1]"])
def test_dora_every_spelling_and_shape(spelling, column):
    g = torch.arange(OUT).float()
    for reader, prefix, module, target in readers():
        a, b = t(R, IN), t(OUT, R, v=2)
        sd = pre(prefix, dict(AR.pair_keys(module, a, b, alpha=4.0), **AR.magnitude_keys(module, g, spelling, column)))
        out = reader(sd)
        assert list(out) == [target]
        kind, inner, mag = out[target]
        assert kind == "dora" and inner[0] == "pair" and inner[1] is a and inner[2] is b and inner[3] == 4.0
        assert tuple(mag.shape) == (OUT,) and torch.equal(mag, g)


def test_dora_refusals():
    a, b, g = t(R, IN), t(OUT, R), t(OUT)
    for reader, prefix, module, _ in readers():
        with pytest.raises(ValueError, match="per-input-column"):                      # LyCORIS's [1, in] variant
            reader(pre(prefix, dict(AR.pair_keys(module, a, b), **{module + ".dora_scale": t(1, IN)})))
        with pytest.raises(ValueError, match="no term"):                               # a magnitude alone
            reader(pre(prefix, AR.magnitude_keys(module, g)))
        with pytest.raises(ValueError, match="two spellings"):                         # PEFT's and LyCORIS's key at once
            reader(pre(prefix, dict(AR.pair_keys(module, a, b), **AR.magnitude_keys(module, g),
                                    **AR.magnitude_keys(module, g, ".dora_scale"))))
        with pytest.raises(ValueError, match=r"expected \[out\]"):
            reader(pre(prefix, dict(AR.pair_keys(module, a, b), **{module + ".dora_scale": t(OUT, 2)})))
    assert tuple(dora_magnitude("m", t(1, 1)).shape) == (1,)                           # [1, 1] is [out, 1] with one row
    with pytest.raises(ValueError, match="no term"):                                   # a Wan delta is no term to normalise
        parse_wan_adapter_state_dict({"blocks.0.ffn.0.diff": t(OUT, IN), "blocks.0.ffn.0.dora_scale": g})


def test_dora_over_lokr_and_loha():
    g = t(OUT)
    for reader, prefix, module, target in readers():
        out = reader(pre(prefix, dict(AR.lokr_keys(module, t(3, 4), t(4, 4)), **AR.magnitude_keys(module, g, ".dora_scale", True))))
        assert out[target][0] == "dora" and out[target][1][0] == "kron" and tuple(out[target][2].shape) == (OUT,)
        out = reader(pre(prefix, dict(AR.loha_keys(module, t(OUT, R), t(R, IN), t(OUT, R), t(R, IN)), **AR.magnitude_keys(module, g))))
        assert out[target][0] == "dora" and out[target][1][0] == "hada"


# ---------------------------------------------------------------------------------------------------- LoKr
@pytest.mark.parametrize("infix", ["", ".default"])
def test_lokr_full_and_factorised_halves(infix):
    w1, w2 = t(3, 4), t(4, 4, v=2)
    w1a, w1b, w2a, w2b = t(3, R), t(R, 4), t(4, R), t(R, 4)
    for reader, prefix, module, target in readers():
        # both halves full: factor 1 whatever alpha says
        out = reader(pre(prefix, AR.lokr_keys(module, w1, w2, alpha=8.0, infix=infix)))
        assert list(out) == [target]
        kind, h1, h2, factor = out[target]
        assert kind == "kron" and h1 is w1 and h2 is w2 and factor == 1.0
        # w2 factorised: alpha / rank; no alpha: 1
        out = reader(pre(prefix, AR.lokr_keys(module, w1, (w2a, w2b), alpha=8.0, infix=infix)))
        kind, h1, h2, factor = out[target]
        assert h1 is w1 and h2[0] is w2a and h2[1] is w2b and factor == 8.0 / R
        assert reader(pre(prefix, AR.lokr_keys(module, w1, (w2a, w2b), infix=infix)))[target][3] == 1.0
        # both factorised, and w1 alone
        out = reader(pre(prefix, AR.lokr_keys(module, (w1a, w1b), (w2a, w2b), alpha=1.0, infix=infix)))
        assert isinstance(out[target][1], tuple) and isinstance(out[target][2], tuple) and out[target][3] == 1.0 / R
        assert reader(pre(prefix, AR.lokr_keys(module, (w1a, w1b), w2, alpha=3.0, infix=infix)))[target][3] == 3.0 / R


def test_lokr_refusals():
    w1, w2 = t(3, 4), t(4, 4)
    for reader, prefix, module, _ in readers():
        with pytest.raises(ValueError, match="Tucker"):
            reader(pre(prefix, dict(AR.lokr_keys(module, w1, w2), **{module + ".lokr_t2": t(2, 2, 3, 3)})))
        with pytest.raises(ValueError, match="two spellings"):                         # lokr_w2 and its factorised form
            reader(pre(prefix, dict(AR.lokr_keys(module, w1, w2), **{module + ".lokr_w2_a": t(4, R), module + ".lokr_w2_b": t(R, 4)})))
        with pytest.raises(ValueError, match="two spellings"):                         # with and without the adapter infix
            reader(pre(prefix, dict(AR.lokr_keys(module, w1, w2), **{module + ".lokr_w1.default": w1})))
        with pytest.raises(ValueError, match="share no rank"):                         # a (x) b with different inner sizes
            reader(pre(prefix, AR.lokr_keys(module, w1, (t(4, 2), t(3, 4)))))
        with pytest.raises(ValueError, match="share no rank"):                         # two factorised halves of different rank
            reader(pre(prefix, AR.lokr_keys(module, (t(3, 2), t(2, 4)), (t(4, 3), t(3, 4)))))
        with pytest.raises(ValueError, match="belong to no"):                          # half a set
            reader(pre(prefix, {module + ".lokr_w1": w1}))
        with pytest.raises(ValueError, match="two kinds"):                             # a pair and a LoKr term on one module
            reader(pre(prefix, dict(AR.lokr_keys(module, w1, w2), **AR.pair_keys(module, t(R, IN), t(OUT, R)))))
        with pytest.raises(ValueError, match="LoKr and LoHa"):
            reader(pre(prefix, dict(AR.lokr_keys(module, w1, w2), **AR.loha_keys(module, t(OUT, R), t(R, IN), t(OUT, R), t(R, IN)))))


# ---------------------------------------------------------------------------------------------------- LoHa
@pytest.mark.parametrize("infix", ["", ".default"])
def test_loha_keys_and_factor(infix):
    w1a, w1b, w2a, w2b = t(OUT, R), t(R, IN, v=2), t(OUT, R, v=3), t(R, IN, v=4)
    for reader, prefix, module, target in readers():
        out = reader(pre(prefix, AR.loha_keys(module, w1a, w1b, w2a, w2b, alpha=1.0, infix=infix)))
        assert list(out) == [target]
        kind, a, b, c, d, factor = out[target]
        assert kind == "hada" and a is w1a and b is w1b and c is w2a and d is w2b and factor == 1.0 / R
        assert reader(pre(prefix, AR.loha_keys(module, w1a, w1b, w2a, w2b, infix=infix)))[target][5] == 1.0


def test_loha_refusals():
    w1a, w1b, w2a, w2b = t(OUT, R), t(R, IN), t(OUT, R), t(R, IN)
    for reader, prefix, module, _ in readers():
        good = AR.loha_keys(module, w1a, w1b, w2a, w2b)
        with pytest.raises(ValueError, match="Tucker"):
            reader(pre(prefix, dict(good, **{module + ".hada_t1": t(R, R, 3, 3)})))
        with pytest.raises(ValueError, match="Tucker"):
            reader(pre(prefix, dict(good, **{module + ".hada_t2": t(R, R, 3, 3)})))
        with pytest.raises(ValueError, match="share no rank"):
            reader(pre(prefix, AR.loha_keys(module, w1a, w1b, t(OUT, 3), t(3, IN))))
        with pytest.raises(ValueError, match="share no rank"):
            reader(pre(prefix, AR.loha_keys(module, w1a, t(3, IN), w2a, w2b)))
        with pytest.raises(ValueError, match="belong to no"):
            reader(pre(prefix, {k: v for k, v in good.items() if "w2_b" not in k}))
        with pytest.raises(ValueError, match="two spellings"):
            reader(pre(prefix, dict(good, **{module + ".hada_w1_a.default": w1a})))


def test_the_factor_rules():
    assert lokr_factor(8.0, 4) == 2.0 and lokr_factor(8.0, None) == 1.0 and lokr_factor(None, 4) == 1.0
    assert loha_factor(8.0, 4) == 2.0 and loha_factor(None, 4) == 1.0
    assert lora_factor(t(4, IN), 8.0) == 2.0                                           # the pair of a DoRA module keeps its rule


# ---------------------------------------------------------------------------------------------------- plain LoRA files
def test_plain_lora_files_give_the_old_readers_entries():
    import test_lora_cpu as TL
    import test_wan_lora_cpu as TW
    a, b = TL.pair(8, 16, 4)
    cases = []
    for infix in ("", ".default", ".my_style"):
        cases.append({f"transformer_blocks.0.attn.to_q.lora_A{infix}.weight": a, f"transformer_blocks.0.attn.to_q.lora_B{infix}.weight": b})
    cases.append({"single_transformer_blocks.1.proj_mlp.lora.down.weight": a, "single_transformer_blocks.1.proj_mlp.lora.up.weight": b,
                  "single_transformer_blocks.1.proj_mlp.alpha": torch.tensor(8.0)})
    cases.append({"x.lora_A.weight": a, "x.lora_B.weight": b, "x.alpha": 2})
    cases.append({"transformer.transformer_blocks.0.ff.net.2.lora_A.weight": a, "transformer.transformer_blocks.0.ff.net.2.lora_B.weight": b,
                  "text_encoder.layers.0.q_proj.lora_A.weight": a, "text_encoder.layers.0.q_proj.lora_B.weight": b})
    for sd in cases:
        for prefix in ("transformer.", "", "unet."):
            old, new = parse_lora_state_dict(sd, prefix=prefix), parse_adapter_state_dict(sd, prefix=prefix)
            assert list(new) == list(old)
            for k in old:
                assert len(new[k]) == 3 and all(x is y or x == y for x, y in zip(new[k], old[k])), k
    # ... and the old reader's refusals
    for bad, match in (({"m.lora_A.weight": a}, "down without up"), ({"m.lora_A.weight": a, "m.lora_B.weight": torch.zeros(8, 5)}, "share no rank"),
                       ({"m.lora_A.weight": a, "m.lora_B.weight": b, "m.weight": torch.zeros(8, 16)}, "belong to no")):
        with pytest.raises(ValueError, match=match):
            parse_adapter_state_dict(bad)
    # Wan: every pair spelling under every prefix, the delta spellings, the diffusers table
    wan = []
    for down_key, up_key in ((".lora_A.weight", ".lora_B.weight"), (".lora_A.default.weight", ".lora_B.default.weight"),
                             (".lora.down.weight", ".lora.up.weight"), (".lora_down.weight", ".lora_up.weight")):
        for prefix in ("", "diffusion_model.", "model.diffusion_model.", "transformer."):
            sd = {prefix + k: v for k, v in TW.pair("blocks.3.self_attn.q", down_key, up_key, rows=12).items()}
            sd[prefix + "blocks.3.self_attn.q.alpha"] = torch.tensor(4.0)
            wan.append(sd)
    wan.append({"diffusion_model.blocks.0.self_attn.norm_q.diff": torch.zeros(8), "diffusion_model.blocks.0.self_attn.q.diff_b": torch.ones(8),
                "diffusion_model.blocks.1.diff_m": torch.zeros(1, 6, 8), "diffusion_model.head.diff_m": torch.zeros(1, 2, 8)})
    table = {}
    for module in TW.DIFFUSERS:
        table.update({"transformer." + k: v for k, v in TW.pair(module, ".lora_A.weight", ".lora_B.weight").items()})
    table["transformer.blocks.2.scale_shift_table.diff"] = torch.zeros(1, 6, 8)
    wan.append(table)
    for sd in wan:
        old, new = parse_wan_lora_state_dict(sd), parse_wan_adapter_state_dict(sd)
        assert list(new) == list(old)
        for k in old:
            assert len(new[k]) == len(old[k]) and all(x is y or x == y for x, y in zip(new[k], old[k])), k
    assert parse_adapter_state_dict({}) == {} and parse_wan_adapter_state_dict({}) == {}


def test_both_hosts_read_through_the_new_readers():
    sd = {"transformer." + k: v for k, v in AR.lokr_keys(MOD, t(3, 4), t(4, 4)).items()}
    host = LoraHost.__new__(LoraHost)
    assert LoraHost._lora_entries(host, sd, "transformer.")[MOD + ".weight"][0] == "kron"
    plain = LoraHost._lora_entries(host, {"transformer." + k: v for k, v in AR.pair_keys(MOD, t(R, IN), t(OUT, R)).items()}, "transformer.")
    assert plain[MOD + ".weight"][0] == "pair" and len(plain[MOD + ".weight"]) == 4
    wan = E.Engine._lora_entries(E.Engine.__new__(E.Engine), {"diffusion_model." + k: v for k, v in
                                                               AR.loha_keys(WAN_MOD, t(OUT, R), t(R, IN), t(OUT, R), t(R, IN)).items()}, "")
    assert wan[WAN_MOD + ".weight"][0] == "hada"
    assert MM.MMDiTEngine._lora_entries is LoraHost._lora_entries


# ---------------------------------------------------------------------------------------------------- the C surface
C_TYPES = {"mc_engine*": _lib._vp, "mc_mmdit*": _lib._vp, "const char*": C.c_char_p, "const void*": _lib._vp, "void*": _lib._vp,
           "const int64_t*": C.POINTER(C.c_int64), "mc_dtype": _lib._i, "float": _lib._f, "mc_stream": _lib._vp, "size_t": _lib._sz,
           "long": _lib._l, "int": _lib._i, "const mc_adapter_term*": _lib._vp, "const float*": _lib._vp}
NEW_CALLS = {"magcache_hip.h": ("mc_lora_set_kron", "mc_lora_set_hada", "mc_lora_set_magnitude", "mc_op_adapter_merge",
                                "mc_op_adapter_merge_scratch"),
             "magcache_mmdit.h": ("mc_mmdit_lora_set_kron", "mc_mmdit_lora_set_hada", "mc_mmdit_lora_set_magnitude")}


def test_the_new_calls_are_declared_exported_and_bound():
    lib = _lib.load()
    for header, names in NEW_CALLS.items():
        hdr = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            m = re.search(r"(mc_status|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
            assert m, f"{name} is not declared in {header}"
            params = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
            types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]
            assert hasattr(lib, name), f"{name} is not exported"
            res, args = _lib.SIGNATURES[name]
            assert res is (_lib._i if m.group(1) == "mc_status" else _lib._sz) and args == [C_TYPES[x] for x in types], (name, types)
    # the struct of the header and the ctypes structure: same fields in the same order, same constants
    hdr = open(os.path.join(ROOT, "include", "magcache_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct mc_adapter_term \{(.*?)\} mc_adapter_term;", hdr, re.S).group(1), flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?\w+\s+", "", decl.strip()))]
    assert fields == [n for n, _ in _lib.McAdapterTerm._fields_], fields
    for name in ("MC_ADAPTER_PAIR", "MC_ADAPTER_KRON", "MC_ADAPTER_HADA"):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == getattr(_lib, name)
    # null engines are refused before anything is touched
    assert lib.mc_lora_set_kron(None, b"a", b"w", None, None, None, None, 0, 1.0, None) == _lib.MC_EINVAL
    assert lib.mc_mmdit_lora_set_hada(None, b"a", b"w", None, None, None, None, None, None, 0, 1.0, None) == _lib.MC_EINVAL
    assert lib.mc_mmdit_lora_set_magnitude(None, b"a", b"w", None, 0, 0, None) == _lib.MC_EINVAL


def term(kind, scale=1.0, a=0x1000, b=0x1000, c=0, d=0, rank=0, r1=0, c1=0, r2=0, c2=0):
    return _lib.McAdapterTerm(kind, scale, a, b, c, d, rank, r1, c1, r2, c2)


def test_the_single_op_refuses_bad_arguments_before_it_touches_the_device():
    """every MC_EINVAL of mc_op_adapter_merge that depends on the arguments alone; the pointers are never read"""
    lib = _lib.load()
    rows, K = 160, 520
    base, out = C.c_void_p(0x10000), C.c_void_p(0x20000)

    def call(terms, rows=rows, K=K, ld_base=K, ld_out=K, base=base, out=out, mag=None, scratch=None, nbytes=0):
        arr = (_lib.McAdapterTerm * max(len(terms), 1))(*terms)
        return lib.mc_op_adapter_merge(base, ld_base, out, ld_out, rows, K, arr, len(terms), mag, scratch, nbytes, None)
    good_kron = term(_lib.MC_ADAPTER_KRON, r1=8, c1=5, r2=20, c2=104)
    for bad in ([term(7)],                                                             # an unknown kind
                [term(_lib.MC_ADAPTER_KRON, r1=8, c1=5, r2=21, c2=104)],               # r1 * r2 != rows: the shape does not factor
                [term(_lib.MC_ADAPTER_KRON, r1=8, c1=5, r2=20, c2=100)],               # c1 * c2 != K
                [term(_lib.MC_ADAPTER_PAIR, rank=0)], [term(_lib.MC_ADAPTER_HADA, c=0x1000, d=0x1000, rank=0)],
                [term(_lib.MC_ADAPTER_HADA, rank=5)],                                  # null u2 / d2
                [good_kron] * (_lib.MC_LORA_MAX_TERMS + 1)):
        assert call(bad) == _lib.MC_EINVAL, lib.mc_last_error()
    assert b"at most" in lib.mc_last_error()
    assert call([good_kron], base=C.c_void_p(0x10002)) == _lib.MC_EINVAL               # misaligned base
    assert call([good_kron], ld_out=K + 4) == _lib.MC_EINVAL                           # a pitch that is no multiple of 8
    assert call([good_kron], ld_base=K - 8) == _lib.MC_EINVAL                          # a pitch below K
    assert call([term(_lib.MC_ADAPTER_KRON, r1=8, c1=5, r2=20, c2=103)], K=515, ld_base=520, ld_out=520) == _lib.MC_EINVAL  # K % 8
    arr = (_lib.McAdapterTerm * 1)(good_kron)
    need = lib.mc_op_adapter_merge_scratch(rows, K, arr, 1)
    assert need == (rows * K * 4 + 255) // 256 * 256                                   # the fp32 image of the part, nothing else
    assert call([good_kron], scratch=C.c_void_p(0x30000), nbytes=need - 1) == _lib.MC_EINVAL and b"scratch" in lib.mc_last_error()
    pair = (_lib.McAdapterTerm * 1)(term(_lib.MC_ADAPTER_PAIR, rank=5))
    old = (_lib.McLoraTerm * 1)(_lib.McLoraTerm(0x1000, 0x1000, 5, 1.0))
    assert lib.mc_op_adapter_merge_scratch(rows, K, pair, 1) == need + lib.mc_op_lora_merge_scratch(rows, K, old, 1)

"""Helpers of tests/test_mmdit_fp8_gpu.py and tests/test_mmdit_fp8_cpu.py: the toy MM-DiT families at width 512 (the MX GEMM
needs K >= 512, so 4 heads), their inputs, their fp32 oracles, and the fake-quant oracle -- the fp32 oracle with the
nn.Linears that mc_mmdit_config.fp8_linear moves to MX fp8 replaced by a wrapper that MX-quantises and dequantises the
bf16-rounded input and the bf16-rounded weight (hip_ops.mx_quantize_ref, the torch restatement of the device quantiser) and
multiplies in fp32.  The oracle's separate q, k, v Linears together stand for the engine's fused q|k|v: a block scale belongs to
one output channel, so fusing changes no scale."""
import copy
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import flux_ref as FR
from oracle import hunyuan_ref as HR

import qwen_image_ref as QR
from hip_ops import mx_quantize_ref

DIM, HEADS = 512, 4


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def mx_round(x):
    """x [..., K] -> the values an MX fp8 operand holds: bf16 rounding, then e4m3 relative to one E8M0 scale per 32 k"""
    x2 = x.detach().to(torch.bfloat16).float().reshape(-1, x.shape[-1])
    q, s = mx_quantize_ref(x2)
    d = q.float().view(x2.shape[0], -1, 32) * torch.exp2(s.float() - 127.0)[..., None]
    return d.view(x.shape)


class MXLinear(nn.Module):
    def __init__(self, lin):
        super().__init__()
        self.w, self.b = mx_round(lin.weight), lin.bias.detach()

    def forward(self, x):
        return F.linear(mx_round(x), self.w, self.b)


# (attribute path suffixes of the Linears per mode: 2 = those that read a LayerNorm or GELU output, 3 adds the readers of the
# attention output)
_MODE2 = ("attn.to_q", "attn.to_k", "attn.to_v", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "net.0.proj", "net.2",
          "proj_mlp", "_attn_qkv", "_mlp.fc1", "_mlp.fc2", "linear1")
_MODE3 = ("attn.to_out.0", "attn.to_add_out", "_attn_proj", "linear2")   # + FLUX's single_transformer_blocks.<i>.proj_out
_BLOCKS = ("transformer_blocks.", "single_transformer_blocks.", "double_blocks.", "single_blocks.")


def fake_quant(model, mode):
    """a copy of the fp32 oracle with the Linears of fp8_linear = `mode` (2 | 3) replaced by MXLinear"""
    m = copy.deepcopy(model)
    picked = []
    for name, mod in list(m.named_modules()):
        if not isinstance(mod, nn.Linear) or not name.startswith(_BLOCKS):
            continue
        hit = any(name.endswith(s) for s in _MODE2)
        if mode == 3:
            hit = hit or any(name.endswith(s) for s in _MODE3)
            hit = hit or (name.startswith("single_transformer_blocks.") and name.endswith(".proj_out"))
        if hit:
            parent = m.get_submodule(name.rsplit(".", 1)[0])
            leaf = name.rsplit(".", 1)[1]
            if leaf.isdigit():
                parent[int(leaf)] = MXLinear(mod)
            else:
                setattr(parent, leaf, MXLinear(mod))
            picked.append(name)
    assert picked, "no Linear replaced"
    return m, picked


# ------------------------------------------------------------------------------------------------ families at width 512
class Flux:
    """geometry = (img_tokens, txt_len)"""
    name, family, branches = "flux", 0, (None,)
    cfg = FR.tiny_config(num_layers=2, num_single_layers=2, heads=HEADS)
    _oracle = None

    @classmethod
    def oracle(cls):
        if cls._oracle is None:
            cls._oracle = FR.init_synthetic_(FR.FluxTransformer2DModel(**cls.cfg), seed=3, std=0.05).eval()
        return cls._oracle

    @classmethod
    def engine_args(cls, geo):
        c = cls.cfg
        return (cls.family, DIM, HEADS, c["num_layers"], c["num_single_layers"], 64, 64, c["joint_attention_dim"], geo[1],
                c["pooled_projection_dim"], geo[0]), {}

    @staticmethod
    def geometry(geo):
        return geo[0], (0, 0, 0), geo[1]

    @staticmethod
    def ids(geo):
        li, lt = geo
        ids = torch.zeros(lt + li, 3)
        ids[lt:, 1] = torch.arange(li) // 8
        ids[lt:, 2] = torch.arange(li) % 8
        return ids

    @classmethod
    def inputs(cls, geo):
        from magcache_amd import mmdit as MM
        li, lt = geo
        g = torch.Generator().manual_seed(1000 * li + lt)
        return SimpleNamespace(img=torch.randn(li, 64, generator=g), txt=[torch.randn(lt, 256, generator=g)], valid=[lt],
                               vec=torch.randn(128, generator=g), rope=MM.flux_rope(cls.ids(geo)), guidance=4000.0)

    @classmethod
    def reference(cls, model, geo, inp, b=None):
        ids, lt = cls.ids(geo), geo[1]
        with torch.no_grad():
            return model(hidden_states=inp.img[None], encoder_hidden_states=inp.txt[0][None], pooled_projections=inp.vec[None],
                         timestep=torch.tensor([0.5]), img_ids=ids[lt:], txt_ids=ids[:lt], guidance=torch.tensor([4.0]))[0][0]


class Hunyuan:
    """geometry = ((F, H, W), txt_len); 23 valid text rows"""
    name, family, branches = "hunyuan", 1, (None,)
    cfg = HR.tiny_config(double=1, single=2, heads=HEADS)
    _oracle = None

    @classmethod
    def oracle(cls):
        if cls._oracle is None:
            cls._oracle = HR.init_synthetic_(HR.HYVideoDiffusionTransformer(**cls.cfg), seed=4, std=0.05).eval()
        return cls._oracle

    @staticmethod
    def tokens(grid):
        return grid[0] * (grid[1] // 2) * (grid[2] // 2)

    @classmethod
    def engine_args(cls, geo):
        c = cls.cfg
        return (cls.family, DIM, HEADS, c["mm_double_blocks_depth"], c["mm_single_blocks_depth"], 16, 16, c["text_states_dim"],
                geo[1], c["text_states_dim_2"], cls.tokens(geo[0])), dict(latent_grid=geo[0], refiner_depth=2)

    @classmethod
    def geometry(cls, geo):
        return cls.tokens(geo[0]), geo[0], geo[1]

    @staticmethod
    def inputs(geo):
        (f, h, w), lt = geo
        g = torch.Generator().manual_seed(100 * f + 10 * h + w + lt)
        return SimpleNamespace(img=torch.randn(16, f, h, w, generator=g), txt=[torch.randn(lt, 256, generator=g)], valid=[23],
                               vec=torch.randn(128, generator=g), rope=HR.get_rotary_pos_embed((f, h // 2, w // 2)),
                               guidance=6000.0)

    @classmethod
    def reference(cls, model, geo, inp, b=None):
        mask = torch.zeros(1, geo[1], dtype=torch.long)
        mask[0, :inp.valid[0]] = 1
        with torch.no_grad():
            return model(x=inp.img[None], t=torch.tensor([500.0]), text_states=inp.txt[0][None], text_mask=mask,
                         text_states_2=inp.vec[None], freqs_cos=inp.rope[0], freqs_sin=inp.rope[1],
                         guidance=torch.tensor([6000.0]), return_dict=False)[0]


class Qwen:
    """geometry = (img_shapes, txt_len): txt_len is the maximum; the cond prompt has 37 rows, the uncond one 5"""
    name, family, branches = "qwen", 2, (0, 1)
    cfg = QR.tiny_config(num_layers=2, heads=HEADS)
    _oracle = None

    @classmethod
    def oracle(cls):
        if cls._oracle is None:
            cls._oracle = QR.init_synthetic_(QR.QwenImageTransformer2DModel(**cls.cfg), seed=5, std=0.05).eval()
        return cls._oracle

    @staticmethod
    def tokens(shapes):
        return sum(f * h * w for f, h, w in shapes)

    @classmethod
    def engine_args(cls, geo):
        c = cls.cfg
        return (cls.family, DIM, HEADS, c["num_layers"], 0, 64, 64, c["joint_attention_dim"], geo[1], 0,
                cls.tokens(geo[0])), {}

    @classmethod
    def geometry(cls, geo):
        return cls.tokens(geo[0]), (0, 0, 0), geo[1]

    @classmethod
    def inputs(cls, geo):
        from magcache_amd import mmdit as MM
        shapes, lt = geo
        li = cls.tokens(shapes)
        g = torch.Generator().manual_seed(7 * li + lt)
        return SimpleNamespace(img=torch.randn(li, 64, generator=g), txt=[torch.randn(n, 256, generator=g) for n in (37, 5)],
                               valid=[37, 5], vec=None, rope=MM.qwen_rope(list(shapes), lt), guidance=0.0)

    @classmethod
    def reference(cls, model, geo, inp, b=0):
        with torch.no_grad():
            return model(hidden_states=inp.img[None], encoder_hidden_states=inp.txt[b][None], timestep=torch.tensor([0.5]),
                         img_shapes=[list(geo[0])], txt_seq_lens=[inp.valid[b]], return_dict=False)[0][0]


FLUX_ODD, FLUX_EXACT = (200, 72), (512, 256)
HUNYUAN_GEO = ((3, 12, 16), 64)
QWEN_GEO, QWEN_EDIT_GEO = (((1, 12, 16),), 64), (((1, 12, 16), (1, 8, 8)), 64)

_refs = {}


def references(fam, geo, mode, b=None):
    """(plain fp32 oracle output, fake-quant oracle output of `mode`), computed once"""
    key = (fam.name, geo, mode, b)
    if key not in _refs:
        inp = fam.inputs(geo)
        pk = (fam.name, geo, 0, b)
        if pk not in _refs:
            _refs[pk] = fam.reference(fam.oracle(), geo, inp, b or 0)
        _refs[key] = fam.reference(fake_quant(fam.oracle(), mode)[0], geo, inp, b or 0)
    return _refs[(fam.name, geo, 0, b)], _refs[key]

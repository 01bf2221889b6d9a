"""Helper of tests/test_mmdit_mxfp4_cpu.py and tests/test_mmdit_mxfp4_gpu.py: the FP4 fake-quant oracle of the toy MM-DiT
families of tests/mmdit_fp8_ref.py -- the fp32 oracle with the nn.Linears that mc_mmdit_config.fp8_linear (2 | 3) picks
quantising the bf16-rounded input and the bf16-rounded weight through the torch restatement of MXFP4 (tests/mxfp4_ref.py:
e2m1 elements relative to one E8M0 scale per 32 inputs) and multiplying in fp32.  The Linears are picked by mmdit_fp8_ref's own
name lists: the option "mx_fp4" changes the format of the quantised Linears, never which ones they are."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import mmdit_fp8_ref as R
import mxfp4_ref as F4


def fp4_round(x):
    """x [..., K] -> the values an MXFP4 operand holds: bf16 rounding, then e2m1 relative to one E8M0 scale per 32 k"""
    x2 = x.detach().to(torch.bfloat16).float().reshape(-1, x.shape[-1])
    codes, e = F4.quantize(x2)
    return F4.dequantize(codes, e).float().view(x.shape)


class FP4Linear(nn.Module):
    def __init__(self, lin):
        super().__init__()
        self.w, self.b = fp4_round(lin.weight), lin.bias.detach()

    def forward(self, x):
        return F.linear(fp4_round(x), self.w, self.b)


def picked_names(model, mode):
    """the Linears of fp8_linear = `mode`, by the name lists of mmdit_fp8_ref"""
    out = []
    for name, mod in model.named_modules():
        if not isinstance(mod, nn.Linear) or not name.startswith(R._BLOCKS):
            continue
        hit = any(name.endswith(s) for s in R._MODE2)
        if mode == 3:
            hit = hit or any(name.endswith(s) for s in R._MODE3)
            hit = hit or (name.startswith("single_transformer_blocks.") and name.endswith(".proj_out"))
        if hit:
            out.append(name)
    return out


def fake_quant(model, mode):
    """a copy of the fp32 oracle with the Linears of fp8_linear = `mode` (2 | 3) replaced by FP4Linear"""
    m = copy.deepcopy(model)
    picked = picked_names(m, mode)
    assert picked, "no Linear replaced"
    for name in picked:
        parent, leaf = m.get_submodule(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1]
        if leaf.isdigit():
            parent[int(leaf)] = FP4Linear(parent[int(leaf)])
        else:
            setattr(parent, leaf, FP4Linear(getattr(parent, leaf)))
    return m, picked


_refs = {}


def plain_reference(fam, geo, b=None):
    """the plain fp32 oracle's output, shared with mmdit_fp8_ref.references (one cache)"""
    key = (fam.name, geo, 0, b)
    if key not in R._refs:
        R._refs[key] = fam.reference(fam.oracle(), geo, fam.inputs(geo), b or 0)
    return R._refs[key]


def references(fam, geo, mode, b=None):
    """(plain fp32 oracle output, FP4 fake-quant oracle output of `mode`), computed once"""
    key = (fam.name, geo, mode, b)
    if key not in _refs:
        _refs[key] = fam.reference(fake_quant(fam.oracle(), mode)[0], geo, fam.inputs(geo), b or 0)
    return plain_reference(fam, geo, b), _refs[key]


# Distance of the FP4 fake-quant oracle from the plain one (relative L2), computed on the CPU from the two oracles alone:
# 2.07e-1 (Qwen-Image, mode 2) .. 3.23e-1 (FLUX 512 + 256, mode 3) over the five cases, both modes and every branch.  The band
# only guards this helper against a wrong scale (O(1)) or a wrapper that does nothing (0, or MX fp8's 4.5e-2 .. 7.1e-2).
Q_BAND = (1.5e-1, 4.0e-1)

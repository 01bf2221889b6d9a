"""CPU restatement of the MX fp8 self-attention (csrc/attention_mx8.hip, csrc/quant.h): the pre-pass's images bit for bit, their
inverse, and a torch model of the kernel.  Images are flat uint8 tensors under the names of ops.h's AttnMx8Images."""
import math

import torch

import attention_cases as A


def slot_key(s):
    """quant.h: mx8_slot_key -- the key (of its 64-key tile) that k slot s of the P V product holds"""
    half, byte = (s >> 4) & 1, (s & 15) | ((s >> 5) << 4)
    r = byte & 15
    return 32 * (byte >> 4) + (r & 3) + 8 * (r >> 2) + 4 * half


SLOT_KEY = torch.tensor([slot_key(s) for s in range(64)])
F8 = torch.float8_e4m3fn


def row_scale_index(heads, rows):
    """[rows, heads * 4] -> position of the scale of (row, 32-channel block) in a Q^ / K^ scale image (mx8_row_scale_index)"""
    row, b = torch.arange(rows)[:, None], torch.arange(heads * 4)[None, :]
    blk = b & 3
    return (b >> 2) * rows * 4 + (row & ~63) * 4 + ((blk & 1) * 32 + (row & 31)) * 4 + ((row >> 5) & 1) * 2 + (blk >> 1)


def v_scale_index(heads, rows):
    """[heads * 128, rows / 32] -> position of the scale of (channel, 32-slot block) in the V^T scale image (mx8_v_scale_index)"""
    c, sb = torch.arange(heads * 128)[:, None], torch.arange(rows // 32)[None, :]
    ch = c & 127
    return (c >> 7) * rows * 4 + (sb >> 1) * 256 + ((sb & 1) * 32 + (ch & 31)) * 4 + (ch >> 5)


def mx_quantize(x):
    """fp32 [n, 32 m] -> e4m3 bytes (x * 2^-e, to nearest even) and E8M0 bytes [n, m]: quant.h's mx_exponent, -127 for a zero block"""
    b = x.reshape(x.shape[0], -1, 32)
    amax = b.abs().amax(-1)
    f, ex = torch.frexp(amax * torch.tensor(1.0 / 448.0, dtype=torch.float32))
    e = torch.where(f == 0.5, ex - 1, ex).clamp(-127, 127)
    e = torch.where(amax > 0, e, torch.full_like(e, -127))
    q = torch.ldexp(b, -e[..., None]).to(F8).view(torch.uint8).reshape(x.shape)
    return q, (e + 127).to(torch.uint8)


def images(q, k, v, heads, rows, valid, scale):
    """what launch_attn_quantize_mx8 writes for bf16 q [Lq, d], k, v [>= rows, d]"""
    Lq = q.shape[0]
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(A.LOG2E, dtype=torch.float32)
    qq, qs = mx_quantize(q.float() * c)
    kq, ks = mx_quantize(k[:rows].float())
    kq[valid:], ks[valid:] = 0, 127
    vz = v[:rows].float().clone()
    vz[valid:] = 0
    vt = vz.T.reshape(heads * 128, rows // 64, 64)[:, :, SLOT_KEY].reshape(heads * 128, rows)
    vq, vs = mx_quantize(vt)
    out = {"q": qq.flatten(), "k": kq.flatten(), "vt": vq.flatten()}
    for name, s, idx in (("qs", qs, row_scale_index(heads, Lq)), ("ks", ks, row_scale_index(heads, rows)), ("vs", vs, v_scale_index(heads, rows))):
        out[name] = torch.empty(s.numel(), dtype=torch.uint8)
        out[name][idx.flatten()] = s.flatten()
    return out


def dequantize(im, heads, Lq, rows):
    """the images (CPU) -> fp32 q^ [Lq, d] (in log2 units: the softmax scale is inside), k^ and v^ [rows, d], keys in their order"""
    d = heads * 128
    def deq(bytes2d, scales2d):
        x = bytes2d.view(F8).float().reshape(bytes2d.shape[0], -1, 32)
        return torch.ldexp(x, scales2d.int()[..., None] - 127).reshape(bytes2d.shape)
    qd = deq(im["q"].reshape(Lq, d), im["qs"][row_scale_index(heads, Lq)])
    kd = deq(im["k"].reshape(rows, d), im["ks"][row_scale_index(heads, rows)])
    vt = deq(im["vt"].reshape(d, rows), im["vs"][v_scale_index(heads, rows)])
    vd = torch.empty(d, rows // 64, 64)
    vd[:, :, SLOT_KEY] = vt.reshape(d, rows // 64, 64)
    return qd, kd, vd.reshape(d, rows).T.contiguous()


def ref64(qd, kd, vd, heads, valid):
    """attn_ref64 on dequantised operands (qd carries scale * log2(e): the scores are in log2 units)"""
    return A.attn_ref64(qd, kd, vd, heads, torch.arange(valid), math.log(2.0))[0]


def model(qd, kd, vd, heads, valid, tile=A.KT):
    """The kernel in torch on the dequantised operands: 64-key tiles, running maximum, fp32 row sum, P as e4m3 at 2^8, bf16 O"""
    Lq = qd.shape[0]
    qs, ks, vs = (A._heads(x, heads) for x in (qd, kd[:valid], vd[:valid]))
    m, l, o = torch.full((heads, Lq, 1), -math.inf), torch.zeros(heads, Lq, 1), torch.zeros(heads, Lq, A.HD)
    for t0 in range(0, valid, tile):
        s = qs @ ks[:, t0:t0 + tile].transpose(1, 2)
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha, p = torch.exp2(m - m_new), torch.exp2(s - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + ((p * 256).to(F8).float() / 256) @ vs[:, t0:t0 + tile]
        m = m_new
    return (o / l).transpose(0, 1).reshape(Lq, heads * A.HD).bfloat16()

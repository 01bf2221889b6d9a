"""GPU: the frame-block causal / windowed self-attention kernel (csrc/attention_band.hip, mc_op_attention_band) against
attention_cases.attn_ref64 called once per query block over range(lo(b), hi(b)), under attention_cases.accept unchanged.

Random operands cannot see a lost or leaked key (it moves O by ~|v| / n), so k, v ~ N(0, 1) and q = 3 k[t(i)]:
  own    t(i) = i: every key is THE key of its own query; a lost key replaces that row of O
  next   t(i) = min(i + block_tokens, valid - 1): the dominant key is the first forbidden one above; a leak through hi replaces the row
  below  t(i) = max(i - window_blocks * block_tokens, 0) (window cases): the dominant key lies just under lo
On the CPU attention_cases.flash_bf16_model, applied per block, passes accept on all 21 combinations (rel-L2 <= 3.2e-3), and the
unmasked fp64 result is 1.2 .. 2.1 rel-L2 away from the masked one in every next / below case whose mask restricts anything."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
# (Lq_pad, valid, block_tokens, window_blocks, heads)
SHAPES = [(256, 256, 64, 0, 1), (256, 250, 24, 0, 3), (512, 500, 100, 1, 1), (512, 500, 100, 2, 2), (768, 700, 40, 3, 1),
          (512, 512, 512, 0, 1), (1024, 1000, 300, 0, 1)]
CASES = [(s, kind) for s in SHAPES for kind in ("own", "next") + (("below",) if s[3] else ())]


def band_ref(q, k, v, heads, valid, bt, win):
    """fp64 O [valid, d]: attn_ref64 once per query block over its visible keys"""
    out = torch.empty(valid, heads * A.HD, dtype=torch.float64)
    for b in range((valid + bt - 1) // bt):
        lo = max(0, b - win + 1) * bt if win else 0
        hi = min((b + 1) * bt, valid)
        out[b * bt:hi] = A.attn_ref64(q[b * bt:hi], k, v, heads, range(lo, hi), A.SCALE)[0]
    return out


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """q [Lq, d], k, v [Lq, d] bf16 on the CPU (padding rows finite) and the reference"""
    Lq, valid, bt, win, heads = shape
    g = torch.Generator().manual_seed(A.SEED)
    k = torch.randn(Lq, heads * A.HD, generator=g).bfloat16()
    v = torch.randn(Lq, heads * A.HD, generator=g).bfloat16()
    i = torch.arange(Lq)
    t = {"own": i, "next": (i + bt).clamp(max=valid - 1), "below": (i - win * bt).clamp(min=0),
         "random": None}[kind]
    q = torch.randn(Lq, heads * A.HD, generator=g).bfloat16() if t is None else (3.0 * k[t].float()).bfloat16()
    return q, k, v, band_ref(q, k, v, heads, valid, bt, win)


def launch(q, k, v, shape, o=None, rows=None):
    Lq, valid, bt, win, heads = shape
    o = torch.full((Lq, heads * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV) if o is None else o
    status = H.L().mc_op_attention_band(H.P(q), q.stride(0), H.P(k), k.stride(0), H.P(v), v.stride(0), H.P(o), o.stride(0), Lq, heads,
                                        rows or Lq, valid, bt, win, A.SCALE, H.S())
    torch.cuda.synchronize()
    return o, status


@pytest.mark.parametrize("shape,kind", CASES + [(SHAPES[3], "random")], ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else p)
def test_band_against_fp64(shape, kind):
    q, k, v, ref = case(shape, kind)
    o, status = launch(q.to(DEV), k.to(DEV), v.to(DEV), shape)
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    assert bool(torch.isfinite(o.float()).all()), "padding rows must be finite"
    print(f"rel-L2 {A.rel_l2(o[:shape[1]].cpu(), ref):.3e}")
    A.accept(o[:shape[1]], ref)


def test_one_block_is_plain_attention():
    """block_tokens >= valid: the launch matches mc_op_attention on the same operands under the same bar"""
    shape = (512, 500, 500, 0, 2)
    q, k, v, ref = case(shape, "own")
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o, status = launch(qd, kd, vd, shape)
    assert status == _lib.MC_OK
    plain = torch.empty_like(o)
    _lib.check(H.L().mc_op_attention(H.P(qd), qd.stride(0), H.P(kd), kd.stride(0), 0, H.P(vd), vd.stride(0), 0, H.P(plain),
                                     plain.stride(0), 512, 2, 512, 500, 1, A.SCALE, H.S()))
    torch.cuda.synchronize()
    A.accept(o[:500], ref)
    A.accept(o[:500], plain[:500].double())


@pytest.mark.parametrize("what", ["Lq_pad 128", "block_tokens 0", "window_blocks -1", "misaligned pointer", "valid 0"])
def test_refusals(what):
    """MC_EINVAL, nothing launched: O untouched"""
    Lq, valid, bt, win = 256, 256, 64, 0
    buf = torch.zeros(3 * 256 * A.HD + 8, dtype=torch.bfloat16, device=DEV)
    off = 4 if what == "misaligned pointer" else 0          # 8 bytes off a 16-byte boundary
    q, k, v = (buf[off + i * 256 * A.HD:off + (i + 1) * 256 * A.HD].view(256, A.HD) for i in range(3))
    if what == "Lq_pad 128":
        Lq = 128
    elif what == "block_tokens 0":
        bt = 0
    elif what == "window_blocks -1":
        win = -1
    elif what == "valid 0":
        valid = 0
    o = torch.full((256, A.HD), float("nan"), dtype=torch.bfloat16, device=DEV)
    _, status = launch(q, k, v, (Lq, valid, bt, win, 1), o=o, rows=256)
    assert status == _lib.MC_EINVAL and "attention_band" in H.L().mc_last_error().decode()
    assert bool(torch.isnan(o).all()), what

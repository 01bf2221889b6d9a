"""GPU: the LoRA merge kernel alone (magcache_amd/csrc/lora_merge.hip) through mc_op_lora_merge:

    out = bf16(W + sum_j s_j * (B_j A_j)),   per term an fp32 product on bf16 MFMAs, the delta summed in fp32 in term order,
                                             one fp32 add of W last, one round-to-nearest-even.

Bit-exact cases use dyadic adapters (entries in {-1, -1/2, 0, 1/2, 1} * 2^-5, power-of-two scales): every product and every
partial sum of B A is then a multiple of 2^-12 below 2^3 and exact in fp32 in any order, so the kernel must reproduce
(W.float() + sum s_j (B_j.float() @ A_j.float())).bfloat16() bit for bit.  The random-value case is held to the fp64 result."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
SHAPES = [(128, 512), (384, 2560), (200, 520)]      # the last is off every tile boundary in both directions
RANKS = [1, 4, 24, 128, 130]                        # below the kernel's rank step (16), an odd multiple, full steps and one element past them
POISON = 0x7FC1                                     # a NaN pattern no computation here produces


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16)


def merge(base, ld_base, out, ld_out, rows, K, terms, scratch=None):
    """terms: [(A [r, K] bf16, B [rows, r] bf16, scale)]; returns the status"""
    arr = (_lib.McLoraTerm * max(len(terms), 1))(*[_lib.McLoraTerm(a.data_ptr(), b.data_ptr(), a.shape[0], float(s))
                                                   for a, b, s in terms])
    sp, sb = (ptr(scratch), scratch.numel()) if scratch is not None else (None, 0)
    return _lib.load().mc_op_lora_merge(base if isinstance(base, C.c_void_p) else ptr(base), ld_base,
                                        out if isinstance(out, C.c_void_p) else ptr(out), ld_out, rows, K, arr, len(terms), sp, sb,
                                        stream())


def dyadic(shape, gen):
    """entries in {-1, -1/2, 0, 1/2, 1} * 2^-5, bf16"""
    return ((torch.randint(-2, 3, shape, generator=gen, device=DEV).float() / 2) * 2.0 ** -5).bfloat16()


def weight(rows, K, gen):
    return (torch.randn(rows, K, generator=gen, device=DEV) * 0.02).bfloat16()


def expect(W, terms):
    delta = None
    for a, b, s in terms:
        d = s * (b.float() @ a.float())
        delta = d if delta is None else delta + d
    return (W.float() + delta).bfloat16()


def run_poisoned(W, terms):
    """merge into the middle row range of a poisoned [3 rows, K + 8] buffer; returns (middle rows, everything else untouched)"""
    rows, K = W.shape
    buf = torch.full((3 * rows, K + 8), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    out = C.c_void_p(buf.data_ptr() + rows * (K + 8) * 2)
    _lib.check(merge(W, K, out, K + 8, rows, K, terms))
    torch.cuda.synchronize()
    b = bits(buf)
    untouched = bool((b[:rows] == POISON).all()) and bool((b[2 * rows:] == POISON).all()) and bool((b[rows:2 * rows, K:] == POISON).all())
    return buf[rows:2 * rows, :K], untouched


@pytest.fixture(scope="module")
def gen():
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.Generator(device=DEV).manual_seed(1234)


@pytest.mark.parametrize("rows,K", SHAPES)
def test_dyadic_single_term_every_rank_is_bit_exact(gen, rows, K):
    W = weight(rows, K, gen)
    for rank in RANKS:
        terms = [(dyadic((rank, K), gen), dyadic((rows, rank), gen), 2.0 if rank % 2 else -0.5)]
        got, untouched = run_poisoned(W, terms)
        want = expect(W, terms)
        assert bool((want != W).any()), "the adapter moves nothing: the case checks nothing"
        assert torch.equal(bits(got), bits(want)), (rows, K, rank, int((bits(got) != bits(want)).sum()))
        assert untouched, (rows, K, rank)


@pytest.mark.parametrize("rows,K", SHAPES)
def test_dyadic_two_terms_opposite_signs_and_a_zero_scale(gen, rows, K):
    W = weight(rows, K, gen)
    t4 = (dyadic((4, K), gen), dyadic((rows, 4), gen), 4.0)
    t130 = (dyadic((130, K), gen), dyadic((rows, 130), gen), -0.25)
    got, untouched = run_poisoned(W, [t4, t130])
    assert torch.equal(bits(got), bits(expect(W, [t4, t130]))) and untouched
    # a term with scale 0 adds nothing, wherever it stands
    zero = (t130[0], t130[1], 0.0)
    for terms in ([zero], [t4, zero], [zero, t4]):
        got, untouched = run_poisoned(W, terms)
        assert torch.equal(bits(got), bits(expect(W, [t for t in terms if t[2] != 0.0] or [(t4[0], t4[1], 0.0)]))) and untouched


def test_dyadic_aliased_out_is_base_and_given_scratch(gen):
    rows, K = 200, 520
    W = weight(rows, K, gen)
    terms = [(dyadic((24, K), gen), dyadic((rows, 24), gen), 1.0), (dyadic((130, K), gen), dyadic((rows, 130), gen), -2.0)]
    want = expect(W, terms)
    inplace = W.clone()
    _lib.check(merge(inplace, K, inplace, K, rows, K, terms))
    torch.cuda.synchronize()
    assert torch.equal(bits(inplace), bits(want))
    # the same with caller-owned scratch (asynchronous form); a scratch one byte short is refused
    arr = (_lib.McLoraTerm * 2)(*[_lib.McLoraTerm(a.data_ptr(), b.data_ptr(), a.shape[0], float(s)) for a, b, s in terms])
    need = _lib.load().mc_op_lora_merge_scratch(rows, K, arr, 2)
    raw = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    out = torch.zeros_like(W)
    _lib.check(merge(W, K, out, K, rows, K, terms, scratch=raw[off:off + need]))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))
    assert merge(W, K, out, K, rows, K, terms, scratch=raw[off:off + need - 1]) == _lib.MC_EINVAL


def test_random_values_against_fp64(gen):
    """|out - exact| <= 1/2 ulp_bf16(exact) + 2^-18 (|W| + sum |s_j| |B_j| |A_j|) for every element -- the rounding of the result
    plus fp32 accumulation error bounded by the magnitudes summed -- and at most 1e-3 of the elements may differ in bits from the
    rounded fp64 value (an fp32 evaluation in another order differs on 3e-5 .. 6e-5 of them; a truncating or mis-stepped
    kernel on half or all)."""
    rows, K = 384, 2560
    W = weight(rows, K, gen)
    terms = []
    for rank, s in ((4, 1.3), (130, -0.7)):
        terms.append(((torch.randn(rank, K, generator=gen, device=DEV) * 0.05).bfloat16(),
                      (torch.randn(rows, rank, generator=gen, device=DEV) * 0.05).bfloat16(), s))
    got, untouched = run_poisoned(W, terms)
    assert untouched
    exact = W.double()
    mag = W.double().abs()
    for a, b, s in terms:
        s32 = float(torch.tensor(s, dtype=torch.float32))              # the scale reaches the kernel as fp32
        exact = exact + s32 * (b.double() @ a.double())
        mag = mag + abs(s32) * (b.double().abs() @ a.double().abs())
    want = exact.float().bfloat16()                                     # fp64 -> fp32 -> bf16: double rounding is possible only
    #                                                                     within 2^-29 relative of a tie, far inside the slack below
    ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(1e-300))) - 7)
    err = (got.double() - exact).abs()
    bound = 0.5 * ulp + 2.0 ** -18 * mag
    worst = float((err / bound).max())
    differ = float((bits(got) != bits(want)).double().mean())
    print(f"lora_merge random: worst err / bound {worst:.4f}, share of elements off the rounded fp64 value {differ:.3e}")
    assert bool((err <= bound).all()), worst
    assert differ <= 1e-3, differ
    assert float((bits(got) != bits(W)).double().mean()) > 0.5, "the adapters moved almost nothing: the case checks nothing"


def test_refusals_launch_nothing(gen):
    rows, K = 128, 512
    W = weight(rows, K, gen)
    a, b = dyadic((4, K), gen), dyadic((rows, 4), gen)
    out = torch.full((rows, K), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    lib = _lib.load()
    # rank 0
    arr = (_lib.McLoraTerm * 1)(_lib.McLoraTerm(a.data_ptr(), b.data_ptr(), 0, 1.0))
    assert lib.mc_op_lora_merge(ptr(W), K, ptr(out), K, rows, K, arr, 1, None, 0, stream()) == _lib.MC_EINVAL
    # more terms than the maximum
    assert merge(W, K, out, K, rows, K, [(a, b, 1.0)] * (_lib.MC_LORA_MAX_TERMS + 1)) == _lib.MC_EINVAL
    assert b"at most" in lib.mc_last_error()
    # misaligned base / out, a pitch that is no multiple of 8, a pitch below K
    assert merge(C.c_void_p(W.data_ptr() + 2), K, out, K, rows - 1, K, [(a, b, 1.0)]) == _lib.MC_EINVAL
    assert merge(W, K, C.c_void_p(out.data_ptr() + 8), K, rows - 1, K, [(a, b, 1.0)]) == _lib.MC_EINVAL
    assert merge(W, K, out, K + 4, rows // 2, K, [(a, b, 1.0)]) == _lib.MC_EINVAL
    assert merge(W, K, out, K - 8, rows, K, [(a, b, 1.0)]) == _lib.MC_EINVAL
    torch.cuda.synchronize()
    assert bool((bits(out) == POISON).all()), "a refused call wrote"
    # the maximum itself is fine
    _lib.check(merge(W, K, out, K, rows, K, [(a, b, 0.125)] * _lib.MC_LORA_MAX_TERMS))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(expect(W, [(a, b, 0.125)] * _lib.MC_LORA_MAX_TERMS)))

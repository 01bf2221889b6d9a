"""GPU: the two kernels behind the Wan engine's adapters (magcache_amd/csrc/lora_merge.hip), alone, through the C ABI.

mc_op_lora_merge_f32:  out_f32 = base_f32 + sum_j s_j (B_j A_j), operands bf16, per term an fp32 accumulator on bf16 MFMAs, the
                       delta summed in fp32 in term order, ONE fp32 add of the base element last, no rounding step.
    Held to the fp64 product of the bf16 operands plus the base, element by element, within
        (rank_pad + n_terms + 2) * 2^-24 * (sum_j |s_j| sum_k |B||A| + |base|):
    products of bf16 values are exact in fp32, so the error is that of the fp32 additions -- at most rank_pad per term (the rank
    zero-padded to the kernel's step of 16), one per term for the scale and the delta sum, one for the base -- each at most
    2^-24 of the magnitudes summed so far.

mc_op_param_delta:     out = base + sum_j s_j delta_j in fp32, the sum from zero in term order, each multiply and add rounded:
    bit-equal to the same expression evaluated term by term in numpy float32."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
NAN_BITS = 0x7FC00123          # a NaN pattern no computation here produces
SCALES = [1.25, -0.75, 0.0, 0.5, 2.0, -1.5, 0.375, 1.0]     # exact in fp32; the zero stands in the middle of two and of eight


def ptr(t):
    return t if isinstance(t, C.c_void_p) else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def merge_f32(base, ld_base, out, ld_out, rows, K, terms):
    arr = (_lib.McLoraTerm * max(len(terms), 1))(*[_lib.McLoraTerm(a.data_ptr(), b.data_ptr(), a.shape[0], float(s))
                                                   for a, b, s in terms])
    return _lib.load().mc_op_lora_merge_f32(ptr(base), ld_base, ptr(out), ld_out, rows, K, arr, len(terms), None, 0, stream())


def make_terms(rows, K, rank, n_terms, gen):
    scales = SCALES[:n_terms] if n_terms != 2 else [SCALES[0], SCALES[3]]
    if n_terms == 3:
        scales = [SCALES[0], 0.0, SCALES[3]]
    return [((torch.randn(rank, K, generator=gen, device=DEV) * 0.3).bfloat16(),
             (torch.randn(rows, rank, generator=gen, device=DEV) * 0.3).bfloat16(), s) for s in scales]


def exact_and_bound(base, terms, rank):
    rank_pad = (rank + 15) // 16 * 16
    exact, mag = base.double(), base.double().abs()
    for a, b, s in terms:
        exact = exact + s * (b.double() @ a.double())
        mag = mag + abs(s) * (b.double().abs() @ a.double().abs())
    return exact, (rank_pad + len(terms) + 2) * 2.0 ** -24 * mag


@pytest.fixture(scope="module")
def gen():
    return torch.Generator(device=DEV).manual_seed(4321)


@pytest.mark.parametrize("rows", [64, 40, 129])
@pytest.mark.parametrize("K", [256, 264, 4])
def test_merge_f32_against_fp64(gen, rows, K):
    """every rank and term count at this shape, into a NaN-filled buffer with ld_out = K + 8; 3 terms = a zero scale in the middle"""
    base = torch.randn(rows, K, generator=gen, device=DEV)
    for rank in (1, 16, 17):
        for n_terms in (1, 2, 3, 8):
            terms = make_terms(rows, K, rank, n_terms, gen)
            buf = torch.full((rows + 2, K + 8), NAN_BITS, dtype=torch.int32, device=DEV)
            out = C.c_void_p(buf.data_ptr() + (K + 8) * 4)
            _lib.check(merge_f32(base, K, out, K + 8, rows, K, terms))
            again = torch.full((rows + 2, K + 8), NAN_BITS, dtype=torch.int32, device=DEV)
            _lib.check(merge_f32(base, K, C.c_void_p(again.data_ptr() + (K + 8) * 4), K + 8, rows, K, terms))
            torch.cuda.synchronize()
            assert bool((buf[0] == NAN_BITS).all()) and bool((buf[-1] == NAN_BITS).all()) and \
                bool((buf[1:-1, K:] == NAN_BITS).all()), ("the guard band was written", rows, K, rank, n_terms)
            assert torch.equal(buf, again), ("two launches differ", rows, K, rank, n_terms)
            got = buf[1:-1, :K].contiguous().view(torch.float32)
            exact, bound = exact_and_bound(base, terms, rank)
            err = (got.double() - exact).abs()
            worst = float((err / bound).max())
            print(f"merge_f32 rows {rows} K {K} rank {rank} terms {n_terms}: worst err / bound {worst:.4f}")
            assert bool((err <= bound).all()), (rows, K, rank, n_terms, worst)
            assert float((got != base).double().mean()) > 0.9, "the adapters moved almost nothing: the case checks nothing"
            # out aliasing base: the same bits
            inplace = base.clone()
            _lib.check(merge_f32(inplace, K, inplace, K, rows, K, terms))
            torch.cuda.synchronize()
            assert torch.equal(bits(inplace), bits(got)), (rows, K, rank, n_terms)


def test_merge_f32_zero_scale_term_adds_nothing(gen):
    rows, K = 40, 264
    base = torch.randn(rows, K, generator=gen, device=DEV)
    t = make_terms(rows, K, 17, 3, gen)
    with_zero, without = torch.empty_like(base), torch.empty_like(base)
    _lib.check(merge_f32(base, K, with_zero, K, rows, K, t))
    _lib.check(merge_f32(base, K, without, K, rows, K, [t[0], t[2]]))
    torch.cuda.synchronize()
    assert torch.equal(bits(with_zero), bits(without))


def test_merge_f32_refusals_write_nothing(gen):
    rows, K = 64, 256
    base = torch.randn(rows, K, generator=gen, device=DEV)
    a, b = make_terms(rows, K, 4, 1, gen)[0][:2]
    out = torch.full((rows, K), NAN_BITS, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    assert merge_f32(base, K, out, K, rows, K, [(a, b, 1.0)] * (_lib.MC_LORA_MAX_TERMS + 1)) == _lib.MC_EINVAL     # a ninth term
    assert b"at most" in lib.mc_last_error()
    assert merge_f32(C.c_void_p(base.data_ptr() + 4), K, out, K, rows - 1, K, [(a, b, 1.0)]) == _lib.MC_EINVAL      # misaligned
    assert merge_f32(base, K, C.c_void_p(out.data_ptr() + 8), K, rows - 1, K, [(a, b, 1.0)]) == _lib.MC_EINVAL
    a6 = a[:, :6].contiguous()                                                                                      # K % 4 != 0
    assert merge_f32(base, K, out, K, rows, 6, [(a6, b, 1.0)]) == _lib.MC_EINVAL
    assert merge_f32(base, K, out, K + 2, rows // 2, K, [(a, b, 1.0)]) == _lib.MC_EINVAL                            # pitch % 4 != 0
    torch.cuda.synchronize()
    assert bool((out == NAN_BITS).all()), "a refused call wrote"
    _lib.check(merge_f32(base, K, out, K, rows, K, [(a, b, 0.125)] * _lib.MC_LORA_MAX_TERMS))                       # the maximum is fine
    torch.cuda.synchronize()
    exact, bound = exact_and_bound(base, [(a, b, 0.125)] * _lib.MC_LORA_MAX_TERMS, 4)
    assert bool(((out.view(torch.float32).double() - exact).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------- mc_op_param_delta
def param_delta(base, out, n, deltas, scales):
    pa = (C.c_void_p * len(deltas))(*[d.data_ptr() if torch.is_tensor(d) else d.value for d in deltas])
    sa = (C.c_float * len(scales))(*scales)
    return _lib.load().mc_op_param_delta(ptr(base), ptr(out), n, pa, sa, len(deltas), stream())


def numpy_delta(base, deltas, scales):
    acc = np.zeros(base.shape, dtype=np.float32)
    for d, s in zip(deltas, scales):
        if np.float32(s) == 0:
            continue
        acc = acc + np.float32(s) * d          # one rounded multiply, one rounded add: numpy contracts nothing
    return base + acc


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
@pytest.mark.parametrize("n_terms", [1, 8])
def test_param_delta_bit_equal_numpy(gen, n, n_terms):
    base = torch.randn(n, generator=gen, device=DEV)
    deltas = [torch.randn(n, generator=gen, device=DEV) * 0.37 for _ in range(n_terms)]
    scales = [1.3, -0.7, 0.0, 0.11, 2.5, -1.9, 0.6, 1.0][:n_terms]      # not all exact in fp32: the kernel gets float(s) too
    out = torch.full((n + 8,), NAN_BITS, dtype=torch.int32, device=DEV)
    _lib.check(param_delta(base, out, n, deltas, scales))
    torch.cuda.synchronize()
    want = numpy_delta(base.cpu().numpy(), [d.cpu().numpy() for d in deltas], scales)
    got = out[:n].view(torch.float32).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, n_terms, int((got.view(np.int32) != want.view(np.int32)).sum()))
    assert bool((out[n:] == NAN_BITS).all()), "written past n"
    assert not np.array_equal(got, base.cpu().numpy())
    # the aliased form, and operands off a 16-byte boundary (single elements throughout): the same bits
    inplace = base.clone()
    _lib.check(param_delta(inplace, inplace, n, deltas, scales))
    shifted = torch.zeros(n + 1, device=DEV)
    shifted[1:] = base
    sh_out = torch.zeros(n + 1, device=DEV)
    _lib.check(param_delta(C.c_void_p(shifted.data_ptr() + 4), C.c_void_p(sh_out.data_ptr() + 4), n, deltas, scales))
    torch.cuda.synchronize()
    assert np.array_equal(inplace.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(sh_out[1:].cpu().numpy().view(np.int32), want.view(np.int32))


def test_param_delta_zero_scales_and_refusals(gen):
    n = 1027
    base = torch.randn(n, generator=gen, device=DEV)
    d0, d1 = torch.randn(n, generator=gen, device=DEV), torch.randn(n, generator=gen, device=DEV)
    a, b, c = torch.empty_like(base), torch.empty_like(base), torch.empty_like(base)
    _lib.check(param_delta(base, a, n, [d0, d1], [0.0, 0.5]))          # a zero scale is skipped ...
    _lib.check(param_delta(base, b, n, [d1], [0.5]))
    _lib.check(param_delta(base, c, n, [d0, d1], [0.0, 0.0]))          # ... and no live term copies base
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(c), bits(base))
    out = torch.full((n,), NAN_BITS, dtype=torch.int32, device=DEV)
    assert param_delta(base, out, 0, [d0], [1.0]) == _lib.MC_EINVAL
    assert param_delta(base, out, n, [d0] * (_lib.MC_LORA_MAX_TERMS + 1), [1.0] * (_lib.MC_LORA_MAX_TERMS + 1)) == _lib.MC_EINVAL
    assert param_delta(base, out, n, [C.c_void_p(d0.data_ptr() + 2)], [1.0]) == _lib.MC_EINVAL
    torch.cuda.synchronize()
    assert bool((out == NAN_BITS).all()), "a refused call wrote"

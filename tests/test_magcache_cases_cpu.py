"""What the exact GPU tests of calib_stats and the per-row fp8 GEMM rest on, checked without a GPU (tests/magcache_cases.py):
  * calib_int_case: the integer row sums stay under 2^24 (exact in fp32 in any order); the fp64 sum of the per-row fp32 rho
    values, and of the 1 - cos values, is the same under any order and equals math.fsum -- so sums[0] and sums[2] of a correct
    kernel are ONE bit pattern whatever the grid; a lost column, a pad column read or a row counted twice moves them;
  * fp8_int_case: |acc| <= 4 K, acc * (sa * sw) + bias and the gated residual are exactly representable in fp32, the bf16
    rounding torch gives is round-to-nearest-even of that fp32 value, and the e4m3 bytes decode to the integers meant."""
import math

import numpy as np
import pytest
import torch

import magcache_cases as MC

CPU_CALIB = [(M, D) for M, D, _ in MC.CALIB_CASES] + [(8193, 5120)]


@pytest.mark.parametrize("M,D", CPU_CALIB)
def test_calib_int_case_sums_are_exact_and_order_free(M, D):
    c = MC.calib_int_case(M, D)
    r, rp = c.r.numpy(), c.rp.numpy()
    assert r.dtype == np.float32 and np.array_equal(r, np.rint(r)) and np.array_equal(rp, np.rint(rp))
    assert np.abs(r).max() <= 7 and np.abs(rp).max() <= 7 and bool((rp[:, 0] != 0).all())
    assert np.abs(r - rp).max() <= 2 and bool((r != rp).any())
    for s in c.dots:
        assert int(np.abs(s).max()) <= 49 * D < 2 ** 24
    assert bool((c.dots[1] > 0).all()) and bool(np.isfinite(c.rho).all()) and bool(np.isfinite(c.omc).all())
    # fp32 accumulation of the squares in two different orders: both exact
    assert np.array_equal(np.cumsum(r * r, axis=1, dtype=np.float32)[:, -1].astype(np.int64), c.dots[0])
    assert np.array_equal(np.cumsum((r * rp)[:, ::-1], axis=1, dtype=np.float32)[:, -1].astype(np.int64), c.dots[2])
    rng = np.random.default_rng(5)
    for v, want in ((c.rho, c.sums[0]), (c.omc, c.sums[2])):
        v64 = v.astype(np.float64)
        exact = math.fsum(v64.tolist())
        for order in (np.arange(M), rng.permutation(M), np.argsort(v64)):
            assert float(np.cumsum(v64[order])[-1]) == exact            # a plain left-to-right sum, no pairwise tree
        assert float(want) == exact
    assert float(c.sums[3]) == M
    # the two-pass standard deviation against the kernel's one-pass form in fp64: the 1e-6 of the GPU test covers it
    one_pass = math.sqrt(max((c.sums[1] - c.sums[0] * c.sums[0] / M) / (M - 1), 0.0))
    assert abs(one_pass - c.std64) <= 1e-8 * c.std64 + 1e-12


def test_calib_rows_restates_the_reference_on_integers():
    """the float32 restatement against the reference's torch expressions in fp64, on a case of every width"""
    for M, D in ((777, 1028), (1031, 5120)):
        c = MC.calib_int_case(M, D)
        want = MC.calib_ref64(c.r, c.rp)
        assert abs(float(c.stats0) - want[0]) < 1e-6 and abs(c.std64 - want[1]) < 1e-6 and abs(float(c.stats2) - want[2]) < 1e-6


def test_calib_random_case_spans_six_decades():
    for D in MC.CALIB_RANDOM_D:
        c = MC.calib_random_case(MC.CALIB_RANDOM_M, D)
        n = c.rp.double().norm(dim=-1)
        assert float(n.max() / n.min()) > 1e5 and bool(torch.isfinite(c.r).all())
        s = MC.calib_ref64(c.r, c.rp)
        assert 0.9 < s[0] < 1.1 and 0.03 < s[1] < 0.07 and 0 < s[2] < 0.02


@pytest.mark.parametrize("M,N,K", MC.FP8_SHAPES)
def test_fp8_int_case_expected_values_are_exact(M, N, K):
    c = MC.fp8_int_case(M, N, K)
    assert K <= 8704 and float(c.acc.abs().max()) <= 4 * K <= 34816
    # the bytes are the integers meant, and every value of [-2, 2] occurs
    assert torch.equal(c.aq.view(torch.float8_e4m3fn).double(), c.ai.double())
    assert torch.equal(c.wq.view(torch.float8_e4m3fn).double(), c.wi.double())
    assert sorted(torch.unique(c.ai).tolist()) == [-2, -1, 0, 1, 2]
    assert int(torch.tensor(1.0).to(torch.float8_e4m3fn).view(torch.uint8)) == 0x38     # the pad byte of the strided test
    for s, lo, hi in ((c.sa, -2, 2), (c.sw, -1, 1), (c.gate, -2, 1)):
        e = torch.log2(s)
        assert torch.equal(e, e.round()) and lo <= float(e.min()) and float(e.max()) <= hi
    assert torch.equal(c.bias * 4, (c.bias * 4).round()) and float(c.bias.abs().max()) <= 2
    # exactly representable in fp32: nothing is lost by the cast, so the kernel's fp32 multiply-add has no rounding
    assert torch.equal(c.c32.double(), c.c64)
    assert torch.equal((c.acc * (c.sa.double()[:, None] * c.sw.double())).float().double(), c.acc * (c.sa.double()[:, None] * c.sw.double()))
    # torch's bf16 is round-to-nearest-even of that value
    assert np.array_equal(c.cb.float().numpy(), MC.bf16_rne(c.c32.numpy()))
    if M > 1:                                                            # ... and it does round somewhere (one row of scale
        assert bool((c.cb.float() != c.c32).any())                       # 1/4 fits 8 bits)
    for xg in (c.x_gate, c.x_nogate):
        assert torch.equal(xg.float().double(), xg)
    assert torch.equal(c.x0.float(), c.x0.float().round())


@pytest.mark.parametrize("M,N,K", MC.bf16_all_shapes())
def test_bf16_int_case_expected_values_are_exact(M, N, K):
    """what test_gemm_bf16_exact_gpu.py rests on: |A| |W|^T < 2^24 (fp32 accumulation exact in any order and under any K split),
    acc + bias and every gated residual round-trip through fp32, the bf16 value is round-to-nearest-even of the fp32 one, and
    the rounding mode is observable: at least 5 % ties and 40 % inexact outputs wherever there are 1000 outputs"""
    c = MC.bf16_int_case(M, N, K)
    assert torch.equal(c.a.double(), c.ai.double()) and torch.equal(c.w.double(), c.wi.double())      # bf16 holds the integers
    assert int(c.ai.abs().max()) <= 8 and int(c.wi.abs().max()) <= 8
    if M * K >= 1000:
        assert sorted(torch.unique(c.ai).tolist()) == list(range(-8, 9))
    bound = float((c.ai.abs().double() @ c.wi.abs().double().t()).max())
    assert bound <= 64 * K < 2 ** 24 and float(c.acc.abs().max()) <= bound
    assert torch.equal(c.bias * 4, (c.bias * 4).round()) and float(c.bias.abs().max()) <= 2
    for k in range(3):
        e = torch.log2(c.table[k])
        assert torch.equal(e, ((torch.arange(N) + k) % 4 - 2).float())
    assert torch.equal(c.gate, c.table[0]) and torch.equal(c.gate2, c.table[1])
    # the selector takes every value inside every full 16-row block
    for b in range(M // 16):
        assert sorted(torch.unique(c.sel[16 * b:16 * b + 16]).tolist()) == [0, 1, 2]
    assert int(c.sel.max()) <= 2
    # exactly representable in fp32: the kernel's fp32 adds and multiplies have no rounding
    for v in (c.acc, c.c32, c.x_gate, c.x_nogate, c.x_sel, c.x_sets):
        assert torch.equal(v.float().double(), v)
    assert torch.equal(c.x0.float(), c.x0.float().round()) and torch.equal(c.x, c.x.round())
    assert torch.equal((c.x_gate - c.x0.double()).float().double(), c.x_gate - c.x0.double())     # the captured residual too
    # torch's bf16 rounding agrees with the bit-pattern restatement, and bf16 holds the result
    assert torch.equal(c.c32.float().bfloat16().double(), c.cb) and torch.equal(c.cb.bfloat16().double(), c.cb)
    ties, inexact = MC.bf16_ties(c.c32)
    print(f"M {M} N {N} K {K}: max |A||W|^T {bound:.0f}, ties {ties:.3f}, inexact {inexact:.3f}")
    if M * N >= 1000:
        assert ties >= 0.05 and inexact >= 0.40
        trunc = (c.c32.float().view(torch.int32) & -65536).view(torch.float32).double()
        assert float((trunc != c.cb).double().mean()) >= 0.20          # a truncating store differs on a fifth of the outputs


@pytest.mark.parametrize("M,N,K", MC.BF16_ROWSPLIT_SHAPES)
def test_bf16_rowsplit_case_is_exact_and_its_second_linear_differs(M, N, K):
    c = MC.bf16_int_case(M, N, K)
    for m_split in (200, 256):
        r = MC.bf16_rowsplit_case(M, N, K, m_split)
        for v in (r.c32, r.x_gate):
            assert torch.equal(v.float().double(), v)
        assert torch.equal(r.cb[:m_split], c.cb[:m_split]) and torch.equal(r.x_gate[:m_split], c.x_gate[:m_split])
        # the wrong weight, the wrong bias or the wrong gate on the second range shows on most of its outputs
        assert float((r.cb[m_split:] != c.cb[m_split:]).double().mean()) > 0.9
        assert bool((r.bias_b != c.bias).any()) and bool((r.gate_b != c.gate).all())

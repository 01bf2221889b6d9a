"""GPU: the kernels of magcache_ops.hip (calib_stats, calib_finalize, skip_add, residual_sub) at the widths, row counts, grids
and strides where they can go wrong, against expected values that are exact (tests/magcache_cases.py, whose premises
test_magcache_cases_cpu.py checks).

calib_stats on integer slabs: the three row sums are exact in fp32 in any order, every step after them is one correctly
rounded fp32 operation, and the fp64 sum of the per-row values is exact in any order, so sums[0], sums[2], stats[0] and
stats[2] are compared BIT FOR BIT with the numpy restatement: whatever the width (ending inside the 1024-element trip or
not), the number of rows per wave, the grid (the last arriver strides over the blocks' partial sums by 256) and the leading
dimensions (pad columns hold 1e30).  sums[1] (rho^2, not order-free in fp64) within 1e-12, stats[1] within 1e-6 of the
two-pass fp64 standard deviation (the cancellation in S2 - S1^2 / n leaves about 1e-9, the rest is one fp32 rounding).
Random slabs over six decades of row norms are held to the bar of test_calib_stats_matches_torch_ops carried over to an fp64
reference: |kernel - fp64| <= |torch fp32 - fp64| + 2e-6.

skip_add / residual_sub are one fp32 operation per element: bitwise against torch at every edge of the two-groups-per-trip
loop, contiguous and strided, with the output's pad columns and the rows behind M checked for their sentinel bits.

(The M * D/4 >= 2^31 bound of skip_add / residual_sub is not exercised: it needs more than 32 GiB.)"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import magcache_cases as MC  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from oracle import magcache_ref as MR  # noqa: E402

DEV = "cuda:0"
POISON = 1e30                 # finite in fp32 and bf16: a pad column that is read blows the sums up, it does not hide as nan
SENT = -7.0


def slab(t, ld):
    """t [M, D] -> a device view [M, D] of an [M, ld] allocation whose pad columns hold POISON"""
    M, D = t.shape
    whole = torch.full((M, ld), POISON, dtype=t.dtype, device=DEV)
    whole[:, :D] = t.to(DEV)
    return whole[:, :D]


def f32_bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(1).view(np.uint32)[0])


def f64_bits(x):
    return int(np.asarray(x, dtype=np.float64).reshape(1).view(np.uint64)[0])


def same_bits(a, b):
    """torch tensors of one dtype (fp32 or fp64): equal bit for bit (torch.equal would take -0 for +0)"""
    it = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def check_exact(c, stats, sums, what):
    stats, sums = stats.numpy(), sums.numpy()
    print(f"{what}: sums {sums.tolist()} want {c.sums.tolist()}; stats {stats.tolist()} want "
          f"{[float(c.stats0), c.std64, float(c.stats2)]}")
    assert sums[3] == c.M, what
    assert f64_bits(sums[0]) == f64_bits(c.sums[0]), what
    assert f64_bits(sums[2]) == f64_bits(c.sums[2]), what
    assert abs(sums[1] - c.sums[1]) <= 1e-12 * c.sums[1], what
    assert f32_bits(stats[0]) == f32_bits(c.stats0), what
    assert f32_bits(stats[2]) == f32_bits(c.stats2), what
    assert abs(float(stats[1]) - c.std64) <= 1e-6 * c.std64, what


# ----------------------------------------------------------------------------- calib_stats: exact
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("M,D,n_blocks", MC.CALIB_CASES)
def test_calib_stats_is_exact_on_integer_slabs(M, D, n_blocks, strided):
    c = MC.calib_int_case(M, D)
    r, rp = slab(c.r, D + 4 if strided else D), slab(c.rp, D + 8 if strided else D)
    assert r.stride(0) == (D + 4 if strided else D)
    stats, sums = H.calib_stats(r, rp, n_blocks)
    check_exact(c, stats, sums, f"M {M} D {D} n_blocks {n_blocks} strided {strided}")


def test_calib_stats_rearms_its_ticket_on_any_scratch():
    """one scratch buffer, all 0xFF bytes (ticket included) before the first launch, used by launches of different grids
    back to back: every result exact; the same launch twice: the same bits"""
    partial = torch.empty(4 * 2048 + 1, dtype=torch.float64, device=DEV)
    partial.view(torch.uint8).fill_(0xFF)
    for M, D, n_blocks in ((4099, 1536, 2048), (777, 1028, 64), (257, 1024, 257)):
        c = MC.calib_int_case(M, D)
        stats, sums = H.calib_stats(c.r.to(DEV), c.rp.to(DEV), n_blocks, partial=partial)
        check_exact(c, stats, sums, f"shared scratch, M {M} D {D} n_blocks {n_blocks}")
    c = MC.calib_int_case(777, 1028)
    r, rp = c.r.to(DEV), c.rp.to(DEV)
    first = H.calib_stats(r, rp, 300, partial=partial)
    second = H.calib_stats(r, rp, 300, partial=partial)
    check_exact(c, *first, "shared scratch, first of two")
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])


@pytest.mark.parametrize("M,D,n_blocks", [(5, 256, 2048), (777, 1028, 64), (4099, 1536, 2048), (1031, 5120, 300)])
def test_calib_two_rank_path_equals_one_launch(M, D, n_blocks):
    """what sequence parallel does: each rank launches with stats = NULL over its rows, the sums are added in fp64,
    launch_calib_finalize makes the statistics"""
    c = MC.calib_int_case(M, D)
    r, rp = c.r.to(DEV), c.rp.to(DEV)
    one_stats, one_sums = H.calib_stats(r, rp, n_blocks)
    check_exact(c, one_stats, one_sums, f"one launch, M {M} D {D}")
    h = M // 2
    parts = []
    for lo, hi in ((0, h), (h, M)):
        stats, sums = H.calib_stats(r[lo:hi], rp[lo:hi], n_blocks, want_stats=False)
        assert bool((stats == H.CALIB_SENTINEL).all())
        assert float(sums[3]) == hi - lo
        parts.append(sums)
    total = parts[0] + parts[1]
    assert total.dtype == torch.float64
    assert f64_bits(total[0]) == f64_bits(c.sums[0]) and f64_bits(total[2]) == f64_bits(c.sums[2]) and float(total[3]) == M
    stats = H.calib_finalize(total.to(DEV))
    print(f"M {M} D {D}: two ranks {stats.tolist()} one launch {one_stats.tolist()}")
    assert same_bits(stats[0], one_stats[0]) and same_bits(stats[2], one_stats[2])
    assert abs(float(stats[1]) - float(one_stats[1])) <= 1e-6 * float(one_stats[1])
    assert abs(float(stats[1]) - c.std64) <= 1e-6 * c.std64


# ----------------------------------------------------------------------------- calib_stats: random values, zero rows
def within_the_fp64_bar(got, r, rp, what):
    """|kernel - fp64| <= |the reference's torch fp32 expressions - fp64| + 2e-6 for every finite statistic; inf / nan where the
    torch expressions have them"""
    ref64 = MC.calib_ref64(r, rp)
    ref32 = MR.calibration_stats(r, rp)
    for k in range(3):
        g = float(got[k])
        print(f"{what} stat {k}: kernel {g!r} torch fp32 {ref32[k]!r} fp64 {ref64[k]!r}")
        assert np.isinf(g) == np.isinf(ref32[k]) and np.isnan(g) == np.isnan(ref32[k]), (what, k)
        if np.isfinite(ref32[k]):
            assert np.isfinite(ref64[k])
            assert abs(g - ref64[k]) <= abs(ref32[k] - ref64[k]) + 2e-6, (what, k)


@pytest.mark.parametrize("D", MC.CALIB_RANDOM_D)
def test_calib_stats_random_rows_over_six_decades_against_fp64(D):
    c = MC.calib_random_case(MC.CALIB_RANDOM_M, D)
    stats, sums = H.calib_stats(c.r.to(DEV), c.rp.to(DEV))
    assert float(sums[3]) == c.M
    within_the_fp64_bar(stats, c.r, c.rp, f"D {D}")


@pytest.mark.parametrize("both", [False, True], ids=["rp-row-zero", "both-rows-zero"])
def test_calib_stats_zero_row(both):
    c = MC.calib_random_case(MC.CALIB_RANDOM_M, 1536)
    r, rp = c.r.clone(), c.rp.clone()
    rp[517] = 0
    if both:
        r[517] = 0
    stats, sums = H.calib_stats(r.to(DEV), rp.to(DEV))
    assert float(sums[3]) == c.M
    assert not np.isfinite(float(stats[0])) and np.isfinite(float(stats[2]))
    within_the_fp64_bar(stats, r, rp, "zero row in rp" + (" and r" if both else ""))


# ----------------------------------------------------------------------------- calib_stats: refusals
def test_calib_stats_refuses_what_its_loads_cannot_take():
    M, D = 16, 64
    flat_r = torch.ones(M * (D + 8) + 8, device=DEV)
    flat_p = torch.ones(M * (D + 8) + 8, device=DEV)
    r, rp = flat_r[:M * D].view(M, D), flat_p[:M * D].view(M, D)
    partial = torch.zeros(4 * 8 + 1, dtype=torch.float64, device=DEV)

    def refused(what, r=r, rp=rp, n_blocks=8, **kw):
        out = (torch.full((4,), SENT, dtype=torch.float64, device=DEV), torch.full((3,), SENT, device=DEV))
        with pytest.raises(_lib.MagCacheHipError) as e:
            H.calib_stats(r, rp, n_blocks, partial=partial, out=out, **kw)
        assert e.value.status == _lib.MC_EINVAL, what
        torch.cuda.synchronize()
        assert bool((out[0] == SENT).all()) and bool((out[1] == SENT).all()), what

    H.calib_stats(r, rp, 8, partial=partial)                     # the base call runs
    H.calib_stats(r, rp, 8, partial=partial, ldr=D + 4, ldrp=D + 8)
    refused("M = 1", M=1)
    refused("D % 4", D=D - 2)
    refused("n_blocks = 0", n_blocks=0)
    refused("ldr % 4", ldr=D + 2)
    refused("ldrp % 4", ldrp=D + 6)
    refused("ldr < D", ldr=D - 4)
    refused("ldrp < D", ldrp=D - 4)
    for off in (1, 2, 3):                                        # 4, 8, 12 bytes off a 16-byte boundary
        refused(f"r + {4 * off} bytes", r=flat_r[off:off + M * D].view(M, D))
        refused(f"rp + {4 * off} bytes", rp=flat_p[off:off + M * D].view(M, D))


# ----------------------------------------------------------------------------- skip_add / residual_sub
# (M, D) -> groups of 4 = M * D / 4 against the kernel's 256 threads x 2 groups per trip: 2 (a few threads of the tail), 256 (the
# tail of every thread), 264 (8 threads in the pair loop), 512 (the pair loop alone), 520 (two blocks), 77 x 256 and 513 x 1536
# (many blocks, one trip), 4099 x 5120 = 5.2 M groups > 2 x 8192 x 256: the grid is capped, a second trip and a tail
SKIP_CASES = [(1, 8), (32, 32), (33, 32), (64, 32), (65, 32), (77, 256), (513, 1536), (4099, 5120)]
TAIL_ROWS = 8


def guarded_out(M, D, ld):
    whole = torch.full((M + TAIL_ROWS, ld), SENT, device=DEV)
    return whole, whole[:M, :D]


def guards_kept(whole, M, D):
    sent = torch.tensor(SENT).view(torch.int32).item()
    w = whole.view(torch.int32)
    return bool((w[:M, D:] == sent).all()) and bool((w[M:] == sent).all())


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("M,D", SKIP_CASES)
def test_skip_add_and_residual_sub_bitwise(M, D, strided):
    g = torch.Generator(device=DEV).manual_seed(1000 * M + D)
    x0v = torch.randn(M, D, generator=g, device=DEV).bfloat16()
    rv = torch.randn(M, D, generator=g, device=DEV) * torch.exp2(torch.randint(-6, 4, (M, 1), generator=g, device=DEV).float())
    ldx0, ldr, ldo = (D + 8, D + 4, D + 12) if strided else (D, D, D)
    x0, r = slab(x0v, ldx0), slab(rv, ldr)
    assert (x0.stride(0), r.stride(0)) == (ldx0, ldr)
    whole, out = guarded_out(M, D, ldo)
    H.skip_add(x0, r, out)
    want = x0v.float() + rv                                     # one fp32 add per element
    assert same_bits(out, want)
    assert guards_kept(whole, M, D)
    assert same_bits(r, rv) and torch.equal(x0, x0v)            # the inputs are inputs
    # r2 = x - x0 with x = the sum above
    x = slab(want, ldr)
    whole2, r2 = guarded_out(M, D, ldo)
    H.residual_sub(x, x0, r2)
    assert same_bits(r2, want - x0v.float())
    assert guards_kept(whole2, M, D)
    assert bool(torch.isfinite(r2).all())


def test_skip_add_and_residual_sub_refusals():
    M, D = 16, 64
    n = M * (D + 16) + 16
    x0b = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    fb = torch.ones(n, device=DEV)
    ob = torch.full((n,), SENT, device=DEV)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream

    def ptr(t, byte_off=0):
        return C.c_void_p(t.data_ptr() + byte_off)

    def both(what, want, x0_off=0, f_off=0, o_off=0, D=D, ldx0=D, ldf=D, ldo=D):
        """skip_add(x0, f, out) and residual_sub(f, x0, out): the same three operands, the fp32 input in its own place"""
        a = lib.mc_op_skip_add(ptr(x0b, x0_off), ldx0, ptr(fb, f_off), ldf, ptr(ob, o_off), ldo, M, D, st)
        b = lib.mc_op_residual_sub(ptr(fb, f_off), ldf, ptr(x0b, x0_off), ldx0, ptr(ob, o_off), ldo, M, D, st)
        assert (a, b) == (want, want), (what, a, b)
        torch.cuda.synchronize()
        if want != _lib.MC_OK:
            assert bool((ob == SENT).all()), what

    both("D % 8", _lib.MC_EINVAL, D=D - 4)
    both("ldx0 % 8", _lib.MC_EINVAL, ldx0=D + 4)
    both("fp32 input ld % 4", _lib.MC_EINVAL, ldf=D + 2)
    both("output ld % 4", _lib.MC_EINVAL, ldo=D + 2)
    both("x0 + 4 bytes", _lib.MC_EINVAL, x0_off=4)
    both("x0 + 2 bytes", _lib.MC_EINVAL, x0_off=2)
    for off in (4, 8, 12):
        both(f"fp32 input + {off} bytes", _lib.MC_EINVAL, f_off=off)
        both(f"output + {off} bytes", _lib.MC_EINVAL, o_off=off)
    both("x0 + 8 bytes, the others + 16: aligned enough", _lib.MC_OK, x0_off=8, f_off=16, o_off=16, ldx0=D + 8, ldf=D + 4, ldo=D + 12)
    assert bool((ob[4:4 + D] == 0.0).all()) and bool((ob[:4] == SENT).all())      # residual_sub ran last: 1 - 1

"""Inputs and expected values of the MagCache op tests and the per-row fp8 GEMM tests (test_magcache_cases_cpu.py checks what
they rest on without a GPU; test_magcache_ops_gpu.py and test_fp8_gemm_rows_gpu.py run the HIP kernels on them).  Everything
here is built on the CPU, once per parameter set (the builders are cached: treat what they return as read-only).

Why these inputs.  Both kernels sum products, and a sum of floats depends on its order, so a test on random data needs a
tolerance that also hides a lost column, a pad column read, a block counted twice or a K chunk skipped when the loss is
small.  Small integers make the sums exact in any order, and power-of-two scales keep them exact, so the expected value is one
bit pattern and the bar is equality.

calib_int_case.  rp is uniform integers in [-7, 7] (column 0 never zero), r = clip(rp + [-2, 2], -7, 7).  |r|^2, |rp|^2 and
r.rp are then integers of magnitude <= 49 D <= 49 * 5120 < 2^24: exact in fp32 whatever the lane, the unrolling and the wave
reduction do.  What follows in calib_stats_kernel is one correctly rounded fp32 operation after another (the build has no
fast-math flag) -- sqrtf twice, one divide for rho, fmaxf, one multiply, one divide for cos, one subtract -- restated below in
numpy float32.  The per-row rho and 1 - cos are fp32 values of about one binade, so their fp64 sum over <= 8193 rows needs
at most 24 + 14 bits and is exact in any order too (asserted by the CPU test); the fp64 sum of rho^2 is not, hence 1e-12.

fp8_int_case.  e4m3 bytes of integers in [-2, 2] for A [M, K] and W [N, K], a_scale[m] = 2^((m % 5) - 2), w_scale[n] =
2^((n % 3) - 1), bias multiples of 0.25 in [-2, 2].  Every partial sum of A W^T is an integer of magnitude <= 4 K <= 34816, the
scales shift its exponent, the bias adds multiples of 1/4 to multiples of 1/8: acc * (sa * sw) + bias is exact in fp32.

bf16_int_case (test_gemm_bf16_exact_gpu.py).  Integers in [-8, 8] as bf16 for A [M, K] and W [N, K]: |A| |W|^T <= 64 K < 2^24 for
every K here, so fp32 accumulation is exact in any order and under any K split; a bias of quarters keeps acc + bias within 24
bits.  Unlike the fp8 case the sums are LARGE against bf16's 8 significant bits: most outputs are no bf16 value and a good share
lie exactly between two, so EPI_BF16 has one right bit pattern only under round-to-nearest-even (truncation, or ties away from
zero, differ).  Gates are powers of two: x + gate * bf16(acc + bias) is exact in fp32 as well."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32

# (M, D, n_blocks): D ends inside the kernel's 1024-element trip (4, 252, 1028), is one trip (256 = one chunk of it, 1024)
# or the engines' widths (1536, 3072, 5120); fewer rows than the block's 4 waves, fewer rows than waves in the grid (5 rows
# under 2048 blocks), grids that are no multiple of the 256 the last-arriver loop strides by (1, 3, 257, 64, 300)
CALIB_CASES = [(2, 4, 1), (3, 252, 3), (5, 256, 2048), (257, 1024, 257), (777, 1028, 64), (4099, 1536, 2048),
               (1031, 3072, 2048), (1031, 5120, 300)]
CALIB_SEED = 20240
CALIB_EPS = F32(1e-8)              # the 1e-8f of the kernel's cosine denominator
CALIB_RANDOM_D = [1536, 3072, 5120]
CALIB_RANDOM_M = 1031

# (M, N, K) of the fp8 GEMM: one row; one row short of a tile; one row into the second tile; a partial second tile with a long
# K; the longest K the Wan engines have (FFN-2 of the 1.3B model, 8960 cut to a multiple of 256); 10 M tiles x 3 N tiles = a
# group of 8 and a group of 2 M tiles, 30 workgroups over 8 XCDs
FP8_SHAPES = [(1, 256, 512), (255, 256, 768), (257, 512, 512), (300, 256, 2560), (64, 256, 8704), (2309, 768, 512)]
FP8_STRIDED_SHAPES = [(257, 512, 512), (2309, 768, 512)]
FP8_SEED = 77


# ----------------------------------------------------------------------------- calib_stats
def calib_rows(r, rp):
    """numpy float32 restatement of calib_stats_kernel's per-row sequence for INTEGER-valued r / rp [M, D] (the three sums
    are then exact, taken here in int64): -> rho, 1 - cos (float32 [M]) and the three integer sums (int64 [M])"""
    ri, pi = r.astype(np.int64), rp.astype(np.int64)
    aa, bb, ab = (ri * ri).sum(1), (pi * pi).sum(1), (ri * pi).sum(1)
    na, nb = np.sqrt(aa.astype(F32)), np.sqrt(bb.astype(F32))
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = na / nb
        den = np.maximum(na, CALIB_EPS) * np.maximum(nb, CALIB_EPS)
        omc = F32(1.0) - ab.astype(F32) / den
    assert rho.dtype == F32 and den.dtype == F32 and omc.dtype == F32
    return rho, omc, (aa, bb, ab)


def calib_expect(rho, omc):
    """the kernel's sums[4] (fp64) and stats[3] (fp32) from the per-row fp32 values.  stats[1] is the two-pass fp64 unbiased
    standard deviation, not the kernel's S2 - S1^2 / n form: the GPU test allows that form's cancellation 1e-6"""
    M = rho.shape[0]
    rho64, omc64 = rho.astype(np.float64), omc.astype(np.float64)
    sums = np.array([rho64.sum(), (rho64 * rho64).sum(), omc64.sum(), float(M)], dtype=np.float64)
    stats0, stats2 = F32(sums[0] / M), F32(sums[2] / M)
    return sums, stats0, float(np.std(rho64, ddof=1)), stats2


@functools.lru_cache(maxsize=None)
def calib_int_case(M, D, seed=CALIB_SEED):
    rng = np.random.default_rng([seed, M, D])
    rp = rng.integers(-7, 8, size=(M, D))
    rp[:, 0] = np.where(rp[:, 0] == 0, 3, rp[:, 0])
    r = np.clip(rp + rng.integers(-2, 3, size=(M, D)), -7, 7)
    rho, omc, dots = calib_rows(r, rp)
    sums, s0, s1, s2 = calib_expect(rho, omc)
    return SimpleNamespace(M=M, D=D, r=torch.from_numpy(r.astype(F32)), rp=torch.from_numpy(rp.astype(F32)), rho=rho, omc=omc,
                           dots=dots, sums=sums, stats0=s0, std64=s1, stats2=s2)


def calib_ref64(r, rp):
    """the three statistics in fp64 (reference magcache_generate.py:167-169 with cosine_similarity's eps = 1e-8 on each
    norm), as Python floats; inf / nan where a norm is zero, like the torch expressions"""
    r, rp = r.double(), rp.double()
    na, nb = r.norm(dim=-1), rp.norm(dim=-1)
    ratio = na / nb
    cos = (r * rp).sum(-1) / (na.clamp_min(1e-8) * nb.clamp_min(1e-8))
    return ratio.mean().item(), ratio.std().item(), (1 - cos).mean().item()


@functools.lru_cache(maxsize=None)
def calib_random_case(M, D, seed=CALIB_SEED):
    """rows of rp scaled by 10^U(-3, 3); r = rp (1 + 0.05 g) + 0.1 |rp|_rms noise, g one normal per row"""
    g = torch.Generator().manual_seed(seed + D)
    rp = torch.randn(M, D, generator=g) * torch.pow(10.0, torch.rand(M, 1, generator=g) * 6 - 3)
    rms = rp.double().pow(2).mean(-1, keepdim=True).sqrt().float()
    r = rp * (1 + 0.05 * torch.randn(M, 1, generator=g)) + 0.1 * rms * torch.randn(M, D, generator=g)
    return SimpleNamespace(M=M, D=D, r=r, rp=rp)


# ----------------------------------------------------------------------------- the per-row fp8 GEMM
def bf16_rne(x32):
    """float32 array -> the float32 value of its bf16 rounding (round to nearest even on the bit pattern; finite inputs)"""
    u = np.ascontiguousarray(x32, dtype=F32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(F32)


@functools.lru_cache(maxsize=None)
def fp8_int_case(M, N, K, seed=FP8_SEED):
    """-> aq [M, K], wq [N, K] uint8 (e4m3 bytes), sa [M], sw [N], bias [N], gate [N] fp32, x [M, N] fp32 (integers), x0 [M, N]
    bf16, and the expected values: acc (fp64, the integer product), c64 = acc * (sa * sw) + bias, c32, cb (bf16), x_gate /
    x_nogate (fp64) = x + gate * float(cb) / x + float(cb).  All CPU tensors."""
    g = torch.Generator().manual_seed(seed + 131 * M + 7 * N + K)
    ai = torch.randint(-2, 3, (M, K), generator=g)
    wi = torch.randint(-2, 3, (N, K), generator=g)
    aq = ai.float().to(torch.float8_e4m3fn).view(torch.uint8)
    wq = wi.float().to(torch.float8_e4m3fn).view(torch.uint8)
    sa = torch.exp2((torch.arange(M) % 5 - 2).float())
    sw = torch.exp2((torch.arange(N) % 3 - 1).float())
    bias = torch.randint(-8, 9, (N,), generator=g).float() * 0.25
    gate = torch.exp2((torch.arange(N) % 4 - 2).float())
    x = torch.randint(-8, 9, (M, N), generator=g).float()
    x0 = torch.randint(-8, 9, (M, N), generator=g).float().bfloat16()
    acc = ai.double() @ wi.double().t()
    c64 = acc * (sa.double()[:, None] * sw.double()[None, :]) + bias.double()
    c32 = c64.float()
    cb = c32.bfloat16()
    return SimpleNamespace(M=M, N=N, K=K, ai=ai, wi=wi, aq=aq, wq=wq, sa=sa, sw=sw, bias=bias, gate=gate, x=x, x0=x0, acc=acc,
                           c64=c64, c32=c32, cb=cb, x_gate=x.double() + gate.double() * cb.double(),
                           x_nogate=x.double() + cb.double())


# ----------------------------------------------------------------------------- the bf16 GEMM
# (M, N, K), the smallest shapes at which each piece of index arithmetic of the three paths changes.
# 128 x 128 kernel: one row x one quad; N off the tile (the column clamp min(n, N - 4)); one row / one quad into a second tile
# with 3 K steps; 3 x 4 tiles; 9 M tiles against GROUP_M = 8 (a group remainder) x 3 N tiles = 27 workgroups over 8 XCDs
BF16_SMALL_SHAPES = [(1, 4, 64), (127, 132, 64), (129, 260, 192), (300, 388, 128), (1100, 260, 64)]
# gemm_bf16_v2: the shortest K (4 K tiles) with one row; one row short of a tile, an odd number of K-tile pairs; one row into a
# second M tile; 3 x 3 tiles; 9 N tiles (MC_V2_GROUP_M_MID); 32 N tiles (MC_V2_GROUP_M_WIDE) x 3 M tiles (a group remainder)
BF16_V2_SHAPES = [(1, 256, 256), (255, 256, 384), (257, 512, 256), (700, 768, 512), (300, 2304, 256), (513, 8192, 256)]
BF16_V2_TRIP_SHAPES = [(700, 768, 512), (257, 512, 256)]      # ... walked by 1, 2 and 4 persistent workgroups
BF16_SPLITK_MN = [(77, 256), (300, 512), (513, 768)]          # split-K: slices 2, 3, 8 x K = 256 s, 512 s
BF16_SPLITK_SLICES = [2, 3, 8]
BF16_COMMON_SHAPE = (300, 512, 512)                           # a shape all three paths accept
BF16_ROWSPLIT_SHAPES = [(513, 768, 512), (700, 768, 512), (700, 768, 1024)]
BF16_SEED = 4242


def bf16_all_shapes():
    s = BF16_SMALL_SHAPES + BF16_V2_SHAPES + [BF16_COMMON_SHAPE] + BF16_ROWSPLIT_SHAPES
    s += [(M, N, k * sl) for M, N in BF16_SPLITK_MN for sl in BF16_SPLITK_SLICES for k in (256, 512)]
    return sorted(set(s))


def bf16_gate_set(N, k):
    """gate vector k of the case: 2^((n + k) % 4 - 2) -- k = 0 the gate, 1 the second gate, 0..2 the rows of the table"""
    return torch.exp2(((torch.arange(N) + k) % 4 - 2).float())


@functools.lru_cache(maxsize=None)
def bf16_int_case(M, N, K, seed=BF16_SEED):
    """-> a [M, K], w [N, K] bf16 (integers in [-8, 8]), bias [N] (multiples of 1/4 in [-2, 2]), gate / gate2 [N] and table [3, N]
    (powers of two), sel uint8 [M] (every value of 0..2 inside every 16-row block), x [M, N] fp32 and x0 [M, N] bf16 (integers in
    [-8, 8]); and, in fp64: acc = a w^T, c32 = acc + bias, cb = the bf16 rounding (nearest even) of c32, x_gate / x_nogate /
    x_sel / x_sets = x + g * cb with g = gate / 1 / (sel ? gate2 : gate) / table[sel].  All CPU tensors."""
    g = torch.Generator().manual_seed(seed + 131 * M + 7 * N + K)
    ai = torch.randint(-8, 9, (M, K), generator=g)
    wi = torch.randint(-8, 9, (N, K), generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g).float() * 0.25
    x = torch.randint(-8, 9, (M, N), generator=g).float()
    x0 = torch.randint(-8, 9, (M, N), generator=g).float().bfloat16()
    table = torch.stack([bf16_gate_set(N, k) for k in range(3)])
    rows = torch.arange(M)
    sel = ((rows + rows // 16) % 3).to(torch.uint8)
    acc = ai.double() @ wi.double().t()
    c32 = acc + bias.double()
    cb = torch.from_numpy(bf16_rne(c32.float().numpy())).double()
    t64 = table.double()
    g_sel = torch.where(sel[:, None] != 0, t64[1][None, :], t64[0][None, :])
    return SimpleNamespace(M=M, N=N, K=K, ai=ai, wi=wi, a=ai.float().bfloat16(), w=wi.float().bfloat16(), bias=bias, gate=table[0],
                           gate2=table[1], table=table, sel=sel, x=x, x0=x0, acc=acc, c32=c32, cb=cb,
                           x_gate=x.double() + t64[0] * cb, x_nogate=x.double() + cb, x_sel=x.double() + g_sel * cb,
                           x_sets=x.double() + t64[sel.long()] * cb)


@functools.lru_cache(maxsize=None)
def bf16_rowsplit_case(M, N, K, m_split, seed=BF16_SEED):
    """bf16_int_case(M, N, K) whose rows [m_split, M) multiply with a second Linear: w_b / bias_b of the case seeded seed + 1 and
    gate_b = its gate2.  -> w_b, bias_b, gate_b and the fp64 c32, cb, x_gate of all M rows"""
    c, c2 = bf16_int_case(M, N, K, seed), bf16_int_case(M, N, K, seed + 1)
    acc = torch.cat([c.acc[:m_split], c.ai[m_split:].double() @ c2.wi.double().t()])
    c32 = acc + torch.cat([c.bias.double().expand(m_split, N), c2.bias.double().expand(M - m_split, N)])
    cb = torch.from_numpy(bf16_rne(c32.float().numpy())).double()
    g = torch.cat([c.gate.double().expand(m_split, N), c.gate2.double().expand(M - m_split, N)])
    return SimpleNamespace(w_b=c2.w, bias_b=c2.bias, gate_b=c.gate2, c32=c32, cb=cb, x_gate=c.x.double() + g * cb)


def bf16_ties(c32):
    """fp64 tensor of fp32-representable values -> (share that lies exactly between two bf16 values, share that is no bf16 value)"""
    low = c32.float().numpy().view(np.uint32) & 0xFFFF
    return float((low == 0x8000).mean()), float((low != 0).mean())


def gelu_tanh64(x):
    """GELU(approximate='tanh') in fp64"""
    x = x.double()
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))

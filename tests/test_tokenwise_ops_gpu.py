"""GPU parity, one test per launcher: the token-wise kernels of elementwise.hip and the quantising GEMM epilogue that the
whole-model tests only reach at toy widths.  Every kernel is called on its own -- through the shipped C ABI where it has
an entry point, otherwise through the mc_test_* wrappers of the reference library (magcache_amd/csrc/test_ops.cpp; the same
elementwise.hip.o / gemm_mxfp8.hip.o objects as the shipped library, see magcache_amd/build.py) -- and compared with a plain
torch fp64 restatement of the same operation that rounds to bf16 where the kernel comment says the kernel does.

Bars.  eps = 2^-24 (fp32 unit roundoff), u = 2^-8 (bf16 unit roundoff: the largest relative error of one rounding; one bf16
ulp is at most 2 u of the value).  A sum of n fp32 terms accumulated to depth d (the longest chain of additions any term goes
through) is within d eps sum|terms| of the exact sum -- the worst case.  For the tree-shaped sums of the gemv and LayerNorm
kernels (d = K / 512 + 12 and the like) that is below the sqrt(K) eps sum|terms| estimate and is the bar.  head_linear and
colmean add along ONE chain (d = K + 1, n_rows + 1): there the bar is c sqrt(K) eps sum|terms| with c = 4 x the maximum
measured on the MI355X (profiles/r07/tolerance_probe.json), and never above the worst case.  Kernels that move data or do one fp32 operation per element are compared with torch.equal.
Every buffer is larger than what the kernel may write; the rest holds a non-zero pattern that is checked afterwards.
The measured margins are recorded with conftest.tolerance_probe (profiles/r07/tolerance_probe.json)."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
from conftest import tolerance_probe  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from oracle import magcache_ref as MR  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
EPS32 = 2.0 ** -24
U16 = 2.0 ** -8
_probe = {}
# 4 x the maxima recorded in profiles/r07/tolerance_probe.json (4 x: seed-to-seed variation of a maximum over ~10^6 elements)
HEAD_LINEAR_C = 4 * 0.788        # tokenwise/head_linear/err_over_sqrtK_eps_sabs
COLMEAN_C = 4 * 0.548             # tokenwise/colmean/err_over_sqrtN_eps_sabs


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def rb(x):
    """round an fp64 tensor to bf16 the way the kernels do (through fp32, to nearest even), back in fp64"""
    return x.float().bfloat16().double()


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def probe(key, value):
    """keep the maximum over the cases of a test and record it"""
    _probe[key] = max(_probe.get(key, 0.0), float(value))
    tolerance_probe("tokenwise/" + key, _probe[key])


def within(got, want, tol, key):
    """|got - want| <= tol element-wise (fp64 tensors); records max(err / tol) under `key`"""
    err = (got.double() - want.double()).abs()
    assert bool(torch.isfinite(got.double()).all()), key
    ratio = float((err / tol.clamp_min(1e-300)).max())
    probe(key, ratio)
    assert ratio <= 1.0, (key, ratio, float(err.max()))


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def refused(fn, *a, **kw):
    with pytest.raises(H.HipStatusError) as e:
        fn(*a, **kw)
    assert e.value.status == H.HIP_INVALID_VALUE
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- headnorm_rope
def headnorm_ref(x, w, cs, eps):
    """x fp64 [M, heads, 128] (bf16 values), w fp32 [128] or None, cs fp32 [M, 64, 2] or None -> (want fp64 bf16-rounded,
    mag = |re cos| + |im sin| per output element, roundings before the rotation)"""
    k = 0
    y = x
    if w is not None:
        rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
        y = rb(x * rstd) * w.double()
        k = 1
        if cs is not None:
            y = rb(y)
            k = 2
    re, im = y[..., 0::2], y[..., 1::2]
    if cs is not None:
        cc, sn = cs[:, None, :, 0].double(), cs[:, None, :, 1].double()
    else:
        cc, sn = torch.ones_like(re), torch.zeros_like(re)
    out = torch.stack([re * cc - im * sn, re * sn + im * cc], dim=-1).flatten(-2)
    mag = torch.stack([(re * cc).abs() + (im * sn).abs(), (re * sn).abs() + (im * cc).abs()], dim=-1).flatten(-2)
    return rb(out), mag, k


@pytest.mark.parametrize("form", ["wq_wk_cs", "cs_only", "wq_wk", "wq_only"])
@pytest.mark.parametrize("M", [1, 5, 1536 + 3])
@pytest.mark.parametrize("n_heads", [1, 2, 3, 4, 5, 24])
def test_headnorm_rope(n_heads, M, form):
    """One wave per (row, q | k, group of 4 heads): ragged groups (n_heads % 4 != 0) run the clamped load / break-on-store
    path, 24 heads are FLUX's 6 full groups, and with M = 1539 the unit index crosses a block of 4 waves inside a row for
    every head count.  Reference per head: bf16(x rsqrt(mean(x^2) + eps)) * w, rounded to bf16 again when RoPE follows, the
    pair rotation with (cos, sin), one bf16 rounding."""
    d = n_heads * 128
    eps = 1e-6
    r0 = 7                                              # table rows skipped by cs_row0
    buf = rnd(M + 2, 3 * d, seed=n_heads * 100 + M, scale=2.0, dtype=torch.bfloat16)   # rows 0 and M + 1: guards
    buf[:, :d] *= 1.5                                   # q and k differ in scale, heads in content (random)
    before = buf.clone()
    x = buf[1:M + 1]
    wq = (1 + rnd(128, seed=2, scale=0.2)) if form != "cs_only" else None
    wk = (0.5 + rnd(128, seed=3, scale=0.2)) if form in ("wq_wk_cs", "wq_wk") else None
    ang = rnd(r0 + M, 64, seed=4, scale=2.0)
    cs_all = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).reshape(r0 + M, 128).contiguous()
    cs = None if form == "wq_wk" else cs_all
    H.headnorm_rope(x, d, wq, wk, eps, cs, r0, n_heads)
    torch.cuda.synchronize()
    # untouched: the v columns, the guard rows
    assert torch.equal(bits(buf[:, 2 * d:]), bits(before[:, 2 * d:]))
    assert torch.equal(bits(buf[0]), bits(before[0])) and torch.equal(bits(buf[M + 1]), bits(before[M + 1]))
    csr = cs_all[r0:].view(M, 64, 2) if cs is not None else None
    worst = worst6 = 0.0
    for part, w in ((0, wq), (1, wk)):
        xin = before[1:M + 1, part * d:(part + 1) * d].double().view(M, n_heads, 128)
        got = x[:, part * d:(part + 1) * d].double().view(M, n_heads, 128)
        want, mag, k = headnorm_ref(xin, w, csr, eps)
        # element-wise: where the kernel's fp32 value and the fp64 one fall on different sides of a rounding tie the two
        # differ by one bf16 ulp <= 2 u of the rounded quantity -- k roundings ahead of the rotation (each moves the
        # output by at most 2 u mag), one after it (2 u |want|); the fp32 rotation itself: 3 eps mag
        within(got, want, 2 * U16 * (k * mag + want.abs()) + 3 * EPS32 * mag + 1e-30, "headnorm_rope/elementwise")
        # in bulk such flips are rare.  The kernel's value ahead of a rounding is within delta = 2^-21 of the fp64 one (the
        # 128-term sum of squares through 1 + 6 additions, rsqrtf, two multiplies: < 8 fp32 ulps); a value lies within
        # delta of a tie with probability <= 2 delta / u = 2^-12, and a flip costs <= 2 u: relative L2 error <=
        # sqrt((k + 1) 2^-12) 2 u = sqrt(k + 1) 2^-13.  (The rotation is orthogonal: it keeps the L2 norm of the errors made
        # ahead of it.)  A missing or an extra rounding changes EVERY element by ~u / 2: 5e-4 .. 2e-3.
        e = rel_l2(got, want)
        # (a bound on an expectation: asserted where >= 2^17 elements make it one -- that is every M = 1539 case)
        if got.numel() >= 1 << 17:
            worst = max(worst, e / (math.sqrt(k + 1) * 2.0 ** -13))
            assert e <= math.sqrt(k + 1) * 2.0 ** -13, (part, e)
        # every size, the few-element cases included: the same model with its spread.  Element i is hit by a flip with
        # probability p <= (k + 1) 2^-12 and then is off by <= 2 u mag_i (mag >= |want|), so the squared error sum has mean
        # <= p (2 u)^2 sum mag^2 and standard deviation <= (2 u)^2 sqrt(p sum mag^4): mean + 6 sigma, plus the fp32 rotation
        p_flip = (k + 1) * 2.0 ** -12
        sq_bar = (2 * U16) ** 2 * (p_flip * float((mag ** 2).sum()) + 6 * math.sqrt(p_flip * float((mag ** 4).sum()))) + \
            (3 * EPS32) ** 2 * float((mag ** 2).sum())
        bar6 = math.sqrt(sq_bar / float((want ** 2).sum()))
        worst6 = max(worst6, e / bar6)
        assert e <= bar6, (part, e, bar6)
    probe("headnorm_rope/rel_l2_over_bar", worst)
    probe("headnorm_rope/rel_l2_over_6sigma_bar", worst6)
    # a row slice with cs_row0 moved along == the same rows of the full call, bit for bit
    if M > 1:
        s0 = M // 2 + 1
        part_buf = before[1 + s0:M + 1].clone()
        H.headnorm_rope(part_buf, d, wq, wk, eps, cs, r0 + s0, n_heads)
        assert torch.equal(bits(part_buf), bits(x[s0:]))


def test_headnorm_rope_refusals():
    x = rnd(4, 256, dtype=torch.bfloat16)
    w = rnd(128)
    refused(H.headnorm_rope, x, 128, w, w, 1e-6, None, 0, 1, M=0)
    refused(H.headnorm_rope, x, 128, w, w, 1e-6, None, 0, 0)
    refused(H.headnorm_rope, x, 127, w, w, 1e-6, None, 0, 1)         # k_col0 off the 4-byte pair grid


# ----------------------------------------------------------------------------- gemv_bf16w / gemv_f32
def gemv_check(kind, N, K, combos, seed, key):
    """y = (acc ? y : 0) + act_out(W act_in(x) + b) against fp64; W bf16 (gemv_bf16w) or fp32 (gemv_f32)"""
    Wt = rnd(N, K, seed=seed, scale=1.0 / math.sqrt(K), dtype=torch.bfloat16 if kind == "bf16w" else torch.float32)
    Wt[:, 0] += 0.25                                    # asymmetric: a column the others do not look like
    x = rnd(K, seed=seed + 1, scale=1.5) + 0.3
    b_full = rnd(N, seed=seed + 2)
    W64 = Wt.double()
    # depth of the fp32 sum: a lane's chain over K (8 or 4 products added per step as a tree of depth 3 or 2), 6 wave-sum
    # steps, the bias; the rounding of the product itself counts as one more
    depth = (K / 512 + 3 if kind == "bf16w" else K / 256 + 2) + 6 + 1 + 1
    cache = {}
    for act_in, act_out, acc, with_bias in combos:
        if act_in not in cache:
            xa = silu64(x.double()) if act_in else x.double()
            cache[act_in] = (W64 @ xa, W64.abs() @ xa.abs())
        dot, sabs = cache[act_in]
        b = b_full if with_bias else None
        pre = dot + (b.double() if with_bias else 0.0)
        sabs_b = sabs + (b.double().abs() if with_bias else 0.0)
        v = silu64(pre) if act_out else pre
        assert float(pre.abs().max()) < 11 and float(x.abs().max()) < 11          # the range the silu bound below is for
        ybuf = rnd(N + 8, seed=seed + 3, scale=2.0) + 5.0           # 4 guard floats on each side
        y0 = ybuf.clone()
        y = ybuf[4:4 + N]
        if kind == "bf16w":
            H.gemv_bf16w(Wt, x, b, y, act_in, act_out, acc)
        else:
            H.gemv_f32(Wt, x, b, y, act_in, act_out)
        want = v + (y0[4:4 + N].double() if acc else 0.0)
        # the device silu is x / (1 + __expf(-x)): the exponent argument x log2(e) is rounded to fp32 (relative error of the
        # exponential <= |x| eps), v_exp_f32 1 ulp, the add, the divide 2.5 ulp -> (|x| + 5) eps < 2^-20 for |x| <= 11.
        # act_in: every term moves by that; act_out: |silu'| <= 1.1 passes the error of the sum on, plus its own.
        tol = (depth * EPS32 + (2.0 ** -20 if act_in else 0.0)) * sabs_b * (1.1 if act_out else 1.0) + \
              (2.0 ** -20 if act_out else 0.0) * v.abs() + 2 * EPS32 * (want.abs() + v.abs()) + 1e-30
        within(y, want, tol, key)
        assert torch.equal(ybuf[:4], y0[:4]) and torch.equal(ybuf[4 + N:], y0[4 + N:])


ALL_COMBOS = [(ai, ao, acc, wb) for ai in (0, 1) for ao in (0, 1) for acc in (0, 1) for wb in (1, 0)]


@pytest.mark.parametrize("N,K", [(16, 8), (17, 512), (30, 520), (3072, 3072), (2 * 3072, 3072), (64, 16384), (27653, 3072)])
def test_gemv_bf16w(N, K):
    """A wave owns 4 rows (the row pointer clamped for N % 16 != 0), the vector is staged in dynamic LDS (64 KiB at
    K = 16384), act_in / act_out apply SiLU, accumulate reads y.  N = 27653: a FLUX-sized modulation matrix with a ragged
    last wave and a ragged last block."""
    combos = ALL_COMBOS if N < 20000 else [(1, 0, 0, 1), (0, 1, 1, 0)]
    gemv_check("bf16w", N, K, combos, seed=N % 97 + K % 89, key="gemv_bf16w/err_over_bound")


def test_gemv_bf16w_refusals():
    Wt = rnd(16, 16400, dtype=torch.bfloat16)
    x, b, y = rnd(16400), rnd(16), rnd(16)
    refused(H.gemv_bf16w, Wt, x, b, y, K=16392)          # beyond the 64 KiB of LDS the vector is staged in
    refused(H.gemv_bf16w, Wt, x, b, y, K=12)             # K % 8 != 0
    refused(H.gemv_bf16w, Wt, x, b, y, N=0, K=16)


@pytest.mark.parametrize("N,K", [(1536, 256), (1536, 1536), (6 * 1536, 1536), (5120, 256), (5120, 5120), (6 * 5120, 5120),
                                 (1, 8), (3, 4), (5, 260), (7, 1028)])
def test_gemv_f32(N, K):
    """the Wan time-embedding MLPs (256 -> d, d -> d, d -> 6 d for the 1.3B and 14B widths), small ragged N, both
    activations on either side"""
    combos = [(ai, ao, 0, wb) for ai in (0, 1) for ao in (0, 1) for wb in (1, 0)]
    gemv_check("f32", N, K, combos, seed=N % 97 + K % 89, key="gemv_f32/err_over_bound")
    refused(H.gemv_f32, rnd(4, 8), rnd(8), None, rnd(4), K=6)


# ----------------------------------------------------------------------------- head_linear
def head_linear_case(M, N, K, with_bias, seed):
    ldx, ldo = K + 8, N + 5
    xbuf = rnd(M, ldx, seed=seed, scale=1.5) + 0.2
    x = xbuf[:, :K]
    Wt = rnd(N, K, seed=seed + 1, scale=1.0 / math.sqrt(K))
    Wt[:, -1] += 0.5
    b = (rnd(N, seed=seed + 2) + torch.arange(N, device=DEV) * 0.01) if with_bias else None    # every column its own bias
    obuf = rnd(M + 1, ldo, seed=seed + 3) + 9.0
    o0 = obuf.clone()
    H.head_linear(xbuf, Wt, b, obuf, M, N, K)
    want = x.double() @ Wt.double().t() + (b.double() if with_bias else 0.0)
    sabs = x.double().abs() @ Wt.double().abs().t() + (b.double().abs() if with_bias else 0.0)
    # one fma chain over K per output, then the bias: fp32 summation noise of order sqrt(K) eps sum|terms|.  The constant is
    # 4 x the measured maximum of err / (sqrt(K) eps sum|terms|) over all cases of this file (HEAD_LINEAR_C), capped by the
    # worst case of a chain of depth K + 1
    probe("head_linear/err_over_sqrtK_eps_sabs", float(((obuf[:M, :N].double() - want).abs() / (math.sqrt(K) * EPS32 * sabs)).max()))
    within(obuf[:M, :N], want, min(K + 1, HEAD_LINEAR_C * math.sqrt(K)) * EPS32 * sabs + 1e-30, "head_linear/err_over_bound")
    assert torch.equal(obuf[:M, N:], o0[:M, N:]) and torch.equal(obuf[M], o0[M])         # guard columns, guard row


@pytest.mark.parametrize("K", [32, 1536, 3072])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("N", [4, 64, 65, 192, 256])
def test_head_linear(N, M, K):
    """64 x 64 blocks, column blocks for N > 64 (Wan2.2 TI2V: N = 192), ragged M and N, ldx > K, ldo > N (the MM-DiT
    engine stores 64-wide rows of fewer features)"""
    head_linear_case(M, N, K, True, seed=N + M + K)


def test_head_linear_null_bias_in_column_blocks():
    """a null bias must read as zero in EVERY column block (the kernel used to offset the pointer before testing it)"""
    head_linear_case(65, 192, 1536, False, seed=5)
    head_linear_case(1000, 256, 32, False, seed=6)


def test_head_linear_refusals():
    x, Wt, o = rnd(4, 64), rnd(4, 64), rnd(4, 300)
    refused(H.head_linear, x, Wt, None, o, 4, 257, 64)
    refused(H.head_linear, x, Wt, None, o, 4, 0, 64)
    refused(H.head_linear, x, Wt, None, o, 4, 4, 48)


# ----------------------------------------------------------------------------- ln_modulate
def ln_ref(x, sc, sh, mode, eps, sel=None, sc2=None, sh2=None):
    """fp64 LayerNorm + modulate; -> (y, amp) with amp = the magnitude the fp32 rounding errors scale with"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    n = (x - mean) * rstd
    a, b = sc.double().expand_as(x), sh.double().expand_as(x)
    if sel is not None:
        pick = sel.bool()[:, None]
        a, b = torch.where(pick, sc2.double().expand_as(x), a), torch.where(pick, sh2.double().expand_as(x), b)
    if mode == 0:
        a = 1.0 + a
    amp = (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd * a.abs() + b.abs()
    return n * a + b, amp


def ln_tol_f32(D, amp):
    # mean and variance: a lane's chain over its 4 D / 256 elements, then 6 wave-sum steps -- each of the two sums within
    # (D / 64 + 6) eps of exact relative to sum|terms|; the error of the mean reaches n as at most mean|x| rstd, the
    # variance's as half of its own times |n| <= (|x| + mean|x|) rstd (together `amp`); rsqrtf, the subtraction, two multiplies and the add: 6 eps more
    return 2.0 * (D / 64 + 6 + 6) * EPS32 * amp + 1e-30


@pytest.mark.parametrize("D", [256 * nv for nv in (1, 2, 4, 5, 6, 8, 12, 16, 20)])
def test_ln_modulate_every_width_modes_and_per_token_selection(D):
    """every instantiation of the NV switch x (modulate, affine) x (bf16, fp32 rows out) x (plain, fused x0) x (no sel, sel
    with both values inside every group of 4 rows -- one block --, sel all zero), M not a multiple of 4"""
    M, eps = 37, 1e-6
    x = rnd(M, D, seed=D, scale=3.0) + 0.5
    x0 = rnd(M, D, seed=D + 1, dtype=torch.bfloat16)
    sc, sh = rnd(D, seed=2, scale=0.3), rnd(D, seed=3)
    sc2, sh2 = rnd(D, seed=4, scale=0.3) - 0.2, rnd(D, seed=5) + 0.7
    sel = ((torch.arange(M, device=DEV) % 4 == 1) | (torch.arange(M, device=DEV) % 4 == 2)).to(torch.uint8)
    zero = torch.zeros(M, dtype=torch.uint8, device=DEV)
    ld = D + 8
    for mode in (0, 1):
        for fused in (False, True):
            xin = x.double() + (x0.double() if fused else 0.0)
            for s in (None, sel, zero):
                want, amp = ln_ref(xin, sc, sh, mode, eps, s, sc2, sh2)
                kw = dict(x0=x0 if fused else None, sc2=sc2 if s is not None else None, sh2=sh2 if s is not None else None, sel=s)
                of = rnd(M + 1, ld, seed=7) + 3.0
                of0 = of.clone()
                H.ln_modulate_sel(x, sc, sh, mode, eps, out_f32=of, M=M, D=D, **kw)
                within(of[:M, :D], want, ln_tol_f32(D, amp), "ln_modulate/f32_err_over_bound")
                assert torch.equal(of[:M, D:], of0[:M, D:]) and torch.equal(of[M], of0[M])
                ob = (rnd(M + 1, ld, seed=8) + 3.0).bfloat16()
                ob0 = ob.clone()
                H.ln_modulate_sel(x, sc, sh, mode, eps, out_bf16=ob, M=M, D=D, **kw)
                # one bf16 rounding of the fp32 value: u |value| on top of the fp32 bound
                within(ob[:M, :D], want, U16 * (want.abs() + ln_tol_f32(D, amp)) + ln_tol_f32(D, amp), "ln_modulate/bf16_err_over_bound")
                assert torch.equal(bits(ob[:M, D:]), bits(ob0[:M, D:])) and torch.equal(bits(ob[M]), bits(ob0[M]))
                # the bf16 row is the rounding of the fp32 row the same kernel makes
                assert torch.equal(bits(ob[:M, :D]), bits(of[:M, :D].bfloat16()))
                if s is zero:                       # sel given but all zero == no sel, bit for bit
                    of2 = torch.zeros(M, D, device=DEV)
                    H.ln_modulate_sel(x, sc, sh, mode, eps, out_f32=of2, x0=kw["x0"])
                    assert torch.equal(of2, of[:M, :D])
                if s is None and not fused:         # and the shipped single-op entry point gives the same bits
                    of3 = torch.zeros(M, D, device=DEV)
                    H.ln_modulate(x, sc, sh, mode, eps, out_f32=of3)
                    assert torch.equal(of3, of[:M, :D])


def test_ln_modulate_refusals():
    x, sc, sh = rnd(8, 1024), rnd(1024), rnd(1024)
    out = torch.zeros(8, 1024, device=DEV)
    sel = torch.zeros(8, dtype=torch.uint8, device=DEV)
    refused(H.ln_modulate_sel, x, sc, sh, 0, 1e-6, out_f32=out, D=768)        # D / 256 = 3 has no instantiation
    refused(H.ln_modulate_sel, x, sc, sh, 0, 1e-6, out_f32=out, D=100)
    refused(H.ln_modulate_sel, x, sc, sh, 0, 1e-6)                            # neither output
    refused(H.ln_modulate_sel, x, sc, sh, 0, 1e-6, out_f32=out, sel=sel)      # sel without sc2 / sh2
    refused(H.ln_modulate_sel, x, sc, sh, 0, 1e-6, out_f32=out, M=0)
    with pytest.raises(_lib.MagCacheHipError):                                # the shipped entry point refuses it too
        H.ln_modulate(x, sc, sh, 0, 1e-6)
    assert float(out.abs().max()) == 0.0


# ----------------------------------------------------------------------------- ln_modulate_fp8
def pow2_amax_hits_half_branch(amax):
    """CPU, the arithmetic of mx_quantize_ref: does frexp(amax * fl32(1 / 448)) give the mantissa 0.5 exactly?"""
    f, _ = torch.frexp(torch.tensor(amax, dtype=torch.float32) * torch.tensor(1.0 / 448.0, dtype=torch.float32))
    return float(f) == 0.5


@pytest.mark.parametrize("sel_kind", ["none", "random", "zero_rows"])
@pytest.mark.parametrize("mx", [False, True], ids=["row_scale", "mx"])
@pytest.mark.parametrize("M", [1, 333, 1024 + 7])
@pytest.mark.parametrize("D", [1536, 3072, 5120])
def test_ln_modulate_fp8_equals_quantising_the_bf16_row(D, M, mx, sel_kind):
    """ops.h: "bit-identical to quantising the bf16 row launch_ln_modulate writes".  The e4m3 bytes and the scales of the fused
    kernel against quantize_rows_fp8 / quantize_rows_mx of that row -- both sides run the same device arithmetic, so equality
    has no tie cases to excuse.  Rows that are zero after modulation (1 + sc2 = 0, sh2 = 0: the amax == 0 branches, whole-row
    and per-block) and a 32-block whose amax is 3.5 = 2^-7 * 448 (the f == 0.5 branch of the E8M0 exponent) are part of it."""
    eps = 1e-6
    x = rnd(M, D, seed=D + M, scale=3.0) + 0.5
    sc, sh = rnd(D, seed=2, scale=0.3), rnd(D, seed=3)
    sc[64:96] = -1.0                                   # block 2 of every row: the values of sh alone, amax exactly 3.5
    sh[64:96] = torch.linspace(-1.0, 1.0, 32, device=DEV)
    sh[70] = -3.5
    sc[128:160], sh[128:160] = -1.0, 0.0               # block 4: all zero in every row (MX: amax == 0 for one block)
    assert pow2_amax_hits_half_branch(3.5) and not pow2_amax_hits_half_branch(3.0)
    sel = sc2 = sh2 = None
    if sel_kind != "none":
        sel = (torch.arange(M, device=DEV) % 3 == 0).to(torch.uint8)
        sc2 = rnd(D, seed=4, scale=0.3) - 0.2 if sel_kind == "random" else torch.full((D,), -1.0, device=DEV)
        sh2 = rnd(D, seed=5) + 0.7 if sel_kind == "random" else torch.zeros(D, device=DEV)
    for mode in (0, 1):
        a, a2 = (sc, sc2) if mode == 0 else (1.0 + sc, None if sc2 is None else 1.0 + sc2)       # the same rows in both modes
        row = (rnd(M, D, seed=9) + 2.0).bfloat16()
        H.ln_modulate_sel(x, a, sh, mode, eps, out_bf16=row, sc2=a2, sh2=sh2, sel=sel)
        q, s = H.ln_modulate_fp8(x, a, sh, mode, eps, mx, sc2=a2, sh2=sh2, sel=sel)
        if mx:
            q2, s2 = H.quantize_rows_mx(row)
            sn, s2n = H.mx_unpermute(s, M), H.mx_unpermute(s2, M)
            assert torch.equal(sn, s2n)
            assert torch.equal(s, s2)                  # and the bytes no row owns still hold the 127 they were filled with
            if M > 1:                                  # row 1 is never selected: its block 2 has amax 3.5, its block 4 is zero
                assert int(sn[1, 2]) == 127 - 7 and int(sn[1, 4]) == 0
            scale = torch.exp2(sn.double() - 127.0).repeat_interleave(32, dim=1)
            qr, sr = H.mx_quantize_ref(row)              # the torch restatement agrees as well
            assert torch.equal(sr, sn) and torch.equal(q.view(torch.float8_e4m3fn).float(), qr.float())
        else:
            q2, s2 = H.quantize_rows_fp8(row)
            assert torch.equal(bits(s), bits(s2))
            scale = s.double()[:, None].expand(M, D)
        assert torch.equal(q, q2)
        if sel_kind == "zero_rows":
            assert float(row[0].float().abs().max()) == 0.0 and int(q[0].max()) == 0
            assert (int(s[0, 0]) == 0) if mx else (float(s[0]) == 1.0)
        # and what the bytes mean: the fp64 LayerNorm at e4m3 precision.  e4m3 keeps 3 mantissa bits (half an ulp = 2^-4
        # of the value) down to 2^-6 of the scale and steps of 2^-9 below (half a step = 2^-10 of the scale); the bf16
        # rounding ahead of it (u) and the fp32 LayerNorm (ln_tol_f32) come on top
        want, amp = ln_ref(x.double(), a, sh, mode, eps, sel, a2, sh2)
        deq = q.view(torch.float8_e4m3fn).double() * scale
        t0 = U16 * want.abs() + 2 * ln_tol_f32(D, amp)
        within(deq, want, torch.maximum(2.0 ** -4 * (want.abs() + t0), 2.0 ** -10 * scale) + t0, "ln_modulate_fp8/dequant_err_over_bound")


def test_ln_modulate_fp8_refusals():
    x, sc, sh = rnd(8, 1024), rnd(1024), rnd(1024)
    q = torch.zeros(8, 1024, dtype=torch.uint8, device=DEV)
    s = torch.zeros(8, device=DEV)
    args = (H.P(x), 1024, H.P(sc), H.P(sh), 0, 1e-6)
    refused(H.T, "ln_modulate_fp8", *args, None, 1024, H.P(s), None, 0, 8, 1024, None, None, None, H.S())          # no q
    refused(H.T, "ln_modulate_fp8", *args, H.P(q), 1024, None, None, 0, 8, 1024, None, None, None, H.S())          # no scales
    refused(H.T, "ln_modulate_fp8", *args, H.P(q), 1024, None, H.P(q), 32, 8, 1024, None, None, None, H.S())       # mx_rows % 64
    refused(H.T, "ln_modulate_fp8", *args, H.P(q), 1024, H.P(s), None, 0, 8, 768, None, None, None, H.S())         # D / 256 = 3


# ----------------------------------------------------------------------------- quantize_rows_fp8 / quantize_rows_mx
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("K", [32, 544])
@pytest.mark.parametrize("M", [1, 67])
def test_quantize_rows_equal_their_torch_restatements(M, K, dtype):
    """The two stand-alone quantisers (csrc/quant.h is their arithmetic) against hip_ops.fp8_rows_quantize_ref /
    mx_quantize_ref, bytes and scales bit for bit, on bf16 and on fp32 rows.  Special 32-blocks (values within [-1, 1] beside
    the one that sets amax): an all-zero row, an all-zero block, amax 3.5 = 2^-7 * 448 and amax 3584 = 2^3 * 448 -- both give
    frexp the mantissa 0.5 exactly, the branch that takes one off the exponent: E8M0 bytes 127 - 7 and 127 + 3.  M = 1 has one
    row, so there the blocks of that row carry the cases (K = 32: one block, amax 3.5) and the all-zero row is M = 67's."""
    nb = K // 32
    x = rnd(M, K, seed=M + K, scale=2.0).view(M, nb, 32)
    special = {}                                        # (row, block) -> amax
    if M == 1:
        special = {(0, 0): 3.5} if nb == 1 else {(0, 0): 0.0, (0, 1): 3.5, (0, nb - 1): 3584.0}
    else:
        x[0] = 0.0                                      # the all-zero row
        special = {(1, 0): 0.0, (2, nb - 1): 3.5, (3, 0): 3584.0, (64, nb // 2): 3.5, (66, nb - 1): 0.0}
    for (r, b), amax in special.items():
        x[r, b] = x[r, b].clamp(-1.0, 1.0) if amax else 0.0
        if amax:
            x[r, b, 5] = -amax
    x = x.view(M, K).to(dtype).contiguous()
    assert pow2_amax_hits_half_branch(3.5) and pow2_amax_hits_half_branch(3584.0)

    q, s = H.quantize_rows_fp8(x)
    qr, sr = H.fp8_rows_quantize_ref(x)
    assert torch.equal(bits(s), bits(sr))
    assert torch.equal(q, qr.view(torch.uint8))
    if M > 1:
        assert float(s[0]) == 1.0 and int(q[0].max()) == 0

    q, s = H.quantize_rows_mx(x)
    qr, sr = H.mx_quantize_ref(x)
    want = torch.full_like(s, 127)                      # the bytes no row owns keep what they were filled with
    want[:, H.mx_perm(torch.arange(M, device=DEV))] = sr.t()
    assert torch.equal(s, want)
    assert torch.equal(q, qr.view(torch.uint8))
    for (r, b), amax in special.items():
        assert int(sr[r, b]) == {0.0: 0, 3.5: 127 - 7, 3584.0: 127 + 3}[amax]
    if M > 1:
        assert int(sr[0].max()) == 0 and int(q[0].max()) == 0


# ----------------------------------------------------------------------------- EPI_GELU_MXFP8
@pytest.mark.parametrize("M,N,K", [(256, 256, 512), (1024, 8960 - 8960 % 256, 1536), (32768, 8960 - 8960 % 256, 1536)])
def test_gemm_mxfp8_gelu_quant_epilogue_equals_quantising_the_gelu_output(M, N, K):
    """ops.h: Cq / c_mx are "the bits launch_quantize_rows_mx would make of Cb" -- of the bf16 GELU output epilogue 1 of the
    same kernel writes.  What the fp8 engine runs for FFN-1 with fused quantisation; no shipped single-op call reaches it.
    At M = 32768 the rows of H.v2_sample_rows are named in the assertion, and the whole output is compared as well."""
    a = rnd(M, K, seed=31, dtype=torch.bfloat16)
    a[:, 40:72] *= 16.0
    w = rnd(N, K, seed=32, scale=0.05, dtype=torch.bfloat16)
    w[5] = 0                                            # an output column that is bias alone
    bias = rnd(N, seed=33)
    bias[96:128] = -100.0                               # a whole 32-column block of GELU(very negative) = -0.0: amax == 0
    aq, sa = H.quantize_rows_mx(a)
    wq, sw = H.quantize_rows_mx(w)
    cb = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    H.gemm_mxfp8(aq, sa, wq, sw, bias, 1, Cb=cb)
    q2, s2 = H.quantize_rows_mx(cb)
    cq, cs = H.gemm_mxfp8_gelu_quant(aq, sa, wq, sw, bias)
    rows = H.v2_sample_rows(M, DEV) if M == 32768 else torch.arange(M, device=DEV)
    assert torch.equal(H.mx_unpermute(cs, M)[rows], H.mx_unpermute(s2, M)[rows])
    assert torch.equal(cq[rows], q2[rows])
    assert torch.equal(cs, s2) and torch.equal(cq, q2)
    assert int(H.mx_unpermute(cs, M)[:, 3].max()) == 0 and float(cb[:, 96:128].float().abs().max()) == 0.0
    # as the A operand of the next MX GEMM (FFN-2): the same bits out.  N is that GEMM's K, and the MX kernel takes K >= 512
    # only (gemm_mxfp8_supported): the N = 256 shape has no second GEMM to run
    if N >= 512:
        N2 = 256
        w2q, s2w = H.quantize_rows_mx(rnd(N2, N, seed=34, scale=0.05, dtype=torch.bfloat16))
        o1 = torch.zeros(M, N2, device=DEV)
        o2 = torch.ones(M, N2, device=DEV)
        H.gemm_mxfp8(cq, cs, w2q, s2w, None, 5, X=o1)
        H.gemm_mxfp8(q2, s2, w2q, s2w, None, 5, X=o2)
        assert torch.equal(o1, o2) and float(o1.abs().max()) > 0


# ----------------------------------------------------------------------------- token_t_prepare
@pytest.mark.parametrize("pattern", ["all_equal", "two_values", "two_plus_others"])
@pytest.mark.parametrize("n_all", [1, 1023, 1024, 1025, 32760, 200000])
def test_token_t_prepare(n_all, pattern):
    """one 1024-thread block: max / min of ALL tokens, the number that is neither, and the sel bytes of this rank's rows
    (row offset, zero padding)"""
    g = torch.Generator(device="cpu").manual_seed(n_all)
    t = torch.full((n_all,), 937.5)
    k = 0
    if pattern != "all_equal" and n_all > 1:
        t[torch.rand(n_all, generator=g) < 0.4] = 12.25
        t[n_all - 1] = 12.25                                # the minimum is there, whatever the draw; the maximum too
        t[0] = 937.5
        if pattern == "two_plus_others" and n_all > 2:
            k = min(n_all - 2, 5)
            idx = (torch.randperm(n_all - 2, generator=g)[:k] + 1)
            t[idx] = 500.0 + torch.arange(k, dtype=torch.float32)
    t = t.to(DEV)
    for row0, n_rows in {(0, n_all), (n_all // 3, n_all - n_all // 3), (n_all // 2, max(1, n_all // 4))}:
        pad = (n_rows + 255) // 256 * 256
        t2 = torch.full((5,), -7.0, device=DEV)
        sel = torch.full((pad + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        H.token_t_prepare(t, n_all, row0, n_rows, pad, t2, sel)
        mx_, mn = float(t.max()), float(t.min())
        assert t2.tolist() == [mx_, mn, float(k), -7.0, -7.0]
        want = ((t[row0:row0 + n_rows] == mn) & (mn != mx_)).to(torch.uint8)
        assert torch.equal(sel[:n_rows], want)
        assert int(sel[n_rows:pad].max() if pad > n_rows else 0) == 0           # the padding is zero ...
        assert bool((sel[pad:] == 0xA5).all())                                  # ... and nothing beyond it is written
        if pattern == "all_equal" or n_all == 1:
            assert int(sel[:pad].max()) == 0 and float(t2[2]) == 0.0


def test_token_t_prepare_refusals():
    t, t2 = rnd(64), torch.zeros(3, device=DEV)
    sel = torch.zeros(64, dtype=torch.uint8, device=DEV)
    refused(H.token_t_prepare, None, 64, 0, 64, 64, t2, sel)
    refused(H.token_t_prepare, t, 0, 0, 64, 64, t2, sel)
    refused(H.token_t_prepare, t, 64, -1, 8, 8, t2, sel)
    refused(H.token_t_prepare, t, 64, 0, 0, 0, t2, sel)
    refused(H.token_t_prepare, t, 64, 60, 8, 8, t2, sel)          # row0 + n_rows > n_all
    refused(H.token_t_prepare, t, 64, 0, 32, 16, t2, sel)         # n_rows_pad < n_rows
    assert int(sel.max()) == 0


# ----------------------------------------------------------------------------- patchify / unpatchify
def test_patchify_unpatchify():
    """patch (1, 2, 2) on an odd-sized grid (F, H/2, W/2) = (3, 5, 7): each op alone against the oracle's statement of it (the
    patch-embedding Conv3d's im2col order; WanModel.unpatchify's einsum) -- inverse errors would cancel in a round trip --, a
    token window (tok0 > 0, fewer tokens than remain), zero pad rows, and the round trip."""
    Cc, Fg, Hp, Wp = 16, 3, 5, 7
    Hh, Ww, L = 2 * Hp, 2 * Wp, Fg * Hp * Wp
    lat = rnd(Cc, Fg, Hh, Ww, seed=1, scale=2.0)
    # the oracle embeds with Conv3d(kernel = stride = (1, 2, 2)).flatten(2).transpose(1, 2): with the identity as weight that
    # IS the im2col matrix, columns in the weight's (c, pt, ph, pw) order
    eye = torch.eye(4 * Cc, dtype=torch.float64, device=DEV).view(4 * Cc, Cc, 1, 2, 2)
    cols = F.conv3d(lat.double()[None], eye, stride=(1, 2, 2)).flatten(2).transpose(1, 2)[0]         # [L, 4 C]
    ldo = 4 * Cc + 8
    for tok0, n_tok, n_rows in [(0, L, L), (0, L, L + 23), (11, 40, 64), (L - 1, 1, 4)]:
        out = (rnd(n_rows + 1, ldo, seed=2) + 3.0).bfloat16()
        o0 = out.clone()
        H.patchify(lat, tok0, n_tok, n_rows, out)
        assert torch.equal(bits(out[:n_tok, :4 * Cc]), bits(cols[tok0:tok0 + n_tok].float().bfloat16()))
        assert float(out[n_tok:n_rows, :4 * Cc].float().abs().max() if n_rows > n_tok else 0.0) == 0.0
        assert torch.equal(bits(out[:, 4 * Cc:]), bits(o0[:, 4 * Cc:])) and torch.equal(bits(out[n_rows]), bits(o0[n_rows]))
    # unpatchify: token vector (ph, pw, c), c fastest
    ldt = 4 * Cc + 3
    tok = rnd(L, ldt, seed=3, scale=2.0)
    stub = types.SimpleNamespace(out_dim=Cc, patch_size=(1, 2, 2))
    want = W.WanModel.unpatchify(stub, [tok[:, :4 * Cc]], torch.tensor([[Fg, Hp, Wp]]))[0]
    out = torch.full((Cc, Fg, Hh, Ww), -9.0, device=DEV)
    H.unpatchify(tok, 0, L, out)
    assert torch.equal(out, want)
    # a window of tokens: only their pixels change
    tok0, n_tok = 11, 40
    out = torch.full((Cc, Fg, Hh, Ww), -9.0, device=DEV)
    H.unpatchify(tok[tok0:], tok0, n_tok, out)
    mask = torch.zeros(L, dtype=torch.bool, device=DEV)
    mask[tok0:tok0 + n_tok] = True
    pix = mask.view(Fg, Hp, 1, Wp, 1).expand(Fg, Hp, 2, Wp, 2).reshape(Fg, Hh, Ww)[None].expand(Cc, -1, -1, -1)
    assert torch.equal(out, torch.where(pix, want, torch.full_like(want, -9.0)))
    # round trip: the bf16-rounded latent comes back exactly (tokens in the head's (ph, pw, c) order from im2col's (c, ph, pw))
    pt = torch.zeros(L, 4 * Cc, dtype=torch.bfloat16, device=DEV)
    H.patchify(lat, 0, L, L, pt)
    back = torch.zeros_like(lat)
    H.unpatchify(pt.float().view(L, Cc, 4).transpose(1, 2).reshape(L, 4 * Cc).contiguous(), 0, L, back)
    assert torch.equal(back, lat.bfloat16().float())
    # refusals: odd H or W, fewer rows than tokens
    refused(H.patchify, lat, 0, 4, 4, pt, dims=(Cc, Fg, Hh - 1, Ww))
    refused(H.patchify, lat, 0, 4, 4, pt, dims=(Cc, Fg, Hh, Ww - 1))
    refused(H.patchify, lat, 0, 8, 4, pt)
    refused(H.unpatchify, tok, 0, 4, back, dims=(Cc, Fg, Hh - 1, Ww))
    refused(H.unpatchify, tok, 0, 4, back, dims=(Cc, Fg, Hh, Ww - 1))


# ----------------------------------------------------------------------------- attn_merge
@pytest.mark.parametrize("n", [1, 2, 9])
def test_attn_merge(n):
    """the log-sum-exp weighted mean of n partial results: fp64 on the bf16 partials, then one bf16 rounding.  One partial
    with an empty key set (lse = -inf, finite garbage in O) contributes nothing; weights 2^60 apart; rows < rows_pad."""
    rows, rows_pad, heads = 100, 128, 2
    d, ldo = heads * 128, heads * 128 + 8
    parts = [rnd(rows, ldo, seed=10 + i, scale=1.0 + i, dtype=torch.bfloat16) for i in range(n)]
    lses = [rnd(heads, rows_pad, seed=30 + i, scale=3.0) + i for i in range(n)]
    if n >= 2:
        lses[0][0, :50] += 60.0                         # partial 0 outweighs the others by 2^60 in half of head 0's rows
        lses[1][1, 10:90] -= 60.0
        empty = n - 1                                   # the last partial saw no key at all in some rows, in both heads
        lses[empty][:, 20:70] = float("-inf")
        parts[empty][20:70] = 1e30
        lses[empty][:, rows:] = float("nan")            # the lse padding is never read
    out = (rnd(rows + 1, ldo, seed=50) + 4.0).bfloat16()
    o0 = out.clone()
    H.attn_merge_raw(parts, lses, out, rows, rows_pad, d)
    lse = torch.stack([t[:, :rows].double() for t in lses])                                  # [n, heads, rows]
    wt = torch.exp2(lse - lse.max(0).values)
    wt = (wt / wt.sum(0)).permute(0, 2, 1)[..., None]                                        # [n, rows, heads, 1]
    o = torch.stack([p[:, :d].double().view(rows, heads, 128) for p in parts])
    o = torch.where(wt == 0, torch.zeros_like(o), o)
    want = (o * wt).sum(0).reshape(rows, d)
    mag = (o.abs() * wt).sum(0).reshape(rows, d)
    # fp32: exp2 (1 ulp), n products and n additions into the numerator, n into the denominator, the reciprocal and the
    # final multiply: <= (2 n + 6) eps of sum w|o| / sum w; then one bf16 rounding
    within(out[:rows, :d], want, U16 * want.abs() + (2 * n + 6) * EPS32 * mag * (1 + U16) + 1e-30, "attn_merge/err_over_bound")
    assert torch.equal(bits(out[:rows, d:]), bits(o0[:rows, d:])) and torch.equal(bits(out[rows]), bits(o0[rows]))
    if n == 1:
        assert torch.equal(bits(out[:rows, :d]), bits(parts[0][:, :d]))     # weight 1 exactly
    refused(H.attn_merge_raw, parts, lses, out, rows_pad + 1, rows_pad, d)
    refused(H.attn_merge_raw, parts, lses, out, rows, rows_pad, d + 64)


# ----------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4099])
def test_cast_bf16(n):
    src = rnd(n + 4, seed=n, scale=3.0)
    dst = torch.full((n + 4,), 5.0, dtype=torch.bfloat16, device=DEV)
    H.cast_bf16(src, dst, n)
    assert torch.equal(bits(dst[:n]), bits(src[:n].bfloat16())) and bool((dst[n:] == 5.0).all())
    dst2 = torch.full((n + 4,), 5.0, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.load().mc_op_cast_bf16(H.P(src), H.P(dst2), n, H.S()))          # the shipped entry point: the same bits
    assert torch.equal(bits(dst2), bits(dst))


@pytest.mark.parametrize("rows_valid", [0, 5, 13])
def test_cast_pad_bf16(rows_valid):
    rows, cols = 13, 20
    src = rnd(rows, cols + 4, seed=1, scale=3.0)
    dst = torch.full((rows + 1, cols + 12), 5.0, dtype=torch.bfloat16, device=DEV)
    H.cast_pad_bf16(src, rows_valid, rows, cols, dst)
    assert torch.equal(bits(dst[:rows_valid, :cols]), bits(src[:rows_valid, :cols].bfloat16()))
    assert float(dst[rows_valid:rows, :cols].float().abs().max() if rows_valid < rows else 0.0) == 0.0
    assert bool((dst[:, cols:] == 5.0).all()) and bool((dst[rows] == 5.0).all())
    refused(H.cast_pad_bf16, src, rows_valid, rows, 18, dst)


def test_add_bf16_and_add_bcast():
    n = 8 * 1031
    a = rnd(n + 8, seed=1, scale=2.0, dtype=torch.bfloat16)
    b = rnd(n + 8, seed=2, scale=0.3, dtype=torch.bfloat16)
    a0 = a.clone()
    H.add_bf16(a, b, n)
    assert torch.equal(bits(a[:n]), bits((a0[:n].float() + b[:n].float()).bfloat16()))       # one fp32 add, one rounding
    assert torch.equal(bits(a[n:]), bits(a0[n:]))
    refused(H.add_bf16, a, b, n + 4)
    na, m = 6 * 256, 3 * 6 * 256 + 100
    va, vb = rnd(na, seed=3), rnd(m + 4, seed=4)
    out = torch.full((m + 4,), 5.0, device=DEV)
    H.add_bcast(va, vb, out, m)
    assert torch.equal(out[:m], va.repeat(4)[:m] + vb[:m]) and bool((out[m:] == 5.0).all())


@pytest.mark.parametrize("dim", [256, 1536, 6])
@pytest.mark.parametrize("t", [0.0, 1.0, 999.0, 487.3125])
def test_sinusoid(dim, t):
    """fp64 inside, one rounding to fp32 at the store: against the oracle's float64 embedding within 1 fp32 ulp (the device's
    pow / cos / sin are not correctly rounded in the last place, and at t = 999 an ulp of the fp64 argument is 1e-13)"""
    want = W.sinusoidal_embedding_1d(dim, torch.tensor([t], dtype=torch.float64))[0].to(DEV)
    tol = 2.0 ** -23 * want.abs() + 1e-12
    out = torch.full((dim + 2,), 5.0, device=DEV)
    H.sinusoid(None, t, dim, out)
    within(out[:dim], want, tol, "sinusoid/err_over_ulp")
    out2 = torch.full((dim + 2,), 5.0, device=DEV)
    H.sinusoid(torch.tensor([t], dtype=torch.float32, device=DEV), -1.0, dim, out2)      # the device value wins
    assert torch.equal(out2, out) and bool((out[dim:] == 5.0).all())


@pytest.mark.parametrize("n_rows,D", [(1, 256), (77, 4096), (300, 100)])
def test_colmean(n_rows, D):
    x = rnd(n_rows + 3, D + 4, seed=D, scale=2.0) + 1.0
    out = torch.full((D + 4,), 5.0, device=DEV)
    H.colmean(x, n_rows, D, out)
    want = x[:n_rows, :D].double().mean(0)
    # one chain of n_rows additions, then the division: sqrt(n_rows) eps sum|terms| x the measured constant (COLMEAN_C),
    # capped by the worst case of a chain of depth n_rows + 1
    sabs = x[:n_rows, :D].double().abs().mean(0)
    probe("colmean/err_over_sqrtN_eps_sabs", float(((out[:D].double() - want).abs() / (math.sqrt(n_rows) * EPS32 * sabs)).max()))
    within(out[:D], want, min(n_rows + 1, COLMEAN_C * math.sqrt(n_rows)) * EPS32 * sabs + 1e-30, "colmean/err_over_bound")
    assert bool((out[D:] == 5.0).all())
    refused(H.colmean, x, 0, D, out)


def test_rope_table_from_cos_sin():
    n, ld = 37, 128 + 4
    cosv, sinv = rnd(n + 1, ld, seed=1), rnd(n + 1, ld, seed=2)
    cs = torch.full((n + 1, 128), 5.0, device=DEV)
    H.rope_table_from_cos_sin(cosv, sinv, n, cs)
    want = torch.stack([cosv[:n, 0:128:2], sinv[:n, 0:128:2]], dim=-1).reshape(n, 128)
    assert torch.equal(cs[:n], want) and bool((cs[n] == 5.0).all())
    refused(H.rope_table_from_cos_sin, cosv, sinv, 0, cs)


@pytest.mark.parametrize("with_eps", [True, False])
def test_cfg_euler(with_eps):
    n, g, dt = 16 * 21 * 30 * 52 + 3, 5.0, -0.0375
    c, u, x0 = rnd(n, seed=1), rnd(n, seed=2, scale=1.5), rnd(n + 2, seed=3, scale=2.0)
    x = x0.clone()
    eps_out = torch.full((n + 2,), 5.0, device=DEV) if with_eps else None
    H.cfg_euler(c, u, g, dt, x, eps_out, n)
    want_x, want_e = MR.cfg_euler_step(x0[:n].double(), c.double(), u.double(), g, dt)
    # eps = u + g (c - u): the subtraction, the product, the sum (or one fma) -- each within eps of its own result
    e_tol = EPS32 * (g * (c.double() - u.double()).abs() * 2 + want_e.abs()) + 1e-30
    if with_eps:
        within(eps_out[:n], want_e, e_tol, "cfg_euler/eps_err_over_bound")
        assert bool((eps_out[n:] == 5.0).all())
    within(x[:n], want_x, abs(dt) * e_tol + EPS32 * (abs(dt) * want_e.abs() + want_x.abs()) + 1e-30, "cfg_euler/x_err_over_bound")
    assert torch.equal(x[n:], x0[n:])

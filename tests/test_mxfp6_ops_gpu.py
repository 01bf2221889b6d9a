"""GPU: mc_op_quantize_rows_mxfp6 and mc_op_gemm_mxfp6 (csrc/gemm_mxfp6.hip, quant.h) against tests/mxfp6_ref.py.

  * quantiser: packed bytes and scale bytes equal the reference bit for bit -- fp32 and bf16 inputs, strided ldx / ldq with
    guard bands that stay poison, rows with every exact tie, amax = 7.5 2^n and its neighbours, powers of two, zero blocks and
    blocks of denormal-small values, M around 16 and 256;
  * GEMM, exact: random e2m3 codes with per-block scale exponents whose total spread (A plus W) is <= 2 and K <= 1024.  Every
    product is a multiple of 2^-6 2^smin and the sum of the magnitudes stays below 2^24 of those units (K 3600 2^spread =
    14.7 M), so fp32 accumulation is exact in any order: the result must torch.equal the float64 product.  No tolerance;
  * one-hot sweeps: row m of A (row n of W) is nonzero at the single k = (m + shift) % K against a dense other operand, so
    every (row mod 256, k, scale block) placement of either operand is checked;
  * epilogues: e2m3 values are e4m3 values, so the same exact operands re-encoded for mc_op_gemm_mxfp8 must give bit-identical
    outputs for every shared epilogue (bf16, GELU, gated residual, residual capture, fp32);
  * row guard (the contract of tests/test_mx_gemm_rows_gpu.py): A holds exactly M rows, the scale bytes of rows >= M are NaN
    (0xFF), outputs behind row M keep their bits, rows < M equal the ceil256(M) launch;
  * refusals: MC_EINVAL and nothing written;
  * random data: relative L2 against float64 of the dequantised operands below 1e-4, the bar tests/test_mxfp4_ops_gpu.py
    uses for the same check (fp32 accumulation of products that are exact in fp32: the distance is accumulation rounding)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import mxfp6_ref as R  # noqa: E402

DEV = "cuda:0"
GUARD = 64
EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE, EPI_F32, EPI_GELU_MXFP8, EPI_GELU_MXFP4 = 0, 1, 2, 3, 5, 8, 13
MIN_N, MIN_K = 256, 512          # the smallest N and K mc_op_gemm_mxfp6 accepts


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------------------------------- quantiser
def special_rows(M, K, dtype, seed):
    """rows whose 32-element blocks cycle through: the 31 exact ties under amax = 7.5 (both signs in turn), near-ties and
    the block maximum's neighbours, powers of two, a zero block, denormal-small values (the exponent clamp), random data"""
    g = gen(seed)
    nb = K // 32
    x = torch.randn(M, nb, 32, generator=g, device=DEV) * torch.exp2(torch.randint(-12, 12, (M, nb, 1), generator=g, device=DEV).float())
    idx = torch.arange(M, device=DEV)[:, None] + torch.arange(nb, device=DEV)[None, :]
    kind = idx % 8
    ties = torch.tensor([7.5] + [t for t, _ in R.TIES], device=DEV)
    ties_neg = ties * torch.where(torch.arange(32, device=DEV) % 2 == 0, 1.0, -1.0)
    near = torch.tensor([7.5, 0.0625001, 0.0624999, 0.9375001, 0.9374999, 1.9375, 1.9374999, 1.9375001, 2.125, 2.1249998, 3.875,
                         3.8750002, 3.8749998, 4.25, 4.2500005, 7.25, 7.2499995, 7.2500005, 0.0, -0.0, 0.03125, -0.03125, 1.0,
                         2.0, 4.0, -7.5, -0.0625, 0.1875, -0.1875, 0.5625, 6.75, -6.25], device=DEV)
    top = torch.tensor([7.5, 7.4999995, 7.0, 3.0] * 8, device=DEV)                 # amax exactly 7.5 2^n
    top_above = torch.tensor([7.5000005, 7.5, 7.0, 3.0] * 8, device=DEV)           # one fp32 ulp more: the exponent steps up
    pow2 = torch.exp2(torch.arange(32, device=DEV).float() - 20.0) * torch.where(torch.arange(32, device=DEV) % 3 == 0, -1.0, 1.0)
    den = torch.tensor([2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -129, 2.0 ** -126, 2.0 ** -133, -(2.0 ** -128), 3 * 2.0 ** -129,
                        2.0 ** -130] * 4, device=DEV)
    shift = torch.exp2((idx % 9 - 4).float())[..., None]
    x = torch.where((kind == 0)[..., None], ties_neg * shift, x)
    x = torch.where((kind == 1)[..., None], pow2 * shift, x)
    x = torch.where((kind == 2)[..., None], torch.zeros_like(x), x)
    x = torch.where((kind == 3)[..., None], den.expand_as(x), x)
    x = torch.where((kind == 4)[..., None], den.expand_as(x) * 2.0 ** -7, x)       # everything rounds to +-0: e = -127
    x = torch.where((kind == 5)[..., None], near * shift, x)
    x = torch.where((kind == 6)[..., None], torch.where((idx % 16 < 8)[..., None], top, top_above) * shift, x)
    return x.view(M, K).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [32, 2080])        # the smallest K; 65 blocks: no power of two, and a lane's second block
@pytest.mark.parametrize("M", [1, 15, 16, 17, 255, 256, 257])
def test_quantiser_bits_equal_the_reference(M, K, dtype):
    x_rows = special_rows(M, K, dtype, seed=M * 7 + K)
    kb = K // 4 * 3
    ldx, ldq = K + 24, (kb + 15) // 16 * 16 + 16                     # strided source and destination
    xbuf = torch.full((M, ldx), 3.0, dtype=dtype, device=DEV)
    xbuf[:, :K] = x_rows
    qbuf = torch.full((M + 1, ldq), 0x5A, dtype=torch.uint8, device=DEV)
    rows_pad = R.ceil256(M)
    s = torch.full((K // 32, rows_pad), 0xEE, dtype=torch.uint8, device=DEV)
    R.op_quantize(xbuf, q=qbuf, s=s, rows_pad=rows_pad, M=M, K=K)
    codes, e = R.quantize(xbuf[:, :K])
    assert torch.equal(qbuf[:M, :kb], R.pack(codes)), "packed codes differ from the reference"
    assert bool((qbuf[:M, kb:] == 0x5A).all()) and bool((qbuf[M] == 0x5A).all()), "bytes outside [M, 3 K / 4] were written"
    assert torch.equal(s, R.scale_image(e, rows_pad, fill=0xEE)), "scale bytes differ (or bytes of rows >= M were written)"


# ---------------------------------------------------------------------------------------------------- GEMM, exact
_exact = {}


def exact_operands(M, N, K, seed=0):
    """random codes, block exponents with spread 1 (A) + 1 (W); (codes, e, packed, scale image) per operand and the float64
    product, once per shape"""
    key = (M, N, K, seed)
    if key not in _exact:
        g = gen(1000 * seed + M + 3 * N + 5 * K)
        ac = torch.randint(0, 64, (M, K), generator=g, device=DEV).to(torch.uint8)
        wc = torch.randint(0, 64, (N, K), generator=g, device=DEV).to(torch.uint8)
        ae = torch.randint(-2, 0, (M, K // 32), generator=g, device=DEV)          # -2 .. -1
        we = torch.randint(1, 3, (N, K // 32), generator=g, device=DEV)           # 1 .. 2
        ref = R.dequantize(ac, ae) @ R.dequantize(wc, we).t()
        _exact[key] = dict(ac=ac, ae=ae, aq=R.pack(ac), sa=R.scale_image(ae, R.ceil256(M)),
                           wc=wc, we=we, wq=R.pack(wc), sw=R.scale_image(we, N), ref=ref)
    return _exact[key]


@pytest.mark.parametrize("K", [MIN_K, 768, 1024])      # 4, 6 and 8 K tiles of 128 (K % 256 == 0: the count is always even)
@pytest.mark.parametrize("N", [MIN_N, 512])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_gemm_is_exact_on_exact_operands(M, N, K):
    o = exact_operands(M, N, K)
    out = torch.full((M, N), -7.0, device=DEV)
    R.op_gemm(o["aq"], o["sa"], o["wq"], o["sw"], None, EPI_F32, X=out)
    assert torch.equal(out.double(), o["ref"])


def _dense_codes(rows, K):
    r = torch.arange(rows, device=DEV)[:, None]
    k = torch.arange(K, device=DEV)[None, :]
    return (1 + (r * 3 + k * 5 + k // 32) % 31 + 32 * ((r + k) % 2)).to(torch.uint8)      # never a zero magnitude


@pytest.mark.parametrize("shift", [0, 173])
@pytest.mark.parametrize("K", [MIN_K, 768])
def test_one_hot_sweep_of_a_places_every_row_k_and_scale_block(K, shift):
    M, N = 600, 256                                                   # M > K: every k is met by a second row; a partial tile
    m = torch.arange(M, device=DEV)
    kb = torch.arange(K // 32, device=DEV)
    ac = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    ac[m, (m + shift) % K] = (1 + m % 31 + 32 * ((m // 31) % 2)).to(torch.uint8)         # one nonzero code per row
    wc = _dense_codes(N, K)
    ae = (m[:, None] * 7 + kb[None, :] * 3) % 50 - 30                             # distinct per (row, block): a single product
    we = (torch.arange(N, device=DEV)[:, None] * 5 + kb[None, :] * 11) % 50 - 20  # is exact whatever the scales are
    out = torch.full((M, N), -7.0, device=DEV)
    R.op_gemm(R.pack(ac), R.scale_image(ae, R.ceil256(M)), R.pack(wc), R.scale_image(we, N), None, EPI_F32, X=out)
    ref = R.dequantize(ac, ae) @ R.dequantize(wc, we).t()
    assert torch.equal(out.double(), ref)
    assert int((ref != 0).sum()) == M * N


@pytest.mark.parametrize("shift", [0, 173])
def test_one_hot_sweep_of_w_places_every_row_k_and_scale_block(shift):
    M, N, K = 300, 768, MIN_K                                         # N > K: every k is met by a second weight row
    n = torch.arange(N, device=DEV)
    kb = torch.arange(K // 32, device=DEV)
    wc = torch.zeros(N, K, dtype=torch.uint8, device=DEV)
    wc[n, (n + shift) % K] = (1 + n % 31 + 32 * ((n // 31) % 2)).to(torch.uint8)
    ac = _dense_codes(M, K)
    ae = (torch.arange(M, device=DEV)[:, None] * 7 + kb[None, :] * 3) % 50 - 30
    we = (n[:, None] * 5 + kb[None, :] * 11) % 50 - 20
    out = torch.full((M, N), -7.0, device=DEV)
    R.op_gemm(R.pack(ac), R.scale_image(ae, R.ceil256(M)), R.pack(wc), R.scale_image(we, N), None, EPI_F32, X=out)
    ref = R.dequantize(ac, ae) @ R.dequantize(wc, we).t()
    assert torch.equal(out.double(), ref)
    assert int((ref != 0).sum()) == M * N


# ---------------------------------------------------------------------------------------------------- epilogues
def test_every_shared_epilogue_equals_the_mx_fp8_gemm_on_the_same_operands():
    M, N, K = 257, 512, 1024
    o = exact_operands(M, N, K, seed=1)
    a8 = R.code_values(o["ac"]).float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()     # exact: e2m3 values are e4m3
    w8 = R.code_values(o["wc"]).float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    assert torch.equal(a8.view(torch.float8_e4m3fn).double(), R.code_values(o["ac"]))
    assert torch.equal(w8.view(torch.float8_e4m3fn).double(), R.code_values(o["wc"]))
    sa, sw = o["sa"], o["sw"]
    g = gen(5)
    bias = torch.randn(N, generator=g, device=DEV) * 50
    gate = torch.randn(N, generator=g, device=DEV)
    x_init = torch.randn(M, N, generator=g, device=DEV) * 100
    x0 = (torch.randn(M, N, generator=g, device=DEV) * 100).to(torch.bfloat16)
    for epi in (EPI_BF16, EPI_GELU):
        c6 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        c8 = torch.ones(M, N, dtype=torch.bfloat16, device=DEV)
        R.op_gemm(o["aq"], sa, o["wq"], sw, bias, epi, Cb=c6)
        H.gemm_mxfp8(a8, sa, w8, sw, bias, epi, Cb=c8)
        assert torch.equal(c6.view(torch.int16), c8.view(torch.int16)), f"epilogue {epi}"
        assert float(c6.float().abs().max()) > 0
    f6, f8 = torch.zeros(M, N, device=DEV), torch.ones(M, N, device=DEV)
    R.op_gemm(o["aq"], sa, o["wq"], sw, bias, EPI_F32, X=f6)
    H.gemm_mxfp8(a8, sa, w8, sw, bias, EPI_F32, X=f8)
    assert torch.equal(f6, f8)
    assert torch.equal(f6, (o["ref"] + bias.double()).float())        # one rounding of the exact sum + bias
    r6, r8 = x_init.clone(), x_init.clone()
    R.op_gemm(o["aq"], sa, o["wq"], sw, bias, EPI_RESID, X=r6, gate=gate)
    H.gemm_mxfp8(a8, sa, w8, sw, bias, EPI_RESID, X=r8, gate=gate)
    assert torch.equal(r6, r8) and not torch.equal(r6, x_init)
    xa, xb = x_init.clone(), x_init.clone()
    ra, rb = torch.zeros(M, N, device=DEV), torch.ones(M, N, device=DEV)
    R.gemm_mxfp6_capture(o["aq"], sa, o["wq"], sw, bias, xa, gate, x0, ra)
    R.gemm_mxfp8_capture(a8, sa, w8, sw, bias, xb, gate, x0, rb)
    assert torch.equal(xa, xb) and torch.equal(ra, rb) and torch.equal(xa, r6)
    assert torch.equal(ra, xa - x0.float())


# ---------------------------------------------------------------------------------------------------- row guard
@pytest.mark.parametrize("M,N,K", [(1, 256, 512), (255, 256, 768), (257, 512, 1024), (300, 256, 512)])
def test_partial_tile_equals_the_padded_launch_and_leaves_the_rows_behind_alone(M, N, K):
    o = exact_operands(M, N, K, seed=2)
    Mp = R.ceil256(M)
    kb = K // 4 * 3
    # exactly M rows, then a poisoned guard in the same allocation: nothing behind row M - 1 may be read (a read of the guard
    # would bring in +-7.5 everywhere; with the NaN scales below it could only go unnoticed by reaching no output, which the
    # equality with the padded launch shows for the rows that exist)
    a_alloc = torch.full((M * kb + 4096,), 0xFF, dtype=torch.uint8, device=DEV)
    aq = a_alloc[:M * kb].view(M, kb)
    aq.copy_(o["aq"])
    sa_nan = R.scale_image(o["ae"], Mp, fill=0xFF)                    # E8M0 NaN in the scale bytes of rows >= M
    aq_pad = torch.full((Mp, kb), 0xDF, dtype=torch.uint8, device=DEV)       # rows >= M: live codes everywhere, NaN scales
    aq_pad[:M] = aq
    g = gen(9)
    bias = torch.randn(N, generator=g, device=DEV)
    gate = torch.randn(N, generator=g, device=DEV)
    x_init = torch.randn(Mp, N, generator=g, device=DEV)
    x0 = torch.randn(Mp, N, generator=g, device=DEV).to(torch.bfloat16)
    # the padded launch: the same rows zero-padded to ceil256(M) with plain scales
    a0 = torch.zeros(Mp, kb, dtype=torch.uint8, device=DEV)
    a0[:M] = aq
    s0 = R.scale_image(o["ae"], Mp, fill=127)

    def guarded(dtype, fill, body=None):
        whole = torch.full((M + GUARD, N), fill, dtype=dtype, device=DEV)
        if body is not None:
            whole[:M] = body
        return whole, whole[:M]

    for epi in (EPI_BF16, EPI_GELU):
        whole, cb = guarded(torch.bfloat16, -7.0)
        R.op_gemm(aq, sa_nan, o["wq"], o["sw"], bias, epi, Cb=cb)
        want = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
        R.op_gemm(a0, s0, o["wq"], o["sw"], bias, epi, Cb=want)
        assert torch.equal(cb.view(torch.int16), want[:M].view(torch.int16)), f"epilogue {epi}: rows < M differ from the padded launch"
        assert bool((whole[M:] == -7.0).all()), f"epilogue {epi}: rows >= M were written"
        assert bool(torch.isfinite(cb.float()).all())

    whole, out = guarded(torch.float32, -7.0)
    R.op_gemm(aq, sa_nan, o["wq"], o["sw"], bias, EPI_F32, X=out)
    want = torch.zeros(Mp, N, device=DEV)
    R.op_gemm(a0, s0, o["wq"], o["sw"], bias, EPI_F32, X=want)
    assert torch.equal(out, want[:M]) and bool((whole[M:] == -7.0).all())
    assert torch.equal(out, (o["ref"] + bias.double()).float())
    # the same M-row launch on the buffer whose rows >= M hold live codes under NaN scales: they reach nothing
    whole, out2 = guarded(torch.float32, -7.0)
    R.op_gemm(aq_pad, sa_nan, o["wq"], o["sw"], bias, EPI_F32, X=out2, M=M)
    assert torch.equal(out2, out) and bool((whole[M:] == -7.0).all())

    whole, x = guarded(torch.float32, -7.0, x_init[:M])
    R.op_gemm(aq, sa_nan, o["wq"], o["sw"], bias, EPI_RESID, X=x, gate=gate)
    want = x_init.clone()
    R.op_gemm(a0, s0, o["wq"], o["sw"], bias, EPI_RESID, X=want, gate=gate)
    assert torch.equal(x, want[:M]) and not torch.equal(x, x_init[:M]) and bool((whole[M:] == -7.0).all())

    xw, x = guarded(torch.float32, -7.0, x_init[:M])
    rw, r = guarded(torch.float32, -9.0)
    R.gemm_mxfp6_capture(aq, sa_nan, o["wq"], o["sw"], bias, x, gate, x0[:M], r)
    want_x, want_r = x_init.clone(), torch.zeros(Mp, N, device=DEV)
    R.gemm_mxfp6_capture(a0, s0, o["wq"], o["sw"], bias, want_x, gate, x0, want_r)
    assert torch.equal(x, want_x[:M]) and torch.equal(r, want_r[:M]) and torch.equal(r, x - x0[:M].float())
    assert bool((xw[M:] == -7.0).all()) and bool((rw[M:] == -9.0).all())
    assert bool((a_alloc[M * kb:] == 0xFF).all())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_einval_and_write_nothing():
    M, N, K = 64, 256, 512
    kb = K // 4 * 3
    o = exact_operands(M, N, K, seed=3)
    out = torch.full((M + GUARD, 2 * N), -7.0, device=DEV)
    cb = torch.full((M + GUARD, N), -7.0, dtype=torch.bfloat16, device=DEV)
    aq, sa, wq, sw = o["aq"], o["sa"], o["wq"], o["sw"]
    # operands long enough for K up to 1024, so that a refused K is the only thing wrong with its call
    a_big, w_big = torch.zeros(M, 768, dtype=torch.uint8, device=DEV), torch.zeros(N, 768, dtype=torch.uint8, device=DEV)
    sa_big = torch.full((32, 256), 127, dtype=torch.uint8, device=DEV)
    sw_big = torch.full((32, N), 127, dtype=torch.uint8, device=DEV)
    a_off = torch.zeros(M * kb + 16, dtype=torch.uint8, device=DEV)[8:8 + M * kb].view(M, kb)
    sa_off = torch.full((sa.numel() + 4,), 127, dtype=torch.uint8, device=DEV)[1:1 + sa.numel()].view_as(sa)
    assert a_off.data_ptr() % 16 == 8 and sa_off.data_ptr() % 4 == 1

    def refused(**kw):
        args = dict(Aq=aq, sa=sa, Wq=wq, sw=sw, bias=None, epi=EPI_F32, X=out)
        args.update(kw)
        with pytest.raises(H._lib.MagCacheHipError) as ei:
            R.op_gemm(**args)
        assert ei.value.status == H._lib.MC_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((cb == -7.0).all()), f"{kw}: something was written"

    refused(M=0)
    refused(M=-3)
    refused(N=0)
    refused(N=128)                                                    # N % 256
    refused(K=256)                                                    # K < 512
    refused(K=0)
    big = dict(Aq=a_big, sa=sa_big, Wq=w_big, sw=sw_big)
    refused(K=640, **big)                                             # K % 256 != 0
    refused(K=256, **big)                                             # K < 512
    refused(lda=kb + 8)                                               # lda % 16
    refused(ldw=kb - 16)                                              # ldw < 3 K / 4
    refused(Aq=a_off)                                                 # A 8 bytes off 16-byte alignment
    refused(sa=sa_off)                                                # scale image off 4-byte alignment
    refused(rows_pad_a=0)                                             # rows_pad < M
    refused(rows_pad_a=192)                                           # shorter than ceil256(M)
    refused(rows_pad_a=288 - 8)                                       # no multiple of 64
    refused(rows_pad_w=128)                                           # shorter than N
    refused(sa=None, rows_pad_a=256)
    refused(sw=None, rows_pad_w=N)
    refused(Aq=None, lda=kb, M=M, K=K)
    refused(epi=EPI_GELU_MXFP8, Cb=cb)                                # no fused producer in this format
    refused(epi=EPI_GELU_MXFP4, Cb=cb)
    refused(epi=EPI_CAPTURE)                                          # the single op has no X0 / R
    refused(epi=4)                                                    # unknown to this kernel
    refused(epi=99)
    refused(epi=EPI_BF16, X=None)                                     # epilogue without its output
    refused(epi=EPI_F32, X=None, Cb=cb)
    R.op_gemm(aq, sa, wq, sw, None, EPI_F32, X=out[:M, :N])           # and the plain call runs
    assert torch.equal(out[:M, :N].double(), o["ref"]) and bool((out[M:] == -7.0).all()) and bool((out[:, N:] == -7.0).all())

    # ---- the quantiser
    x = torch.randn(M, 128, device=DEV)
    q = torch.full((M, 96), 0x5A, dtype=torch.uint8, device=DEV)
    s = torch.full((4, 256), 0xEE, dtype=torch.uint8, device=DEV)

    def q_refused(**kw):
        args = dict(x=x, q=q, s=s, rows_pad=256)
        args.update(kw)
        with pytest.raises(H._lib.MagCacheHipError) as ei:
            R.op_quantize(**args)
        assert ei.value.status == H._lib.MC_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((q == 0x5A).all()) and bool((s == 0xEE).all()), f"{kw}: something was written"

    q_refused(M=0)
    q_refused(K=0)
    q_refused(K=48)                                                   # K % 32
    q_refused(ldx=132)                                                # ldx % 8
    q_refused(K=128, ldx=64)                                          # ldx < K
    q_refused(ldq=104)                                                # ldq % 16
    q_refused(ldq=80)                                                 # ldq < 3 K / 4
    q_refused(rows_pad=32)                                            # shorter than M rounded up to 64
    q_refused(rows_pad=200)                                           # no multiple of 64
    q_refused(x=x.view(-1)[2:2 + (M - 1) * 128].view(M - 1, 128), M=M - 1)      # x 8 bytes off 16-byte alignment


# ---------------------------------------------------------------------------------------------------- random data
@pytest.mark.parametrize("M,N,K", [(300, 256, 2560), (272, 512, 1792)])
def test_gemm_on_quantised_random_data_against_float64_of_the_dequantised_operands(M, N, K):
    g = gen(M)
    a = (torch.randn(M, K, generator=g, device=DEV)).to(torch.bfloat16)
    a[:, 3] *= 30.0
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device=DEV)
    aq, sa = R.op_quantize(a)
    wq, sw = R.op_quantize(w)
    out = torch.zeros(M, N, device=DEV)
    R.op_gemm(aq, sa, wq, sw, bias, EPI_F32, X=out)
    ref = R.dequantize(R.unpack(aq), R.scale_rows(sa, M)) @ R.dequantize(R.unpack(wq), R.scale_rows(sw, N)).t() + bias.double()
    err = rel_l2(out, ref)
    coarse = rel_l2(ref, a.double() @ w.double().t() + bias.double())
    print(f"M {M} N {N} K {K}: relative L2 vs the fp64 product of the dequantised operands {err:.2e}; "
          f"the W6A6 quantisation itself {coarse:.2e}")
    assert err < 1e-4

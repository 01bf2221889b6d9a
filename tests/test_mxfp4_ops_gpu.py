"""GPU: mc_op_quantize_rows_mxfp4 and mc_op_gemm_mxfp4 (csrc/gemm_mxfp4.hip, quant.h) against tests/mxfp4_ref.py.

  * quantiser: packed bytes and scale bytes equal the reference bit for bit -- fp32 and bf16 inputs, strided ldx / ldq, rows
    with exact ties, powers of two, zero blocks and blocks of denormal-small values, M around 16 and 256;
  * GEMM, exact: random e2m1 codes with per-block scale exponents whose total spread (A plus W) is <= 4 and K <= 1024.  Every
    product is a multiple of 0.25 2^smin and every partial sum stays below 2^24 of those units (K 144 2^spread = 2.4 M), so
    fp32 accumulation is exact in any order: the result must torch.equal the float64 product.  No tolerance;
  * one-hot sweep: row m of A is nonzero at the single k = m % K, so every (row, k, scale block) placement is checked once;
  * epilogues: e2m1 values are e4m3 values, so the same exact operands re-encoded for mc_op_gemm_mxfp8 must give bit-identical
    outputs for every shared epilogue (bf16, GELU, gated residual, residual capture, fp32);
  * row guard (the contract of tests/test_mx_gemm_rows_gpu.py): A holds exactly M rows, the scale bytes of rows >= M are NaN
    (0xFF), outputs behind row M keep their bits, rows < M equal the ceil256(M) launch;
  * refusals: MC_EINVAL and nothing written;
  * random data: relative L2 against float64 of the dequantised operands below 1e-4, the bar of the MX fp8 GEMM tests
    (tests/test_mx_gemm_rows_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import mxfp4_ref as R  # noqa: E402

DEV = "cuda:0"
GUARD = 64
EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE, EPI_F32, EPI_GELU_MXFP8 = 0, 1, 2, 3, 5, 8
MIN_N, MIN_K = 256, 512          # the smallest N and K mc_op_gemm_mxfp4 accepts


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------------------------------- quantiser
def special_rows(M, K, dtype, seed):
    """rows whose 32-element blocks cycle through: exact ties (amax = 6 2^n), powers of two, a zero block, denormal-small
    values (the exponent clamp), small negatives that round to -0, random data"""
    g = gen(seed)
    nb = K // 32
    x = torch.randn(M, nb, 32, generator=g, device=DEV) * torch.exp2(torch.randint(-12, 12, (M, nb, 1), generator=g, device=DEV).float())
    kind = (torch.arange(M, device=DEV)[:, None] + torch.arange(nb, device=DEV)[None, :]) % 6
    ties = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -6.0,
                         0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 0.0, -0.0, 0.125, -0.125, 0.2500001, 0.7499999, 5.000001, 3.4999998,
                         2.4999998, 1.2500001], device=DEV)
    pow2 = torch.exp2(torch.arange(32, device=DEV).float() - 20.0) * torch.where(torch.arange(32, device=DEV) % 3 == 0, -1.0, 1.0)
    den = torch.tensor([2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -129, 2.0 ** -126, 2.0 ** -133, -(2.0 ** -128), 3 * 2.0 ** -129,
                        2.0 ** -130] * 4, device=DEV)
    shift = torch.exp2(((torch.arange(M, device=DEV)[:, None] + torch.arange(nb, device=DEV)[None, :]) % 9 - 4).float())[..., None]
    x = torch.where((kind == 0)[..., None], ties * shift, x)
    x = torch.where((kind == 1)[..., None], pow2 * shift, x)
    x = torch.where((kind == 2)[..., None], torch.zeros_like(x), x)
    x = torch.where((kind == 3)[..., None], den.expand_as(x), x)
    x = torch.where((kind == 4)[..., None], den.expand_as(x) * 2.0 ** -7, x)       # everything rounds to +-0: e = -127
    return x.view(M, K).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", [32, 2080])        # the smallest K; 65 blocks: no power of two, and a lane's second block
@pytest.mark.parametrize("M", [1, 15, 16, 17, 255, 256, 257])
def test_quantiser_bits_equal_the_reference(M, K, dtype):
    x_rows = special_rows(M, K, dtype, seed=M * 7 + K)
    ldx, ldq = K + 24, K // 2 + 16                                   # strided source and destination
    xbuf = torch.full((M, ldx), 3.0, dtype=dtype, device=DEV)
    xbuf[:, :K] = x_rows
    qbuf = torch.full((M + 1, ldq), 0x5A, dtype=torch.uint8, device=DEV)
    rows_pad = R.ceil256(M)
    s = torch.full((K // 32, rows_pad), 0xEE, dtype=torch.uint8, device=DEV)
    R.op_quantize(xbuf, q=qbuf, s=s, rows_pad=rows_pad, M=M, K=K)
    codes, e = R.quantize(xbuf[:, :K])
    assert torch.equal(qbuf[:M, :K // 2], R.pack(codes)), "packed codes differ from the reference"
    assert bool((qbuf[:M, K // 2:] == 0x5A).all()) and bool((qbuf[M] == 0x5A).all()), "bytes outside [M, K / 2] were written"
    assert torch.equal(s, R.scale_image(e, rows_pad, fill=0xEE)), "scale bytes differ (or bytes of rows >= M were written)"


# ---------------------------------------------------------------------------------------------------- GEMM, exact
_exact = {}


def exact_operands(M, N, K, seed=0):
    """random codes, block exponents with spread 2 (A) + 2 (W); (codes, e, packed, scale image) per operand and the float64
    product, once per shape"""
    key = (M, N, K, seed)
    if key not in _exact:
        g = gen(1000 * seed + M + 3 * N + 5 * K)
        ac = torch.randint(0, 16, (M, K), generator=g, device=DEV).to(torch.uint8)
        wc = torch.randint(0, 16, (N, K), generator=g, device=DEV).to(torch.uint8)
        ae = torch.randint(-3, 0, (M, K // 32), generator=g, device=DEV)          # -3 .. -1
        we = torch.randint(1, 4, (N, K // 32), generator=g, device=DEV)           # 1 .. 3
        ref = R.dequantize(ac, ae) @ R.dequantize(wc, we).t()
        _exact[key] = dict(ac=ac, ae=ae, aq=R.pack(ac), sa=R.scale_image(ae, R.ceil256(M)),
                           wc=wc, we=we, wq=R.pack(wc), sw=R.scale_image(we, N), ref=ref)
    return _exact[key]


@pytest.mark.parametrize("K", [MIN_K, 768, 1024])      # 2, 3 (odd) and 4 K tiles
@pytest.mark.parametrize("N", [MIN_N, 512])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_gemm_is_exact_on_exact_operands(M, N, K):
    o = exact_operands(M, N, K)
    out = torch.full((M, N), -7.0, device=DEV)
    R.op_gemm(o["aq"], o["sa"], o["wq"], o["sw"], None, EPI_F32, X=out)
    assert torch.equal(out.double(), o["ref"])


@pytest.mark.parametrize("K", [MIN_K, 768])
def test_one_hot_sweep_places_every_row_k_and_scale_block(K):
    M, N = 600, 256                                                   # M > K: every k is met by a second row; a partial tile
    m = torch.arange(M, device=DEV)
    n = torch.arange(N, device=DEV)
    k = torch.arange(K, device=DEV)
    ac = torch.zeros(M, K, dtype=torch.uint8, device=DEV)
    ac[m, m % K] = (1 + m % 7 + 8 * ((m // 7) % 2)).to(torch.uint8)              # one nonzero code per row
    wc = (1 + (n[:, None] * 3 + k[None, :] * 5 + k[None, :] // 32) % 7 + 8 * ((n[:, None] + k[None, :]) % 2)).to(torch.uint8)
    kb = torch.arange(K // 32, device=DEV)
    ae = (m[:, None] * 7 + kb[None, :] * 3) % 50 - 30                             # distinct per (row, block): a single product
    we = (n[:, None] * 5 + kb[None, :] * 11) % 50 - 20                            # is exact whatever the scales are
    out = torch.full((M, N), -7.0, device=DEV)
    R.op_gemm(R.pack(ac), R.scale_image(ae, R.ceil256(M)), R.pack(wc), R.scale_image(we, N), None, EPI_F32, X=out)
    ref = R.dequantize(ac, ae) @ R.dequantize(wc, we).t()
    assert torch.equal(out.double(), ref)
    assert int((ref != 0).sum()) == M * N


# ---------------------------------------------------------------------------------------------------- epilogues
def test_every_shared_epilogue_equals_the_mx_fp8_gemm_on_the_same_operands():
    M, N, K = 257, 512, 1024
    o = exact_operands(M, N, K, seed=1)
    a8 = R.code_values(o["ac"]).float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()     # exact: e2m1 values are e4m3
    w8 = R.code_values(o["wc"]).float().to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    assert torch.equal(a8.view(torch.float8_e4m3fn).double(), R.code_values(o["ac"]))
    sa, sw = o["sa"], o["sw"]
    g = gen(5)
    bias = torch.randn(N, generator=g, device=DEV) * 50
    gate = torch.randn(N, generator=g, device=DEV)
    x_init = torch.randn(M, N, generator=g, device=DEV) * 100
    x0 = (torch.randn(M, N, generator=g, device=DEV) * 100).to(torch.bfloat16)
    for epi in (EPI_BF16, EPI_GELU):
        c4 = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        c8 = torch.ones(M, N, dtype=torch.bfloat16, device=DEV)
        R.op_gemm(o["aq"], sa, o["wq"], sw, bias, epi, Cb=c4)
        H.gemm_mxfp8(a8, sa, w8, sw, bias, epi, Cb=c8)
        assert torch.equal(c4.view(torch.int16), c8.view(torch.int16)), f"epilogue {epi}"
        assert float(c4.float().abs().max()) > 0
    f4, f8 = torch.zeros(M, N, device=DEV), torch.ones(M, N, device=DEV)
    R.op_gemm(o["aq"], sa, o["wq"], sw, bias, EPI_F32, X=f4)
    H.gemm_mxfp8(a8, sa, w8, sw, bias, EPI_F32, X=f8)
    assert torch.equal(f4, f8)
    assert torch.equal(f4, (o["ref"] + bias.double()).float())        # one rounding of the exact sum + bias ... in fp32: acc + b
    r4, r8 = x_init.clone(), x_init.clone()
    R.op_gemm(o["aq"], sa, o["wq"], sw, bias, EPI_RESID, X=r4, gate=gate)
    H.gemm_mxfp8(a8, sa, w8, sw, bias, EPI_RESID, X=r8, gate=gate)
    assert torch.equal(r4, r8) and not torch.equal(r4, x_init)
    xa, xb = x_init.clone(), x_init.clone()
    ra, rb = torch.zeros(M, N, device=DEV), torch.ones(M, N, device=DEV)
    R.gemm_mxfp4_capture(o["aq"], sa, o["wq"], sw, bias, xa, gate, x0, ra)
    R.gemm_mxfp8_capture(a8, sa, w8, sw, bias, xb, gate, x0, rb)
    assert torch.equal(xa, xb) and torch.equal(ra, rb) and torch.equal(xa, r4)
    assert torch.equal(ra, xa - x0.float())


# ---------------------------------------------------------------------------------------------------- row guard
@pytest.mark.parametrize("M,N,K", [(1, 256, 512), (255, 256, 768), (257, 512, 1024), (300, 256, 512)])
def test_partial_tile_equals_the_padded_launch_and_leaves_the_rows_behind_alone(M, N, K):
    o = exact_operands(M, N, K, seed=2)
    Mp = R.ceil256(M)
    aq = o["aq"].clone()                                              # exactly M rows: nothing behind row M - 1 may be read
    sa_nan = R.scale_image(o["ae"], Mp, fill=0xFF)                    # E8M0 NaN in the scale bytes of rows >= M
    aq_pad = torch.full((Mp, K // 2), 0x7F, dtype=torch.uint8, device=DEV)   # rows >= M: +-6 everywhere, NaN scales
    aq_pad[:M] = aq
    g = gen(9)
    bias = torch.randn(N, generator=g, device=DEV)
    gate = torch.randn(N, generator=g, device=DEV)
    x_init = torch.randn(Mp, N, generator=g, device=DEV)
    x0 = torch.randn(Mp, N, generator=g, device=DEV).to(torch.bfloat16)
    # the padded launch: the same rows zero-padded to ceil256(M) with plain scales
    a0 = torch.zeros(Mp, K // 2, dtype=torch.uint8, device=DEV)
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
    R.gemm_mxfp4_capture(aq, sa_nan, o["wq"], o["sw"], bias, x, gate, x0[:M], r)
    want_x, want_r = x_init.clone(), torch.zeros(Mp, N, device=DEV)
    R.gemm_mxfp4_capture(a0, s0, o["wq"], o["sw"], bias, want_x, gate, x0, want_r)
    assert torch.equal(x, want_x[:M]) and torch.equal(r, want_r[:M]) and torch.equal(r, x - x0[:M].float())
    assert bool((xw[M:] == -7.0).all()) and bool((rw[M:] == -9.0).all())


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_einval_and_write_nothing():
    M, N, K = 64, 256, 512
    o = exact_operands(M, N, K, seed=3)
    out = torch.full((M + GUARD, 2 * N), -7.0, device=DEV)
    cb = torch.full((M + GUARD, N), -7.0, dtype=torch.bfloat16, device=DEV)
    aq, sa, wq, sw = o["aq"], o["sa"], o["wq"], o["sw"]
    # operands long enough for K up to 1024, so that a refused K is the only thing wrong with its call
    a_big, w_big = torch.zeros(M, 512, dtype=torch.uint8, device=DEV), torch.zeros(N, 512, dtype=torch.uint8, device=DEV)
    sa_big = torch.full((32, 256), 127, dtype=torch.uint8, device=DEV)
    sw_big = torch.full((32, N), 127, dtype=torch.uint8, device=DEV)
    a_off = torch.zeros(M * (K // 2) + 16, dtype=torch.uint8, device=DEV)[8:8 + M * (K // 2)].view(M, K // 2)
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
    refused(K=640, **big)                                             # a K the kernel cannot tile (no multiple of 256)
    refused(K=256, **big)                                             # K < 512
    refused(lda=K // 2 + 8)                                           # lda % 16
    refused(ldw=K // 2 - 16)                                          # ldw < K / 2
    refused(Aq=a_off)                                                 # A 8 bytes off 16-byte alignment
    refused(sa=sa_off)                                                # scale image off 4-byte alignment
    refused(rows_pad_a=192)                                           # shorter than ceil256(M)
    refused(rows_pad_a=288 - 8)                                       # no multiple of 64
    refused(rows_pad_w=128)                                           # shorter than N
    refused(sa=None, rows_pad_a=256)
    refused(sw=None, rows_pad_w=N)
    refused(Aq=None, lda=K // 2, M=M, K=K)
    refused(epi=EPI_GELU_MXFP8, Cb=cb)                                # no fused FP4 producer
    refused(epi=EPI_CAPTURE)                                          # the single op has no X0 / R
    refused(epi=4)
    refused(epi=EPI_BF16, X=None)                                     # epilogue without its output
    refused(epi=EPI_F32, X=None, Cb=cb)
    R.op_gemm(aq, sa, wq, sw, None, EPI_F32, X=out[:M, :N])           # and the plain call runs
    assert torch.equal(out[:M, :N].double(), o["ref"]) and bool((out[M:] == -7.0).all()) and bool((out[:, N:] == -7.0).all())

    # ---- the quantiser
    x = torch.randn(M, 128, device=DEV)
    q = torch.full((M, 64), 0x5A, dtype=torch.uint8, device=DEV)
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
    q_refused(ldq=72)                                                 # ldq % 16
    q_refused(ldq=48)                                                 # ldq < K / 2
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
          f"the W4A4 quantisation itself {coarse:.2e}")
    assert err < 1e-4

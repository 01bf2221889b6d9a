"""GPU: the per-row-scaled fp8 GEMM (gemm_fp8_big.hip, fp8_linear = 1 of the Wan engine) on inputs whose result is exact
(tests/magcache_cases.py: fp8_int_case; its premises are checked by test_magcache_cases_cpu.py).

A and W hold the integers -2..2 as e4m3 bytes, the row / channel scales and the gate are powers of two, the bias is multiples of
1/4: every partial sum of A W^T is an integer of magnitude <= 4 K < 2^16, and acc * (sa * sw) + bias has no rounding in fp32.  So
whatever the order in which the matrix cores and the K loop add, there is ONE right bit pattern per output, and a K chunk
skipped or read twice, a row of the wrong tile, a tile the grouped / XCD-remapped rasterisation visits twice or not at all, or
a pad byte read as data changes it.  Per shape:

  * EPI_F32 == fp32(acc * (sa * sw) + bias), EPI_BF16 == torch's bf16 rounding of it, EPI_RESID_GATE == x + gate * that bf16
    (with a gate vector and with gate = NULL), EPI_RESID_CAPTURE: X the same and R == X_new - float(X0) -- all bit for bit;
    EPI_GELU_BF16 against the fp64 tanh-GELU of the exact bf16 pre-activation at the bar of the bf16 GEMM's epilogue 1;
  * 64 sentinel rows behind row M - 1 of every output (Cb, X, R) keep their bits; A and a_scale have exactly M rows;
  * rows [0, M) equal, bit for bit, a launch over ceil256(M) rows of the zero-padded operand;
  * at two shapes lda = K + 16 and ldw = K + 32 with pad bytes 0x38 (e4m3 1.0: read as data they change every sum), ldc / ldx /
    ldx0 / ldr = N + 8 with sentinel columns that keep their bits.

Measured on an MI355X: v_mfma_scale_f32_32x32x64_f8f6f4 returns these integer sums exactly -- every bitwise assertion below
holds at every shape, no deviation at all, so nothing here falls back to a tolerance.  What the first run of this file did
find: with fewer than 32 valid rows in the last M tile (M = 1, 257, 2309) one 64-k chunk of half the columns of those rows
was wrong in every epilogue.  The compiler had sunk the accumulators' last MFMAs behind the epilogue's row guard and reloaded
a spilled operand there under the guard's EXEC mask; the kernel now pins the accumulators in front of the guard.

EPI_RESID_CAPTURE has no shipped single-op call: it goes through mc_test_gemm_fp8_capture of the reference library, which
links the shipped gemm_fp8_big object."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import magcache_cases as MC  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 64
EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE, EPI_F32 = 0, 1, 2, 3, 5
SENT_X, SENT_R = -7.0, -9.0
ONE_E4M3 = 0x38


def ceil256(m):
    return (m + 255) // 256 * 256


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def guarded(rows, cols, dtype, fill, body=None, ld=None):
    """[rows + GUARD, ld] filled with `fill`; [0, rows) x [0, cols) = body where given.  -> (whole, that block)"""
    whole = torch.full((rows + GUARD, ld or cols), fill, dtype=dtype, device=DEV)
    if body is not None:
        whole[:rows, :cols] = body
    return whole, whole[:rows, :cols]


def kept(whole, rows, cols, fill):
    """everything of `whole` outside [0, rows) x [0, cols) still holds the bits of `fill`"""
    want = bits(torch.full((1,), fill, dtype=whole.dtype, device=DEV))[0]
    w = bits(whole).view(whole.shape)
    return bool((w[rows:] == want).all()) and bool((w[:rows, cols:] == want).all())


def where_it_differs(got, want, what):
    """a line on the deviation before a bitwise assertion: whole tiles / rows / K-chunk-sized amounts are the kernel's, noise of
    rounding size everywhere would be the matrix core's"""
    d = (got.double() - want.double()).abs()
    bad = d != 0
    if bool(bad.any()):
        rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
        rel = (d / want.double().abs().clamp_min(1e-30))[bad]
        print(f"{what}: {int(bad.sum())} of {bad.numel()} differ, rows {rows[:8].tolist()}..{int(rows[-1])} ({rows.numel()}), "
              f"cols {cols[:8].tolist()}..{int(cols[-1])} ({cols.numel()}), max abs {float(d.max()):.6g}, max rel {float(rel.max()):.3g}")
    else:
        print(f"{what}: values equal")


_dev = {}


def operands(M, N, K):
    """the case of a shape on the device, once; plus A and a_scale zero-padded to ceil256(M) rows (scale 1 on the pad rows)"""
    if (M, N, K) not in _dev:
        c = MC.fp8_int_case(M, N, K)
        d = {k: getattr(c, k).to(DEV) for k in ("aq", "wq", "sa", "sw", "bias", "gate", "x", "x0", "c32", "cb")}
        d["x_gate"], d["x_nogate"] = c.x_gate.float().to(DEV), c.x_nogate.float().to(DEV)
        d["gelu"] = MC.gelu_tanh64(c.cb).float().to(DEV)
        Mp = ceil256(M)
        d["aq_pad"] = torch.zeros(Mp, K, dtype=torch.uint8, device=DEV)
        d["aq_pad"][:M] = d["aq"]
        d["sa_pad"] = torch.ones(Mp, device=DEV)
        d["sa_pad"][:M] = d["sa"]
        d["x_pad"] = torch.zeros(Mp, N, device=DEV)
        d["x_pad"][:M] = d["x"]
        d["x0_pad"] = torch.zeros(Mp, N, dtype=torch.bfloat16, device=DEV)
        d["x0_pad"][:M] = d["x0"]
        _dev[(M, N, K)] = d
    return _dev[(M, N, K)]


@pytest.mark.parametrize("M,N,K", MC.FP8_SHAPES)
def test_every_epilogue_is_exact_and_a_partial_tile_is_the_padded_launch(M, N, K):
    o = operands(M, N, K)
    aq, sa, wq, sw, bias, gate = o["aq"], o["sa"], o["wq"], o["sw"], o["bias"], o["gate"]
    aqp, sap = o["aq_pad"], o["sa_pad"]
    Mp = ceil256(M)
    assert aq.shape == (M, K) and sa.shape == (M,) and aq.is_contiguous()

    # ---- fp32 store
    whole, out = guarded(M, N, torch.float32, SENT_X)
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_F32, X=out)
    where_it_differs(out, o["c32"], f"M {M} N {N} K {K} EPI_F32")
    assert same_bits(out, o["c32"])
    assert kept(whole, M, N, SENT_X)
    pad = torch.full((Mp, N), SENT_X, device=DEV)
    H.gemm_fp8(aqp, sap, wq, sw, bias, EPI_F32, X=pad)
    assert same_bits(out, pad[:M])

    # ---- bf16 store, GELU
    whole, cb = guarded(M, N, torch.bfloat16, SENT_X)
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_BF16, Cb=cb)
    assert same_bits(cb, o["cb"])
    assert kept(whole, M, N, SENT_X)
    padb = torch.full((Mp, N), SENT_X, dtype=torch.bfloat16, device=DEV)
    H.gemm_fp8(aqp, sap, wq, sw, bias, EPI_BF16, Cb=padb)
    assert same_bits(cb, padb[:M])

    whole, cg = guarded(M, N, torch.bfloat16, SENT_X)
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_GELU, Cb=cg)
    torch.testing.assert_close(cg.float(), o["gelu"], rtol=2e-2, atol=2e-2)
    assert kept(whole, M, N, SENT_X)
    H.gemm_fp8(aqp, sap, wq, sw, bias, EPI_GELU, Cb=padb)
    assert same_bits(cg, padb[:M])

    # ---- gated residual, with the gate vector and with gate = NULL
    for g, want in ((gate, o["x_gate"]), (None, o["x_nogate"])):
        whole, x = guarded(M, N, torch.float32, SENT_X, o["x"])
        H.gemm_fp8(aq, sa, wq, sw, bias, EPI_RESID, X=x, gate=g)
        where_it_differs(x, want, f"M {M} N {N} K {K} EPI_RESID_GATE gate {g is not None}")
        assert same_bits(x, want)
        assert kept(whole, M, N, SENT_X)
        padx = o["x_pad"].clone()
        H.gemm_fp8(aqp, sap, wq, sw, bias, EPI_RESID, X=padx, gate=g)
        assert same_bits(x, padx[:M])

    # ---- gated residual + MagCache capture
    xw, x = guarded(M, N, torch.float32, SENT_X, o["x"])
    rw, r = guarded(M, N, torch.float32, SENT_R)
    H.gemm_fp8_capture(aq, sa, wq, sw, bias, x, gate, o["x0"], r)
    assert same_bits(x, o["x_gate"])
    assert same_bits(r, x - o["x0"].float())                       # one fp32 subtraction
    assert kept(xw, M, N, SENT_X) and kept(rw, M, N, SENT_R)
    padx, padr = o["x_pad"].clone(), torch.full((Mp, N), SENT_R, device=DEV)
    H.gemm_fp8_capture(aqp, sap, wq, sw, bias, padx, gate, o["x0_pad"], padr)
    assert same_bits(x, padx[:M]) and same_bits(r, padr[:M])


@pytest.mark.parametrize("M,N,K", MC.FP8_STRIDED_SHAPES)
def test_leading_dimensions_beyond_the_row(M, N, K):
    o = operands(M, N, K)
    sa, sw, bias, gate = o["sa"], o["sw"], o["bias"], o["gate"]
    a_whole = torch.full((M, K + 16), ONE_E4M3, dtype=torch.uint8, device=DEV)
    w_whole = torch.full((N, K + 32), ONE_E4M3, dtype=torch.uint8, device=DEV)
    a_whole[:, :K], w_whole[:, :K] = o["aq"], o["wq"]
    aq, wq = a_whole[:, :K], w_whole[:, :K]
    assert (aq.stride(0), wq.stride(0)) == (K + 16, K + 32)
    ld = N + 8

    whole, out = guarded(M, N, torch.float32, SENT_X, ld=ld)
    assert out.stride(0) == ld
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_F32, X=out)
    where_it_differs(out, o["c32"], f"M {M} N {N} K {K} strided EPI_F32")
    assert same_bits(out, o["c32"])
    assert kept(whole, M, N, SENT_X)

    whole, cb = guarded(M, N, torch.bfloat16, SENT_X, ld=ld)
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_BF16, Cb=cb)
    assert same_bits(cb, o["cb"])
    assert kept(whole, M, N, SENT_X)

    whole, x = guarded(M, N, torch.float32, SENT_X, o["x"], ld=ld)
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_RESID, X=x, gate=gate)
    assert same_bits(x, o["x_gate"])
    assert kept(whole, M, N, SENT_X)

    xw, x = guarded(M, N, torch.float32, SENT_X, o["x"], ld=ld)
    rw, r = guarded(M, N, torch.float32, SENT_R, ld=ld)
    _, x0 = guarded(M, N, torch.bfloat16, 1e30, o["x0"], ld=ld)
    H.gemm_fp8_capture(aq, sa, wq, sw, bias, x, gate, x0, r)
    assert same_bits(x, o["x_gate"])
    assert same_bits(r, x - o["x0"].float())
    assert kept(xw, M, N, SENT_X) and kept(rw, M, N, SENT_R)


def test_refusals_leave_the_outputs_alone():
    M, N, K = 255, 256, 768
    o = operands(M, N, K)
    aq, sa, wq, sw, bias = o["aq"], o["sa"], o["wq"], o["sw"], o["bias"]
    out = torch.full((M, N), SENT_X, device=DEV)
    cb = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
    a_odd = torch.zeros(M, K + 8, dtype=torch.uint8, device=DEV)[:, :K]
    w_odd = torch.zeros(N, K + 8, dtype=torch.uint8, device=DEV)[:, :K]
    cases = {"N % 256": (aq, sa, wq[:128], sw), "K % 256": (aq[:, :640], sa, wq[:, :640], sw), "K = 256": (aq[:, :256], sa, wq[:, :256], sw),
             "lda % 16": (a_odd, sa, wq, sw), "ldw % 16": (aq, sa, w_odd, sw), "a_scale NULL": (aq, None, wq, sw),
             "w_scale NULL": (aq, sa, wq, None)}
    for what, (a, s_a, w, s_w) in cases.items():
        for epi, kw in ((EPI_F32, {"X": out}), (EPI_BF16, {"Cb": cb}), (EPI_RESID, {"X": out})):
            with pytest.raises(_lib.MagCacheHipError) as e:
                H.gemm_fp8(a, s_a, w, s_w, bias, epi, **kw)
            assert e.value.status == _lib.MC_EINVAL, what
        r = torch.full((M, N), SENT_R, device=DEV)
        with pytest.raises(H.HipStatusError) as e:
            H.gemm_fp8_capture(a, s_a, w, s_w, bias, out, None, o["x0"], r)
        assert e.value.status == H.HIP_INVALID_VALUE, what
        torch.cuda.synchronize()
        assert bool((out == SENT_X).all()) and bool((cb == SENT_X).all()) and bool((r == SENT_R).all()), what
    H.gemm_fp8(aq, sa, wq, sw, bias, EPI_F32, X=out)                # the unmodified call runs
    assert same_bits(out, o["c32"])

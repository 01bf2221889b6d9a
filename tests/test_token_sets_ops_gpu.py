"""GPU parity of the table forms an engine with token_timestep_sets runs (up to 64 modulation sets per forward): the
distinct-value pass, the batched time chain, LayerNorm + modulate with a set stride and the gated-residual GEMM epilogues that
take their gate vector from row min(sel[m], n_sets - 1) of a table.  Each form is pinned to the form it generalises: the same
bits as the single-set / two-set launch of the same row, on every kernel that has it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import token_sets_ops as TS  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def refused(fn, *args, **kw):
    with pytest.raises(H.HipStatusError) as ex:
        fn(*args, **kw)
    assert ex.value.status == H.HIP_INVALID_VALUE


# ----------------------------------------------------------------------------- the distinct-value pass
N_ALL, CAP = 3 * 1024 + 5, 8
VALUES = [999.0, 937.5, 750.25, 500.0, 312.5, 100.0, 12.25, 3.0, 0.5]       # descending; k of them are drawn


def draw(k, seed):
    """N_ALL tokens drawn from the first k of VALUES, every value present -> (t on the device, the index of each token)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randint(0, k, (N_ALL,), generator=g)
    idx[torch.randperm(N_ALL, generator=g)[:k]] = torch.arange(k)
    return torch.tensor(VALUES)[idx].to(DEV), idx.to(DEV)


@pytest.mark.parametrize("k", [1, 2, 8])
def test_token_t_sets_exact(k):
    """k <= cap distinct values: the table holds them in descending order, padded with the last; sel is the index torch
    computes; nothing overflows.  k <= 2: the selector and t2[0..2] are token_t_prepare's."""
    t, idx = draw(k, seed=k)
    t2, vals, sel = TS.token_t_sets(t, 0, N_ALL, N_ALL + 59, CAP)
    assert vals.tolist() == VALUES[:k] + [VALUES[k - 1]] * (CAP - k)
    assert t2.tolist() == [VALUES[0], VALUES[k - 1], 0.0, float(k)]
    assert torch.equal(sel[:N_ALL], idx.to(torch.uint8)) and int(sel[N_ALL:].max()) == 0
    if k <= 2:
        p2 = torch.full((5,), -7.0, device=DEV)
        psel = torch.full((N_ALL + 59,), 0xEE, dtype=torch.uint8, device=DEV)
        H.token_t_prepare(t, N_ALL, 0, N_ALL, N_ALL + 59, p2, psel)
        assert torch.equal(psel, sel) and p2[:3].tolist() == t2[:3].tolist()


def test_token_t_sets_overflow_nan_zero_and_window():
    # one value more than the table holds: the smallest value's tokens have no set, are counted and select cap - 1
    t, idx = draw(9, seed=9)
    t2, vals, sel = TS.token_t_sets(t, 0, N_ALL, N_ALL, CAP)
    n_small = int((idx == 8).sum())
    assert vals.tolist() == VALUES[:8] and t2.tolist() == [VALUES[0], VALUES[8], float(n_small), 8.0]
    assert torch.equal(sel, idx.clamp(max=CAP - 1).to(torch.uint8))
    # one NaN token: counted, modulated with set cap - 1, never in the table
    t, idx = draw(3, seed=10)
    t[1234] = float("nan")
    t2, vals, sel = TS.token_t_sets(t, 0, N_ALL, N_ALL, CAP)
    assert vals.tolist() == VALUES[:3] + [VALUES[2]] * 5 and t2.tolist() == [VALUES[0], VALUES[2], 1.0, 3.0]
    want = idx.to(torch.uint8)
    want[1234] = CAP - 1
    assert torch.equal(sel, want)
    # -0.0 and 0.0 are one value
    t = torch.full((N_ALL,), 700.0)
    t[::3] = 0.0
    t[1::3] = -0.0
    t2, vals, sel = TS.token_t_sets(t.to(DEV), 0, N_ALL, N_ALL, CAP)
    assert t2.tolist() == [700.0, 0.0, 0.0, 2.0] and vals.tolist() == [700.0] + [0.0] * 7
    assert torch.equal(sel.cpu(), (t != 700.0).to(torch.uint8))
    # a shard's window: the values of the WHOLE tensor, the selector of the window, zeros in the pad, nothing beyond it
    t, idx = draw(8, seed=11)
    t[:1000] = VALUES[0]                # the window [1000, 2029) alone lacks nothing, the head holds one value only
    idx[:1000] = 0
    sel = torch.full((1280 + 7,), 0xEE, dtype=torch.uint8, device=DEV)
    t2, vals = torch.full((4,), -7.0, device=DEV), torch.full((CAP,), -7.0, device=DEV)
    TS.TS("token_t_sets", H.P(t), N_ALL, 1000, 1029, 1280, CAP, H.P(t2), H.P(vals), H.P(sel), H.S())
    assert vals.tolist() == VALUES[:8] and t2.tolist() == [VALUES[0], VALUES[7], 0.0, 8.0]
    assert torch.equal(sel[:1029], idx[1000:2029].to(torch.uint8))
    assert int(sel[1029:1280].max()) == 0 and bool((sel[1280:] == 0xEE).all())


def test_token_t_sets_refusals():
    t = rnd(64)
    for args in [(None, 64, 0, 64, 64, 8), (t, 0, 0, 64, 64, 8), (t, 64, 60, 8, 8, 8), (t, 64, 0, 32, 16, 8), (t, 64, 0, 64, 64, 0),
                 (t, 64, 0, 64, 64, 65)]:
        t2, vals = torch.zeros(4, device=DEV), torch.zeros(64, device=DEV)
        sel = torch.zeros(64, dtype=torch.uint8, device=DEV)
        refused(TS.TS, "token_t_sets", H.P(args[0]), *args[1:], H.P(t2), H.P(vals), H.P(sel), H.S())


# ----------------------------------------------------------------------------- the batched time chain
@pytest.mark.parametrize("act_in,act_out", [(0, 1), (0, 0), (1, 0)], ids=["time0", "time1", "tproj"])
@pytest.mark.parametrize("K", [256, 1536])
@pytest.mark.parametrize("R", [1, 2, 3, 64])
def test_gemv_f32_rows_is_the_single_gemv_per_row(R, K, act_in, act_out):
    """every row of the multi-row GEMV holds the bits launch_gemv_f32 gives for that right-hand side alone (the engine's three
    uses: sinusoid -> silu out, plain, silu in); x and y rows strided as in "temb", the gaps untouched"""
    N = 768
    Wt, b = rnd(N, K, seed=K + R, scale=1.0 / math.sqrt(K)), rnd(N, seed=3)
    xb, yb = rnd(R, K + 40, seed=R), torch.full((R, N + 24), 5.0, device=DEV)
    TS.gemv_f32_rows(Wt, xb[:, :K], b, yb[:, :N], act_in, act_out)
    for r in range(R):
        y1 = torch.empty(N, device=DEV)
        H.gemv_f32(Wt, xb[r, :K].contiguous(), b, y1, act_in, act_out)
        assert torch.equal(yb[r, :N], y1), r
    assert bool((yb[:, N:] == 5.0).all())


def test_gemv_f32_rows_refusals():
    Wt, x, y = rnd(8, 16), rnd(2, 16), torch.zeros(2, 8, device=DEV)
    refused(TS.TS, "gemv_f32_rows", H.P(Wt), H.P(x), 16, None, H.P(y), 8, 0, 8, 16, 0, 0, H.S())       # R = 0
    refused(TS.TS, "gemv_f32_rows", H.P(Wt), H.P(x), 16, None, H.P(y), 8, 65, 8, 16, 0, 0, H.S())      # R > 64
    refused(TS.TS, "gemv_f32_rows", H.P(Wt), H.P(x), 16, None, H.P(y), 8, 2, 8, 6, 0, 0, H.S())        # K % 4
    assert float(y.abs().max()) == 0.0


def test_sinusoid_rows_and_add_bcast_rows_are_the_single_launches():
    vals = torch.tensor([999.0, 937.5, 500.0, 12.25, 0.0], device=DEV)
    dim = 256
    out = torch.full((5, dim + 8), 5.0, device=DEV)
    TS.sinusoid_rows(vals, dim, out)
    for r in range(5):
        o1 = torch.empty(dim, device=DEV)
        H.sinusoid(vals[r:r + 1].contiguous(), -1.0, dim, o1)
        assert torch.equal(out[r, :dim], o1)
    assert bool((out[:, dim:] == 5.0).all())
    # emod: sets x layers of 6 d; ehead: the d-periodic form (na = d, n = 2 d)
    R, d, NLy = 5, 128, 3
    a = rnd(R, 6 * d + 16, seed=1)
    mods = [rnd(6 * d, seed=10 + j) for j in range(NLy)]
    em = torch.full((R, NLy * 6 * d + 4), 5.0, device=DEV)
    TS.add_bcast_rows(a, 6 * d, mods, 6 * d, em)
    hm = rnd(2 * d, seed=20)
    eh = torch.full((R, 2 * d), 5.0, device=DEV)
    TS.add_bcast_rows(a, d, [hm], 2 * d, eh)
    for r in range(R):
        for j in range(NLy):
            o1 = torch.empty(6 * d, device=DEV)
            H.add_bcast(a[r, :6 * d].contiguous(), mods[j], o1, 6 * d)
            assert torch.equal(em[r, j * 6 * d:(j + 1) * 6 * d], o1)
        o2 = torch.empty(2 * d, device=DEV)
        H.add_bcast(a[r, :d].contiguous(), hm, o2, 2 * d)
        assert torch.equal(eh[r], o2)
    assert bool((em[:, NLy * 6 * d:] == 5.0).all())


# ----------------------------------------------------------------------------- LayerNorm + modulate
LN_M, LN_SETS = 37, 5


def ln_sel(n_sets=LN_SETS):
    m = torch.arange(LN_M)
    return ((3 * m + m // 4) % n_sets).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("D", [256, 1536, 5120])
def test_ln_modulate_sets_rows_equal_single_set_rows(D):
    """bf16 and fp32 outputs, the fused x0 + x row, and the fp8 / MX / MXFP4 producers: row m of the table form == the same
    row of the single-set launch with set sel[m]'s vectors; n_sets = 2 == the sc2 / sh2 form; a byte of 200 behaves as 4"""
    x, x0 = rnd(LN_M, D, seed=D, scale=2.0) + 0.3, rnd(LN_M, D, seed=D + 1, dtype=torch.bfloat16)
    stride = 6 * D + 8                                        # sets further apart than one vector, as in "emod"
    tab = rnd(LN_SETS * stride, seed=D + 2, scale=0.5)
    sc, sh = tab[D:], tab                                     # scale at +D, shift at +0, as the engine passes them
    sel = ln_sel()
    sel_big = sel.clone()
    sel_big[sel == 4] = 200
    rows_of = [torch.nonzero(sel == k).flatten() for k in range(LN_SETS)]
    for x0_ in (None, x0):
        for f32 in (False, True):
            def run(fn, *a, **kw):
                o = torch.zeros(LN_M, D, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
                fn(*a, **{("out_f32" if f32 else "out_bf16"): o, "x0": x0_, **kw})
                return o
            got = run(TS.ln_modulate_sets, x, sc, sh, 0, 1e-6, sel, stride, LN_SETS)
            assert torch.equal(got, run(TS.ln_modulate_sets, x, sc, sh, 0, 1e-6, sel_big, stride, LN_SETS))
            for k in range(LN_SETS):
                one = run(H.ln_modulate_sel, x, sc[k * stride:], sh[k * stride:], 0, 1e-6)
                assert torch.equal(got[rows_of[k]], one[rows_of[k]]), (k, f32)
            s2 = ln_sel(2)
            two = run(H.ln_modulate_sel, x, sc, sh, 0, 1e-6, sc2=sc[stride:], sh2=sh[stride:], sel=s2)
            assert torch.equal(run(TS.ln_modulate_sets, x, sc, sh, 0, 1e-6, s2, stride, 2), two)
    for mx in (False, True):
        q, s = TS.ln_modulate_fp8_sets(x, sc, sh, 0, 1e-6, mx, sel, stride, LN_SETS)
        qb, sb = TS.ln_modulate_fp8_sets(x, sc, sh, 0, 1e-6, mx, sel_big, stride, LN_SETS)
        assert torch.equal(q, qb) and torch.equal(s, sb)
        s = H.mx_unpermute(s, LN_M) if mx else s
        for k in range(LN_SETS):
            q1, s1 = H.ln_modulate_fp8(x, sc[k * stride:], sh[k * stride:], 0, 1e-6, mx)
            s1 = H.mx_unpermute(s1, LN_M) if mx else s1
            assert torch.equal(q[rows_of[k]], q1[rows_of[k]]) and torch.equal(s[rows_of[k]], s1[rows_of[k]]), (k, mx)
    q, s = TS.ln_modulate_mxfp4(x, sc, sh, 0, 1e-6, sel, stride, LN_SETS)
    s = H.mx_unpermute(s, LN_M)
    for k in range(LN_SETS):
        q1, s1 = TS.ln_modulate_mxfp4(x, sc[k * stride:], sh[k * stride:], 0, 1e-6)
        s1 = H.mx_unpermute(s1, LN_M)
        assert torch.equal(q[rows_of[k]], q1[rows_of[k]]) and torch.equal(s[rows_of[k]], s1[rows_of[k]]), k


def test_ln_modulate_sets_refusals():
    x, tab = rnd(8, 256), rnd(4 * 512)
    sel = torch.zeros(8, dtype=torch.uint8, device=DEV)
    out = torch.zeros(8, 256, dtype=torch.bfloat16, device=DEV)
    refused(TS.ln_modulate_sets, x, tab[256:], tab, 0, 1e-6, None, 512, 4, out_bf16=out)      # a stride without a selector
    refused(TS.ln_modulate_sets, x, tab[256:], tab, 0, 1e-6, sel, 512, 0, out_bf16=out)
    refused(TS.ln_modulate_sets, x, tab[256:], tab, 0, 1e-6, sel, 512, 65, out_bf16=out)
    refused(TS.ln_modulate_sets, x, tab[256:], tab, 0, 1e-6, sel, 510, 4, out_bf16=out)       # rows of the table off 16 bytes
    assert float(out.float().abs().max()) == 0.0


# ----------------------------------------------------------------------------- gated-residual GEMM epilogues
def gemm_sel(M, n_sets):
    m = torch.arange(M)
    return ((5 * m + m // 16) % n_sets).to(torch.uint8).to(DEV)


@pytest.mark.parametrize("n_sets", [3, 64])
@pytest.mark.parametrize("M,N,K", [(300, 512, 512), (1000, 768, 1024), (22000, 768, 1024)], ids=["small128", "v2-ragged", "v2-persistent"])
def test_gemm_resid_sets_all_kernels(M, N, K, n_sets):
    """The table form of the gated residual (+ capture) on the by-shape dispatch, the 128^2 kernel, gemm_bf16_v2 and the
    8-wave reference kernel: against the fp64 product with the tolerances of
    test_gemm_resid_capture_and_per_token_gates_all_kernels, R == X_new - X0 exactly, the same bits from all kernels, and
    nothing written outside M x N of padded buffers.  (22000 rows: 86 x 3 = 258 tiles of 256^2 on 256 CUs -- persistent
    workgroups take a second tile -- with a ragged last row tile.)"""
    A = rnd(M, K, seed=61, dtype=torch.bfloat16)
    Wt = rnd(N, K, seed=62, scale=0.03, dtype=torch.bfloat16)
    bias = rnd(N, seed=63)
    stride = N + 8
    gates = rnd(n_sets * stride, seed=64)
    sel = gemm_sel(M, n_sets)
    PADM, PADN = 3, 8
    x_in = rnd(M + PADM, N + PADN, seed=66)
    X0 = rnd(M, N, seed=67, dtype=torch.bfloat16)
    ref = (A.double() @ Wt.double().t() + bias.double()).float().bfloat16().float()
    g = gates.view(n_sets, stride)[sel.long(), :N]
    want = x_in[:M, :N] + ref * g
    outs = {}
    for kern in (0, 2, 4, 1):
        with H.gemm_kernel(kern) as kl:
            X, R = x_in.clone(), torch.full((M + PADM, N + PADN), 3.0, device=DEV)
            H.check_on(kl, TS.gemm_resid_sets(kl, A, Wt, bias, X, gates, stride, n_sets, sel, X0=X0, R=R, M=M, N=N))
            X2 = x_in.clone()
            H.check_on(kl, TS.gemm_resid_sets(kl, A, Wt, bias, X2, gates, stride, n_sets, sel, M=M, N=N))
        outs[kern] = (X, R, X2)
        torch.testing.assert_close(X[:M, :N], want, rtol=1e-2, atol=2e-2 * math.sqrt(K / 1536))
        assert torch.equal(R[:M, :N], X[:M, :N] - X0.float()) and torch.equal(X, X2)
        assert torch.equal(X[M:], x_in[M:]) and torch.equal(X[:, N:], x_in[:, N:])
        assert bool((R[M:] == 3.0).all()) and bool((R[:, N:] == 3.0).all())
    for kern in (2, 4, 1):
        for a, b in zip(outs[0], outs[kern]):
            assert torch.equal(a, b), kern


@pytest.mark.parametrize("M,N,K", [(300, 512, 512), (1000, 768, 1024)], ids=["small128", "v2-ragged"])
def test_gemm_resid_sets_degenerate_selectors(M, N, K):
    """n_sets = 2 == mc_op_gemm_bf16_resid_sel; an all-zero selector == the plain gated form; a selector of all n_sets - 1 (and
    of bytes far above it: clamped) reads the last table row"""
    A = rnd(M, K, seed=71, dtype=torch.bfloat16)
    Wt = rnd(N, K, seed=72, scale=0.03, dtype=torch.bfloat16)
    bias, x_in = rnd(N, seed=73), rnd(M, N, seed=74)
    X0 = rnd(M, N, seed=75, dtype=torch.bfloat16)
    n_sets, stride = 5, N + 4
    gates = rnd(n_sets * stride, seed=76)
    row = lambda k: gates[k * stride:k * stride + N].contiguous()     # noqa: E731
    for kern in (0, 1, 4, 2):
        with H.gemm_kernel(kern) as kl:
            def sets(sel, ns, capture=True):
                X, R = x_in.clone(), torch.zeros(M, N, device=DEV)
                H.check_on(kl, TS.gemm_resid_sets(kl, A, Wt, bias, X, gates, stride, ns, sel, X0=X0 if capture else None,
                                                  R=R if capture else None))
                return X, R
            s2 = gemm_sel(M, 2)
            Xa, Ra = x_in.clone(), torch.zeros(M, N, device=DEV)
            H.check_on(kl, kl.mc_op_gemm_bf16_resid_sel(H.P(A), K, H.P(Wt), K, H.P(bias), M, N, K, 1, H.P(Xa), N, H.P(row(0)),
                                                        H.P(row(1)), H.P(s2), H.P(X0), N, H.P(Ra), N, H.S()))
            X, R = sets(s2, 2)
            assert torch.equal(X, Xa) and torch.equal(R, Ra), kern
            for k, sel in ((0, torch.zeros(M, dtype=torch.uint8, device=DEV)),
                           (n_sets - 1, torch.full((M,), n_sets - 1, dtype=torch.uint8, device=DEV)),
                           (n_sets - 1, torch.full((M,), 255, dtype=torch.uint8, device=DEV))):
                Xp, Rp = x_in.clone(), torch.zeros(M, N, device=DEV)
                H.gemm(A, Wt, bias, 3, X=Xp, gate=row(k), X0=X0, R=Rp)
                X, R = sets(sel, n_sets)
                assert torch.equal(X, Xp) and torch.equal(R, Rp), (kern, k)
                Xq = x_in.clone()
                H.gemm(A, Wt, bias, 2, X=Xq, gate=row(k))
                assert torch.equal(sets(sel, n_sets, capture=False)[0], Xq), (kern, k)


def test_gemm_resid_sets_argument_errors():
    lib = _lib.load()
    M, N, K = 64, 256, 256
    A, Wt = rnd(M, K, dtype=torch.bfloat16), rnd(N, K, dtype=torch.bfloat16)
    x_in, gates = rnd(M, N, seed=1), rnd(4 * N, seed=2)
    sel = torch.zeros(M, dtype=torch.uint8, device=DEV)
    X = x_in.clone()
    for g, stride, ns, s in ((gates, N, 0, sel), (gates, N, 65, sel), (None, N, 4, sel), (gates, N - 4, 4, sel), (gates, N, 4, None),
                             (gates, N + 2, 2, sel)):
        assert TS.gemm_resid_sets(lib, A, Wt, None, X, g, stride, ns, s) == _lib.MC_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(X, x_in)                                       # nothing was launched


def test_gemm_mxfp8_resid_table_form():
    """the MX fp8 GEMM's gated residual (gemm_epilogue.h, shared by the fp8 / MXFP4 / MXFP6 GEMMs): n_sets = 2 == its own
    gate_sel form; n_sets = 3 == per row, the single-gate launch with that row's table row (selected in torch)"""
    M, N, K = 300, 512, 512
    Aq, sa = H.quantize_rows_mx(rnd(M, K, seed=1, dtype=torch.bfloat16))
    Wq, sw = H.quantize_rows_mx(rnd(N, K, seed=2, scale=0.03, dtype=torch.bfloat16))
    bias, x_in = rnd(N, seed=3), rnd(M, N, seed=4)
    stride = N + 4
    gates = rnd(3 * stride, seed=5)
    row = lambda k: gates[k * stride:k * stride + N].contiguous()     # noqa: E731
    s2 = gemm_sel(M, 2)
    Xa, Xb = x_in.clone(), x_in.clone()
    TS.gemm_mxfp8_resid_rows(Aq, sa, Wq, sw, bias, Xa, row(0), row(1), s2)
    TS.gemm_mxfp8_resid_rows(Aq, sa, Wq, sw, bias, Xb, gates, None, s2, stride, 2)
    assert torch.equal(Xa, Xb)
    s3 = gemm_sel(M, 3)
    X3 = x_in.clone()
    TS.gemm_mxfp8_resid_rows(Aq, sa, Wq, sw, bias, X3, gates, None, s3, stride, 3)
    want = torch.empty_like(x_in)
    for k in range(3):
        Xk = x_in.clone()
        H.gemm_mxfp8(Aq, sa, Wq, sw, bias, 2, X=Xk, gate=row(k))
        want[s3 == k] = Xk[s3 == k]
    assert torch.equal(X3, want)
    assert not torch.equal(X3, Xb)                                    # (the third row of the table was used)
    X4 = x_in.clone()
    refused(TS.gemm_mxfp8_resid_rows, Aq, sa, Wq, sw, bias, X4, gates, None, s3, N - 4, 3)
    assert torch.equal(X4, x_in)

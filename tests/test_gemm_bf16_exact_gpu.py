"""GPU: the bf16 GEMM -- the default Linear of both engines -- on inputs whose result is exact (tests/magcache_cases.py:
bf16_int_case; its premises are checked by test_magcache_cases_cpu.py), on each of its three paths, through the shipped library
alone: the 128 x 128 kernel (gemm_bf16.hip, gemm_kernel = 1), the persistent 256 x 256 gemm_bf16_v2 (gemm_kernel = 4) and v2
split-K + splitk_reduce_kernel (gemm_splitk = 2, 3, 8 with a workspace).  Every test forces its path and asks
mc_op_gemm_bf16_kernel / mc_op_gemm_bf16_splitk that this IS the path, so that none is compared with itself unnoticed.

A and W hold integers in [-8, 8], the bias quarters, the gates powers of two: every partial sum of A W^T is an integer below
2^24, so whatever the order in which the matrix cores, the K loop and the K slices add there is ONE right bit pattern per
output.  The sums are large against bf16's 8 bits: 8-22 % of the outputs lie exactly between two bf16 values and 49-89 % are no
bf16 value, so EPI_BF16 pins round-to-nearest-even (a truncating store differs on a fifth of the outputs and more).

Shapes (M, N, K) -- magcache_cases.py says what each is the smallest case of:
  128 x 128    (1, 4, 64) (127, 132, 64) (129, 260, 192) (300, 388, 128) (1100, 260, 64)
  v2           (1, 256, 256) (255, 256, 384) (257, 512, 256) (700, 768, 512) (300, 2304, 256) (513, 8192, 256); (700, 768, 512)
               and (257, 512, 256) again with gemm_v2_max_grid = 1, 2, 4: one workgroup walking all 9 tiles, trips of 5 / 4 and of
               3 / 2 / 2 / 2 -- the hand-over "next tile's K tiles 0, 1 prefetched under the epilogue" in every trip but the last
  split-K      slices 2, 3, 8 x K = 256 s, 512 s x (M, N) = (77, 256), (300, 512), (513, 768), each also with gemm_v2_max_grid = 2
               (a workgroup walks several (slice, tile) units)
Per shape and path, bit for bit: EPI_F32 == acc + bias, EPI_BF16 == its bf16 rounding cb, EPI_RESID_GATE == x + gate * cb with
a gate vector, with gate = NULL, with per-row gates (mc_op_gemm_bf16_resid_sel) and with a gate table (_resid_sets),
EPI_RESID_CAPTURE the same X and R == X_new - float(X0); on the 128 x 128 kernel EPI_EMBED with m_valid = M - 5.  (Split-K
exists for epilogues 0-3 without per-row gates; the rest is not split by the library.)  The activations (1, and 6, 7 on the
128 x 128 kernel, the only one that has them) against the fp64 activation of the exact cb at rtol = atol = 2e-2; epilogue 1
gives the same bits on all three paths at (300, 512, 512).  Then: mc_op_gemm_bf16_rowsplit (one v2 launch at m_split = 256,
K = 1024, two launches otherwise, under split-K the reduce kernel's second operand set), mc_op_gemm_bf16_gelu_split, one-hot
sweeps of A and of W (every k of every row placed, no accumulation), operands with lda = K + 8 / ldw = K + 24 and live pad, 64 NaN
rows behind A, outputs with ld = N + 8 and sentinel columns and rows, and the calls launch_gemm_bf16 refuses (gemm_bf16_args_ok
in ops.h: MC_EINVAL and nothing written).

Measured on an MI355X: nothing deviated.  Every bitwise assertion below holds on all three paths at every shape, so no kernel
bug was found and nothing here falls back to a tolerance; epilogue 1 gives identical bits on the three paths.  The largest
distance of each activation from the bf16 rounding of its fp64 value, over the outputs whose expected magnitude is at least
2^-6: 0 bf16 ulp for epilogue 1 (tanh-GELU: all paths and shapes, the GELU half of the split included), 0 for epilogue 6
(erf-GELU) and 0 for epilogue 7 (SiLU); below 2^-6 the largest absolute deviation was 8.6e-6, 2.1e-5 and 2.1e-5.  (The
pre-activations here are quarters, and 0.4-2 % of them lie inside (-4, 4): the activation's curve is sampled at few points; its
accuracy on random data stays with test_gemm_bf16_epilogues.)  The whole file runs in about 5 seconds.

What the work on this file did change is the host side: the launchers checked the shape and lda % 8, ldw % 8 only, and
most of the calls test_refusals_leave_the_outputs_alone makes would have reached the device.  They are refused by
gemm_bf16_args_ok now; each case was confirmed refused on the host before it was first run on a GPU."""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import magcache_cases as MC  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from test_fp8_gemm_rows_gpu import GUARD, bits, guarded, kept, same_bits, where_it_differs  # noqa: E402

DEV = "cuda:0"
EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE, EPI_EMBED, EPI_F32, EPI_GELU_ERF, EPI_SILU, EPI_GELU_SPLIT = 0, 1, 2, 3, 4, 5, 6, 7, 10
SENT_X, SENT_R = -7.0, -9.0
SMALL, V2 = 1, 4                     # gemm_kernel values
WS_BYTES = 32 << 20                  # 8 slices x 9 tiles x 256 KiB = 18 MiB is the most a shape here needs
_ws = None


@contextlib.contextmanager
def path(kernel, slices=0, max_grid=0):
    """force a path for the enclosed calls: the kernel, for split-K the slice count and a workspace (slices = 0: never split),
    and the number of persistent workgroups of gemm_bf16_v2.  Everything is put back whatever happens inside."""
    global _ws
    lib = _lib.load()
    try:
        _lib.check(lib.mc_set_option(b"gemm_kernel", kernel))
        _lib.check(lib.mc_set_option(b"gemm_splitk", slices))
        _lib.check(lib.mc_set_option(b"gemm_v2_max_grid", max_grid))
        if slices:
            if _ws is None:
                _ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
            _lib.check(lib.mc_op_set_splitk_workspace(H.P(_ws), _ws.numel()))
        yield lib
    finally:
        torch.cuda.synchronize()
        lib.mc_set_option(b"gemm_kernel", 0)
        lib.mc_set_option(b"gemm_splitk", 1)
        lib.mc_set_option(b"gemm_v2_max_grid", 0)
        lib.mc_op_set_splitk_workspace(None, 0)


@pytest.fixture(autouse=True)
def defaults_restored():
    yield
    lib = _lib.load()
    v = C.c_int(-1)
    for key, want in ((b"gemm_kernel", 0), (b"gemm_splitk", 1), (b"gemm_v2_max_grid", 0)):
        _lib.check(lib.mc_get_option(key, C.byref(v)))
        assert v.value == want, key
    assert lib.mc_op_gemm_bf16_splitk(512, 3072, 12288, EPI_RESID) == 1      # no workspace left behind


def is_path(lib, M, N, K, epi, kernel, slices=0):
    """the dispatch runs `epi` at this shape on the kernel (and with the slice count) the test means to check"""
    return lib.mc_op_gemm_bf16_kernel(M, N, K, epi) == kernel and lib.mc_op_gemm_bf16_splitk(M, N, K, epi) == max(slices, 1)


def _ld(t):
    return t.stride(0) if t is not None else 0


def gemm_resid_sel(A, W, bias, X, gate, gate2, sel, X0=None, R=None):
    """EPI_RESID_GATE (EPI_RESID_CAPTURE with X0 and R) with the gate vector chosen per row: sel[m] ? gate2 : gate"""
    M, K = A.shape
    _lib.check(H.L().mc_op_gemm_bf16_resid_sel(H.P(A), A.stride(0), H.P(W), W.stride(0), H.P(bias), M, W.shape[0], K, int(R is not None),
                                               H.P(X), X.stride(0), H.P(gate), H.P(gate2), H.P(sel), H.P(X0), _ld(X0), H.P(R), _ld(R), H.S()))


def gemm_resid_sets(A, W, bias, X, table, sel, X0=None, R=None):
    """the same with row min(sel[m], n_sets - 1) of a table [n_sets, >= N] of gate vectors"""
    M, K = A.shape
    _lib.check(H.L().mc_op_gemm_bf16_resid_sets(H.P(A), A.stride(0), H.P(W), W.stride(0), H.P(bias), M, W.shape[0], K, int(R is not None),
                                                H.P(X), X.stride(0), H.P(table), table.stride(0), table.shape[0], H.P(sel), H.P(X0),
                                                _ld(X0), H.P(R), _ld(R), H.S()))


def gemm_rowsplit(A, W, W_b, bias, bias_b, m_split, epi, Cb=None, X=None, gate=None, gate_b=None):
    """rows [m_split, M) multiply with W_b / bias_b / gate_b"""
    M, K = A.shape
    _lib.check(H.L().mc_op_gemm_bf16_rowsplit(H.P(A), A.stride(0), H.P(W), H.P(W_b), W.stride(0), H.P(bias), H.P(bias_b), M, W.shape[0], K,
                                              m_split, epi, H.P(Cb), _ld(Cb), H.P(X), _ld(X), H.P(gate), H.P(gate_b), H.S()))


def gemm_gelu_split(A, W, bias, n_split, Cb, Cb2):
    """columns [0, n_split) -> Cb (bf16), columns [n_split, N) -> Cb2 (tanh-GELU)"""
    M, K = A.shape
    _lib.check(H.L().mc_op_gemm_bf16_gelu_split(H.P(A), A.stride(0), H.P(W), W.stride(0), H.P(bias), M, W.shape[0], K, n_split, H.P(Cb),
                                                _ld(Cb), H.P(Cb2), _ld(Cb2), H.S()))


_dev = {}


def operands(M, N, K):
    """the case of a shape on the device, once (read-only): operands, and the expected values as the dtype the kernel stores"""
    if (M, N, K) not in _dev:
        c = MC.bf16_int_case(M, N, K)
        d = {k: getattr(c, k).to(DEV) for k in ("a", "w", "bias", "gate", "gate2", "table", "sel", "x", "x0")}
        for k in ("c32", "x_gate", "x_nogate", "x_sel", "x_sets"):
            d[k] = getattr(c, k).float().to(DEV)
        d["cb"] = c.cb.bfloat16().to(DEV)
        _dev[(M, N, K)] = d
    return _dev[(M, N, K)]


def act64(epi, cb):
    x = cb.double()
    if epi == EPI_GELU:
        return MC.gelu_tanh64(x)
    if epi == EPI_GELU_ERF:
        return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))
    return x * torch.sigmoid(x)


def bf16_ulps(got, want64):
    """largest distance, in bf16 steps, between bf16 `got` and the bf16 rounding of the fp64 `want64`, over the outputs whose
    expected magnitude is at least 2^-6 (below that the bar is its absolute term, and the tail of an activation is a ratio of
    two tiny numbers); and the largest absolute deviation over the rest"""
    def key(t):
        b = bits(t).int() & 0xFFFF
        return torch.where(b >= 0x8000, -(b & 0x7FFF), b)
    big = want64.abs() >= 2.0 ** -6
    d = (key(got) - key(want64.float().bfloat16())).abs()
    rest = (got.double() - want64).abs()[~big]
    return int(d[big].max()) if bool(big.any()) else 0, float(rest.max()) if rest.numel() else 0.0


def check_activation(tag, epi, got, cb):
    want = act64(epi, cb)
    ulps, rest = bf16_ulps(got, want)
    print(f"{tag} epilogue {epi}: largest distance {ulps} bf16 ulp where |expected| >= 2^-6, {rest:.3g} absolute below; "
          f"{int((cb.float().abs() < 4).sum())} of {got.numel()} outputs with |pre-activation| < 4")
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-2, atol=2e-2)


def exact(got, want, what):
    where_it_differs(got, want, what)
    assert same_bits(got, want), what


def check_shape(lib, M, N, K, kernel, slices=0):
    """every epilogue the path has at this shape, each output with 64 sentinel rows behind it"""
    o = operands(M, N, K)
    a, w, bias, gate = o["a"], o["w"], o["bias"], o["gate"]
    tag = f"M {M} N {N} K {K} kernel {kernel} slices {slices}"
    assert a.shape == (M, K) and a.is_contiguous() and w.shape == (N, K)

    for epi in (EPI_BF16, EPI_GELU, EPI_RESID, EPI_CAPTURE):
        assert is_path(lib, M, N, K, epi, kernel, slices), (tag, epi)

    whole, cb = guarded(M, N, torch.bfloat16, SENT_X)
    H.gemm(a, w, bias, EPI_BF16, Cb=cb)
    exact(cb, o["cb"], f"{tag} EPI_BF16")                                   # round-to-nearest-even, ties included
    assert kept(whole, M, N, SENT_X)

    whole, cg = guarded(M, N, torch.bfloat16, SENT_X)
    H.gemm(a, w, bias, EPI_GELU, Cb=cg)
    check_activation(tag, EPI_GELU, cg, o["cb"])
    assert kept(whole, M, N, SENT_X)

    for g, want in ((gate, o["x_gate"]), (None, o["x_nogate"])):
        whole, x = guarded(M, N, torch.float32, SENT_X, o["x"])
        H.gemm(a, w, bias, EPI_RESID, X=x, gate=g)
        exact(x, want, f"{tag} EPI_RESID_GATE gate {g is not None}")
        assert kept(whole, M, N, SENT_X)

    xw, x = guarded(M, N, torch.float32, SENT_X, o["x"])
    rw, r = guarded(M, N, torch.float32, SENT_R)
    H.gemm(a, w, bias, EPI_CAPTURE, X=x, gate=gate, X0=o["x0"], R=r)
    exact(x, o["x_gate"], f"{tag} EPI_RESID_CAPTURE X")
    exact(r, x - o["x0"].float(), f"{tag} EPI_RESID_CAPTURE R")            # one fp32 subtraction
    assert kept(xw, M, N, SENT_X) and kept(rw, M, N, SENT_R)
    if slices:
        return              # the library splits K for these four forms only

    assert is_path(lib, M, N, K, EPI_F32, kernel)
    whole, out = guarded(M, N, torch.float32, SENT_X)
    H.gemm(a, w, bias, EPI_F32, X=out)
    exact(out, o["c32"], f"{tag} EPI_F32")
    assert kept(whole, M, N, SENT_X)

    # per-row gates: two vectors, and a table of three; with and without the capture
    for capture in (False, True):
        for form, want in (("sel", o["x_sel"]), ("sets", o["x_sets"])):
            xw, x = guarded(M, N, torch.float32, SENT_X, o["x"])
            rw, r = guarded(M, N, torch.float32, SENT_R)
            kw = {"X0": o["x0"], "R": r} if capture else {}
            if form == "sel":
                gemm_resid_sel(a, w, bias, x, gate, o["gate2"], o["sel"], **kw)
            else:
                gemm_resid_sets(a, w, bias, x, o["table"], o["sel"], **kw)
            exact(x, want, f"{tag} per-row gates ({form}) capture {capture}")
            if capture:
                exact(r, x - o["x0"].float(), f"{tag} per-row gates ({form}) R")
            assert kept(xw, M, N, SENT_X) and kept(rw, M, N, SENT_R)

    if kernel != SMALL:
        return
    # the forms only the 128 x 128 kernel has
    for epi in (EPI_GELU_ERF, EPI_SILU):
        assert is_path(lib, M, N, K, epi, SMALL)
        whole, ca = guarded(M, N, torch.bfloat16, SENT_X)
        H.gemm(a, w, bias, epi, Cb=ca)
        check_activation(tag, epi, ca, o["cb"])
        assert kept(whole, M, N, SENT_X)
    m_valid = M - 5
    lo = max(m_valid, 0)
    xw, x = guarded(M, N, torch.float32, SENT_X)
    cw, c0 = guarded(M, N, torch.bfloat16, SENT_X)
    H.gemm(a, w, bias, EPI_EMBED, X=x, X0out=c0, m_valid=m_valid)
    exact(x[:lo], o["cb"][:lo].float(), f"{tag} EPI_EMBED X")
    exact(c0[:lo], o["cb"][:lo], f"{tag} EPI_EMBED X0out")
    assert not bool(bits(x[lo:]).any()) and not bool(bits(c0[lo:]).any())          # +0.0 from m_valid on
    assert kept(xw, M, N, SENT_X) and kept(cw, M, N, SENT_X)


@pytest.mark.parametrize("M,N,K", MC.BF16_SMALL_SHAPES)
def test_128x128_kernel_is_exact_in_every_epilogue(M, N, K):
    with path(SMALL) as lib:
        check_shape(lib, M, N, K, SMALL)


@pytest.mark.parametrize("M,N,K", MC.BF16_V2_SHAPES)
def test_v2_is_exact_in_every_epilogue(M, N, K):
    with path(V2) as lib:
        check_shape(lib, M, N, K, V2)


@pytest.mark.parametrize("max_grid", [0, 1, 2, 4])
@pytest.mark.parametrize("M,N,K", MC.BF16_V2_TRIP_SHAPES)
def test_v2_is_exact_when_a_workgroup_walks_several_tiles(M, N, K, max_grid):
    with path(V2, max_grid=max_grid) as lib:
        check_shape(lib, M, N, K, V2)


@pytest.mark.parametrize("M,N", MC.BF16_SPLITK_MN)
@pytest.mark.parametrize("k_per_slice", [256, 512])
@pytest.mark.parametrize("slices", MC.BF16_SPLITK_SLICES)
def test_split_k_and_its_reduce_are_exact(slices, k_per_slice, M, N):
    for max_grid in (0, 2):
        with path(V2, slices=slices, max_grid=max_grid) as lib:
            check_shape(lib, M, N, k_per_slice * slices, V2, slices)


def test_the_three_paths_give_the_same_gelu_bits():
    """the 128 x 128 kernel, v2 and the split-K reduce apply gelu_tanh_fast (v2: its packed-fp32 pair form) to identical
    pre-activation bits: the bf16 results are identical too"""
    M, N, K = MC.BF16_COMMON_SHAPE
    o = operands(M, N, K)
    outs = {}
    for name, kernel, slices in (("128x128", SMALL, 0), ("v2", V2, 0), ("split-K", V2, 2)):
        with path(kernel, slices=slices) as lib:
            assert is_path(lib, M, N, K, EPI_GELU, kernel, slices), name
            outs[name] = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
            H.gemm(o["a"], o["w"], o["bias"], EPI_GELU, Cb=outs[name])
    for name in ("v2", "split-K"):
        exact(outs[name], outs["128x128"], f"EPI_GELU_BF16 {name} against the 128x128 kernel")


# ----------------------------------------------------------------------------- one-hot sweeps: placement without accumulation
_PATHS = [("128x128", SMALL, 0), ("v2", V2, 0), ("split-K", V2, 2)]


def dense(rows, K, seed):
    """random bf16 without a zero: every product with a one-hot row is a non-zero fp32 value, exact (8 x 8 significant bits)"""
    t = torch.randn(rows, K, generator=torch.Generator().manual_seed(seed)).bfloat16()
    return torch.where(t == 0, torch.ones_like(t), t).to(DEV)


def one_hot(rows, K, shift, seed):
    """row i is non-zero at k = (i + shift) % K only"""
    t = torch.zeros(rows, K, dtype=torch.bfloat16, device=DEV)
    i = torch.arange(rows, device=DEV)
    t[i, (i + shift) % K] = dense(rows, 1, seed)[:, 0]
    return t


def check_one_hot(lib, name, a, w, kernel, slices):
    M, K = a.shape
    N = w.shape[0]
    want = (a.double() @ w.double().t()).float()            # one non-zero term per output: exact
    assert bool((want != 0).all())
    if slices:
        # no fp32 store under split-K: x = 0 + 1 * bf16(product) shows the placement, to bf16 precision
        assert is_path(lib, M, N, K, EPI_RESID, kernel, slices), name
        x = torch.zeros(M, N, device=DEV)
        H.gemm(a, w, None, EPI_RESID, X=x)
        exact(x, want.bfloat16().float(), f"one-hot {name} M {M} N {N} K {K} EPI_RESID_GATE on zeros")
        return
    assert is_path(lib, M, N, K, EPI_F32, kernel), name
    out = torch.full((M, N), SENT_X, device=DEV)
    H.gemm(a, w, None, EPI_F32, X=out)
    exact(out, want, f"one-hot {name} M {M} N {N} K {K} EPI_F32")


@pytest.mark.parametrize("shift", [0, 173])
@pytest.mark.parametrize("name,kernel,slices,M,N,K", [("128x128", SMALL, 0, 300, 132, 256), ("v2", V2, 0, 600, 256, 512),
                                                      ("split-K", V2, 2, 600, 256, 512)], ids=["128x128", "v2", "split-K"])
def test_one_hot_rows_of_a_pick_the_right_k(name, kernel, slices, M, N, K, shift):
    with path(kernel, slices=slices) as lib:
        check_one_hot(lib, name, one_hot(M, K, shift, 7), dense(N, K, 8), kernel, slices)


@pytest.mark.parametrize("shift", [0, 173])
@pytest.mark.parametrize("name,kernel,slices", _PATHS, ids=[p[0] for p in _PATHS])
def test_one_hot_rows_of_w_pick_the_right_k(name, kernel, slices, shift):
    M, N, K = 300, 768, 512
    with path(kernel, slices=slices) as lib:
        check_one_hot(lib, name, dense(M, K, 9), one_hot(N, K, shift, 10), kernel, slices)


# ----------------------------------------------------------------------------- strides and guard bands
@pytest.mark.parametrize("name,kernel,slices,M,N,K", [("v2", V2, 0, 257, 512, 256), ("v2", V2, 0, 700, 768, 512),
                                                      ("128x128", SMALL, 0, 129, 260, 192), ("split-K", V2, 2, 300, 512, 512)],
                         ids=["v2-257", "v2-700", "128x128", "split-K"])
def test_leading_dimensions_beyond_the_row_and_guard_bands(name, kernel, slices, M, N, K):
    """lda = K + 8, ldw = K + 24 with a pad of 1.0 (read as data it changes every sum), 64 rows of NaN behind A in the same
    allocation, every output with ld = N + 8: sentinel columns and 64 sentinel rows keep their bits, results stay exact"""
    o = operands(M, N, K)
    bias, gate = o["bias"], o["gate"]
    a_whole = torch.full((M + GUARD, K + 8), 1.0, dtype=torch.bfloat16, device=DEV)
    a_whole[M:] = float("nan")
    w_whole = torch.full((N, K + 24), 1.0, dtype=torch.bfloat16, device=DEV)
    a_whole[:M, :K], w_whole[:, :K] = o["a"], o["w"]
    a, w = a_whole[:M, :K], w_whole[:, :K]
    assert (a.stride(0), w.stride(0)) == (K + 8, K + 24)
    ld = N + 8
    tag = f"strided {name} M {M} N {N} K {K}"
    with path(kernel, slices=slices) as lib:
        for epi in (EPI_BF16, EPI_RESID, EPI_CAPTURE):
            assert is_path(lib, M, N, K, epi, kernel, slices)
        if not slices:
            assert is_path(lib, M, N, K, EPI_F32, kernel)
            whole, out = guarded(M, N, torch.float32, SENT_X, ld=ld)
            assert out.stride(0) == ld
            H.gemm(a, w, bias, EPI_F32, X=out)
            exact(out, o["c32"], f"{tag} EPI_F32")
            assert kept(whole, M, N, SENT_X)

        whole, cb = guarded(M, N, torch.bfloat16, SENT_X, ld=ld)
        H.gemm(a, w, bias, EPI_BF16, Cb=cb)
        exact(cb, o["cb"], f"{tag} EPI_BF16")
        assert kept(whole, M, N, SENT_X)

        whole, x = guarded(M, N, torch.float32, SENT_X, o["x"], ld=ld)
        H.gemm(a, w, bias, EPI_RESID, X=x, gate=gate)
        exact(x, o["x_gate"], f"{tag} EPI_RESID_GATE")
        assert kept(whole, M, N, SENT_X)

        xw, x = guarded(M, N, torch.float32, SENT_X, o["x"], ld=ld)
        rw, r = guarded(M, N, torch.float32, SENT_R, ld=ld)
        _, x0 = guarded(M, N, torch.bfloat16, 1e30, o["x0"], ld=ld)
        H.gemm(a, w, bias, EPI_CAPTURE, X=x, gate=gate, X0=x0, R=r)
        exact(x, o["x_gate"], f"{tag} EPI_RESID_CAPTURE X")
        exact(r, x - o["x0"].float(), f"{tag} EPI_RESID_CAPTURE R")
        assert kept(xw, M, N, SENT_X) and kept(rw, M, N, SENT_R)


# ----------------------------------------------------------------------------- two Linears as one call
@pytest.mark.parametrize("name,kernel,slices", _PATHS, ids=[p[0] for p in _PATHS])
@pytest.mark.parametrize("M,N,K", MC.BF16_ROWSPLIT_SHAPES)
def test_rowsplit_takes_the_second_linear_from_m_split_on(M, N, K, name, kernel, slices):
    """m_split = 256 is one gemm_bf16_v2 launch at K = 1024 (under split-K: one partial launch and the reduce kernel choosing
    bias_b / gate_b per tile), two launches at K = 512; m_split = 200 is two launches everywhere"""
    o = operands(M, N, K)
    for m_split in (256, 200):
        rc = MC.bf16_rowsplit_case(M, N, K, m_split)
        w_b, bias_b, gate_b = rc.w_b.to(DEV), rc.bias_b.to(DEV), rc.gate_b.to(DEV)
        tag = f"rowsplit {name} M {M} N {N} K {K} m_split {m_split}"
        with path(kernel, slices=slices) as lib:
            if m_split == 256 and K >= 1024:                # the one-launch form: the whole problem on the path meant
                assert is_path(lib, M, N, K, EPI_BF16, kernel, slices) and is_path(lib, M, N, K, EPI_RESID, kernel, slices)
            whole, cb = guarded(M, N, torch.bfloat16, SENT_X)
            gemm_rowsplit(o["a"], o["w"], w_b, o["bias"], bias_b, m_split, EPI_BF16, Cb=cb)
            exact(cb, rc.cb.bfloat16().to(DEV), f"{tag} EPI_BF16")
            assert kept(whole, M, N, SENT_X)
            whole, x = guarded(M, N, torch.float32, SENT_X, o["x"])
            gemm_rowsplit(o["a"], o["w"], w_b, o["bias"], bias_b, m_split, EPI_RESID, X=x, gate=o["gate"], gate_b=gate_b)
            exact(x, rc.x_gate.float().to(DEV), f"{tag} EPI_RESID_GATE")
            assert kept(whole, M, N, SENT_X)


@pytest.mark.parametrize("name,kernel,max_grid", [("128x128", SMALL, 0), ("v2", V2, 0), ("v2", V2, 2)], ids=["128x128", "v2", "v2-grid2"])
def test_gelu_split_writes_the_exact_bf16_half_and_the_gelu_half(name, kernel, max_grid):
    """n_split = 256 of N = 768: one launch with two destinations on v2 (the tile's column picks the epilogue, also while a
    workgroup walks tiles of both kinds), two launches on the 128 x 128 kernel; Cb2 strided like the engines' am[:, d:]"""
    M, N, K = 700, 768, 512
    ns = 256
    o = operands(M, N, K)
    with path(kernel, max_grid=max_grid) as lib:
        assert lib.mc_op_gemm_bf16_kernel(M, N, K, EPI_GELU_SPLIT) == kernel
        whole, cb = guarded(M, ns, torch.bfloat16, SENT_X, ld=ns + 8)
        am = torch.full((M + GUARD, N), SENT_X, dtype=torch.bfloat16, device=DEV)
        cb2 = am[:M, ns:]
        gemm_gelu_split(o["a"], o["w"], o["bias"], ns, cb, cb2)
        exact(cb, o["cb"][:, :ns], f"gelu split {name} bf16 half")
        check_activation(f"gelu split {name}", EPI_GELU, cb2, o["cb"][:, ns:])
        assert kept(whole, M, ns, SENT_X)
        assert bool((am[:M, :ns] == SENT_X).all()) and bool((am[M:] == SENT_X).all())
        # ... and the GELU half holds the bits the plain GELU launch gives
        cg = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
        H.gemm(o["a"], o["w"], o["bias"], EPI_GELU, Cb=cg)
        exact(cb2, cg[:, ns:], f"gelu split {name} GELU half against EPI_GELU_BF16")


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,kernel,slices", _PATHS, ids=[p[0] for p in _PATHS])
def test_refusals_leave_the_outputs_alone(name, kernel, slices):
    """what gemm_bf16_args_ok (ops.h) and the entry points refuse, on every forced path: MC_EINVAL on the host, nothing launched,
    the sentinels of every output intact; then the unmodified call runs"""
    M, N, K = MC.BF16_COMMON_SHAPE
    o = operands(M, N, K)
    ptr = lambda t: t.data_ptr()        # noqa: E731
    a_room = torch.zeros(M + 1, K, dtype=torch.bfloat16, device=DEV)          # room for the pointers 8 bytes off
    w_room = torch.zeros(N + 1, K, dtype=torch.bfloat16, device=DEV)
    cb = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
    cb2 = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
    x0out = torch.full((M, N), SENT_X, dtype=torch.bfloat16, device=DEV)
    x = torch.full((M, N), SENT_X, device=DEV)
    r = torch.full((M, N), SENT_R, device=DEV)
    base = dict(A=ptr(o["a"]), lda=K, W=ptr(o["w"]), ldw=K, bias=ptr(o["bias"]), M=M, N=N, K=K, epi=EPI_BF16, Cb=ptr(cb), ldc=N,
                X=ptr(x), ldx=N, gate=ptr(o["gate"]), X0=ptr(o["x0"]), ldx0=N, R=ptr(r), ldr=N, X0out=ptr(x0out), ldx0out=N, m_valid=M)
    order = ("A", "lda", "W", "ldw", "bias", "M", "N", "K", "epi", "Cb", "ldc", "X", "ldx", "gate", "X0", "ldx0", "R", "ldr", "X0out",
             "ldx0out", "m_valid")

    def plain(lib, **kw):
        v = dict(base, **kw)
        args = [C.c_void_p(v[k]) if k in ("A", "W", "bias", "Cb", "X", "gate", "X0", "R", "X0out") else v[k] for k in order]
        return lib.mc_op_gemm_bf16(*args, H.S())

    cases = {
        "M = 0": dict(M=0), "M < 0": dict(M=-1), "N = 0": dict(N=0), "N % 4": dict(N=N - 2), "K = 0": dict(K=0), "K % 64": dict(K=K - 32),
        "lda % 8": dict(lda=K + 4), "ldw % 8": dict(ldw=K + 4), "lda < K": dict(lda=K - 8), "ldw < K": dict(ldw=K - 8),
        "A NULL": dict(A=None), "W NULL": dict(W=None), "A off 16 bytes": dict(A=ptr(a_room) + 8), "W off 16 bytes": dict(W=ptr(w_room) + 8),
        "ldc < N": dict(ldc=N - 4), "ldx < N": dict(epi=EPI_F32, ldx=N - 4), "ldx < N (residual)": dict(epi=EPI_RESID, ldx=N - 4),
        "ldx0 < N": dict(epi=EPI_CAPTURE, ldx0=N - 4), "ldr < N": dict(epi=EPI_CAPTURE, ldr=N - 4),
        "ldx0out < N": dict(epi=EPI_EMBED, ldx0out=N - 4),
        "ldc % 4": dict(ldc=N + 2), "ldx % 4": dict(epi=EPI_RESID, ldx=N + 2), "ldx % 4 (fp32 store)": dict(epi=EPI_F32, ldx=N + 2),
        "ldr % 4": dict(epi=EPI_CAPTURE, ldr=N + 2), "ldx0 % 4": dict(epi=EPI_CAPTURE, ldx0=N + 2),
        "Cb off 8 bytes": dict(Cb=ptr(cb) + 4), "X off 16 bytes": dict(epi=EPI_RESID, X=ptr(x) + 8),
        "bias off 16 bytes": dict(bias=ptr(o["bias"]) + 8), "gate off 16 bytes": dict(epi=EPI_RESID, gate=ptr(o["gate"]) + 8),
        "bf16 without Cb": dict(Cb=None), "GELU without Cb": dict(epi=EPI_GELU, Cb=None), "erf-GELU without Cb": dict(epi=EPI_GELU_ERF, Cb=None),
        "residual without X": dict(epi=EPI_RESID, X=None), "fp32 store without X": dict(epi=EPI_F32, X=None),
        "capture without X0": dict(epi=EPI_CAPTURE, X0=None), "capture without R": dict(epi=EPI_CAPTURE, R=None),
        "capture without X": dict(epi=EPI_CAPTURE, X=None), "embed without X0out": dict(epi=EPI_EMBED, X0out=None),
        "embed without X": dict(epi=EPI_EMBED, X=None),
        "epilogue 99": dict(epi=99), "EPI_SPLITK_PARTIAL": dict(epi=9), "EPI_GELU_MXFP8": dict(epi=8), "EPI_RESID_GATE_SEL": dict(epi=11),
        "EPI_GELU_SPLIT without a split": dict(epi=EPI_GELU_SPLIT), "epilogue -1": dict(epi=-1),
    }
    P_ = H.P
    a, w, bias, gate = o["a"], o["w"], o["bias"], o["gate"]
    with path(kernel, slices=slices) as lib:
        for epi in (EPI_BF16, EPI_RESID):
            assert is_path(lib, M, N, K, epi, kernel, slices)
        for what, kw in cases.items():
            assert plain(lib, **kw) == _lib.MC_EINVAL, what
        rowsplit = {"m_split = M": (M, P_(w), EPI_BF16), "m_split > M": (M + 1, P_(w), EPI_BF16), "W_b NULL": (256, None, EPI_BF16),
                    "W_b NULL (residual)": (256, None, EPI_RESID), "rowsplit with the fp32 store": (256, P_(w), EPI_F32)}
        for what, (ms, wb, epi) in rowsplit.items():
            st = lib.mc_op_gemm_bf16_rowsplit(P_(a), K, P_(w), wb, K, P_(bias), P_(bias), M, N, K, ms, epi, P_(cb), N, P_(x), N, P_(gate),
                                              P_(gate), H.S())
            assert st == _lib.MC_EINVAL, what
        for what, (ns, c2) in {"n_split = 0": (0, P_(cb2)), "n_split = N": (N, P_(cb2)), "n_split = 6": (6, P_(cb2)),
                               "Cb2 NULL": (256, None)}.items():
            st = lib.mc_op_gemm_bf16_gelu_split(P_(a), K, P_(w), K, P_(bias), M, N, K, ns, P_(cb), N, c2, N, H.S())
            assert st == _lib.MC_EINVAL, what
        st = lib.mc_op_gemm_bf16_resid_sel(P_(a), K, P_(w), K, P_(bias), M, N, K, 0, P_(x), N, P_(gate), None, P_(o["sel"]), None, 0,
                                           None, 0, H.S())
        assert st == _lib.MC_EINVAL, "resid_sel without gate2"
        torch.cuda.synchronize()
        for t, fill in ((cb, SENT_X), (cb2, SENT_X), (x0out, SENT_X), (x, SENT_X), (r, SENT_R)):
            assert bool((t == fill).all())
        assert plain(lib) == _lib.MC_OK                                       # the unmodified call runs
        exact(cb, o["cb"], f"refusals {name}: the plain call afterwards")

"""Test-side helpers for the table forms of an engine with token_timestep_sets: ctypes signatures and torch wrappers of the
mc_test_* entry points csrc/test_ops.cpp adds for them (reference library only, as hip_ops.T's), and of the shipped
mc_op_gemm_bf16_resid_sets."""
import ctypes as C

import torch

import hip_ops as H
from hip_ops import P, S

_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
SIGNATURES = {
    "mc_test_token_t_sets": [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "mc_test_sinusoid_rows": [_vp, _i, _i, _vp, _l, _vp],
    "mc_test_gemv_f32_rows": [_vp, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i, _i, _vp],
    "mc_test_add_bcast_rows": [_vp, _l, _i, _i, _vp, _i, _i, _vp, _l, _vp],
    "mc_test_ln_modulate_sets": [_vp, _l, _vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _l, _i, _i, _vp, _l, _i, _vp],
    "mc_test_ln_modulate_fp8_sets": [_vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _vp, _l, _i, _i, _vp, _l, _i, _vp],
    "mc_test_ln_modulate_mxfp4_sets": [_vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _l, _i, _i, _vp, _l, _i, _vp],
    "mc_test_ln_modulate_mxfp4": [_vp, _l, _vp, _vp, _i, _f, _vp, _l, _vp, _l, _i, _i, _vp, _vp, _vp, _vp],
    "mc_test_gemm_mxfp8_resid_rows": [_vp, _l, _vp, _l, _vp, _l, _vp, _l, _vp, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _l, _i, _vp],
}
_bound = False


def TS(name, *args):
    """call mc_test_<name> of the reference library; a non-zero hipError_t raises hip_ops.HipStatusError"""
    global _bound
    lib = H.ref_lib()
    if not _bound:
        for n, argtypes in SIGNATURES.items():
            fn = getattr(lib, n)
            fn.restype, fn.argtypes = C.c_int, argtypes
        _bound = True
    status = getattr(lib, "mc_test_" + name)(*args)
    if status != 0:
        raise H.HipStatusError(name, status)


def token_t_sets(t, row0, n_rows, n_rows_pad, cap, n_all=None):
    """-> (t2 fp32 [4], vals fp32 [cap], sel uint8 [n_rows_pad]) on the device; sel starts as 0xEE, vals / t2 as -7"""
    n_all = t.numel() if n_all is None else n_all
    t2 = torch.full((4,), -7.0, device=t.device)
    vals = torch.full((cap,), -7.0, device=t.device)
    sel = torch.full((n_rows_pad,), 0xEE, dtype=torch.uint8, device=t.device)
    TS("token_t_sets", P(t), n_all, row0, n_rows, n_rows_pad, cap, P(t2), P(vals), P(sel), S())
    return t2, vals, sel


def sinusoid_rows(t, dim, out):
    TS("sinusoid_rows", P(t), t.numel(), dim, P(out), out.stride(0), S())


def gemv_f32_rows(W, x, b, y, act_in=0, act_out=0):
    TS("gemv_f32_rows", P(W), P(x), x.stride(0), P(b), P(y), y.stride(0), x.shape[0], W.shape[0], W.shape[1], act_in, act_out, S())


def add_bcast_rows(a, na, bs, n, out):
    """a [R, >= na] fp32, bs: list of fp32 vectors of n elements, out [R, len(bs) * n]"""
    ptrs = (C.c_void_p * len(bs))(*[b.data_ptr() for b in bs])
    TS("add_bcast_rows", P(a), a.stride(0), a.shape[0], na, ptrs, len(bs), n, P(out), out.stride(0), S())


def ln_modulate_sets(x, sc, sh, mode, eps, sel, set_stride, n_sets, out_bf16=None, out_f32=None, x0=None):
    TS("ln_modulate_sets", P(x), x.stride(0), P(x0), H._ld(x0), P(sc), P(sh), mode, eps, P(out_bf16), H._ld(out_bf16),
       P(out_f32), H._ld(out_f32), x.shape[0], x.shape[1], P(sel), set_stride, n_sets, S())


def ln_modulate_fp8_sets(x, sc, sh, mode, eps, mx, sel, set_stride, n_sets):
    """as hip_ops.ln_modulate_fp8, the table form"""
    M, D = x.shape
    q = torch.full((M, D), 0x55, dtype=torch.uint8, device=x.device)
    if mx:
        rows_pad = (M + 255) // 256 * 256
        s = torch.full((D // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
        TS("ln_modulate_fp8_sets", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), None, P(s), rows_pad, M, D,
           P(sel), set_stride, n_sets, S())
    else:
        s = torch.full((M,), -1.0, dtype=torch.float32, device=x.device)
        TS("ln_modulate_fp8_sets", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), P(s), None, 0, M, D,
           P(sel), set_stride, n_sets, S())
    return q, s


def ln_modulate_mxfp4(x, sc, sh, mode, eps, sel=None, set_stride=0, n_sets=0):
    """-> (packed e2m1 codes uint8 [M, D / 2], E8M0 scales uint8 [D / 32, rows_pad]); set_stride 0: the single-set launch"""
    M, D = x.shape
    rows_pad = (M + 255) // 256 * 256
    q = torch.full((M, D // 2), 0x55, dtype=torch.uint8, device=x.device)
    s = torch.full((D // 32, rows_pad), 127, dtype=torch.uint8, device=x.device)
    if set_stride:
        TS("ln_modulate_mxfp4_sets", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), P(s), rows_pad, M, D, P(sel),
           set_stride, n_sets, S())
    else:
        TS("ln_modulate_mxfp4", P(x), x.stride(0), P(sc), P(sh), mode, eps, P(q), q.stride(0), P(s), rows_pad, M, D, None, None,
           None, S())
    return q, s


def gemm_resid_sets(lib, A, W, bias, X, gates, gate_stride, n_sets, sel, X0=None, R=None, M=None, N=None):
    """mc_op_gemm_bf16_resid_sets of `lib`; returns the status (0 = MC_OK)"""
    M = A.shape[0] if M is None else M
    N = W.shape[0] if N is None else N
    return lib.mc_op_gemm_bf16_resid_sets(P(A), A.stride(0), P(W), W.stride(0), P(bias), M, N, A.shape[1], 1 if R is not None else 0,
                                          P(X), X.stride(0), P(gates), gate_stride, n_sets, P(sel), P(X0), H._ld(X0), P(R),
                                          H._ld(R), S())


def gemm_mxfp8_resid_rows(Aq, sa, Wq, sw, bias, X, gate, gate2, sel, gate_stride=0, n_sets=0):
    M, K = Aq.shape
    TS("gemm_mxfp8_resid_rows", P(Aq), Aq.stride(0), P(sa), sa.shape[1], P(Wq), Wq.stride(0), P(sw), sw.shape[1], P(bias), M,
       Wq.shape[0], K, P(X), X.stride(0), P(gate), P(gate2), P(sel), gate_stride, n_sets, S())

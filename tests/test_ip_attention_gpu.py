"""The IP-Adapter cross-attention kernel alone (mc_op_ip_attention, csrc/ip_attention.hip):
    out[m, head] = sum_j scale_j softmax(q_n[m, head] K_j[head]^T / sqrt(128)) V_j[head]
with q_n the per-head RMS-normalised q the kernel forms itself from the raw q columns of a q|k|v buffer.  Every operand sits
inside a poisoned allocation with a leading dimension larger than its width; the pad rows of every K|V cache hold NaN."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402

import hip_ops as H  # noqa: E402
from hip_ops import P, S  # noqa: E402

DEV = "cuda:0"
EPS = 1e-6
U8 = 2.0 ** -8


def qkv_buffer(rows, heads, gen, scale=1.0):
    """(buffer, q view): a [rows + 2, 3 d + 8] bf16 allocation of random numbers; q = rows [1, 1 + rows), columns [0, d)"""
    d = heads * 128
    buf = (torch.randn(rows + 2, 3 * d + 8, generator=gen, device=DEV) * scale).bfloat16()
    return buf, buf[1:1 + rows, :d]


def cache(keys, heads, gen, k=None, v=None):
    """[K | V] rows of one adapter: [round up to 32 of keys + 1, 2 d + 8] bf16, everything that is no key or value NaN"""
    d = heads * 128
    buf = torch.full(((keys + 31) // 32 * 32 + 1, 2 * d + 8), float("nan"), device=DEV).bfloat16()
    buf[:keys, :d] = (torch.randn(keys, d, generator=gen, device=DEV) if k is None else k).bfloat16()
    buf[:keys, d:2 * d] = (torch.randn(keys, d, generator=gen, device=DEV) if v is None else v).bfloat16()
    return buf


def launch(q, wq, adapters, out, rows, heads, ldq=None, ldo=None):
    """adapters: (cache, keys, scale) or (pointer, ld, keys, scale)"""
    arr = (_lib.McIpKeys * max(len(adapters), 1))()
    for j, a in enumerate(adapters):
        if len(a) == 3:
            arr[j] = _lib.McIpKeys(a[0].data_ptr(), a[0].stride(0), a[1], a[2])
        else:
            arr[j] = _lib.McIpKeys(*a)
    return _lib.load().mc_op_ip_attention(P(q), q.stride(0) if ldq is None else ldq, P(wq), EPS, arr, len(adapters), P(out),
                                          out.stride(0) if ldo is None else ldo, rows, heads, S())


def out_buffer(rows, heads):
    d = heads * 128
    buf = torch.full((rows + 2, d + 8), -7.0, device=DEV).bfloat16()
    return buf, buf[1:1 + rows, :d]


def run(q, wq, adapters, rows, heads):
    obuf, out = out_buffer(rows, heads)
    st = launch(q, wq, adapters, out, rows, heads)
    assert st == _lib.MC_OK, _lib.load().mc_last_error()
    torch.cuda.synchronize()
    guard = obuf.clone()
    guard[1:1 + rows, :heads * 128] = -7.0
    assert bool((guard == -7.0).all()), "rows outside the range or columns past d were written"
    return out.clone()


def head_norm(q, wq, heads):
    """q_n as the engine's head norm kernel leaves it without a RoPE table (mc_test_headnorm_rope on a copy)"""
    d = heads * 128
    x = torch.zeros(q.shape[0], 2 * d, device=DEV, dtype=torch.bfloat16)
    x[:, :d] = q
    H.headnorm_rope(x, d, wq, wq, EPS, None, 0, heads)
    return x[:, :d].clone()


# ----------------------------------------------------------------------------- equal scores
@pytest.mark.parametrize("keys", [1, 4, 5, 16, 31, 32, 33, 64, 127, 128, 129, 255, 256])
def test_equal_scores_weigh_every_key_once(keys):
    """K = 0: every valid key has weight 1 / keys.  V[j, c] = (c == j) makes column j the weight of key j: 1 / keys within
    2^-8 for j < keys, exactly 0 behind them -- a key counted twice, a pad key counted or a NaN of the pad rows would show."""
    g = torch.Generator(device=DEV).manual_seed(keys)
    wq = torch.ones(128, device=DEV)
    v = torch.zeros(keys, 128, device=DEV)
    n = min(keys, 128)
    v[torch.arange(n), torch.arange(n)] = 1.0
    kv = cache(keys, 1, g, k=torch.zeros(keys, 128, device=DEV), v=v)
    for rows in (1, 63, 65, 257):
        _, q = qkv_buffer(rows, 1, g)
        out = run(q, wq, [(kv, keys, 1.0)], rows, 1).float()
        assert bool(torch.isfinite(out).all())
        assert float((out[:, :n] * keys - 1).abs().max()) <= U8, (keys, rows)
        assert bool((out[:, n:] == 0).all()), (keys, rows)


# ----------------------------------------------------------------------------- one key
def test_one_key_returns_its_value_row_bitwise():
    g = torch.Generator(device=DEV).manual_seed(3)
    heads, rows = 2, 70
    d = heads * 128
    wq = torch.rand(128, generator=g, device=DEV) + 0.5
    buf, q = qkv_buffer(rows, heads, g)
    # K = 25 sign(q row 0): the raw score of row 0 is about +200 / head, that of row 1 (= -row 0) about -200
    buf[2, :d] = -buf[1, :d]
    k = 25.0 * torch.sign(q[0].float())[None]
    kv = cache(1, heads, g, k=k)
    qn = head_norm(q, wq, heads).double()
    raw = (qn.view(rows, heads, 128) * kv[0, :d].double().view(1, heads, 128)).sum(-1) / math.sqrt(128)
    assert float(raw.max()) > 200 and float(raw.min()) < -200
    v = kv[0, d:2 * d]
    out = run(q, wq, [(kv, 1, 1.0)], rows, heads)
    assert torch.equal(out, v[None].expand(rows, d))
    s = 0.3
    out = run(q, wq, [(kv, 1, s)], rows, heads)
    want = (v.float() * torch.tensor(s, dtype=torch.float32, device=DEV)).bfloat16()
    assert torch.equal(out, want[None].expand(rows, d))


# ----------------------------------------------------------------------------- score spike
def test_score_spike_selects_that_key_at_every_tile_edge():
    """one key 60 above all others: q_n = 1 (q = 1, weight 1), K = 0 but the spike's row of sixes (128 * 6 / sqrt(128) = 67.9)"""
    g = torch.Generator(device=DEV).manual_seed(5)
    keys, rows = 256, 33
    wq = torch.ones(128, device=DEV)
    q = torch.ones(rows, 128, device=DEV).bfloat16()
    v = torch.randn(keys, 128, generator=g, device=DEV).bfloat16()
    for tile in range(8):
        for pos in (32 * tile, 32 * tile + 31):
            k = torch.zeros(keys, 128, device=DEV)
            k[pos] = 6.0
            kv = cache(keys, 1, g, k=k, v=v)
            out = run(q, wq, [(kv, keys, 1.0)], rows, 1).float()
            want = v[pos].float()[None]
            assert bool(((out - want).abs() <= U8 * want.abs()).all()), pos


# ----------------------------------------------------------------------------- general case
def reference(qn, adapters, heads):
    """float64, from the same bf16 q_n, K and V; returns (out, elementwise bound)"""
    rows, d = qn.shape
    out = torch.zeros(rows, heads, 128, dtype=torch.float64, device=DEV)
    bound = torch.zeros(heads, 128, dtype=torch.float64, device=DEV)
    qh = qn.double().view(rows, heads, 128)
    for kv, keys, scale in adapters:
        if scale == 0:
            continue
        k = kv[:keys, :d].double().view(keys, heads, 128)
        v = kv[:keys, d:2 * d].double().view(keys, heads, 128)
        p = torch.softmax(torch.einsum("rhc,khc->rhk", qh, k) / math.sqrt(128), dim=-1)
        out += scale * torch.einsum("rhk,khc->rhc", p, v)
        bound += abs(scale) * v.abs().amax(0)
    return out.view(rows, d), (2.0 ** -7 * bound).view(1, d)


@pytest.mark.parametrize("n_adapters", [1, 2, 4])
@pytest.mark.parametrize("heads", [1, 2, 3, 24])
def test_general_case_against_float64(heads, n_adapters):
    """|out - ref| <= 2^-7 sum_j |scale_j| max_k |V_j[k, c]|: twice the derived 2^-8 (P rounded to bf16 in front of P V and
    the final rounding, 2^-9 each on a convex combination of the values; the fp32 score and softmax error is far below)."""
    g = torch.Generator(device=DEV).manual_seed(heads * 10 + n_adapters)
    rows = 65 if heads == 24 else 161
    wq = torch.rand(128, generator=g, device=DEV) + 0.5
    buf, q = qkv_buffer(rows, heads, g, scale=3.0)
    before = buf.clone()
    keys = [37, 4, 256, 100][:n_adapters]
    scales = [0.7, 0.0, -1.3, 0.5][:n_adapters]
    adapters = [(cache(k, heads, g), k, s) for k, s in zip(keys, scales)]
    out = run(q, wq, adapters, rows, heads)
    assert torch.equal(buf, before), "the q, k or v columns were written"
    ref, bound = reference(head_norm(q, wq, heads), adapters, heads)
    err = (out.double() - ref).abs()
    print("heads %d, %d adapters: max error / bound = %.3f" % (heads, n_adapters, float((err / bound).max())))
    assert bool((err <= bound).all())
    if n_adapters > 1:   # the adapter with scale 0 is left out: bitwise the launch without it
        live = [a for a in adapters if a[2] != 0]
        assert torch.equal(out, run(q, wq, live, rows, heads))


# ----------------------------------------------------------------------------- agreement with the head norm
@pytest.mark.parametrize("heads,rows", [(1, 1), (2, 77), (24, 130)])
def test_normalised_q_is_the_head_norm_kernels_bitwise(heads, rows):
    """the q_n the attention uses (the kernel stopped after its first step: mc_test_ip_qnorm of the test library) equals
    launch_headnorm_rope without a table bit for bit, on rows of very different magnitude"""
    g = torch.Generator(device=DEV).manual_seed(heads + rows)
    d = heads * 128
    wq = torch.randn(128, generator=g, device=DEV)
    buf, q = qkv_buffer(rows, heads, g)
    q *= (10.0 ** torch.randint(-3, 4, (rows, 1), generator=g, device=DEV).float()).bfloat16()
    lib = H.ref_lib()
    fn = lib.mc_test_ip_qnorm
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_float, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    obuf, out = out_buffer(rows, heads)
    assert fn(P(q), q.stride(0), P(wq), EPS, P(out), out.stride(0), rows, heads, S()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, head_norm(q, wq, heads))


# ----------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    g = torch.Generator(device=DEV).manual_seed(9)
    heads, rows = 1, 8
    wq = torch.ones(128, device=DEV)
    _, q = qkv_buffer(rows, heads, g)
    kv = cache(256, heads, g)
    obuf, out = out_buffer(rows, heads)
    ok = (kv, 4, 1.0)
    bad = [
        dict(adapters=[(kv, 0, 1.0)]), dict(adapters=[(kv, 257, 1.0)]), dict(adapters=[ok] * 5), dict(adapters=[]),
        dict(adapters=[(kv.data_ptr() + 4, kv.stride(0), 4, 1.0)]), dict(adapters=[(kv.data_ptr() + 8, kv.stride(0), 4, 1.0)]),
        dict(adapters=[(kv.data_ptr(), kv.stride(0) + 1, 4, 1.0)]), dict(adapters=[(kv.data_ptr(), 128, 4, 1.0)]),
        dict(adapters=[ok], ldq=q.stride(0) + 1), dict(adapters=[ok], ldo=out.stride(0) + 1), dict(adapters=[ok], rows=0),
    ]
    for b in bad:
        st = launch(q, wq, b["adapters"], out, b.get("rows", rows), heads, ldq=b.get("ldq"), ldo=b.get("ldo"))
        assert st == _lib.MC_EINVAL, b
    lib = _lib.load()
    arr = (_lib.McIpKeys * 1)(_lib.McIpKeys(kv.data_ptr(), kv.stride(0), 4, 1.0))
    for dq, dw, do in ((4, 0, 0), (8, 0, 0), (0, 4, 0), (0, 0, 4), (0, 0, 8)):
        st = lib.mc_op_ip_attention(C.c_void_p(q.data_ptr() + dq), q.stride(0), C.c_void_p(wq.data_ptr() + dw), EPS, arr, 1,
                                    C.c_void_p(out.data_ptr() + do), out.stride(0), rows, heads, S())
        assert st == _lib.MC_EINVAL, (dq, dw, do)
    assert b"ip_attention" in lib.mc_last_error()
    torch.cuda.synchronize()
    assert bool((obuf == -7.0).all())                      # nothing ran
    assert launch(q, wq, [ok], out, rows, heads) == _lib.MC_OK

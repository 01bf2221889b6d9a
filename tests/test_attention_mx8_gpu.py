"""GPU: the opt-in MX fp8 self-attention (csrc/attention_mx8.hip; option "attn_mx8") against tests/attention_mx8_ref.py: the pre-pass's
images bit for bit; every key once, in its own slot; spikes across tiles; random operands against the torch model of the kernel
(the format's own cost is printed); refusals; the Wan engine under the option."""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import attention_mx8_ref as R  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
NAMES = ("q", "qs", "k", "ks", "vt", "vs")
GUARD, POISON = 256, 0xA5
VALID = [1, 63, 64, 65, 129, 300]


def prepass(q, k, v, heads, rows, valid):
    """launch the pre-pass on device views q [Lq, d], k, v [>= rows, d]; returns the images as guarded device buffers"""
    Lq, d = q.shape[0], heads * A.HD
    size = {"q": Lq * d, "qs": Lq * d // 32, "k": rows * d, "ks": rows * d // 32, "vt": rows * d, "vs": rows * d // 32}
    buf = {n: torch.full((size[n] + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV) for n in NAMES}
    im = {n: buf[n][GUARD:GUARD + size[n]] for n in NAMES}
    _lib.check(H.L().mc_op_attn_quantize_mx8(H.P(q), q.stride(0), H.P(k), k.stride(0), H.P(v), v.stride(0), Lq, heads, rows, valid,
                                             A.SCALE, *(H.P(im[n]) for n in NAMES), H.S()))
    return buf, im


def attend(im, Lq, heads, rows, valid, o=None, ldo=None, n_shards=1, lse=None):
    o = torch.full((Lq, heads * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV) if o is None else o
    status = H.L().mc_op_attention_mx8(*(H.P(im[n]) for n in NAMES), H.P(o), ldo or o.stride(0), Lq, heads, rows, valid, n_shards,
                                       H.P(lse), H.S())
    return o, status


@functools.lru_cache(maxsize=None)
def every_key(valid, rows):
    """the every-key case in one strided [L, 3d] buffer, k / v padding rows 1000, through the pre-pass: case, guarded buffers, images"""
    c = A.every_key_case(A.every_key_lq(valid, 1), 2, rows, valid, 1, A.SEED)
    Lq, d = c.q.shape
    qkv = torch.zeros(max(Lq, rows), 3 * d, dtype=torch.bfloat16)
    qkv[:Lq, :d], qkv[:rows, d:2 * d], qkv[:rows, 2 * d:] = c.q, c.k, c.v
    qkv[valid:rows, d:] = 1000.0
    g = qkv.to(DEV)
    buf, im = prepass(g[:Lq, :d], g[:, d:2 * d], g[:, 2 * d:], 2, rows, valid)
    return c, qkv, buf, im


@pytest.mark.parametrize("valid", VALID)
def test_prepass_images_bit_for_bit(valid):
    for rows in (A.ceil64(valid), A.ceil64(valid) + 128):
        c, qkv, buf, im = every_key(valid, rows)
        Lq, d = c.q.shape
        want = R.images(qkv[:Lq, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], 2, rows, valid, A.SCALE)
        for n in NAMES:
            assert torch.equal(im[n].cpu(), want[n]), (rows, n, int((im[n].cpu() != want[n]).sum()))
            assert bool((buf[n][:GUARD] == POISON).all()) and bool((buf[n][-GUARD:] == POISON).all()), (rows, n, "guard bytes")


@pytest.mark.parametrize("valid", VALID)
def test_every_key_once_in_its_own_slot(valid):
    for rows in (A.ceil64(valid), A.ceil64(valid) + 128):
        c, _, _, im = every_key(valid, rows)
        Lq = c.q.shape[0]
        o, status = attend(im, Lq, 2, rows, valid)
        assert status == _lib.MC_OK
        A.accept(o, R.ref64(*R.dequantize({n: im[n].cpu() for n in NAMES}, 2, Lq, rows), 2, valid))


@pytest.mark.parametrize("spike_key", A.SPIKE_KEYS)
def test_rescale_across_tiles(spike_key):
    for gap in (30, 130, 300):
        for vs in A.SPIKE_V_SCALES:
            c = A.spike_case(A.SPIKE_L, A.SPIKE_HEADS, A.SPIKE_VALID, spike_key, gap, vs, A.SEED)
            g = c.qkv.to(DEV)
            d = c.heads * A.HD
            _, im = prepass(g[:, :d], g[:, d:2 * d], g[:, 2 * d:], c.heads, A.SPIKE_L, A.SPIKE_VALID)
            o, status = attend(im, A.SPIKE_L, c.heads, A.SPIKE_L, A.SPIKE_VALID)
            assert status == _lib.MC_OK
            qd, kd, vd = R.dequantize({n: im[n].cpu() for n in NAMES}, c.heads, A.SPIKE_L, A.SPIKE_L)
            # check_spike's checks with the dequantised value row and the model of this kernel in the reference's place
            want = SimpleNamespace(v=vd, spike_key=spike_key, v_scale=vs, o_ref=R.model(qd, kd, vd, c.heads, A.SPIKE_VALID))
            A.check_spike(want, o)


@pytest.mark.parametrize("Lq,valid", [(256, 300), (768, 129)])
@pytest.mark.parametrize("heads", [1, 5])
def test_random_operands_against_the_model_of_this_kernel(Lq, valid, heads):
    rows, d = A.ceil64(valid), heads * A.HD
    g = torch.Generator().manual_seed(A.SEED + heads)
    q, k, v = (torch.randn(n, d, generator=g).bfloat16() for n in (Lq, rows, rows))
    _, im = prepass(q.to(DEV), k.to(DEV), v.to(DEV), heads, rows, valid)
    o, status = attend(im, Lq, heads, rows, valid)
    assert status == _lib.MC_OK
    model = R.model(*R.dequantize({n: im[n].cpu() for n in NAMES}, heads, Lq, rows), heads, valid)
    A.accept(o, model)
    exact = A.attn_ref64(q, k, v, heads, torch.arange(valid), A.SCALE)[0]
    cost_mx8 = A.rel_l2(model, exact)
    cost_bf16 = A.rel_l2(A.flash_bf16_model(q, k, v, heads, torch.arange(valid), A.SCALE)[0], exact)
    print(f"rel-L2 from the fp64 reference, Lq {Lq} valid {valid} heads {heads}: MX fp8 model {cost_mx8:.3e}, bf16 model {cost_bf16:.3e}, "
          f"kernel {A.rel_l2(o.cpu(), exact):.3e}")
    assert cost_mx8 > cost_bf16, "the MX fp8 format costs accuracy: a pass at the bf16 distance is the bf16 path"


@pytest.mark.parametrize("what,kw", [("n_shards", dict(n_shards=2)), ("lse", dict(lse=True)), ("Lq_pad", dict(Lq=128)), ("shard_rows", dict(rows=96)),
                                     ("valid", dict(valid=0)), ("ldo", dict(ldo=260))])
def test_refusals_leave_o_alone(what, kw):
    _, _, _, im = every_key(65, 128)
    o = torch.full((256, 264), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(2, 256, device=DEV) if kw.get("lse") else None
    _, status = attend(im, kw.get("Lq", 256), 2, kw.get("rows", 128), kw.get("valid", 65), o=o, ldo=kw.get("ldo", 264),
                       n_shards=kw.get("n_shards", 1), lse=lse)
    assert status == _lib.MC_EINVAL and "attention_mx8" in H.L().mc_last_error().decode()
    assert bool(torch.isnan(o).all()), what


# ------------------------------------------------------------------------------------------------ 6: the engine
GRID = (2, 14, 18)                       # 126 tokens: a masked tail tile
TOY = W.tiny_config(num_layers=2, num_heads=4, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64)
# rel-L2 from the fp32 oracle, MX fp8 attention over bf16 attention, measured on MI355X (profiles/r16/NOTES.md); the bar is twice it, rounded up
MX8_OVER_BF16_MEASURED, MX8_OVER_BF16_BAR = 1.38, 3.0      # 5.198e-3 / 3.767e-3


def test_engine_under_attn_mx8():
    oracle = W.init_synthetic_(W.WanModel(**TOY), seed=0, std=0.05)
    wd = {k: v.to(DEV) for k, v in oracle.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    L = GRID[0] * (GRID[1] // 2) * (GRID[2] // 2)
    lat, ctx, t = torch.randn(16, *GRID, generator=g), torch.randn(21, TOY["text_dim"], generator=g), torch.tensor([500.0])
    oracle.set_fp32_attention(True)
    ref = oracle.forward([lat], t, [ctx], L, autocast=False)[0]

    def forward(**kw):
        e = Engine(TOY, GRID, device=DEV, n_branches=2, calibration=False, **kw)
        e.load_weights(wd)
        return e, e.forward(lat.to(DEV), t.to(DEV), ctx.to(DEV)).float().cpu()
    (plain, o16), (off, o_off), (mx8, o8) = forward(), forward(attn_mx8=False), forward(attn_mx8=True)
    assert plain.attn_mx8 is False and off.attn_mx8 is False and mx8.attn_mx8 is True
    assert H.L().mc_engine_attn_mx8(mx8.h) == 1
    assert torch.equal(o16, o_off), "attn_mx8=False is the engine created without the argument"
    assert bool(torch.isfinite(o8).all()) and not torch.equal(o8, o16)
    e8, e16 = A.rel_l2(o8, ref), A.rel_l2(o16, ref)
    print(f"rel-L2 from the fp32 oracle: attn_mx8 {e8:.3e}, bf16 {e16:.3e}, ratio {e8 / e16:.3f}")
    with pytest.raises(_lib.MagCacheHipError) as ei:
        Engine(TOY, (2, 16, 16), device=DEV, n_branches=2, calibration=False, sp_phases=True, attn_mx8=True)
    assert ei.value.status == _lib.MC_EINVAL and "attn_mx8" in str(ei.value)
    v = C.c_int(-1)
    _lib.check(H.L().mc_get_option(b"attn_mx8", C.byref(v)))
    assert v.value == 0, "a refused create puts the option back"
    assert e8 <= MX8_OVER_BF16_BAR * e16, (e8, e16)

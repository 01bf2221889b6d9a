"""GPU: the Wan engine's opt-in MXFP6 Linears (mc_set_option("mx_fp6", 1) on top of fp8_linear 2 | 3; Engine(..., mx_fp6=True)),
on the toy widths of tests/test_wan_mxfp4_gpu.py (dim 512 / ffn 512; dim 1280 / ffn 768).

  1. the option is latched by mc_create: an engine created under it reports mx_fp6 and computes other bits than the MX fp8 and
     the MXFP4 engine; one created after the reset computes the MX fp8 bits exactly; a bf16 engine does not care; "mx_fp4" and
     "mx_fp6" both 1 at create time is MC_EINVAL and the message names both;
  2. the first Linear: after embed + block_pre_attn(0) the engine's q|k|v rows are mc_op_quantize_rows_mxfp6 + mc_op_gemm_mxfp6
     run by hand on the engine's "xn" rows and weights (+ the q / k norm and RoPE ops), bit for bit;
  3. two ranks in one process: q and k|v rows of the row-range launches equal the 1-rank engine's, bit for bit;
  4. LoRA: an engine with adapters equals an engine loaded with the pre-merged weights, bitwise (the touched rows were
     requantised in the engine's format);
  5. a switched grid equals a fresh engine, bitwise;
  6. against the fp32 oracle at toy size the errors are ordered bf16 < {MX fp8, MXFP6} < MXFP4, MXFP6 <= 1.5 x MX fp8 of the
     same run (per GEMM it is <= 1.09 x; the margin is for a two-layer toy), MXFP6 <= 0.5 x MXFP4, and MXFP6 stays below 1.5 x
     its measured relative L2 (profiles/r14/tolerance_probe.json: wan_mxfp6_vs_fp32_oracle; seed 0 weights std 0.05, input
     seed 3, grid 2 x 16 x 16, dim 512, ffn 512, 2 layers)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
import mxfp6_ref as R  # noqa: E402
import test_wan_geometry_gpu as TG  # noqa: E402  (trace / inputs / assert_same of the geometry tests)
import test_wan_lora_gpu as TL  # noqa: E402  (adapters, host-merged weights and the trace of the LoRA tests)
from conftest import tolerance_probe as _probe  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine, synthetic_weights  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
GRID = (2, 16, 16)                       # 128 tokens
TOY = W.tiny_config(num_layers=2, num_heads=4, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64)      # K = 512 everywhere
TOY_ODD = W.tiny_config(num_layers=1, num_heads=10, ffn_dim=768, text_len=64, text_dim=128, freq_dim=64)  # K = 1280 and 768
# measured on MI355X (profiles/r14/tolerance_probe.json: wan_mxfp6_vs_fp32_oracle); the bar is 1.5 x this
MXFP6_REL_L2_MEASURED = 1.98e-2


def bits(t):
    return t.detach().clone().contiguous().view(torch.int32).cpu()


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


def option(value=None, key=b"mx_fp6"):
    lib = _lib.load()
    if value is not None:
        _lib.check(lib.mc_set_option(key, value))
    got = C.c_int(-1)
    _lib.check(lib.mc_get_option(key, C.byref(got)))
    return got.value


def weights(cfg):
    return {n: t for n, t in synthetic_weights(cfg, seed=0, std=0.05, device=DEV)}


def make(cfg, wd, grid=GRID, **kw):
    e = Engine(cfg, grid, device=DEV, n_branches=2, calibration=False, **kw)
    e.load_weights(wd)
    return e


def io(cfg, grid=GRID):
    g = torch.Generator(device=DEV).manual_seed(21)
    return (torch.randn(cfg["in_dim"], *grid, generator=g, device=DEV), torch.randn(40, cfg["text_dim"], generator=g, device=DEV),
            torch.tensor([620.0], device=DEV))


def run(e, cfg, grid=GRID):
    lat, ctx, t = io(cfg, grid)
    out = bits(e.forward(lat, t, ctx))
    assert bool(torch.isfinite(out.view(torch.float32)).all())
    return out


# ------------------------------------------------------------------------------------------------ 1
def test_option_is_latched_by_create_and_both_formats_are_refused():
    lib = _lib.load()
    wd = weights(TOY)
    mx8 = dict(TOY, fp8_linear=2)
    assert option() == 0 and option(key=b"mx_fp4") == 0
    before = make(mx8, wd)
    bf16 = make(TOY, wd)
    assert before.mx_fp6 is False and bf16.mx_fp6 is False
    want8, want16 = run(before, TOY), run(bf16, TOY)
    assert lib.mc_set_option(b"mx_fp6", 2) == _lib.MC_EINVAL and option() == 0
    try:
        assert lib.mc_set_option(b"mx_fp6", 1) == _lib.MC_OK and option() == 1
        under = make(mx8, wd)
        under3 = make(dict(TOY, fp8_linear=3), wd)
        bf16_under = make(TOY, wd)
        rows_under = make(dict(TOY, fp8_linear=1), wd)
        # both element formats at once: refused, whatever fp8_linear says, and the message names both options
        option(1, key=b"mx_fp4")
        for cfg in (mx8, TOY):
            with pytest.raises(_lib.MagCacheHipError) as ei:
                make(cfg, wd)
            assert ei.value.status == _lib.MC_EINVAL and "mx_fp4" in str(ei.value) and "mx_fp6" in str(ei.value)
    finally:
        option(0)
        option(0, key=b"mx_fp4")
    after = make(mx8, wd)
    assert under.mx_fp6 is True and under3.mx_fp6 is True and under.mx_fp4 is False
    assert bf16_under.mx_fp6 is False and rows_under.mx_fp6 is False and after.mx_fp6 is False
    got6 = run(under, TOY)                      # runs after the reset: the engine kept what it read
    assert not torch.equal(got6, want8) and not torch.equal(got6, want16)
    assert not torch.equal(run(under3, TOY), got6)
    assert torch.equal(run(after, TOY), want8), "an engine created after the reset must be the MX fp8 engine"
    assert torch.equal(run(before, TOY), want8)
    assert torch.equal(run(bf16_under, TOY), want16), "the option must do nothing to a bf16 engine"
    # the Python switch: set around the create call only, the previous value put back; a config key does the same
    kw = make(mx8, wd, mx_fp6=True)
    key = make(dict(mx8, mx_fp6=True), wd)
    assert option() == 0 and kw.mx_fp6 is True and key.mx_fp6 is True and kw.mx_fp4 is False
    assert torch.equal(run(kw, TOY), got6) and torch.equal(run(key, TOY), got6)
    assert make(TOY, wd, mx_fp6=True).mx_fp6 is False
    with pytest.raises(_lib.MagCacheHipError):
        make(mx8, wd, mx_fp4=True, mx_fp6=True)
    assert option() == 0 and option(key=b"mx_fp4") == 0, "a refused create puts both options back"
    got4 = run(make(mx8, wd, mx_fp4=True), TOY)
    assert not torch.equal(got4, got6)
    f6, f4, f8, f16 = (x.view(torch.float32) for x in (got6, got4, want8, want16))
    e6, e4, e8 = rel_l2(f6, f16), rel_l2(f4, f16), rel_l2(f8, f16)
    print(f"toy forward vs the bf16 engine: MX fp8 {e8:.3e}, MXFP6 {e6:.3e}, MXFP4 {e4:.3e}")
    assert e6 < e4 and e6 < 2 * e8


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("cfg", [dict(TOY, fp8_linear=2), dict(TOY_ODD, fp8_linear=3)], ids=["k512", "k1280"])
def test_first_linear_equals_the_single_ops_by_hand(cfg):
    wd = weights(cfg)
    e = make(cfg, wd, mx_fp6=True)
    assert e.mx_fp6
    lat, ctx, t = io(cfg)
    d = cfg["dim"]
    L = GRID[0] * (GRID[1] // 2) * (GRID[2] // 2)
    e.embed(lat, t, ctx)
    e.block_pre_attn(0)
    torch.cuda.synchronize()
    xn = e.buffer("xn", torch.bfloat16).view(-1, d)
    Lp = xn.shape[0]
    got = e.buffer("qkv", torch.bfloat16)[:Lp * 3 * d].view(Lp, 3 * d)
    p = "blocks.0.self_attn."
    w = torch.cat([wd[p + n + ".weight"] for n in "qkv"]).to(torch.bfloat16).contiguous()
    b = torch.cat([wd[p + n + ".bias"] for n in "qkv"]).float().contiguous()
    aq, sa = R.op_quantize(xn.contiguous())
    wq, sw = R.op_quantize(w, rows_pad=3 * d)
    want = torch.zeros(Lp, 3 * d, dtype=torch.bfloat16, device=DEV)
    R.op_gemm(aq, sa, wq, sw, b, 0, Cb=want)
    assert torch.equal(got[:L, 2 * d:].contiguous().view(torch.int16), want[:L, 2 * d:].contiguous().view(torch.int16)), "v rows"
    cs = H.rope_table(GRID[0], GRID[1] // 2, GRID[2] // 2, 0, Lp).to(DEV)
    H.rmsnorm_rope(want, wd[p + "norm_q.weight"].float().contiguous(), cfg["eps"], cs, D=d)
    H.rmsnorm_rope(want[:, d:], wd[p + "norm_k.weight"].float().contiguous(), cfg["eps"], cs, D=d)
    assert torch.equal(got[:L].contiguous().view(torch.int16), want[:L].contiguous().view(torch.int16)), "q|k|v rows"
    assert float(got[:L].float().abs().max()) > 0
    # and the engine's operands are the ops' bits: packed rows of 3 d / 4 bytes
    kb = d // 4 * 3
    assert torch.equal(e.buffer("aq")[:Lp * kb].view(Lp, kb)[:L], aq[:L])
    assert torch.equal(R.unpack(aq[:L]), R.quantize(xn[:L])[0])


# ------------------------------------------------------------------------------------------------ 3
def test_two_ranks_in_one_process_equal_the_one_rank_engine():
    cfg = dict(TOY, fp8_linear=2)
    grid = (2, 32, 32)                          # 512 tokens -> 256 per rank
    L = 512
    d = cfg["dim"]
    wd = weights(cfg)
    lat, ctx, t = io(cfg, grid)
    eng = []
    for r in range(2):
        e = Engine(cfg, grid, device=DEV, sp_rank=r, sp_size=2, n_branches=1, calibration=False, mx_fp6=True)
        e.load_weights(wd)
        e.sp_set_chunks(2)
        assert e.mx_fp6
        eng.append(e)
    one = Engine(cfg, grid, device=DEV, n_branches=1, calibration=False, mx_fp6=True)
    one.load_weights(wd)
    one.embed(lat, t, ctx)
    one.block_pre_attn(0)
    qkv1 = one.buffer("qkv", torch.bfloat16)[:L * 3 * d].view(L, 3 * d)
    for r, e in enumerate(eng):
        e.embed(lat, t, ctx)
        e.block_pre_attn(0)
        rows = slice(r * (L // 2), (r + 1) * (L // 2))
        q_sp = e.buffer("qkv", torch.bfloat16)[:(L // 2) * d].view(-1, d)
        kvl = e.buffer("kv_local", torch.bfloat16).view(-1, 2 * d)[:L // 2]
        assert torch.equal(q_sp.view(torch.int16), qkv1[rows, :d].contiguous().view(torch.int16)), f"q rows of rank {r}"
        assert torch.equal(kvl.contiguous().view(torch.int16), qkv1[rows, d:].contiguous().view(torch.int16)), f"k|v rows of rank {r}"
    assert float(qkv1.float().abs().max()) > 0 and bool(torch.isfinite(qkv1.float()).all())


# ------------------------------------------------------------------------------------------------ 4
def test_lora_equals_premerged_weights_bitwise():
    cfg = dict(TOY, fp8_linear=3, mx_fp6=True)          # the d x d Linears are MXFP6 too: self_attn.o and cross_attn.q / .o pairs
    wd = TL.weights(cfg)
    a, b = TL.two_adapters(wd)
    A = TL.make_engine(cfg, wd)
    assert A.mx_fp6
    plain = TL.trace(A)
    assert TL.load(A, a, "a", 0.8) == [] and TL.load(A, b, "b", -1.3) == []
    got = TL.trace(A)
    B = TL.make_engine(cfg, TL.host_merged(wd, [(a, 0.8), (b, -1.3)]))
    TL.assert_same(got, TL.trace(B), "adapters vs host-merged weights (mx_fp6)")
    assert not torch.equal(got[0], plain[0])
    A.unload_lora()
    TL.assert_same(TL.trace(A), plain, "after unload_lora")


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("g_from,g_to", [(TG.G105, TG.G495), (TG.G495, TG.G105)], ids=lambda g: "x".join(map(str, g)))
def test_switched_grid_equals_a_fresh_engine(g_from, g_to):
    cfg = dict(W.tiny_config(num_heads=4, ffn_dim=512), fp8_linear=2, mx_fp6=True)
    kind = tuple(sorted(cfg.items()))                    # TG.inputs takes a hashable config
    fresh = TG.make_engine(cfg, g_to)
    assert fresh.mx_fp6
    want = TG.trace(fresh, kind, g_to, False)
    e = TG.make_engine(cfg, g_from)
    e.reserve([g_from, g_to])
    lat, ctx, _, _ = TG.inputs(kind, g_from)
    e.set_context(0, ctx[0])
    e.forward(lat, 700.0, None, branch=0)
    torch.cuda.synchronize()
    e.ws.fill_(0xFF)                                     # every byte a NaN: the switch may rely on nothing it finds there
    e.set_geometry(g_to)
    assert e.mx_fp6
    TG.assert_same(TG.trace(e, kind, g_to, False), want, f"mx_fp6 {g_from} -> {g_to}")


# ------------------------------------------------------------------------------------------------ 6
def test_errors_against_the_fp32_oracle_are_ordered_and_bounded():
    oracle = W.init_synthetic_(W.WanModel(**TOY), seed=0, std=0.05)
    wd = {k: v.to(DEV) for k, v in oracle.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    L = GRID[0] * (GRID[1] // 2) * (GRID[2] // 2)
    lat, ctx = torch.randn(16, *GRID, generator=g), torch.randn(21, TOY["text_dim"], generator=g)
    oracle.set_fp32_attention(True)
    ref = oracle.forward([lat], torch.tensor([500.0]), [ctx], L, autocast=False)[0]
    tt = torch.tensor([500.0], device=DEV)
    err = {}
    mx = dict(TOY, fp8_linear=2)
    for name, cfg, kw in (("bf16", TOY, {}), ("mxfp8", mx, {}), ("mxfp6", mx, dict(mx_fp6=True)), ("mxfp4", mx, dict(mx_fp4=True))):
        e = make(cfg, wd, **kw)
        err[name] = rel_l2(e.forward(lat.to(DEV), tt, ctx.to(DEV)), ref)
    print("relative L2 against the fp32 oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    _probe("wan_mxfp6_vs_fp32_oracle", dict(err, weights_seed=0, weights_std=0.05, input_seed=3, grid=list(GRID), dim=TOY["dim"],
                                            ffn_dim=TOY["ffn_dim"], num_layers=TOY["num_layers"]))
    assert err["bf16"] < err["mxfp8"] < err["mxfp4"] and err["bf16"] < err["mxfp6"] < err["mxfp4"], err
    assert err["mxfp6"] <= 1.5 * err["mxfp8"], err
    assert err["mxfp6"] <= 0.5 * err["mxfp4"], err
    assert err["mxfp6"] < 1.5 * MXFP6_REL_L2_MEASURED, err

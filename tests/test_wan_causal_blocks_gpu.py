"""GPU: frame-block causal self-attention on the Wan engine (mc_set_causal_blocks; csrc/attention_band.hip): the whole forward
against oracle/wan_dit_ref with every block's self_attn._attn replaced, on the instance, by a block-masked version of
attention_ref / attention_ref_fp32.  Tiny synthetic model; 63 and 35 tokens per frame (no multiple of 32)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib, model as M  # noqa: E402
from magcache_amd.engine import Engine  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
CFG = W.tiny_config(num_layers=2, num_heads=2, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64)
GRID, GRID2 = (6, 14, 18), (5, 10, 14)          # 6 x 63 = 378 tokens: three blocks of two frames; 5 x 35 = 175: the last block is short
FRAMES = 2


def tokens(grid):
    return grid[0] * (grid[1] // 2) * (grid[2] // 2)


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


def inputs(grid, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(CFG["in_dim"], *grid, generator=g), torch.randn(23, CFG["text_dim"], generator=g), torch.tensor([612.5])


@pytest.fixture(scope="module")
def oracle():
    return W.init_synthetic_(W.WanModel(**CFG), seed=13, std=0.05).eval()


def mask_oracle(oracle, bt, win):
    """bt tokens per block, or None: the oracle as it is"""
    def masked(attn):
        def _attn(q, k, v, k_lens):
            base = W.attention_ref_fp32 if attn.fp32_attention else W.attention_ref
            out = []
            for b in range((q.size(1) + bt - 1) // bt):
                lo, hi = (max(0, b - win + 1) * bt if win else 0), min((b + 1) * bt, q.size(1))
                out.append(base(q[:, b * bt:hi], k[:, lo:hi], v[:, lo:hi]))
            return torch.cat(out, 1)
        return _attn
    for blk in oracle.blocks:
        if bt is None:
            blk.self_attn.__dict__.pop("_attn", None)
        else:
            blk.self_attn._attn = masked(blk.self_attn)


def oracle_errors(oracle, got, lat, t, ctx, grid, win):
    """distance of the engine and of the bf16-autocast oracle from the fp32 oracle, both oracles masked"""
    L = tokens(grid)
    mask_oracle(oracle, FRAMES * L // grid[0], win)
    try:
        ref_bf = oracle.forward([lat], t, [ctx], L, autocast=True)[0]
        oracle.set_fp32_attention(True)
        ref_32 = oracle.forward([lat], t, [ctx], L, autocast=False)[0]
    finally:
        oracle.set_fp32_attention(False)
        mask_oracle(oracle, None, 0)
    return rel_l2(got, ref_32), rel_l2(ref_bf, ref_32), ref_32


def shim(name, oracle, grid=GRID, **kw):
    m = type(name, (M.WanModelHIP,), {})(CFG, grid, device=DEV, calibration=False, **kw)
    m.load_state_dict(oracle.state_dict())
    return m


def run(m, lat, t, ctx, grid):
    return m([lat.to(DEV)], t=t.to(DEV), context=[ctx.to(DEV)], seq_len=tokens(grid))[0].clone()


@pytest.mark.parametrize("win", [0, 2])
def test_engine_vs_masked_oracle(oracle, win):
    lat, ctx, t = inputs(GRID)
    m = shim("WanModelHIP_Causal%d" % win, oracle, causal_block_frames=FRAMES, causal_window_blocks=win)
    assert m.engine.causal_blocks == (FRAMES, win)
    got = run(m, lat, t, ctx, GRID)
    e_hip, e_bf, ref_32 = oracle_errors(oracle, got, lat, t, ctx, GRID, win)
    plain = oracle.forward([lat], t, [ctx], tokens(GRID), autocast=False)[0]
    print(f"window {win}: e_hip {e_hip:.3e} e_bf {e_bf:.3e}; the unmasked oracle is {rel_l2(plain, ref_32):.3e} away")
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)


def test_off_is_identical(oracle):
    lat, ctx, t = inputs(GRID)
    never, toggled = shim("WanModelHIP_CausalNever", oracle), shim("WanModelHIP_CausalOff", oracle)
    toggled.engine.set_causal_blocks(2)
    on = run(toggled, lat, t, ctx, GRID)
    toggled.engine.set_causal_blocks(0)
    assert toggled.engine.causal_blocks == (0, 0)
    want = run(never, lat, t, ctx, GRID)
    assert torch.equal(run(toggled, lat, t, ctx, GRID), want) and not torch.equal(on, want)


def test_block_follows_set_geometry(oracle):
    m = shim("WanModelHIP_CausalGeo", oracle, dynamic_geometry=True, causal_block_frames=FRAMES)
    lat, ctx, t = inputs(GRID)
    run(m, lat, t, ctx, GRID)
    lat, ctx, t = inputs(GRID2, seed=9)
    got = run(m, lat, t, ctx, GRID2)
    assert m.latent_grid == GRID2 and m.engine.causal_blocks == (FRAMES, 0)
    e_hip, e_bf, _ = oracle_errors(oracle, got, lat, t, ctx, GRID2, 0)
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)


@pytest.mark.parametrize("kw,names", [(dict(sp_phases=True), "sequence parallel"), (dict(attn_mx8=True), "attn_mx8")])
def test_refusals(kw, names):
    e = Engine(CFG, (2, 16, 16), device=DEV, n_branches=2, calibration=False, **kw)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.set_causal_blocks(1)
    assert ex.value.status == _lib.MC_EINVAL and names in str(ex.value)
    assert e.causal_blocks == (0, 0)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.set_causal_blocks(-1)
    assert ex.value.status == _lib.MC_EINVAL

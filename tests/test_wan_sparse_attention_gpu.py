"""GPU: tile-sparse self-attention on the Wan engine (mc_set_attention_tile_mask; csrc/attention_sparse.hip): the whole forward
against oracle/wan_dit_ref with the self_attn._attn of every block >= dense_layers replaced, on the instance, by a version of
attention_ref / attention_ref_fp32 that runs per (mask head, 128-row query tile) over the tile's visible keys.  Tiny synthetic
model; 378 tokens in 4 x 8 tiles, 175 in 2 x 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402
from test_wan_causal_blocks_gpu import CFG, DEV, GRID, GRID2, inputs, oracle, rel_l2, run, shim, tokens  # noqa: E402,F401


def make_mask(grid, mh):
    """bool [mh, Lp / 128, Lp / 64]: a seeded random half of the tiles, another per head, the diagonal forced"""
    nqt = (tokens(grid) + 255) // 256 * 2
    g = torch.Generator().manual_seed(7)
    return (torch.rand(mh, nqt, 2 * nqt, generator=g) < 0.5) | (torch.arange(2 * nqt)[None, :] // 2 == torch.arange(nqt)[:, None])


def mask_oracle(oracle, mask, dense_layers=0):
    """mask None: the oracle as it is"""
    def masked(attn):
        def _attn(q, k, v, k_lens):
            base = W.attention_ref_fp32 if attn.fp32_attention else W.attention_ref
            L, H = q.size(1), q.size(2)
            out = torch.empty_like(q, dtype=torch.float32 if attn.fp32_attention else q.dtype)
            for m in range(mask.shape[0]):
                hs = slice(0, H) if mask.shape[0] == 1 else slice(m, m + 1)
                for qt in range((L + 127) // 128):
                    keys = mask[m, qt].repeat_interleave(64)[:L].nonzero()[:, 0]
                    rows = slice(qt * 128, min((qt + 1) * 128, L))
                    out[:, rows, hs] = base(q[:, rows, hs], k[:, keys][:, :, hs], v[:, keys][:, :, hs])
            return out
        return _attn
    for i, blk in enumerate(oracle.blocks):
        blk.self_attn.__dict__.pop("_attn", None)
        if mask is not None and i >= dense_layers:
            blk.self_attn._attn = masked(blk.self_attn)


def oracle_errors(oracle, got, lat, t, ctx, grid, mask, dense_layers=0):
    """distance of the engine and of the bf16-autocast oracle from the fp32 oracle, both oracles masked"""
    L = tokens(grid)
    mask_oracle(oracle, mask, dense_layers)
    try:
        ref_bf = oracle.forward([lat], t, [ctx], L, autocast=True)[0]
        oracle.set_fp32_attention(True)
        ref_32 = oracle.forward([lat], t, [ctx], L, autocast=False)[0]
    finally:
        oracle.set_fp32_attention(False)
        mask_oracle(oracle, None)
    return rel_l2(got, ref_32), rel_l2(ref_bf, ref_32), ref_32


@pytest.mark.parametrize("mh,dense_layers", [(1, 0), (2, 0), (1, 1), (2, 1)])
def test_engine_vs_masked_oracle(oracle, mh, dense_layers):
    lat, ctx, t = inputs(GRID)
    mask = make_mask(GRID, mh)
    m = shim("WanModelHIP_Sparse%d%d" % (mh, dense_layers), oracle, attention_tile_mask=mask, sparse_dense_layers=dense_layers)
    state = m.engine.attention_tile_mask
    assert state[:4] == (mh, 4, 8, dense_layers) and abs(state[4] - float(mask[:, :3, :6].double().mean())) < 1e-12
    got = run(m, lat, t, ctx, GRID)
    e_hip, e_bf, ref_32 = oracle_errors(oracle, got, lat, t, ctx, GRID, mask, dense_layers)
    plain = oracle.forward([lat], t, [ctx], tokens(GRID), autocast=False)[0]
    print(f"density {state[4]:.3f}: e_hip {e_hip:.3e} e_bf {e_bf:.3e}; the unmasked oracle is {rel_l2(plain, ref_32):.3e} away")
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)


def test_off_is_identical(oracle):
    lat, ctx, t = inputs(GRID)
    never, toggled = shim("WanModelHIP_SparseNever", oracle), shim("WanModelHIP_SparseOff", oracle)
    toggled.set_attention_tile_mask(make_mask(GRID, 2))
    on = run(toggled, lat, t, ctx, GRID)
    toggled.set_attention_tile_mask(None)
    assert toggled.engine.attention_tile_mask is None
    want = run(never, lat, t, ctx, GRID)
    assert torch.equal(run(toggled, lat, t, ctx, GRID), want) and not torch.equal(on, want)


def test_after_set_geometry(oracle):
    """the callable form masks the new grid; a tensor stays with the grid it was built for and the next forward says so"""
    m = shim("WanModelHIP_SparseGeo", oracle, dynamic_geometry=True, attention_tile_mask=lambda grid: make_mask(grid, 1))
    fixed = shim("WanModelHIP_SparseGeoFixed", oracle, dynamic_geometry=True, attention_tile_mask=make_mask(GRID, 1))
    lat, ctx, t = inputs(GRID)
    run(m, lat, t, ctx, GRID)
    lat, ctx, t = inputs(GRID2, seed=9)
    got = run(m, lat, t, ctx, GRID2)
    assert m.latent_grid == GRID2 and m.engine.attention_tile_mask[:3] == (1, 2, 4)
    e_hip, e_bf, _ = oracle_errors(oracle, got, lat, t, ctx, GRID2, make_mask(GRID2, 1))
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        run(fixed, lat, t, ctx, GRID2)
    assert ex.value.status == _lib.MC_ESTATE and "512" in str(ex.value) and "256" in str(ex.value)


@pytest.mark.parametrize("kw,first,names", [(dict(sp_phases=True), None, "sequence parallel"), (dict(attn_mx8=True), None, "attn_mx8"),
                                            ({}, "causal", "mc_set_causal_blocks"), ({}, "mask", "tile mask"), ({}, None, "query tile 1")])
def test_refusals(kw, first, names):
    grid = (2, 16, 16) if kw else GRID
    e = Engine(CFG, grid, device=DEV, n_branches=2, calibration=False, **kw)
    mask = make_mask(grid, 1)
    if first == "causal":
        e.set_causal_blocks(2)
    if names == "query tile 1":
        mask[0, 1, :6] = False                     # its only visible tiles are padding
    with pytest.raises(_lib.MagCacheHipError) as ex:
        if first == "mask":
            e.set_attention_tile_mask(mask)
            e.set_causal_blocks(2)
        else:
            e.set_attention_tile_mask(mask)
    assert ex.value.status == _lib.MC_EINVAL and names in str(ex.value)
    assert (e.attention_tile_mask is None) == (first != "mask") and e.causal_blocks == ((2, 0) if first == "causal" else (0, 0))

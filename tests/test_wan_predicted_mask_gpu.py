"""GPU: the predicted tile mask on the Wan engine (mc_set_attention_tile_mass; csrc/attention_predict.hip feeding
csrc/attention_sparse.hip).  A forward is stepped through the phase calls so that every predicted layer's q | k | v rows and
mask can be held: the mask must be what mc_op_attention_tile_predict gives on those rows, and the forward must be the oracle's
with each layer's self-attention masked per tile by that layer's own mask, under the bounds of test_wan_sparse_attention_gpu.
Tiny synthetic model; 378 tokens in 4 x 8 tiles (3 x 6 valid), 175 in 2 x 4.  The toy weights give near-flat pooled attention
(six valid key tiles of about a sixth each): at mass 0.9 every valid tile is kept (density 1.0, measured), so the tests run at
mass 0.5, where the density over valid tiles is 0.528 in both layers; e_hip 3.0e-3 against e_bf 3.1e-3 (measured)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine  # noqa: E402
from magcache_amd.sparse_masks import pack_tile_mask  # noqa: E402
from test_wan_causal_blocks_gpu import CFG, DEV, GRID, GRID2, inputs, oracle, rel_l2, run, shim, tokens  # noqa: E402,F401
from test_wan_sparse_attention_gpu import make_mask, mask_oracle  # noqa: E402

MASS = 0.5
SCALE = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(128.0)))      # the engine's kAttnScale, rounded as it is: fp32 1 / sqrt(128)


def stepped_forward(e, lat, t, ctx, dense_layers):
    """-> the output, and per predicted layer (its "qkv" rows as block_pre_attn left them, the mask block_post_attn left)"""
    d, L = CFG["dim"], e.seq_len
    Lp = (L + 255) // 256 * 256
    e.embed(lat.to(DEV), float(t), ctx.to(DEV))
    kept = {}
    for l in range(CFG["num_layers"]):
        e.block_pre_attn(l)
        qkv = e.buffer("qkv", torch.bfloat16)[:Lp * 3 * d].view(Lp, 3 * d).clone()
        e.block_post_attn(l, 0, _lib.MC_MODE_FULL)
        if l >= dense_layers:
            kept[l] = (qkv, e.read_attention_tile_mask())
    e.head(0, _lib.MC_MODE_FULL)
    tok = e.buffer("head_tokens", torch.float32).view(-1, e.head_stride)[:L].contiguous()
    out = torch.empty((CFG["out_dim"],) + tuple(e.grid), dtype=torch.float32, device=DEV)
    e.unpatchify(tok, 0, L, out)
    torch.cuda.synchronize()
    return out, kept


@pytest.mark.parametrize("dense_layers", [0, 1])
def test_stepped_forward_vs_the_op_and_the_masked_oracle(oracle, dense_layers):
    lat, ctx, t = inputs(GRID)
    L, d, heads = tokens(GRID), CFG["dim"], CFG["num_heads"]
    m = shim("WanModelHIP_Mass%d" % dense_layers, oracle, attention_tile_mass=MASS, sparse_dense_layers=dense_layers)
    assert m.engine.attention_tile_mass == (pytest.approx(MASS), dense_layers)
    got, kept = stepped_forward(m.engine, lat, t, ctx, dense_layers)
    assert sorted(kept) == list(range(dense_layers, CFG["num_layers"]))
    vq, vk = (L + 127) // 128, (L + 63) // 64
    fns = {}
    for l, (qkv, mask) in kept.items():
        Lp = qkv.shape[0]
        assert mask.shape == (heads, Lp // 128, Lp // 64)
        # (a) the op on the kept q and k columns gives the same words
        bits = torch.zeros(heads, Lp // 128, (Lp // 64 + 31) // 32, dtype=torch.int32, device=DEV)
        scratch = torch.empty(H.L().mc_op_attention_tile_predict_scratch(Lp, heads, Lp), dtype=torch.uint8, device=DEV)
        k = qkv[:, d:]
        _lib.check(H.L().mc_op_attention_tile_predict(H.P(qkv), qkv.stride(0), H.P(k), k.stride(0), Lp, heads, Lp, L, SCALE, MASS,
                                                      H.P(bits), H.P(scratch), H.S()))
        torch.cuda.synchronize()
        assert torch.equal(bits.cpu(), pack_tile_mask(mask)), l
        # (b) neither empty nor full over the valid tiles, (c) every valid query tile keeps its own key tiles, nothing behind vk
        assert 0.0 < float(mask[:, :vq, :vk].double().mean()) < 1.0
        for qt in range(vq):
            assert bool(mask[:, qt, [kt for kt in (2 * qt, 2 * qt + 1) if kt < vk]].all())
        assert not bool(mask[:, :, vk:].any())
        mask_oracle(oracle, mask, l)                      # layer l's masked attention, with its own mask in the closure
        fns[l] = oracle.blocks[l].self_attn._attn
    mask_oracle(oracle, None)
    try:
        for l, fn in fns.items():
            oracle.blocks[l].self_attn._attn = fn
        ref_bf = oracle.forward([lat], t, [ctx], L, autocast=True)[0]
        oracle.set_fp32_attention(True)
        ref_32 = oracle.forward([lat], t, [ctx], L, autocast=False)[0]
    finally:
        oracle.set_fp32_attention(False)
        mask_oracle(oracle, None)
    e_hip, e_bf = rel_l2(got, ref_32), rel_l2(ref_bf, ref_32)
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)


def test_off_is_identical(oracle):
    lat, ctx, t = inputs(GRID)
    never, toggled = shim("WanModelHIP_MassNever", oracle), shim("WanModelHIP_MassOff", oracle)
    toggled.set_attention_tile_mass(MASS)
    on = run(toggled, lat, t, ctx, GRID)
    toggled.set_attention_tile_mass(0)
    assert toggled.engine.attention_tile_mass is None
    want = run(never, lat, t, ctx, GRID)
    assert torch.equal(run(toggled, lat, t, ctx, GRID), want) and not torch.equal(on, want)


def test_after_set_geometry(oracle):
    """the shim sets the mass again for the new grid; a bare engine keeps the old buffers and the next forward says so"""
    m = shim("WanModelHIP_MassGeo", oracle, dynamic_geometry=True, attention_tile_mass=MASS)
    lat, ctx, t = inputs(GRID)
    run(m, lat, t, ctx, GRID)
    assert m.engine.read_attention_tile_mask().shape == (CFG["num_heads"], 4, 8)
    lat, ctx, t = inputs(GRID2, seed=9)
    run(m, lat, t, ctx, GRID2)
    assert m.latent_grid == GRID2 and m.engine.read_attention_tile_mask().shape == (CFG["num_heads"], 2, 4)
    e = Engine(CFG, GRID, device=DEV, n_branches=2, calibration=False)
    e.load_weights(oracle.state_dict())
    e.set_attention_tile_mass(MASS)
    e.set_geometry(GRID2)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.forward(lat.to(DEV), float(t), ctx.to(DEV))
    assert ex.value.status == _lib.MC_ESTATE and "512" in str(ex.value) and "256" in str(ex.value)


@pytest.mark.parametrize("kw,first,then,names", [
    (dict(sp_phases=True), None, "mass", "sequence parallel"), (dict(attn_mx8=True), None, "mass", "attn_mx8"),
    ({}, "causal", "mass", "mc_set_causal_blocks"), ({}, "mask", "mass", "static tile mask"),
    ({}, "mass", "causal", "tile mass"), ({}, "mass", "mask", "tile mass"), ({}, None, "mass 1.5", "mass"), ({}, None, "dense -1", "dense_layers")])
def test_refusals(kw, first, then, names):
    grid = (2, 16, 16) if kw else GRID
    e = Engine(CFG, grid, device=DEV, n_branches=2, calibration=False, **kw)
    call = {"causal": lambda: e.set_causal_blocks(2), "mask": lambda: e.set_attention_tile_mask(make_mask(grid, 1)),
            "mass": lambda: e.set_attention_tile_mass(MASS), "mass 1.5": lambda: e.set_attention_tile_mass(1.5),
            "dense -1": lambda: e.set_attention_tile_mass(MASS, -1)}
    if first:
        call[first]()
    with pytest.raises(_lib.MagCacheHipError) as ex:
        call[then]()
    assert ex.value.status == _lib.MC_EINVAL and names in str(ex.value)
    assert (e.attention_tile_mass is not None) == (first == "mass")
    assert (e.attention_tile_mask is not None) == (first == "mask") and e.causal_blocks == ((2, 0) if first == "causal" else (0, 0))

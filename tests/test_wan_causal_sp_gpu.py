"""GPU: frame-block causal self-attention on sequence-parallel Wan engines (mc_set_causal_blocks_sharded;
csrc/attention_band_shards.hip).  Ranks 0 and 1 of sp_size 2 in one process, the gather played by device copies, as in
test_wan_sparse_sp_gpu.py.  Grid (6, 14, 18): 63 tokens per frame, 378 tokens, Lr = 189 per rank (no multiple of 64) padded to
256; with two frames per block the blocks are tokens [0, 126), [126, 252), [252, 378): the middle one straddles the rank boundary
at 189 and both inner edges fall inside a 64-key tile.  The result must lie within test_wan_causal_blocks_gpu.py's bar of the
masked fp32 oracle AND, under the same bar, of the one-GPU engine under mc_set_causal_blocks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine, MC_MODE_FULL  # noqa: E402
from test_wan_causal_blocks_gpu import CFG, DEV, FRAMES, GRID, inputs, oracle, oracle_errors, rel_l2, tokens  # noqa: E402,F401

L = tokens(GRID)


def engine(oracle, **kw):
    e = Engine(CFG, GRID, device=DEV, n_branches=1, calibration=False, **kw)
    e.load_weights({k: v.to(DEV) for k, v in oracle.state_dict().items()})
    return e


def phases(eng, lat, t, ctx):
    """one forward of the ranks in `eng` through the phase calls -> fp32 [out_dim, F, H, W] on the host"""
    P, d = len(eng), CFG["dim"]
    for e in eng:
        e.embed(lat.to(DEV), t, ctx.to(DEV))
    R, Lc, _ = eng[0].sp_round_info(0)
    kvl = [e.buffer("kv_local", torch.bfloat16).view(-1, 2 * d) for e in eng]
    kvg = [e.buffer("kv_gather", torch.bfloat16).view(-1, P, Lc, 2 * d) for e in eng]
    for layer in range(CFG["num_layers"]):
        for e in eng:
            e.block_pre_attn(layer)
        for c in range(R):
            for dst in range(P):
                for src in range(P):
                    kvg[dst][c, src].copy_(kvl[src][c * Lc:(c + 1) * Lc])
        for e in eng:
            e.block_attn_local(layer)
            e.block_post_attn(layer, 0, MC_MODE_FULL)      # attends the rounds
    rows = []
    for e in eng:
        e.head(0, MC_MODE_FULL)
        rows.append(e.buffer("head_tokens", torch.float32).view(-1, e.head_stride)[:L // P].clone())
    out = torch.empty((CFG["out_dim"],) + GRID, dtype=torch.float32, device=DEV)
    eng[0].unpatchify(torch.cat(rows).contiguous(), 0, L, out)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def one_rank(oracle):
    return engine(oracle)


@pytest.mark.parametrize("win", [0, 2])
@pytest.mark.parametrize("chunks", [1, 2])
def test_two_ranks_vs_one_gpu_and_oracle(oracle, one_rank, chunks, win):
    lat, ctx, t = inputs(GRID)
    eng = [engine(oracle, sp_rank=r, sp_size=2) for r in range(2)]
    for e in eng:
        e.sp_set_chunks(chunks)
        e.set_sharded_causal_blocks(FRAMES, win)
        assert e.causal_blocks == (FRAMES, win)
    got = phases(eng, lat, t, ctx)
    one_rank.set_causal_blocks(FRAMES, win)
    want = one_rank.forward(lat.to(DEV), t, ctx.to(DEV)).cpu()
    e_hip, e_bf, _ = oracle_errors(oracle, got, lat, t, ctx, GRID, win)
    e_one = rel_l2(got, want)
    print(f"chunks {chunks} window {win}: e_hip {e_hip:.3e} e_bf {e_bf:.3e}; from the one-GPU causal engine {e_one:.3e}")
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)
    assert e_one < 2 * e_bf + 1e-3 and e_one < 2e-2, (e_one, e_bf)


def test_off_restores_the_dense_chain(oracle):
    lat, ctx, t = inputs(GRID)
    eng = [engine(oracle, sp_rank=r, sp_size=2) for r in range(2)]
    before = phases(eng, lat, t, ctx)
    for e in eng:
        e.set_sharded_causal_blocks(FRAMES)
    on = phases(eng, lat, t, ctx)
    for e in eng:
        e.set_sharded_causal_blocks(0, 0)
        assert e.causal_blocks == (0, 0)
    assert torch.equal(phases(eng, lat, t, ctx), before) and not torch.equal(on, before)


def test_refusals(oracle, one_rank):
    e = engine(oracle, sp_phases=True)
    mx8 = Engine(CFG, (2, 16, 16), device=DEV, n_branches=1, calibration=False, attn_mx8=True)
    for call, args, status, words in [(one_rank.set_sharded_causal_blocks, (1,), _lib.MC_ESTATE, "sequence-parallel"),
                                      (mx8.set_sharded_causal_blocks, (1,), _lib.MC_EINVAL, "attn_mx8"),
                                      (e.set_sharded_causal_blocks, (-1,), _lib.MC_EINVAL, ">= 0")]:
        with pytest.raises(_lib.MagCacheHipError) as ex:
            call(*args)
        assert ex.value.status == status and words in str(ex.value)
    e.set_sharded_causal_blocks(FRAMES, 1)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.set_sharded_attention_tile_mask(torch.ones(1, 4, 8, dtype=torch.bool))
    assert ex.value.status == _lib.MC_EINVAL and "mc_set_causal_blocks_sharded" in str(ex.value)
    assert e.causal_blocks == (FRAMES, 1) and e.attention_tile_mask is None

"""GPU: the static tile mask on sequence-parallel Wan engines (mc_set_attention_tile_mask_sharded; csrc/attention_sparse_shards.hip).
Ranks 0 and 1 of sp_size 2 in one process, the gather played by device copies, against the masked fp32 oracle of
test_wan_sparse_attention_gpu.py.  Grid (2, 32, 32): 512 tokens, Lr = Lp = 256 per rank, so the per-shard tile space is the
global one and rank r's mask is rows [2r, 2r + 2) of the one-GPU mask.

Distance from the one-rank engine under the same mask, measured on an MI355X: 9.4e-4 .. 1.03e-3 rel-L2 over the four cases
below; the dense chain at this geometry is 1.032e-3 (one round) and 1.028e-3 (two rounds) from the one-rank dense engine.  The
bar is twice the dense chain's figure: one more bf16 pass of the partial O, as tests/test_engine_gpu.py explains for its 3e-3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd.engine import Engine, MC_MODE_FULL  # noqa: E402
from test_wan_causal_blocks_gpu import CFG, DEV, inputs, oracle, rel_l2  # noqa: E402,F401
from test_wan_sparse_attention_gpu import make_mask, oracle_errors  # noqa: E402

GRID = (2, 32, 32)
L = 512
DENSE_CHAIN = {1: 1.032e-3, 2: 1.028e-3}     # sp_chunks -> rel-L2 of the two-rank dense chain from the one-rank dense engine (measured)


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


@pytest.mark.parametrize("mh,dense_layers", [(1, 0), (2, 1)])
@pytest.mark.parametrize("chunks", [1, 2])
def test_two_ranks_vs_masked_oracle(oracle, one_rank, chunks, mh, dense_layers):
    lat, ctx, t = inputs(GRID)
    mask = make_mask(GRID, mh)
    eng = [engine(oracle, sp_rank=r, sp_size=2) for r in range(2)]
    for r, e in enumerate(eng):
        e.sp_set_chunks(chunks)
    one_rank.set_attention_tile_mask(None)
    dense = rel_l2(phases(eng, lat, t, ctx), one_rank.forward(lat.to(DEV), t, ctx.to(DEV)).cpu())
    for r, e in enumerate(eng):
        e.set_sharded_attention_tile_mask(mask[:, 2 * r:2 * r + 2], dense_layers)
        assert e.attention_tile_mask[:4] == (mh, 2, 8, dense_layers)
    got = phases(eng, lat, t, ctx)
    one_rank.set_attention_tile_mask(mask, dense_layers)
    sparse = rel_l2(got, one_rank.forward(lat.to(DEV), t, ctx.to(DEV)).cpu())
    e_hip, e_bf, _ = oracle_errors(oracle, got, lat, t, ctx, GRID, mask, dense_layers)
    print(f"chunks {chunks}: e_hip {e_hip:.3e} e_bf {e_bf:.3e}; from the one-rank engine: sparse {sparse:.3e}, dense chain {dense:.3e}")
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)
    assert sparse < 2 * DENSE_CHAIN[chunks], (sparse, dense)


def test_world_of_one_and_off(oracle, one_rank):
    """sp_phases on one GPU: the local launch covers every key, so the sharded call gives the one-GPU sparse engine's result;
    off again is the dense engine bit for bit"""
    lat, ctx, t = inputs(GRID)
    mask = make_mask(GRID, 2)
    e = engine(oracle, sp_phases=True)
    before = phases([e], lat, t, ctx)
    e.set_sharded_attention_tile_mask(mask, 1)
    assert e.attention_tile_mask[:4] == (2, 4, 8, 1)
    on = phases([e], lat, t, ctx)
    one_rank.set_attention_tile_mask(mask, 1)
    want = one_rank.forward(lat.to(DEV), t, ctx.to(DEV)).cpu()
    print(f"world of one: {rel_l2(on, want):.3e} from the one-GPU sparse engine, bitwise {torch.equal(on, want)}")
    assert rel_l2(on, want) < DENSE_CHAIN[1] and not torch.equal(on, before)     # one kernel in place of another: no extra pass
    e.set_sharded_attention_tile_mask(None)
    assert e.attention_tile_mask is None and torch.equal(phases([e], lat, t, ctx), before)


def test_refusals(oracle, one_rank):
    mask = make_mask(GRID, 1)
    e = engine(oracle, sp_phases=True)
    for call, arg, status, words in [(e.set_attention_tile_mask, mask, _lib.MC_EINVAL, "sequence parallel"),
                                     (one_rank.set_sharded_attention_tile_mask, mask, _lib.MC_ESTATE, "sequence-parallel"),
                                     (e.set_sharded_attention_tile_mask, mask[:, :, :6], _lib.MC_EINVAL, "4 x 6")]:
        with pytest.raises(_lib.MagCacheHipError) as ex:
            call(arg)
        assert ex.value.status == status and words in str(ex.value)
    assert e.attention_tile_mask is None

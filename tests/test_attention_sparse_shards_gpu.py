"""GPU: the sharded tile-sparse self-attention kernel (csrc/attention_sparse_shards.hip, mc_op_attention_sparse_partial) against
attention_cases.attn_ref64 called once per (mask head, query tile) over that tile's visible valid keys, O and the
log2-sum-exp under attention_cases.accept unchanged.

Operands are attention_cases.every_key_case: every visited key is the dominant key of some query, padding rows and the rows of
the skipped shard are hostile (k twice a valid key, v = 1000).  The bitmap is a seeded random half of the ADDRESSED bits (tile t
of visited shard s = bit bit0 + s * stride + t, t < ceil(valid / 64)) with one forced tile per query tile; every bit outside
those ranges -- padding tiles, the skipped shard, the rest of the words -- is SET, so a kernel that takes one for a tile reads a
hostile row.
What the choice can see was checked once on the CPU over the 64 parameter sets of the first test: the fp64 reference of the
mask with the first visible tile of every query tile dropped (where two are visible) fails accept in all 60 sets that have such
a tile, and with the first hidden tile of every query tile added in all 52 sets that have a hidden tile (one addressed tile --
(64, 1) on one shard -- admits neither mutation)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.sparse_masks import pack_tile_mask  # noqa: E402

DEV = "cuda:0"
HEADS = 2
SHARDS = [(64, 1), (128, 65), (128, 128), (192, 129)]           # (shard_rows, valid)
SPLITS = [(1, -1), (3, -1), (3, 0), (3, 2)]                     # (n_shards, skip)
MAPPINGS = ["packed", "midword"]                                 # (0, shard_rows / 64, as many words as needed); (27, 3, 2 words)


def mapping_of(name, shard_rows, n_shards):
    """bit0, bit_shard_stride, row_words"""
    return (0, shard_rows // 64, (n_shards * shard_rows // 64 + 31) // 32) if name == "packed" else (27, 3, 2)


def addressed(shard_rows, valid, n_shards, skip, bit0, stride):
    """(shard, tile, bit) of every key tile a launch may visit, in the kernel's order"""
    return [(s, t, bit0 + s * stride + t) for s in range(n_shards) if s != skip for t in range((valid + 63) // 64)]


def tile_mask(nqt, mh, words, addr, vis):
    """bool [mh, nqt, 32 * words]: vis [mh, nqt, len(addr)] at the addressed bits, every other bit set"""
    mask = torch.ones(mh, nqt, 32 * words, dtype=torch.bool)
    mask[:, :, [b for _, _, b in addr]] = vis
    return mask


def reference(c, addr, vis, shard_rows, valid):
    """fp64 O [Lq, d] and lse [heads, Lq] of the visible valid keys; rows of a query tile that sees nothing: 0 and -inf"""
    Lq, mh = c.q.shape[0], vis.shape[0]
    o = torch.zeros(Lq, HEADS * A.HD, dtype=torch.float64)
    lse = torch.full((HEADS, Lq), -float("inf"), dtype=torch.float64)
    for m in range(mh):
        cols, hs, nh = (slice(None), slice(None), HEADS) if mh == 1 else (slice(m * A.HD, (m + 1) * A.HD), slice(m, m + 1), 1)
        for qt in range(Lq // 128):
            keys = [s * shard_rows + t * 64 + torch.arange(min(64, valid - t * 64)) for (s, t, _), on in zip(addr, vis[m, qt]) if on]
            if keys:
                r = slice(qt * 128, (qt + 1) * 128)
                o[r, cols], lse[hs, r] = A.attn_ref64(c.q[r, cols], c.k[:, cols], c.v[:, cols], nh, torch.cat(keys), A.SCALE)
    return o, lse


@functools.lru_cache(maxsize=None)
def random_case(shard_rows, valid, n_shards, skip, mh, mapping):
    c = A.every_key_case(A.every_key_lq(valid, n_shards, skip), HEADS, shard_rows, valid, n_shards, A.SEED, skip)
    bit0, stride, words = mapping_of(mapping, shard_rows, n_shards)
    addr = addressed(shard_rows, valid, n_shards, skip, bit0, stride)
    nqt = c.q.shape[0] // 128
    vis = torch.rand(mh, nqt, len(addr), generator=torch.Generator().manual_seed(A.SEED)) < 0.5
    vis[:, torch.arange(nqt), (3 * torch.arange(nqt) + 1) % len(addr)] = True
    return c, tile_mask(nqt, mh, words, addr, vis), reference(c, addr, vis, shard_rows, valid)


def launch(q, k, v, o, shard_rows, valid, n_shards, skip, mask, mapping, lse_out=None, lse_in=None, null_bits=False):
    """q, k, v, o on the device; mask bool [mh, nqt, 32 * words] or packed device words; mapping (bit0, stride, words)"""
    bits = pack_tile_mask(mask).to(DEV) if mask.dtype == torch.bool else mask
    status = H.L().mc_op_attention_sparse_partial(
        H.P(q), q.stride(0), H.P(k), k.stride(0), shard_rows * k.stride(0), H.P(v), v.stride(0), shard_rows * v.stride(0), H.P(o),
        o.stride(0), q.shape[0], HEADS, shard_rows, valid, n_shards, A.SCALE, skip, None if lse_out is None else H.P(lse_out),
        None if lse_in is None else H.P(lse_in), None if null_bits else H.P(bits), mask.shape[0], mapping[2], mapping[0], mapping[1],
        None, H.S())
    torch.cuda.synchronize()
    return status


def fresh(Lq):
    """O and lse buffers no launch has written: NaN"""
    return (torch.full((Lq, HEADS * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV),
            torch.full((HEADS, Lq), float("nan"), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("mh", [1, 2])
@pytest.mark.parametrize("n_shards,skip", SPLITS)
@pytest.mark.parametrize("shard_rows,valid", SHARDS)
def test_against_fp64(shard_rows, valid, n_shards, skip, mh, mapping):
    c, mask, (o_ref, lse_ref) = random_case(shard_rows, valid, n_shards, skip, mh, mapping)
    o, lse = fresh(c.q.shape[0])
    status = launch(c.q.to(DEV), c.k.to(DEV), c.v.to(DEV), o, shard_rows, valid, n_shards, skip, mask,
                    mapping_of(mapping, shard_rows, n_shards), lse_out=lse)
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    print(f"rel-L2 {A.rel_l2(o.cpu(), o_ref):.3e}, lse max err {float((lse.cpu().double() - lse_ref).abs().max()):.3e}")
    A.accept(o, o_ref, lse, lse_ref)


def test_chain_with_empty_tiles():
    """the local shard (1) alone, then the others merged into it; query tile 1 sees nothing locally, 2 nothing in the others,
    3 nothing at all"""
    shard_rows, valid, n = 128, 65, 3
    c = A.every_key_case(512, HEADS, shard_rows, valid, n, A.SEED)
    mapping = (0, 2, 1)
    addr = addressed(shard_rows, valid, n, -1, 0, 2)
    local = torch.tensor([s == 1 for s, _, _ in addr])
    vis = torch.rand(1, 4, len(addr), generator=torch.Generator().manual_seed(A.SEED)) < 0.5
    vis[0, 0, [0, 2]] = True
    vis[0, 1] &= ~local
    vis[0, 1, 5] = True
    vis[0, 2] &= local
    vis[0, 2, 3] = True
    vis[0, 3] = False
    mask = tile_mask(4, 1, 1, addr, vis)
    o_ref, lse_ref = reference(c, addr, vis, shard_rows, valid)
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    o, lse = fresh(512)
    assert launch(q, k[shard_rows:], v[shard_rows:], o, shard_rows, valid, 1, -1, mask, (2, 0, 1), lse_out=lse) == _lib.MC_OK
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
    assert bool((o[128:256] == 0).all()) and bool((lse[:, 128:256] == -float("inf")).all()), "empty without lse_in: zeros and -inf"
    assert launch(q, k, v, o, shard_rows, valid, n, 1, mask, mapping, lse_out=lse, lse_in=lse) == _lib.MC_OK
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
    assert bool((o[384:] == 0).all()) and bool((lse[:, 384:] == -float("inf")).all()), "empty in both launches"
    A.accept(o, o_ref, lse, lse_ref)


def test_all_bits_set_is_the_dense_partial():
    shard_rows, valid, n, skip = 192, 129, 3, 2
    c = A.every_key_build(valid, shard_rows, n, skip)
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    Lq = q.shape[0]
    (o, lse), (o_d, lse_d) = fresh(Lq), fresh(Lq)
    ones = torch.ones(1, Lq // 128, 64, dtype=torch.bool)
    assert launch(q, k, v, o, shard_rows, valid, n, skip, ones, (27, 3, 2), lse_out=lse) == _lib.MC_OK
    _lib.check(H.L().mc_op_attention_partial(H.P(q), q.stride(0), H.P(k), k.stride(0), shard_rows * k.stride(0), H.P(v), v.stride(0),
                                             shard_rows * v.stride(0), H.P(o_d), o_d.stride(0), Lq, HEADS, shard_rows, valid, n, A.SCALE,
                                             skip, H.P(lse_d), None, H.S()))
    torch.cuda.synchronize()
    A.accept(o, c.o_ref, lse, c.lse_ref)
    A.accept(o, o_d.double(), lse, lse_d.double())


@pytest.mark.parametrize("what", ["bit range", "mask_heads 3", "null bits", "misaligned lse_out", "skip leaves no shard"])
def test_refusals(what):
    """MC_EINVAL, nothing launched: O untouched"""
    q, k, v = (torch.zeros(256, HEADS * A.HD, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    o, lse = fresh(256)
    bits = torch.full((3, 2, 1), -1, dtype=torch.int32, device=DEV)
    n, skip, mapping = (1, 0, (0, 4, 1)) if what == "skip leaves no shard" else (1, -1, (29 if what == "bit range" else 0, 4, 1))
    status = launch(q, k, v, o, 256, 256, n, skip, bits[:3 if what == "mask_heads 3" else 1], mapping,
                    lse_out=lse.view(-1)[1:] if what == "misaligned lse_out" else lse, null_bits=what == "null bits")
    assert status == _lib.MC_EINVAL and "attention_sparse_shards" in H.L().mc_last_error().decode()
    assert bool(torch.isnan(o).all()), what

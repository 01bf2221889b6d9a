"""GPU: the tile-sparse joint attention kernel (csrc/attention_joint.hip, mc_op_attention_joint_sparse) against
attention_cases.attn_ref64 per (head, query tile) over the keys the rule of include/magcache_mmdit.h makes visible, under
attention_cases.accept unchanged (the bar of tests/test_attention_sparse_gpu.py: the arithmetic per tile is the same).
Operands as there: k, v ~ N(0, 1), q_i = 3 k[t(i)], so that a lost or leaked tile replaces rows of O: in every query tile the even
rows aim at its visible valid keys, the odd rows at its INVISIBLE ones.  Padding rows of k are twice a valid key, v = 1000 there."""
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
# name: (Lq_pad = rows, first text row, text rows, valid text rows, valid)
SHAPES = {"text-first": (2304, 0, 512, 512, 2304),       # FLUX: kalways in word 0, no tail, the dense items are the lowest tiles
          "text-last": (2304, 2000, 256, 100, 2100),     # HunyuanVideo: kalways = key tiles 31..32 across the word boundary, a tail
                                                         # tile (2100 % 64 = 52), a mixed boundary tile, dense items last in memory
          "smallest": (256, 192, 64, 10, 202),           # one word, kalways is the tail tile
          "no-text": (512, 0, 0, 0, 500)}                # empty ranges: the plain bitmap rule
PATTERNS = ["rand", "rand+diag", "zero-row", "ones"]


def ranges(name):
    """(q0, q1, k0, k1): the tiles that intersect the text rows / the valid text rows"""
    _, t0, tn, tv, _ = SHAPES[name]
    return (t0 // 128, (t0 + tn + 127) // 128, t0 // 64, (t0 + tv + 63) // 64) if tn else (0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def mask_of(name, mh, pattern):
    """bool [mh, nqt, nkt]: the caller's bits; "zero-row": the first query tile outside qdense has none"""
    Lq = SHAPES[name][0]
    nqt, nkt = Lq // 128, Lq // 64
    if pattern == "ones":
        return torch.ones(mh, nqt, nkt, dtype=torch.bool)
    m = torch.rand(mh, nqt, nkt, generator=torch.Generator().manual_seed(A.SEED)) < 0.5
    if pattern == "rand+diag":
        m |= torch.arange(nkt)[None, :] // 2 == torch.arange(nqt)[:, None]
    if pattern == "zero-row":
        q0, q1, _, _ = ranges(name)
        m[:, 0 if q0 > 0 else q1] = False
    return m


def visible(name, mh, pattern, m, qt):
    """the rule: the valid keys query tile qt of mask head m sees, and the valid keys it does not"""
    Lq, _, _, _, valid = SHAPES[name]
    q0, q1, k0, k1 = ranges(name)
    kt = torch.arange(Lq // 64)
    tiles = mask_of(name, mh, pattern)[m, qt] | ((kt >= k0) & (kt < k1)) | (q0 <= qt < q1)
    seen = tiles.repeat_interleave(64)[:valid]
    return seen.nonzero()[:, 0], (~seen).nonzero()[:, 0]


@functools.lru_cache(maxsize=None)
def case(name, mh, pattern):
    """q, k, v [Lq, d] bf16 on the CPU and the fp64 reference [Lq, d] (rows of a query tile that sees nothing: 0)"""
    Lq, _, _, _, valid = SHAPES[name]
    d = HEADS * A.HD
    g = torch.Generator().manual_seed(A.SEED)
    k = torch.randn(Lq, d, generator=g).bfloat16()
    v = torch.randn(Lq, d, generator=g).bfloat16()
    k[valid:] = (2.0 * k[(torch.arange(Lq - valid) * 7) % valid].float()).bfloat16()
    v[valid:] = 1000.0
    q = torch.randn(Lq, d, generator=g).bfloat16()
    ref = torch.zeros(Lq, d, dtype=torch.float64)
    r = torch.arange(128)
    for h in range(HEADS):
        c = slice(h * A.HD, (h + 1) * A.HD)
        for qt in range(Lq // 128):
            rows = slice(qt * 128, (qt + 1) * 128)
            seen, unseen = visible(name, mh, pattern, h % mh, qt)
            for pool, sel in ((seen, r % 2 == 0), (unseen if len(unseen) else seen, r % 2 == 1)):
                if len(pool):
                    q[rows, c][sel] = (3.0 * k[pool[(r[sel] * len(pool)) // 128], c].float()).bfloat16()
            if len(seen):
                ref[rows, c] = A.attn_ref64(q[rows, c], k[:, c], v[:, c], 1, seen, A.SCALE)[0]
    return q, k, v, ref


def launch(q, k, v, name, mh, bits, rg=None, order=None):
    Lq, valid = SHAPES[name][0], SHAPES[name][4]
    o = torch.full((Lq, HEADS * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV)
    q0, q1, k0, k1 = ranges(name) if rg is None else rg
    status = H.L().mc_op_attention_joint_sparse(H.P(q), q.stride(0), H.P(k), k.stride(0), H.P(v), v.stride(0), H.P(o), o.stride(0), Lq,
                                                HEADS, k.shape[0], valid, None if bits is None else H.P(bits), mh, q0, q1, k0, k1,
                                                None if order is None else H.P(order), A.SCALE, H.S())
    torch.cuda.synchronize()
    return o, status


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("mh", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_joint_against_fp64(name, mh, pattern):
    q, k, v, ref = case(name, mh, pattern)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o, status = launch(qd, kd, vd, name, mh, pack_tile_mask(mask_of(name, mh, pattern)).to(DEV))
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    assert bool(torch.isfinite(o.float()).all()), "padding rows must be finite"
    Lq, valid = SHAPES[name][0], SHAPES[name][4]
    if pattern == "zero-row" and name == "no-text":
        assert bool((o[:128] == 0).all()), "a query tile that sees no key writes zeros"
    print(f"rel-L2 {A.rel_l2(o[:valid].cpu(), ref[:valid]):.3e}")
    A.accept(o[:valid], ref[:valid])
    if pattern == "ones":   # all bits set is plain attention
        plain = torch.empty_like(o)
        _lib.check(H.L().mc_op_attention(H.P(qd), qd.stride(0), H.P(kd), kd.stride(0), 0, H.P(vd), vd.stride(0), 0, H.P(plain),
                                         plain.stride(0), Lq, HEADS, Lq, valid, 1, A.SCALE, H.S()))
        torch.cuda.synchronize()
        A.accept(o[:valid], plain[:valid].double())
        dense, status = launch(qd, kd, vd, name, mh, None, rg=(0, Lq // 128, 0, 0))   # qdense everywhere: no bitmap is read
        assert status == _lib.MC_OK and torch.equal(dense, o)


def test_reversed_order_table_gives_the_same_bits():
    name, mh = "text-last", 2
    q, k, v, _ = case(name, mh, "rand")
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    bits = pack_tile_mask(mask_of(name, mh, "rand")).to(DEV)
    order = torch.arange(SHAPES[name][0] // 128 * HEADS - 1, -1, -1, dtype=torch.int32, device=DEV)
    assert torch.equal(launch(qd, kd, vd, name, mh, bits, order=order)[0], launch(qd, kd, vd, name, mh, bits)[0])


@pytest.mark.parametrize("rg,null", [((0, 3, 0, 0), False), ((0, 0, 2, 1), False), ((-1, 1, 0, 0), False), ((0, 1, 0, 4), True)],
                         ids=["q1 > nqt", "k0 > k1", "q0 < 0", "null mask, one sparse tile"])
def test_refused_ranges_launch_nothing(rg, null):
    q, k, v, _ = case("smallest", 1, "ones")
    bits = None if null else torch.full((1, 2, 1), -1, dtype=torch.int32, device=DEV)
    o, status = launch(q.to(DEV), k.to(DEV), v.to(DEV), "smallest", 1, bits, rg=rg)
    assert status == _lib.MC_EINVAL and "attention_joint_sparse" in H.L().mc_last_error().decode() and bool(torch.isnan(o).all())

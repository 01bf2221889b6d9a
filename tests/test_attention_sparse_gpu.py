"""GPU: the tile-sparse self-attention kernel (csrc/attention_sparse.hip, mc_op_attention_sparse) against
attention_cases.attn_ref64 called once per (mask head, query tile) over that tile's visible valid keys, under
attention_cases.accept unchanged.

Random operands cannot see a lost or leaked key (it moves O by ~|v| / n), so k, v ~ N(0, 1) and q_i = 3 k[t(i)]:
  own     t(i) runs evenly over the visible valid keys of row i's tile: every visible tile of every query tile hosts dominant keys,
          a lost tile replaces those rows of O
  hidden  t(i) runs over the valid keys of the tile's INVISIBLE tiles (where one exists): a leaked tile replaces the row
Padding rows of k are twice a valid key and v = 1000 there: a padding key that is read in takes its row outright.
On the CPU attention_cases.flash_bf16_model, applied per query tile, passes accept on all 17 combinations (rel-L2 <= 3.6e-3;
the own cases, whose dominant key carries all the weight, 1e-8 .. 3e-7), and the unmasked fp64 result is 2.0 .. 2.7 rel-L2 away
from the masked one, and fails accept, in every hidden case."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.sparse_masks import pack_tile_mask  # noqa: E402

DEV = "cuda:0"
# (Lq_pad, valid, heads, mask_heads, pattern); the key shard has Lq_pad rows, `padbits` 128 more (two padding tiles)
SHAPES = [(256, 256, 1, 1, "diag"), (512, 500, 1, 1, "sink+diag"), (512, 500, 1, 1, "tail"), (768, 700, 2, 2, "rand"),
          (768, 700, 2, 1, "rand"), (2304, 2250, 1, 1, "word2"), (2304, 2250, 1, 1, "padbits"), (512, 500, 1, 1, "empty")]
CASES = [(s, kind) for s in SHAPES for kind in ("own", "hidden")] + [(SHAPES[3], "random")]


def key_rows(shape):
    return shape[0] + (128 if shape[4] == "padbits" else 0)


@functools.lru_cache(maxsize=None)
def mask_of(shape):
    """bool [mask_heads, nqt, 32 * words]: the bits as packed, those at padding tiles and beyond nkt included"""
    Lq, valid, heads, mh, pattern = shape
    nqt, bits = Lq // 128, (key_rows(shape) // 64 + 31) // 32 * 32
    qt, kt = torch.arange(nqt)[:, None], torch.arange(bits)[None, :]
    diag, last = (kt // 2 == qt), (valid - 1) // 64
    one = {"diag": diag, "sink+diag": diag | (kt == 0), "tail": (kt == last) & (qt >= 0), "padbits": diag | (kt > last),
           "word2": torch.where(qt % 2 == 1, (kt == 33) | (kt == 35), diag | (kt == 0)),
           "empty": (diag | (kt == 0)) & (qt != 1)}.get(pattern)
    if one is not None:
        return one[None].clone()
    g = torch.Generator().manual_seed(A.SEED)
    return ((torch.rand(mh, nqt, bits, generator=g) < 0.5) & (kt < key_rows(shape) // 64)) | diag


def visible(shape, m, qt):
    """the valid keys query tile qt of mask head m sees, and those it does not"""
    tiles = mask_of(shape)[m, qt, :key_rows(shape) // 64]
    seen = tiles.repeat_interleave(64)[:shape[1]]
    return seen.nonzero()[:, 0], (~seen).nonzero()[:, 0]


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """q [Lq, d], k, v [rows, d] bf16 on the CPU and the fp64 reference [Lq, d] (rows of an empty query tile: 0)"""
    Lq, valid, heads, mh, _ = shape
    rows, d = key_rows(shape), heads * A.HD
    g = torch.Generator().manual_seed(A.SEED)
    k = torch.randn(rows, d, generator=g).bfloat16()
    v = torch.randn(rows, d, generator=g).bfloat16()
    k[valid:] = (2.0 * k[(torch.arange(rows - valid) * 7) % valid].float()).bfloat16()
    v[valid:] = 1000.0
    q = torch.randn(Lq, d, generator=g).bfloat16()
    ref = torch.zeros(Lq, d, dtype=torch.float64)
    r = torch.arange(128)
    for h in range(heads if kind != "random" else 0):
        for qt in range(Lq // 128):
            seen, unseen = visible(shape, h % mh, qt)
            pool = unseen if kind == "hidden" and len(unseen) else seen
            if len(pool):
                q[qt * 128:(qt + 1) * 128, h * A.HD:(h + 1) * A.HD] = (3.0 * k[pool[(r * len(pool)) // 128], h * A.HD:(h + 1) * A.HD].float()).bfloat16()
    for m in range(mh):
        c = slice(0, d) if mh == 1 else slice(m * A.HD, (m + 1) * A.HD)
        for qt in range(Lq // 128):
            seen = visible(shape, m, qt)[0]
            if len(seen):
                ref[qt * 128:(qt + 1) * 128, c] = A.attn_ref64(q[qt * 128:(qt + 1) * 128, c], k[:, c], v[:, c], heads if mh == 1 else 1, seen, A.SCALE)[0]
    return q, k, v, ref


def launch(q, k, v, shape, o=None, order=None, bits=None, null_mask=False):
    Lq, valid, heads, mh, _ = shape
    o = torch.full((Lq, heads * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV) if o is None else o
    bits = pack_tile_mask(mask_of(shape)).to(DEV) if bits is None else bits
    status = H.L().mc_op_attention_sparse(H.P(q), q.stride(0), H.P(k), k.stride(0), H.P(v), v.stride(0), H.P(o), o.stride(0), Lq, heads,
                                          k.shape[0], valid, None if null_mask else H.P(bits), mh, None if order is None else H.P(order),
                                          A.SCALE, H.S())
    torch.cuda.synchronize()
    return o, status


@pytest.mark.parametrize("shape,kind", CASES, ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else p)
def test_sparse_against_fp64(shape, kind):
    q, k, v, ref = case(shape, kind)
    o, status = launch(q.to(DEV), k.to(DEV), v.to(DEV), shape)
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    assert bool(torch.isfinite(o.float()).all()), "padding rows must be finite"
    if shape[4] == "empty":
        assert bool((o[128:256] == 0).all()), "a query tile that sees no key writes zeros"
    print(f"rel-L2 {A.rel_l2(o[:shape[1]].cpu(), ref[:shape[1]]):.3e}")
    A.accept(o[:shape[1]], ref[:shape[1]])


def test_all_bits_set_is_plain_attention():
    shape = (768, 700, 2, 1, "rand")
    q, k, v, _ = case(shape, "own")
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    ones = torch.full((1, 6, 1), -1, dtype=torch.int32, device=DEV)
    o, status = launch(qd, kd, vd, shape, bits=ones)
    assert status == _lib.MC_OK
    plain = torch.empty_like(o)
    _lib.check(H.L().mc_op_attention(H.P(qd), qd.stride(0), H.P(kd), kd.stride(0), 0, H.P(vd), vd.stride(0), 0, H.P(plain),
                                     plain.stride(0), 768, 2, 768, 700, 1, A.SCALE, H.S()))
    torch.cuda.synchronize()
    A.accept(o[:700], A.attn_ref64(q[:700], k, v, 2, range(700), A.SCALE)[0])
    A.accept(o[:700], plain[:700].double())


def test_any_order_gives_the_same_bits():
    shape = SHAPES[3]
    q, k, v, _ = case(shape, "own")
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    order = torch.randperm(6 * 2, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    assert torch.equal(launch(qd, kd, vd, shape, order=order)[0], launch(qd, kd, vd, shape)[0])


@pytest.mark.parametrize("what", ["Lq_pad 128", "mask_heads 3", "null mask", "misaligned Q", "valid 0"])
def test_refusals(what):
    """MC_EINVAL, nothing launched: O untouched"""
    Lq, valid, mh = 256, 256, 1
    buf = torch.zeros(3 * 256 * A.HD + 8, dtype=torch.bfloat16, device=DEV)
    q, k, v = (buf[i * 256 * A.HD:(i + 1) * 256 * A.HD].view(256, A.HD) for i in range(3))
    if what == "Lq_pad 128":
        Lq = 128
    elif what == "mask_heads 3":
        mh = 3
    elif what == "misaligned Q":
        q = buf[4:4 + 256 * A.HD].view(256, A.HD)          # 8 bytes off a 16-byte boundary
    elif what == "valid 0":
        valid = 0
    o = torch.full((256, A.HD), float("nan"), dtype=torch.bfloat16, device=DEV)
    bits = torch.full((3, 2, 1), -1, dtype=torch.int32, device=DEV)
    _, status = launch(q, k, v, (Lq, valid, 1, mh, "diag"), o=o, bits=bits, null_mask=what == "null mask")
    assert status == _lib.MC_EINVAL and "attention_sparse" in H.L().mc_last_error().decode()
    assert bool(torch.isnan(o).all()), what

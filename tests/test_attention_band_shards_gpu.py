"""GPU: the frame-block causal / windowed self-attention kernel over key shards (csrc/attention_band_shards.hip,
mc_op_attention_band_partial) against attention_cases.attn_ref64 called once per query block over its visible keys, O and the
log2-sum-exp under attention_cases.accept unchanged.

Operands are test_attention_band_gpu.py's dominant-key construction in GLOBAL token coordinates, one kind per head: a table of
keys per global token, q = 3 x the key at
  head 0  own    the row's own token: a lost key replaces that row of O
  head 1  next   hi(b), the first forbidden token above: a leak through hi replaces the row
  head 2  below  lo(b) - 1 with a window (own without): the dominant key lies just under lo
and every shard row holds its global token's key.  Padding rows and the skipped shard are hostile as in
attention_cases.every_key_case (k twice some query's dominant key, v = 1000).  A query block that sees no key: zeros and -inf.
Checked once on the CPU over the 192 parameter sets of the first test: the fp64 reference with hi moved up by one key fails
accept in head 1 in all 111 sets in which that key is a visited valid one, and with lo moved down by one key in head 2 in all
53 such window sets."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
HEADS, LQ = 3, 256
SHARDS = [(128, 65), (128, 128), (192, 129)]                    # (shard_rows, valid)
SPLITS = [(1, -1), (3, -1), (3, 0), (3, 2)]                     # (n_shards, skip)
BANDS = [(24, 0), (100, 2), (40, 3), (10000, 0)]                # (block_tokens, window_blocks)
PLACES = ["rank0", "rank1", "rank2", "round"]                   # q_tok0 = 0, valid, 2 valid over the contiguous split; a gather round


def place_of(name, valid):
    """q_tok0, key_tok0, key_tok_stride"""
    return (valid, 40, valid + 30) if name == "round" else (PLACES.index(name) * valid, 0, valid)


def bounds(tok, bt, win, hi_shift=0, lo_shift=0):
    b = tok // bt
    return ((b - win + 1).clamp(min=0) * bt if win else torch.zeros_like(b)) - lo_shift, (b + 1) * bt + hi_shift


@functools.lru_cache(maxsize=None)
def operands(shard_rows, valid, n_shards, skip, bt, win, place):
    q_tok0, key_tok0, stride = place_of(place, valid)
    g = torch.Generator().manual_seed(A.SEED)
    gq = q_tok0 + torch.arange(LQ).clamp(max=valid - 1)                      # global token of every query row
    n_tok = max(int(gq.max()), key_tok0 + (n_shards - 1) * stride + valid) + 1
    table = torch.randn(n_tok, HEADS * A.HD, generator=g).bfloat16()         # the key of every global token
    lo, hi = bounds(gq, bt, win)
    target = torch.stack([gq, hi, lo - 1 if win else gq]).clamp(0, n_tok - 1)   # [heads, LQ]
    q = torch.cat([3.0 * table[target[h], h * A.HD:(h + 1) * A.HD].float() for h in range(HEADS)], 1).bfloat16()
    rows = torch.arange(n_shards * shard_rows)
    s, j = rows // shard_rows, rows % shard_rows
    tok = key_tok0 + s * stride + j                                           # global token of every key row
    live = (j < valid) & (s != skip)
    k = table[tok.clamp(max=n_tok - 1)].clone()
    v = torch.randn(len(rows), HEADS * A.HD, generator=g).bfloat16()
    pad = (~live).nonzero()[:, 0]
    for h in range(HEADS):
        c = slice(h * A.HD, (h + 1) * A.HD)
        k[pad, c] = (2.0 * table[target[h, (pad * 7 + 5 * h) % valid], c].float()).bfloat16()
    v[pad] = 1000.0
    return q, k, v, gq, tok, live


def reference(q, k, v, gq, tok, live, bt, win, hi_shift=0, lo_shift=0):
    """fp64 O [LQ, d] and lse [HEADS, LQ]: attn_ref64 once per query block over its visible keys"""
    o = torch.zeros(LQ, HEADS * A.HD, dtype=torch.float64)
    lse = torch.full((HEADS, LQ), -float("inf"), dtype=torch.float64)
    for b in torch.unique(gq // bt):
        r = (gq // bt == b).nonzero()[:, 0]
        lo, hi = bounds(b * bt, bt, win, hi_shift, lo_shift)
        keys = (live & (tok >= lo) & (tok < hi)).nonzero()[:, 0]
        if len(keys):
            o[r], lse[:, r] = A.attn_ref64(q[r], k, v, HEADS, keys, A.SCALE)
    return o, lse


def launch(q, k, v, o, shard_rows, valid, n_shards, skip, bt, win, q_tok0, q_valid, key_tok0, stride, lse_out=None, lse_in=None):
    status = H.L().mc_op_attention_band_partial(
        H.P(q), q.stride(0), H.P(k), k.stride(0), shard_rows * k.stride(0), H.P(v), v.stride(0), shard_rows * v.stride(0), H.P(o),
        o.stride(0), q.shape[0], q.shape[1] // A.HD, shard_rows, valid, n_shards, A.SCALE, skip, None if lse_out is None else H.P(lse_out),
        None if lse_in is None else H.P(lse_in), bt, win, q_tok0, q_valid, key_tok0, stride, H.S())
    torch.cuda.synchronize()
    return status


def fresh(Lq=LQ, heads=HEADS):
    """O and lse buffers no launch has written: NaN"""
    return (torch.full((Lq, heads * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV),
            torch.full((heads, Lq), float("nan"), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("bt,win", BANDS)
@pytest.mark.parametrize("n_shards,skip", SPLITS)
@pytest.mark.parametrize("shard_rows,valid", SHARDS)
def test_against_fp64(shard_rows, valid, n_shards, skip, bt, win, place):
    q, k, v, gq, tok, live = operands(shard_rows, valid, n_shards, skip, bt, win, place)
    o_ref, lse_ref = reference(q, k, v, gq, tok, live, bt, win)
    q_tok0, key_tok0, stride = place_of(place, valid)
    o, lse = fresh()
    status = launch(q.to(DEV), k.to(DEV), v.to(DEV), o, shard_rows, valid, n_shards, skip, bt, win, q_tok0, valid, key_tok0, stride,
                    lse_out=lse)
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    print(f"rel-L2 {A.rel_l2(o.cpu(), o_ref):.3e}, rows without a key {int((lse_ref[0] == -float('inf')).sum())}")
    A.accept(o, o_ref, lse, lse_ref)


@pytest.mark.parametrize("place,bt,win,first", [("rank0", 13, 0, 0), ("rank2", 24, 2, 1)])
def test_chain(place, bt, win, first):
    """shard `first` alone with lse_out, then the others with lse_in / lse_out in place.  rank0, causal, blocks that end at the
    shard's end: every other shard is invisible, O is not touched and lse is handed on.  rank2 under a window, shard 1 first:
    the rows of blocks 7 and 8 (and all of query tile 1) see nothing in the first launch and take the second alone"""
    shard_rows, valid, n = 128, 65, 3
    q, k, v, gq, tok, live = operands(shard_rows, valid, n, -1, bt, win, place)
    o_ref, lse_ref = reference(q, k, v, gq, tok, live, bt, win)
    q_tok0, _, stride = place_of(place, valid)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o, lse = fresh()
    at = first * shard_rows
    assert launch(qd, kd[at:], vd[at:], o, shard_rows, valid, 1, -1, bt, win, q_tok0, valid, first * stride, 0, lse_out=lse) == _lib.MC_OK
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
    o1, lse1 = o.clone(), lse.clone()
    if win:
        assert bool((o1[38:] == 0).all()) and bool((lse1[:, 38:] == -float("inf")).all()) and bool(torch.isfinite(lse1[:, :38]).all())
    assert launch(qd, kd, vd, o, shard_rows, valid, n, first, bt, win, q_tok0, valid, 0, stride, lse_out=lse, lse_in=lse) == _lib.MC_OK
    assert not bool(torch.isnan(o.float()).any()) and not bool(torch.isnan(lse).any())
    if not win:
        assert torch.equal(o, o1) and torch.equal(lse, lse1), "no visible key: O untouched, lse handed on"
    A.accept(o, o_ref, lse, lse_ref)


def test_one_block_is_the_dense_partial():
    shard_rows, valid, n, skip = 192, 129, 3, 2
    c = A.every_key_build(valid, shard_rows, n, skip)
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    Lq = q.shape[0]
    (o, lse), (o_d, lse_d) = fresh(Lq, 2), fresh(Lq, 2)
    assert launch(q, k, v, o, shard_rows, valid, n, skip, 10 ** 6, 0, 0, Lq, 0, valid, lse_out=lse) == _lib.MC_OK
    _lib.check(H.L().mc_op_attention_partial(H.P(q), q.stride(0), H.P(k), k.stride(0), shard_rows * k.stride(0), H.P(v), v.stride(0),
                                             shard_rows * v.stride(0), H.P(o_d), o_d.stride(0), Lq, 2, shard_rows, valid, n, A.SCALE,
                                             skip, H.P(lse_d), None, H.S()))
    torch.cuda.synchronize()
    A.accept(o, c.o_ref, lse, c.lse_ref)
    A.accept(o, o_d.double(), lse, lse_d.double())


@pytest.mark.parametrize("what", ["block_tokens 0", "q_valid 0", "key_tok0 -1", "a token at 2^31", "skip leaves no shard"])
def test_refusals(what):
    """MC_EINVAL, nothing launched: O untouched"""
    q, k, v = (torch.zeros(256, A.HD, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    o, lse = fresh(256, 1)
    bt, q_valid, key_tok0, skip = {"block_tokens 0": (0, 256, 0, -1), "q_valid 0": (64, 0, 0, -1), "key_tok0 -1": (64, 256, -1, -1),
                                   "a token at 2^31": (64, 256, 2 ** 31 - 255, -1), "skip leaves no shard": (64, 256, 0, 0)}[what]
    status = launch(q, k, v, o, 256, 256, 1, skip, bt, 0, 0, q_valid, key_tok0, 0, lse_out=lse)
    assert status == _lib.MC_EINVAL and "attention_band_shards" in H.L().mc_last_error().decode()
    assert bool(torch.isnan(o).all()), what

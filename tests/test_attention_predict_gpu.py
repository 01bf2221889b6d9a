"""GPU: the tile-mask predictor (csrc/attention_predict.hip, mc_op_attention_tile_predict) against an fp64 restatement of its
rule, bit for bit.  Random q and k give flat shares and decide nothing, so key tile t sits around a direction e_t of its own
(orthonormal, times 4) and the q rows of a query tile weight those directions so that the pooled scores are a permutation --
another per (head, query tile) -- of vk evenly spaced levels over 4 nats, plus N(0, 0.02) noise, rounded to bf16.  Every row
>= valid of q and k is 100 times a valid row: a padding row pooled as data moves its tile's mean by orders of magnitude.
Precondition, asserted on the reference alone before any GPU call: per (head, query tile) no cumulative share of the sorted list
lies within 1e-3 of the mass, and the share at the cut differs from both neighbours by more than 1e-3 relative.  fp32 rounding
of a 128-term dot product, of a mean over <= 128 rows and of sums over <= 36 shares stays below 1e-5 relative, so inside that
margin the kernel's decisions are the fp64 ones and the words must be EQUAL.  SEED is one for which this holds at every case."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.sparse_masks import pack_tile_mask, unpack_tile_mask  # noqa: E402

DEV = "cuda:0"
SEED = 26
# (Lq_pad, valid, heads, key rows): nothing partial | partly valid last tiles, two heads | 36 key tiles: two words | two padding key tiles
SHAPES = [(256, 256, 1, 256), (512, 500, 2, 512), (2304, 2250, 1, 2304), (512, 500, 2, 640)]
MASSES = [0.5, 0.9, 1e-6]      # 1e-6: the forced tiles alone reach it


@functools.lru_cache(maxsize=None)
def case(shape):
    """q [Lq_pad, heads * 128], k [rows, heads * 128], bf16 on the CPU"""
    Lq, valid, heads, rows = shape
    vk = (valid + 63) // 64
    g = torch.Generator().manual_seed(SEED)
    q, k = torch.zeros(Lq, heads, A.HD), torch.zeros(rows, heads, A.HD)
    for h in range(heads):
        e = torch.linalg.qr(torch.randn(A.HD, vk, generator=g))[0].t()                      # [vk, 128], orthonormal rows
        k[:vk * 64, h] = (4.0 * e).repeat_interleave(64, 0)
        for qt in range(Lq // 128):
            s = torch.linspace(0, 4, vk)[torch.randperm(vk, generator=g)]                   # the pooled scores, in nats
            q[qt * 128:(qt + 1) * 128, h] = (s / (A.SCALE * 4.0)) @ e
    q, k = q + 0.02 * torch.randn(q.shape, generator=g), k + 0.02 * torch.randn(k.shape, generator=g)
    q[valid:] = 100.0 * q[(torch.arange(Lq - valid) * 7) % valid]
    k[valid:] = 100.0 * k[(torch.arange(rows - valid) * 5) % valid]
    return q.reshape(Lq, -1).bfloat16(), k.reshape(rows, -1).bfloat16()


@functools.lru_cache(maxsize=None)
def reference(shape, mass):
    """the rule in fp64 -> bool [heads, nqt, nkt]; asserts the precondition on the way"""
    Lq, valid, heads, rows = shape
    q, k = case(shape)
    nqt, nkt, vk = Lq // 128, rows // 64, (valid + 63) // 64
    live_q, live_k = (torch.arange(Lq) < valid).double(), (torch.arange(rows) < valid).double()
    n_q, n_k = live_q.view(nqt, 128).sum(1), live_k.view(nkt, 64).sum(1)
    qm = (q.double() * live_q[:, None]).view(nqt, 128, heads, A.HD).sum(1) / n_q.clamp_min(1)[:, None, None]
    km = (k.double() * live_k[:, None]).view(nkt, 64, heads, A.HD).sum(1) / n_k.clamp_min(1)[:, None, None]
    s = A.SCALE * torch.einsum("qhc,khc->hqk", qm, km)[:, :, :vk]
    w = n_k[:vk] * torch.exp(s - s.max(-1, keepdim=True).values)
    p = w / w.sum(-1, keepdim=True)
    mask = torch.zeros(heads, nqt, nkt, dtype=torch.bool)
    for h in range(heads):
        for qt in range(nqt):
            forced = [t for t in (2 * qt, 2 * qt + 1) if t < vk]
            mask[h, qt, forced] = True
            if n_q[qt] == 0:
                continue
            rest = p[h, qt].clone()
            rest[forced] = -1.0
            vals = rest.sort(descending=True).values[:vk - len(forced)]
            cum = torch.cat([p[h, qt, forced].sum()[None], p[h, qt, forced].sum() + vals.cumsum(0)])      # cum[i]: forced + the i largest
            assert float((cum - mass).abs().min()) > 1e-3, (shape, mass, h, qt)
            n = int((cum >= mass).nonzero()[0])                                                       # tiles kept beside the forced ones
            if n:
                near = vals[max(n - 2, 0):n + 1]
                assert len(near) < 2 or float((near[:-1] / near[1:]).min()) > 1 + 1e-3, (shape, mass, h, qt)
                mask[h, qt, :vk] |= p[h, qt] >= vals[n - 1]
    return mask


def predict(q, k, shape, mass, bits=None, Lq=None, valid=None, rows=None):
    _, _, heads, _ = shape
    Lq, valid, rows = (shape[0] if Lq is None else Lq), (shape[1] if valid is None else valid), (k.shape[0] if rows is None else rows)
    if bits is None:
        bits = torch.full((heads, Lq // 128, (rows // 64 + 31) // 32), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    scratch = torch.empty(H.L().mc_op_attention_tile_predict_scratch(max(Lq, 256), heads, rows) + 16, dtype=torch.uint8, device=DEV)
    status = H.L().mc_op_attention_tile_predict(H.P(q), q.stride(0), H.P(k), k.stride(0), Lq, heads, rows, valid, A.SCALE, mass,
                                                H.P(bits), H.P(scratch), H.S())
    torch.cuda.synchronize()
    return bits, status


@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predicted_words_equal_the_fp64_rule(shape, mass):
    want = reference(shape, mass)
    q, k = (x.to(DEV) for x in case(shape))
    bits, status = predict(q, k, shape, mass)
    assert status == _lib.MC_OK, H.L().mc_last_error().decode()
    assert torch.equal(bits.cpu(), pack_tile_mask(want)), (unpack_tile_mask(bits, want.shape[2]) != want).nonzero()
    assert torch.equal(predict(q, k, shape, mass)[0], bits), "the same input gives the same bits"


def test_predicted_mask_feeds_the_sparse_kernel():
    """producer and consumer agree on the layout: O over the predicted tiles against fp64 over the same tiles"""
    shape = SHAPES[1]
    Lq, valid, heads, rows = shape
    q, k = case(shape)
    v = torch.randn(rows, heads * A.HD, generator=torch.Generator().manual_seed(SEED)).bfloat16()
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    bits, status = predict(qd, kd, shape, 0.9)
    assert status == _lib.MC_OK
    o = torch.full((Lq, heads * A.HD), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.check(H.L().mc_op_attention_sparse(H.P(qd), qd.stride(0), H.P(kd), kd.stride(0), H.P(vd), vd.stride(0), H.P(o), o.stride(0),
                                            Lq, heads, rows, valid, H.P(bits), heads, None, A.SCALE, H.S()))
    torch.cuda.synchronize()
    mask = unpack_tile_mask(bits, rows // 64)
    ref = torch.zeros(Lq, heads * A.HD, dtype=torch.float64)
    for h in range(heads):
        c = slice(h * A.HD, (h + 1) * A.HD)
        for qt in range(Lq // 128):
            keys = mask[h, qt].repeat_interleave(64)[:valid].nonzero()[:, 0]
            ref[qt * 128:(qt + 1) * 128, c] = A.attn_ref64(q[qt * 128:(qt + 1) * 128, c], k[:, c], v[:, c], 1, keys, A.SCALE)[0]
    A.accept(o[:valid], ref[:valid])


@pytest.mark.parametrize("what", ["mass 0", "mass 1.5", "Lq_pad 128", "misaligned K", "valid 0", "nkt over the limit"])
def test_refusals(what):
    """MC_EINVAL, nothing launched: the mask buffer keeps its pattern"""
    shape = (256, 256, 1, 256)
    rows = 64 * 2049 if what == "nkt over the limit" else 256
    buf = torch.zeros((256 + rows) * A.HD + 8, dtype=torch.bfloat16, device=DEV)
    q = buf[:256 * A.HD].view(256, A.HD)
    off = 256 * A.HD + (4 if what == "misaligned K" else 0)                      # 8 bytes off a 16-byte boundary
    k = buf[off:off + rows * A.HD].view(rows, A.HD)
    bits = torch.full((1, 2, (rows // 64 + 31) // 32), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    _, status = predict(q, k, shape, {"mass 0": 0.0, "mass 1.5": 1.5}.get(what, 0.9), bits=bits,
                        Lq=128 if what == "Lq_pad 128" else None, valid=0 if what == "valid 0" else None)
    assert status == _lib.MC_EINVAL and "attention_tile_predict" in H.L().mc_last_error().decode()
    assert bool((bits == 0x5a5a5a5a).all()), what

"""Inputs, references and the acceptance bar of the attention edge tests (test_attention_edges_cpu.py checks the inputs and
the bar on a torch model of a bf16 flash kernel, test_attention_edges_gpu.py runs the two HIP kernels on them).  No GPU needed:
everything here is built and referenced on the CPU, once per parameter set (the builders are cached; treat what they return
as read-only).

Why these inputs.  With random keys a lost, doubled or wrongly included key moves O by about |v| / valid, which is under
the suite's 2e-2 bar for every case but valid = 1.  every_key_case makes every valid key THE key of some query (weight
>= 0.999), so losing it replaces that row of O, including a padding row hands some query the value 1000, and visiting it
twice adds one to that row's log2-sum-exp.  spike_case puts one key a chosen number of log2 units above the rest of one
query's scores, anywhere in the key sequence: attention_v5's lazy softmax reference moves at a row sum of 2^60 and the
workgroup starts over in the exact loop at 2^120."""
import functools
import math
from types import SimpleNamespace

import torch

HD = 128                                 # head_dim of both kernels
SCALE = 1.0 / math.sqrt(HD)
LOG2E = 1.4426950408889634
KT = 64                                  # keys per tile of both kernels


# ----------------------------------------------------------------------------- references
def _heads(x, heads, rows=None):
    x = x if rows is None else x[rows]
    return x.reshape(x.shape[0], heads, HD).transpose(0, 1)              # [heads, n, 128]


def _scores64(q, k, heads, key_rows, scale):
    """scaled scores in nats, fp64 [heads, Lq, len(key_rows)]"""
    return _heads(q.double(), heads) @ _heads(k.double(), heads, key_rows).transpose(1, 2) * scale


def attn_ref64(q, k, v, heads, key_rows, scale):
    """fp64 attention of q [Lq, heads*128] over the rows `key_rows` of k / v (any strides).  Returns O fp64 [Lq, heads*128]
    and the log2-sum-exp of the scaled scores, fp64 [heads, Lq]: the layout and the unit of AttnParams.lse_out."""
    s = _scores64(q, k, heads, key_rows, scale)
    o = torch.softmax(s, -1) @ _heads(v.double(), heads, key_rows)
    return o.transpose(0, 1).reshape(q.shape[0], heads * HD), torch.logsumexp(s, -1) * LOG2E


def flash_bf16_model(q, k, v, heads, key_rows, scale, prev=None, tile=KT):
    """What a correct bf16 flash kernel computes, in plain torch: Q pre-multiplied by scale * log2(e) and rounded to bf16, the
    keys `key_rows` (a list: it may drop, repeat or add rows -- the mutations of the CPU tests) visited `tile` at a time
    with a running maximum, P rounded to bf16 for the P V product, fp32 accumulation, O rounded to bf16.
    prev = (O bf16, lse): the result of an earlier launch over other keys, merged like AttnParams.lse_in.
    Returns O bf16 [Lq, heads*128] and lse fp32 [heads, Lq] (log2 units)."""
    key_rows = torch.as_tensor(key_rows, dtype=torch.long)
    Lq = q.shape[0]
    qs = _heads((q.float() * (scale * LOG2E)).bfloat16().float(), heads)
    m = torch.full((heads, Lq, 1), -math.inf)
    l = torch.zeros(heads, Lq, 1)
    o = torch.zeros(heads, Lq, HD)
    for t0 in range(0, len(key_rows), tile):
        rows = key_rows[t0:t0 + tile]
        s = qs @ _heads(k.float(), heads, rows).transpose(1, 2)
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.bfloat16().float() @ _heads(v.float(), heads, rows)
        m = m_new
    o = o / l
    lse = (m + torch.log2(l)).squeeze(-1)
    if prev is not None:
        o_prev, lse_prev = prev
        both = torch.logaddexp2(lse, lse_prev.float())
        o = (o * torch.exp2(lse - both)[..., None]
             + _heads(o_prev.float(), heads) * torch.exp2(lse_prev.float() - both)[..., None])
        lse = both
    return o.transpose(0, 1).reshape(Lq, heads * HD).bfloat16(), lse


# ----------------------------------------------------------------------------- the acceptance bar
def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def accept(o, o_ref, lse=None, lse_ref=None, v_scale=1.0):
    """The suite's bar for a bf16 attention result against attn_ref64 (tests/test_ops_gpu.py): O rtol = atol = 2e-2 and
    rel_l2 < 1e-2, the log2-sum-exp rtol = 1e-2, atol = 5e-2.  Raises AssertionError.
    v_scale: the suite's atol is stated for |v| ~ 1 ("|O| <= max|v| ~ 4").  Attention is linear in V, so a case that
    multiplies V by v_scale is judged on O / v_scale: the same check, on the same numbers, as the case with v_scale = 1.
    (Taken literally at v_scale = 1000 the atol vanishes next to |O| and the bar turns into rtol = 2e-2 on EVERY element;
    an element that cancels to |z| sigma with |z| < 0.05 misses that after one bf16 rounding of P, which is what
    flash_bf16_model does too: tests/test_attention_edges_cpu.py shows it.)"""
    got, want = o.detach().cpu().double() / v_scale, o_ref.detach().cpu().double() / v_scale
    assert bool(torch.isfinite(got).all()), "O is not finite"
    torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-2)
    e = rel_l2(got, want)
    assert e < 1e-2, f"rel_l2 {e}"
    if lse is not None:
        torch.testing.assert_close(lse.detach().cpu().double(), lse_ref.detach().cpu().double(), rtol=1e-2, atol=5e-2)


def bf16_ulp(x):
    """spacing of the bf16 numbers at |x| (8 significant bits)"""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


# ----------------------------------------------------------------------------- every key counted once
def ceil64(n):
    return (n + 63) // 64 * 64


def visited_rows(shard_rows, valid, n_shards, skip_shard=-1):
    """the rows of k / v a launch visits, in order: `valid` rows at the start of every shard but `skip_shard`"""
    return torch.cat([s * shard_rows + torch.arange(valid) for s in range(n_shards) if s != skip_shard])


def every_key_lq(valid, n_shards, skip_shard=-1):
    """the smallest multiple of 256 that holds one query per visited valid key"""
    n = valid * (n_shards - (1 if skip_shard >= 0 else 0))
    return (n + 255) // 256 * 256


@functools.lru_cache(maxsize=64)
def every_key_case(Lq, heads, shard_rows, valid, n_shards, seed, skip_shard=-1):
    """q [Lq, d], k, v [n_shards * shard_rows, d] in bf16, d = heads * 128; keys and values N(0, 1).  In every head, query
    row r is beta times the visited valid key number (r + 17 * head) mod n: with Lq >= n every visited key is the dominant
    key of a query in every head, and the heads disagree about which.  beta starts at 3 (a gap of ~25 nats at 128
    channels) and grows until the MEASURED weight of the dominant key in attn_ref64 is >= 0.999 for every (row, head).
    Padding rows [valid, shard_rows) of every shard are finite and hostile: k is twice the dominant key of some query of
    the same head (an included padding row takes that query outright), v = 1000.  So is every row of the shard left out: a
    launch that visits it anyway is as wrong as one that reads padding.
    Returns q, k, v, key_rows (visited, in order), dom [heads, Lq] (position in key_rows of each row's dominant key),
    min_weight, beta, and the fp64 reference o_ref, lse_ref over key_rows."""
    assert shard_rows % 64 == 0 and 1 <= valid <= shard_rows
    d = heads * HD
    g = torch.Generator().manual_seed(seed)
    rows = n_shards * shard_rows
    k = torch.randn(rows, d, generator=g).bfloat16()
    v = torch.randn(rows, d, generator=g).bfloat16()
    key_rows = visited_rows(shard_rows, valid, n_shards, skip_shard)
    n = len(key_rows)
    assert Lq >= n, "one query per visited key"
    dom = torch.stack([(torch.arange(Lq) + 17 * h) % n for h in range(heads)])              # [heads, Lq]
    pad_rows = torch.tensor([r for r in range(rows) if r % shard_rows >= valid or r // shard_rows == skip_shard],
                            dtype=torch.long)
    for h in range(heads):
        c = slice(h * HD, (h + 1) * HD)
        src = key_rows[(torch.arange(len(pad_rows)) * 7 + 5 * h) % n]
        k[pad_rows, c] = (2.0 * k[src, c].float()).bfloat16()
    v[pad_rows] = 1000.0
    beta = 3.0
    while True:
        q = torch.cat([(beta * k[key_rows[dom[h]], h * HD:(h + 1) * HD].float()) for h in range(heads)], 1).bfloat16()
        w = torch.softmax(_scores64(q, k, heads, key_rows, SCALE), -1)
        min_weight = float(w.gather(2, dom[..., None]).min())
        if min_weight >= 0.999 or beta >= 5.0:
            break
        beta += 0.25
    o_ref, lse_ref = attn_ref64(q, k, v, heads, key_rows, SCALE)
    return SimpleNamespace(q=q, k=k, v=v, heads=heads, shard_rows=shard_rows, valid=valid, n_shards=n_shards,
                           skip_shard=skip_shard, key_rows=key_rows, dom=dom, min_weight=min_weight, beta=beta,
                           o_ref=o_ref, lse_ref=lse_ref)


# ----------------------------------------------------------------------------- one score far above the rest
SPIKE_ROW = 7


@functools.lru_cache(maxsize=64)
def spike_case(L, heads, valid, spike_key, gap_log2, v_scale, seed, shard_rows=0):
    """The layout of test_attention_strided_qkv_and_online_softmax_rescale: q | k | v interleaved in one [L, 3d] bf16 buffer,
    N(0, 1).  Per head, with u the query SPIKE_ROW as drawn: the key `spike_key` becomes 6 u and the query a u, with a solved
    so that the spike's scaled score is gap_log2 log2 units above the next-highest score of that query -- solved on the
    bf16-rounded operands, and the gap that attn_ref64's scores then show is returned (gaps [heads]).  v is multiplied by
    v_scale.  Valid keys: the first `valid` rows, or with shard_rows > 0 the first `valid` rows of every shard_rows rows.
    Returns qkv, views q, k, v, key_rows, gaps, and the fp64 reference o_ref, lse_ref over key_rows."""
    d = heads * HD
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(L, 3 * d, generator=g).bfloat16()
    qkv[:, 2 * d:] = (qkv[:, 2 * d:].float() * v_scale).bfloat16()
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    key_rows = torch.arange(valid) if shard_rows == 0 else visited_rows(shard_rows, valid, L // shard_rows)
    pos = int((key_rows == spike_key).nonzero()[0, 0])                  # the spike must be a valid key
    u = q[SPIKE_ROW].float().clone()
    k[spike_key] = (6.0 * u).bfloat16()

    def gaps_now():
        s = _scores64(q[SPIKE_ROW:SPIKE_ROW + 1], k, heads, key_rows, SCALE)[:, 0] * LOG2E      # [heads, keys], log2 units
        rest = s.clone()
        rest[:, pos] = -math.inf
        return s[:, pos] - rest.max(-1).values

    a = torch.ones(heads, dtype=torch.float64)
    for _ in range(3):                                                  # the gap is linear in a up to the rounding of a u
        q[SPIKE_ROW] = (a.float().repeat_interleave(HD) * u).bfloat16()
        a = a * gap_log2 / gaps_now()
    q[SPIKE_ROW] = (a.float().repeat_interleave(HD) * u).bfloat16()
    gaps = gaps_now()
    o_ref, lse_ref = attn_ref64(q, k, v, heads, key_rows, SCALE)
    return SimpleNamespace(qkv=qkv, q=q, k=k, v=v, heads=heads, key_rows=key_rows, spike_key=spike_key, gaps=gaps,
                           v_scale=v_scale, o_ref=o_ref, lse_ref=lse_ref)


def check_spike(case, o, lse=None):
    """the checks of a spike case on a kernel's (or the model's) result: O finite; row SPIKE_ROW equals the spike key's v
    row within one bf16 ulp of that value (every other weight of that row is below 2^-20 at a gap of 30 and 509 keys, far
    under half an ulp); every other row meets the bar; the spike row's log2-sum-exp meets the lse bar."""
    o = o.detach().cpu()
    assert bool(torch.isfinite(o.float()).all()), "O is not finite"
    want7 = case.v[case.spike_key].double()
    err = (o[SPIKE_ROW].double() - want7).abs()
    assert bool((err <= bf16_ulp(want7)).all()), f"spike row: {float((err / bf16_ulp(want7)).max())} ulp"
    others = torch.arange(o.shape[0]) != SPIKE_ROW
    accept(o[others], case.o_ref[others], v_scale=case.v_scale)
    if lse is not None:
        lse = lse.detach().cpu().double()
        assert bool(torch.isfinite(lse).all()), "lse is not finite"
        torch.testing.assert_close(lse[:, SPIKE_ROW], case.lse_ref[:, SPIKE_ROW], rtol=1e-2, atol=5e-2)
        torch.testing.assert_close(lse[:, others], case.lse_ref[:, others], rtol=1e-2, atol=5e-2)


# ----------------------------------------------------------------------------- the parameter sets of the GPU file
SEED = 11
EVERY_KEY_VALID = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300]
EVERY_KEY_HEADS = 2


def every_key_params(valid):
    """(shard_rows, n_shards, skip_shard) of the every-key-once test for one `valid`"""
    return [(sr, ns, skip) for sr in (ceil64(valid), ceil64(valid) + 128) for ns, skips in ((1, (-1,)), (3, (-1, 0, 2)))
            for skip in skips]


def every_key_build(valid, shard_rows, n_shards, skip):
    return every_key_case(every_key_lq(valid, n_shards, skip), EVERY_KEY_HEADS, shard_rows, valid, n_shards, SEED, skip)


SPIKE_L, SPIKE_HEADS, SPIKE_VALID = 512, 2, 509
SPIKE_GAPS = sorted(list(range(30, 141, 10)) + [119, 200, 300])     # 119: just under attention_v5's 2^120 restart threshold
SPIKE_KEYS = [0, 70, 300, 440, 508]      # first tile, second tile, middle, second-last tile, last valid key (masked tail tile)
SPIKE_V_SCALES = [1.0, 1000.0]

SHARD_ROWS, SHARD_VALID, SHARD_N = 128, 127, 4
SHARD_GAPS = [50, 90, 119, 130, 300]
SHARD_SPIKES = [0 * 128 + 5, 2 * 128 + 70, 3 * 128 + 126]           # shard 0 / 2 / 3; first tile, tail tile, last valid key
MERGE_CASES = [(1, 1 * 128 + 70), (1, 3 * 128 + 126), (0, 0 * 128 + 5), (0, 2 * 128 + 70)]   # (local shard, spike key)

GRIDS = [(256, 5), (256, 7), (768, 3), (768, 5), (768, 7), (512, 9)]
GRID_SHARD_ROWS, GRID_VALID = 192, 129


def shard_spike_build(spike_key, gap, v_scale):
    return spike_case(SHARD_ROWS * SHARD_N, SPIKE_HEADS, SHARD_VALID, spike_key, gap, v_scale, SEED, shard_rows=SHARD_ROWS)


def grid_build(Lq, heads):
    return every_key_case(Lq, heads, GRID_SHARD_ROWS, GRID_VALID, 1, SEED)

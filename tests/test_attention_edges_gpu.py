"""GPU: both attention kernels on the inputs of tests/attention_cases.py, against its fp64 reference at the suite's bar.
  * every key counted once: every valid key is the dominant key of a query and every padding row would win one, at every
    `valid` around the 64-key tile and the shard edges, with extra padding tiles, over 1 and 3 shards, with a shard left out;
  * one score 2^30 .. 2^300 above the rest of its row, in the first, a middle, the second-last and the masked last tile,
    with |V| ~ 1 and ~ 1000; again over four shards and across the merge of two launches -- attention_v5 moves its lazy
    softmax reference at a row sum of 2^60 and its workgroup starts over in the exact loop at 2^120;
  * grids of 5 .. 27 workgroups that are no multiple of 8, every (head, query block) with an answer of its own.
tests/test_attention_edges_cpu.py shows that a correct bf16 kernel passes all of it and that the listed errors do not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(params=[3, 5], ids=["attn-8x32", "attn-4x64"])
def attn_variant(request):
    """both shipped kernels: attention_v3.hip (8 waves x 32 rows) forced, attention_v5.hip (4 waves x 64 rows) forced"""
    lib = _lib.load()
    _lib.check(lib.mc_set_option(b"attn_kernel", request.param))
    yield request.param
    _lib.check(lib.mc_set_option(b"attn_kernel", 0))


def run_partial(q, k, v, heads, shard_rows, valid, n_shards, shard_stride, skip=-1, prev=None):
    """one launch of attention_partial with lse_out; prev = (O, lse) of an earlier launch to merge with.  O starts as NaN
    bits (0x7fc0) unless it carries the earlier result: a row the kernel does not write fails the finiteness check."""
    Lq, d = q.shape[0], heads * A.HD
    if prev is None:
        o = torch.full((Lq, d), float("nan"), dtype=torch.bfloat16, device=DEV)
    else:
        o = prev[0].clone()
    lse = torch.full((heads, Lq), float("nan"), device=DEV)
    H.attention_partial(q, k, v, o, heads, shard_rows, valid, n_shards, A.SCALE, shard_stride, skip_shard=skip, lse_out=lse,
                        lse_in=None if prev is None else prev[1])
    return o, lse


@pytest.mark.parametrize("valid", A.EVERY_KEY_VALID)
def test_every_key_counted_once(valid, attn_variant):
    for shard_rows, n_shards, skip in A.every_key_params(valid):
        c = A.every_key_build(valid, shard_rows, n_shards, skip)
        q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
        d = c.heads * A.HD
        o, lse = run_partial(q, k, v, c.heads, shard_rows, valid, n_shards, shard_rows * d, skip)
        try:
            A.accept(o, c.o_ref, lse, c.lse_ref)
        except AssertionError as e:
            raise AssertionError(f"shard_rows {shard_rows}, n_shards {n_shards}, skip_shard {skip}: {e}") from None
        if skip < 0:                                                   # the plain entry point: the same bits
            o2 = torch.full_like(o, float("nan"))
            H.attention(q, k, v, o2, c.heads, shard_rows, valid, n_shards, A.SCALE, k_shard_stride=shard_rows * d,
                        v_shard_stride=shard_rows * d)
            assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), (shard_rows, n_shards)


def spike_views(c):
    qkv = c.qkv.to(DEV)
    d = c.heads * A.HD
    return qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]


def checked(c, o, lse, what):
    try:
        A.check_spike(c, o, lse)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


@pytest.mark.parametrize("spike_key", A.SPIKE_KEYS)
def test_spike_sweep(spike_key, attn_variant):
    for gap in A.SPIKE_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.spike_case(A.SPIKE_L, A.SPIKE_HEADS, A.SPIKE_VALID, spike_key, gap, vs, A.SEED)
            q, k, v = spike_views(c)
            o, lse = run_partial(q, k, v, c.heads, A.SPIKE_L, A.SPIKE_VALID, 1, 0)
            checked(c, o, lse, f"gap 2^{gap}, v_scale {vs}")


@pytest.mark.parametrize("spike_key", A.SHARD_SPIKES)
def test_spike_in_a_later_shard(spike_key, attn_variant):
    """Four shards of 128 rows with 127 valid keys, the spike in shard 0, 2 or 3.  (Key 510, the last valid key of the last
    tile, at a gap of 2^119 and v_scale 1000 is the case that found attention_v5's pipelined last tile without a row-sum
    check: below the 2^120 restart threshold, P ~ 2^119 times V overflowed the fp32 accumulators, O = inf.)"""
    stride = A.SHARD_ROWS * 3 * A.SPIKE_HEADS * A.HD
    for gap in A.SHARD_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.shard_spike_build(spike_key, gap, vs)
            q, k, v = spike_views(c)
            o, lse = run_partial(q, k, v, c.heads, A.SHARD_ROWS, A.SHARD_VALID, A.SHARD_N, stride)
            checked(c, o, lse, f"gap 2^{gap}, v_scale {vs}")


@pytest.mark.parametrize("local,spike_key", A.MERGE_CASES)
def test_spike_on_either_side_of_a_merge(local, spike_key, attn_variant):
    """the local shard first, then the other three merged into it through lse_in: the same bars as a single pass"""
    stride = A.SHARD_ROWS * 3 * A.SPIKE_HEADS * A.HD
    r0 = local * A.SHARD_ROWS
    for gap in A.SHARD_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.shard_spike_build(spike_key, gap, vs)
            q, k, v = spike_views(c)
            first = run_partial(q, k[r0:r0 + A.SHARD_ROWS], v[r0:r0 + A.SHARD_ROWS], c.heads, A.SHARD_ROWS, A.SHARD_VALID, 1, 0)
            o, lse = run_partial(q, k, v, c.heads, A.SHARD_ROWS, A.SHARD_VALID, A.SHARD_N, stride, skip=local, prev=first)
            checked(c, o, lse, f"gap 2^{gap}, v_scale {vs}")


@pytest.mark.parametrize("Lq,heads", A.GRIDS)
def test_grids_that_are_no_multiple_of_8(Lq, heads, attn_variant):
    c = A.grid_build(Lq, heads)
    o, lse = run_partial(c.q.to(DEV), c.k.to(DEV), c.v.to(DEV), heads, A.GRID_SHARD_ROWS, A.GRID_VALID, 1, 0)
    A.accept(o, c.o_ref, lse, c.lse_ref)

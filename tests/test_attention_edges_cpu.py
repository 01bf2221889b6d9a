"""The inputs and the bar of tests/test_attention_edges_gpu.py, checked without a GPU (tests/attention_cases.py):
  * every parameter set of the GPU file has the properties its checks rest on (dominant weights, coverage, spike gaps);
  * a correct bf16 flash kernel (flash_bf16_model) passes the GPU file's acceptance function on every one of them;
  * the same model with a wrong key list -- a key dropped, a padding row included, a key visited twice, a tile or the wrong
    shard skipped -- is rejected by it.  The mutations are the proof that the GPU tests can fail for these errors."""
import pytest
import torch

import attention_cases as A


def model(c, key_rows=None, prev=None):
    return A.flash_bf16_model(c.q, c.k, c.v, c.heads, c.key_rows if key_rows is None else key_rows, A.SCALE, prev=prev)


# ----------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("valid", A.EVERY_KEY_VALID)
def test_every_key_inputs_and_model(valid):
    for p in A.every_key_params(valid):
        c = A.every_key_build(valid, *p)
        n = len(c.key_rows)
        assert c.min_weight >= 0.999, (p, c.min_weight)
        w = torch.softmax(A._scores64(c.q, c.k, c.heads, c.key_rows, A.SCALE), -1)
        assert torch.equal(w.argmax(-1), c.dom)                        # the dominant key is the one the builder meant
        for h in range(c.heads):                                       # every visited valid key, in every head
            assert torch.equal(torch.unique(c.dom[h]), torch.arange(n)), p
        pad = (torch.arange(c.k.shape[0]) % c.shard_rows >= valid) | (torch.arange(c.k.shape[0]) // c.shard_rows == c.skip_shard)
        assert bool(torch.isfinite(c.k.float()).all()) and bool((c.v[pad] == 1000).all())
        if pad.any():                                                  # an included padding row beats a dominant key
            s = A._scores64(c.q, c.k, c.heads, torch.arange(c.k.shape[0]), A.SCALE)
            assert bool((s[:, :, pad].max(-1).values.max(-1).values > s[:, :, ~pad].max()).all())
        o, lse = model(c)
        A.accept(o, c.o_ref, lse, c.lse_ref)


@pytest.mark.parametrize("Lq,heads", A.GRIDS)
def test_grid_inputs_and_model(Lq, heads):
    c = A.grid_build(Lq, heads)
    assert c.min_weight >= 0.999
    for h in range(heads):
        assert torch.equal(torch.unique(c.dom[h]), torch.arange(A.GRID_VALID))
    # every (head, query block) has its own answer: no two blocks of O agree
    blocks = c.o_ref.reshape(Lq // 256, 256, heads, A.HD).permute(0, 2, 1, 3).reshape(-1, 256 * A.HD)
    for i in range(len(blocks)):
        for j in range(i):
            assert A.rel_l2(blocks[i], blocks[j]) > 0.5
    o, lse = model(c)
    A.accept(o, c.o_ref, lse, c.lse_ref)


@pytest.mark.parametrize("spike_key", A.SPIKE_KEYS)
def test_spike_inputs_and_model(spike_key):
    for gap in A.SPIKE_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.spike_case(A.SPIKE_L, A.SPIKE_HEADS, A.SPIKE_VALID, spike_key, gap, vs, A.SEED)
            assert float((c.gaps - gap).abs().max()) <= 1.0, (gap, c.gaps)
            # what the one-ulp check of the spike row rests on: every other key of that row weighs less than 2^-20
            rest = 1 - torch.softmax(A._scores64(c.q[A.SPIKE_ROW:A.SPIKE_ROW + 1], c.k, c.heads, c.key_rows, A.SCALE), -1)[:, 0, spike_key]
            assert float(rest.max()) < 2.0 ** -20
            A.check_spike(c, *model(c))


@pytest.mark.parametrize("spike_key", A.SHARD_SPIKES)
def test_sharded_spike_inputs_and_model(spike_key):
    for gap in A.SHARD_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.shard_spike_build(spike_key, gap, vs)
            assert len(c.key_rows) == A.SHARD_N * A.SHARD_VALID
            assert float((c.gaps - gap).abs().max()) <= 1.0, (gap, c.gaps)
            A.check_spike(c, *model(c))


@pytest.mark.parametrize("local,spike_key", A.MERGE_CASES)
def test_merged_spike_inputs_and_model(local, spike_key):
    """two launches: the local shard, then the rest merged into it"""
    first = A.visited_rows(A.SHARD_ROWS, A.SHARD_VALID, A.SHARD_N)[local * A.SHARD_VALID:(local + 1) * A.SHARD_VALID]
    rest = A.visited_rows(A.SHARD_ROWS, A.SHARD_VALID, A.SHARD_N, skip_shard=local)
    for gap in A.SHARD_GAPS:
        for vs in A.SPIKE_V_SCALES:
            c = A.shard_spike_build(spike_key, gap, vs)
            assert float((c.gaps - gap).abs().max()) <= 1.0, (gap, c.gaps)
            A.check_spike(c, *model(c, rest, prev=model(c, first)))


def test_the_bar_is_applied_at_the_scale_of_v():
    """accept(..., v_scale) judges O / v_scale.  Taken literally at v_scale = 1000 the suite's atol = 2e-2 is nothing next to
    |O| ~ 1000 and the bar becomes rtol = 2e-2 on every element: the model of a correct kernel misses it on ~6 % of the
    elements (the ones that cancel), while the same case passes with V brought back to the scale the bar was written for."""
    c = A.spike_case(A.SPIKE_L, A.SPIKE_HEADS, A.SPIKE_VALID, 300, 100, 1000.0, A.SEED)
    o, _ = model(c)
    A.accept(o, c.o_ref, v_scale=1000.0)
    with pytest.raises(AssertionError):
        A.accept(o, c.o_ref)


# ----------------------------------------------------------------------------- the mutations
def mutation_case(valid, skip=-1):
    return A.every_key_build(valid, A.ceil64(valid) + 128, 3, skip)


def rejected(c, key_rows, lse_only=False):
    o, lse = model(c, key_rows)
    if lse_only:                                                       # O alone does not see it ...
        A.accept(o, c.o_ref)
    with pytest.raises(AssertionError):                                # ... the full bar does
        A.accept(o, c.o_ref, lse, c.lse_ref)


@pytest.mark.parametrize("valid", A.EVERY_KEY_VALID)
def test_mutations_are_rejected(valid):
    c = mutation_case(valid)
    rows = c.key_rows.tolist()
    sr = c.shard_rows
    for s in range(3):
        last, pad = s * sr + valid - 1, s * sr + valid
        at = rows.index(last)
        rejected(c, rows[:at] + rows[at + 1:])                         # the last valid key of a shard dropped
        rejected(c, rows[:at + 1] + [pad] + rows[at + 1:])             # the first padding row of a shard included
        rejected(c, rows[:at + 1] + [last] + rows[at + 1:], lse_only=True)           # the shard's last key twice
        first = rows.index(s * sr)
        rejected(c, rows[:first + 1] + [s * sr] + rows[first + 1:], lse_only=True)   # ... its first key twice
    for s in (1, 2):                                                   # the first tile of a non-first shard skipped
        rejected(c, [r for r in rows if not (s * sr <= r < s * sr + 64)])
    for skip, wrong in ((0, 1), (2, 1), (-1, 0), (0, -1)):             # the skipped shard off by one (or skipped / not at all)
        c = mutation_case(valid, skip)
        rejected(c, A.visited_rows(sr, valid, 3, skip_shard=wrong).tolist())

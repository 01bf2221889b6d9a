"""CPU: magcache_amd/sparse_masks.py -- the interval construction of temporal_decay_tile_mask against the tile cover of its
element rule evaluated pair by pair, and the packing of a mask into the kernel's words."""
import numpy as np
import pytest
import torch

from magcache_amd import sparse_masks as S


def decay_rule(grid, dense, sink):
    """the element rule as the docstring states it, on broadcast index arrays"""
    tpf = (grid[1] // 2) * (grid[2] // 2)

    def vis(i, j):
        d = np.abs(i // tpf - j // tpf)
        s = np.floor(np.log2(np.maximum(d, dense) / dense)) + 1
        return (d < dense) | (j // tpf < sink) | (np.abs(i % tpf - j % tpf) * 2.0 ** s < tpf)
    return vis


@pytest.mark.parametrize("grid", [(6, 14, 18), (5, 10, 14)])
@pytest.mark.parametrize("dense,sink", [(1, 1), (2, 0)])
def test_temporal_decay_is_the_tile_cover_of_its_rule(grid, dense, sink):
    L = grid[0] * (grid[1] // 2) * (grid[2] // 2)
    got = S.temporal_decay_tile_mask(grid, dense_frames=dense, sink_frames=sink)
    want = S.tile_cover(decay_rule(grid, dense, sink), L)
    assert got.dtype == torch.bool and got.shape == (1, S.padded_len(L) // 128, S.padded_len(L) // 64)
    assert torch.equal(got[0], want)
    qt = torch.arange((L + 127) // 128)
    assert bool(got[0, qt, 2 * qt].all()), "the diagonal is always visible"


@pytest.mark.parametrize("nkt", [4, 32, 36, 70])
def test_packing_round_trips(nkt):
    m = torch.rand(2, 3, nkt, generator=torch.Generator().manual_seed(nkt)) < 0.5
    words = S.pack_tile_mask(m)
    assert words.dtype == torch.int32 and words.shape == (2, 3, (nkt + 31) // 32) and words.is_contiguous()
    assert torch.equal(S.unpack_tile_mask(words, nkt), m)
    w = words.numpy().view(np.uint32)
    kt = 3 if nkt == 4 else nkt - 1
    assert bool((w[1, 2, kt >> 5] >> (kt & 31)) & 1) == bool(m[1, 2, kt])

"""sparse_masks.shard_tile_cover against a brute-force loop over element pairs, at shard lengths that are no multiple of the
tile (L / P = 150, 100, 165, 110), and against tile_cover on one shard."""
import numpy as np
import pytest
import torch

from magcache_amd.sparse_masks import padded_len, shard_tile_cover, tile_cover


def band(i, j):
    return (np.abs(i - j) < 40) | (j < 3)


def rule(kind, L):
    if kind == "band":
        return band, band(np.arange(L)[:, None], np.arange(L)[None, :])
    m = torch.rand(L, L, generator=torch.Generator().manual_seed(L)) < 0.002
    return m, m.numpy()


@pytest.mark.parametrize("kind", ["band", "random"])
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("L", [300, 330])
def test_shard_tile_cover_is_the_brute_force_cover(L, P, kind):
    vis, elems = rule(kind, L)
    Lr = L // P
    tpr = padded_len(Lr) // 64
    for rank in range(P):
        want = np.zeros((padded_len(Lr) // 128, P * tpr), dtype=bool)
        for i, j in zip(*elems.nonzero()):
            if i // Lr == rank:
                want[(i - rank * Lr) // 128, (j // Lr) * tpr + (j % Lr) // 64] = True
        got = shard_tile_cover(vis, L, rank, P)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), want), (rank, P)
        assert 0 < want.sum() < want.size


@pytest.mark.parametrize("kind", ["band", "random"])
def test_one_shard_is_tile_cover(kind):
    vis, _ = rule(kind, 300)
    assert torch.equal(shard_tile_cover(vis, 300, 0, 1), tile_cover(vis, 300))

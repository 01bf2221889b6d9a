"""CPU: the tile-sparse joint attention is declared, exported and bound; sparse_masks.joint_tile_mask agrees with its element
rule in both row orders."""
import os
import re

import numpy as np
import pytest
import torch

from magcache_amd import _lib
from magcache_amd.sparse_masks import joint_tile_mask, tile_cover

NAMES = ("mc_op_attention_joint_sparse", "mc_mmdit_set_attention_tile_mask", "mc_mmdit_set_attention_tile_mass",
         "mc_mmdit_attention_tile_state", "mc_mmdit_read_attention_tile_mask")


def test_calls_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "magcache_mmdit.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # host-side refusal without a device: a null operand is MC_EINVAL before any launch
    assert lib.mc_op_attention_joint_sparse(None, 384, None, 384, None, 384, None, 384, 256, 1, 256, 256, None, 1, 0, 2, 0, 0, None,
                                            0.1, None) == _lib.MC_EINVAL
    assert b"attention_joint_sparse" in lib.mc_last_error()


@pytest.mark.parametrize("text_first,lt,li", [(True, 64, 288), (False, 32, 324), (True, 100, 300), (False, 256, 130), (True, 128, 128)])
def test_joint_tile_mask_is_the_tile_cover_of_its_element_rule(text_first, lt, li):
    nqi, nki = (li + 127) // 128, (li + 63) // 64
    img = torch.rand(2, nqi, nki, generator=torch.Generator().manual_seed(lt + li)) < 0.4
    got = joint_tile_mask(img, text_first, lt, li)
    img0, S = (lt if text_first else 0), lt + li
    assert got.shape == (2, (S + 255) // 256 * 2, (S + 255) // 256 * 4)
    for h in range(2):
        m = img[h].numpy()

        def vis(i, j):
            both = (i >= img0) & (i < img0 + li) & (j >= img0) & (j < img0 + li)
            return both & m[np.clip(i - img0, 0, li - 1) // 128, np.clip(j - img0, 0, li - 1) // 64]
        assert torch.equal(got[h], tile_cover(vis, S)), h
    with pytest.raises(ValueError):
        joint_tile_mask(img[:, :, :nki - 1], text_first, lt, li)

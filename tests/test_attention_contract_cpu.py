"""CPU: the argument contract of the four attention launchers (ops.h: attention_shape_ok, attention_plain_form and each
kernel's own conditions), asked through mc_test_attention_accepts of the reference library.  Nothing is launched and no
pointer is dereferenced: the pointers below are integers.

The table is the specification.  Every verdict is written out by hand from the conditions of the launchers:
  v3    shape; ldo % 4; ldk * 128 and ldv * 128 below 2^31; no pointer check, no check of skip / lse
  v5    shape; ldo % 8; O, lse_in, lse_out 16-byte aligned (null counts as aligned); ldq * 512 and ldo * 512 below 2^31;
        ((n_shards - 1) stride + (shard_rows + 256) ld) * 2 below 2^32 for K and for V; 0 <= stride, stride * 2 below 2^32;
        at least one shard visited after the skip
  band  shape; plain form; block_tokens >= 1, window_blocks >= 0; shard_rows * ld * 2 (K, V) and Lq_pad * ld * 2 (Q, O) below
        2^32; with a window at most 16383 query tiles of 128 rows
  mx8   shape; plain form; Lq_pad * d and shard_rows * d below 2^32 (d = n_heads * 128); six images non-null, 16-byte aligned
  shape       Lq_pad > 0 and % 256 == 0, shard_rows % 64 == 0, 1 <= shard_valid <= shard_rows, n_heads > 0, n_shards >= 1,
              ldq, ldk, ldv % 8 == 0
  plain form  one shard, no skip, no lse, ldo % 8 == 0, every ld >= d, Q, K, V, O non-null and 16-byte aligned
"""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hip_ops as H  # noqa: E402

KERNELS = ("v3", "v5", "band", "mx8")
ARGS = ("Q", "ldq", "K", "ldk", "kss", "V", "ldv", "vss", "O", "ldo", "Lq_pad", "n_heads", "shard_rows", "shard_valid", "n_shards",
        "skip_shard_p1", "lse_in", "lse_out", "block_tokens", "window_blocks", "q_img", "q_sc", "k_img", "k_sc", "vt_img", "v_sc")
# two heads (d = 256), one shard of 128 rows with 100 keys, a causal band of 32-token blocks: every kernel accepts it
VALID = dict(Q=0x10000, ldq=256, K=0x20000, ldk=256, kss=0, V=0x30000, ldv=256, vss=0, O=0x40000, ldo=256, Lq_pad=256, n_heads=2,
             shard_rows=128, shard_valid=100, n_shards=1, skip_shard_p1=0, lse_in=None, lse_out=None, block_tokens=32,
             window_blocks=0, q_img=0x100000, q_sc=0x200000, k_img=0x300000, k_sc=0x400000, vt_img=0x500000, v_sc=0x600000)
ALL, NONE = "v3 v5 band mx8", ""
TWO_SHARDS = dict(n_shards=2, kss=128 * 256, vss=128 * 256)

# (case, what differs from VALID, the kernels that accept it)
TABLE = [
    ("valid", {}, ALL),
    ("Lq_pad 128", dict(Lq_pad=128), NONE),
    ("Lq_pad 0", dict(Lq_pad=0), NONE),
    ("shard_rows 96", dict(shard_rows=96, shard_valid=90), NONE),
    ("valid 0", dict(shard_valid=0), NONE),
    ("valid > rows", dict(shard_valid=129), NONE),
    ("valid == rows", dict(shard_valid=128), ALL),
    ("n_heads 0", dict(n_heads=0), NONE),
    ("n_shards 0", dict(n_shards=0), NONE),
    ("n_shards 2", TWO_SHARDS, "v3 v5"),
    ("skip set, two shards", dict(TWO_SHARDS, skip_shard_p1=1), "v3 v5"),
    # the v3 launcher itself does not look at the skip (launch_attention refuses this form before it picks a kernel)
    ("skip set, one shard: none left to visit", dict(skip_shard_p1=1), "v3"),
    ("lse_out set", dict(lse_out=0x50000), "v3 v5"),
    ("lse_in set", dict(lse_in=0x50000), "v3 v5"),
    ("lse_out misaligned by 8", dict(lse_out=0x50008), "v3"),
    ("lse_in misaligned by 4", dict(lse_in=0x50004), "v3"),
    ("ldq % 8 != 0", dict(ldq=260), NONE),
    ("ldk % 8 != 0", dict(ldk=260), NONE),
    ("ldv % 8 != 0", dict(ldv=260), NONE),
    ("ldo 4 mod 8", dict(ldo=260), "v3"),
    ("ldo 2 mod 4", dict(ldo=258), NONE),
    ("ldq < n_heads * 128", dict(ldq=128), "v3 v5"),
    ("ldk < n_heads * 128", dict(ldk=128), "v3 v5"),
    ("ldo < n_heads * 128", dict(ldo=128), "v3 v5"),
    # inherited: the plain form compares ld with d as unsigned, so only band's 32-bit row offsets refuse a negative one
    ("negative ldq", dict(ldq=-256), "v3 v5 mx8"),
    ("O misaligned by 8", dict(O=0x40008), "v3"),
    ("K misaligned by 8", dict(K=0x20008), "v3 v5"),
    ("null Q", dict(Q=None), "v3 v5"),
    ("null V", dict(V=None), "v3 v5"),
    ("null O", dict(O=None), "v3 v5"),
    # v3: ldk * 128 < 2^31.  At 2^24 the 128 rows are also band's 2^32 bytes and far past v5's span; mx8 has no such bound
    ("ldk at the v3 bound", dict(ldk=1 << 24), "mx8"),
    ("ldk just under the v3 bound", dict(ldk=(1 << 24) - 8), "v3 band mx8"),
    ("ldv at the v3 bound", dict(ldv=1 << 24), "mx8"),
    ("ldv just under the v3 bound", dict(ldv=(1 << 24) - 8), "v3 band mx8"),
    # v5: (shard_rows + 256) * ldk * 2 < 2^32 with one shard ...
    ("K span at the v5 bound, one shard", dict(shard_rows=(1 << 23) - 256), "v3 band mx8"),
    ("K span just under the v5 bound, one shard", dict(shard_rows=(1 << 23) - 320), ALL),
    # ... and (kss + (128 + 256) * 256) * 2 < 2^32 with two
    ("K span at the v5 bound, two shards", dict(TWO_SHARDS, kss=(1 << 31) - 384 * 256), "v3"),
    ("K span just under the v5 bound, two shards", dict(TWO_SHARDS, kss=(1 << 31) - 384 * 256 - 1), "v3 v5"),
    ("V span at the v5 bound, two shards", dict(TWO_SHARDS, vss=(1 << 31) - 384 * 256), "v3"),
    ("negative K shard stride", dict(TWO_SHARDS, kss=-8), "v3"),
    ("block_tokens 0", dict(block_tokens=0), "v3 v5 mx8"),
    ("window_blocks -1", dict(window_blocks=-1), "v3 v5 mx8"),
    ("window, 16384 query tiles", dict(Lq_pad=16384 * 128, window_blocks=1), "v3 v5 mx8"),
    ("no window, 16384 query tiles", dict(Lq_pad=16384 * 128), ALL),
    ("window, 16382 query tiles", dict(Lq_pad=16382 * 128, window_blocks=1), ALL),
    # mx8: Lq_pad * d < 2^32; band's Lq_pad * ldq * 2 is past 2^32 in both
    ("Lq_pad * d at 2^32", dict(Lq_pad=1 << 24), "v3 v5"),
    ("Lq_pad * d just under 2^32", dict(Lq_pad=(1 << 24) - 256), "v3 v5 mx8"),
    ("V^T image misaligned by 8", dict(vt_img=0x500008), "v3 v5 band"),
    ("null q scale image", dict(q_sc=None), "v3 v5 band"),
]


@pytest.fixture(scope="module")
def accepts():
    fn = H.ref_lib().mc_test_attention_accepts
    fn.restype, fn.argtypes = C.c_int, H.TEST_SIGNATURES["mc_test_attention_accepts"]
    return lambda kernel, args: fn(kernel.encode(), *[args[a] for a in ARGS])


@pytest.mark.parametrize("name,diff,verdict", TABLE, ids=[t[0] for t in TABLE])
def test_attention_contract(accepts, name, diff, verdict):
    assert set(diff) <= set(ARGS) and set(verdict.split()) <= set(KERNELS)
    args = dict(VALID, **diff)
    got = {k: accepts(k, args) for k in KERNELS}
    assert got == {k: int(k in verdict.split()) for k in KERNELS}


def test_unknown_kernel_is_not_a_verdict(accepts):
    assert accepts("v4", VALID) == -1

"""GPU: the MagCache residual capture where the last main layer of a VACE model receives a hint.  There the residual is taken by a
launch of its own behind the hint and not by FFN-2's epilogue; both ways share the bookkeeping that follows (statistics, flags,
slot swap).  Toy configs, inputs and helpers are those of tests/test_wan_geometry_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import hip_ops as H  # noqa: E402
from magcache_amd.engine import MC_MODE_CALIB, MC_MODE_SKIP  # noqa: E402
from test_wan_geometry_gpu import G105, bits, condition, inputs, make_engine, toy  # noqa: E402


def test_vace_hint_on_the_last_layer_calibrates_what_full_forwards_cache():
    """toy("vace"): three layers, control blocks on 0 and 2.  A CALIB forward runs the kernels of a FULL one on the same inputs,
    so it must leave the same output and residual bit for bit, have statistics from its second forward on -- the calibration
    kernel's own over the two residuals, bit for bit (tests/test_ops_gpu.py pins that kernel to torch) -- and a SKIP forward
    must read the slot the calibration swapped in.  The other branch stays untouched."""
    e = make_engine(toy("vace"), G105)
    condition(e, "vace", G105)
    lat, ctx, _, _ = inputs("vace", G105)
    steps = ((lat, 700.0), (lat * 0.9 + 0.05, 550.0))
    skip = lambda: bits(e.forward(lat, 400.0, ctx[1], branch=1, mode=MC_MODE_SKIP))   # noqa: E731
    want = [(bits(e.forward(x, t, ctx[1], branch=1)), e.residual(1).clone()) for x, t in steps]
    want_skip = skip()
    e.reset()
    for i, (x, t) in enumerate(steps):
        got = bits(e.forward(x, t, ctx[1], branch=1, mode=MC_MODE_CALIB))
        assert torch.equal(got, want[i][0]), f"CALIB forward {i}: output"
        assert torch.equal(bits(e.residual(1)), bits(want[i][1])), f"CALIB forward {i}: residual"
        assert e.calib_has_stats(1) == (i == 1) and not e.calib_has_stats(0)
    stats, _ = H.calib_stats(want[1][1], want[0][1])
    assert bool(torch.isfinite(stats).all()) and bool(stats.any())
    assert not torch.equal(bits(want[0][1]), bits(want[1][1]))
    assert torch.equal(bits(e.buffer("calib_stats", torch.float32)[3:6]), bits(stats))
    assert torch.equal(skip(), want_skip)

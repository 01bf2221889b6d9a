"""Qwen-Image / Qwen-Image-Edit host logic without a GPU: the MagCache decision of the monkey-patch shims vs the
reference's own functions (tests/golden/qwen_image_golden.npz, tools/gen_golden_qwen.py), the linspace interpolation,
the RoPE tables vs the QwenEmbedRope restatement, the sigma schedule, the C ABI declarations."""
import json
import os
import re

import numpy as np
import pytest
import torch

from magcache_amd import _lib
from magcache_amd import mmdit as MM
from magcache_amd.sampler import qwen_image_sigmas

import qwen_image_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "qwen_image_golden.npz"))
    return g, json.loads(str(g["meta"]))


class _StubEngine:
    def reset(self):
        pass

    def residual(self, branch=None):
        return torch.zeros(1)


def _stub_model(modes):
    """a QwenImageTransformer2DModelHIP without an engine: _run records (mode, branch)"""
    cls = type("QwenStub", (MM.QwenImageTransformer2DModelHIP,), {})
    m = cls.__new__(cls)
    m.engine = _StubEngine()
    cls._run = lambda self, *a: modes.append((a[-2], a[-1])) or torch.zeros(1, 1, 1)
    return m


@pytest.mark.parametrize("key", ["qwen_image", "qwen_image_edit"])
@pytest.mark.parametrize("steps", [50, 9, 30])
def test_qwen_schedule_matches_reference(golden, key, steps):
    g, meta = golden
    modes = []
    m = _stub_model(modes)
    MM.init_qwen_magcache(m, steps, 0.06, 2, 0.2, edit=(key == "qwen_image_edit"))
    np.testing.assert_array_equal(type(m).mag_ratios, meta["mag_ratios"][f"{key}|steps{steps}"])
    for _ in range(2 * steps):
        m(hidden_states=None, encoder_hidden_states=None, timestep=None, img_shapes=None, txt_seq_lens=None)
    assert [int(mo == MM.MC_MODE_SKIP) for mo, _ in modes] == meta["sched"][f"{key}|steps{steps}"]
    assert [b for _, b in modes] == [i % 2 for i in range(2 * steps)]
    assert m.cnt == 0                                  # wrapped; the accumulators are not reset (reference :242-244)


def test_qwen_golden_loops_are_reference_schedules(golden):
    """the skip lists of the recorded sampling loops (model in the loop) equal the host rule's"""
    g, meta = golden
    for name, steps, kw, edit in (("t2i", 50, {}, False), ("interp", 9, dict(magcache_thresh=0.24, K=4), False),
                                  ("edit", 12, dict(magcache_thresh=0.24, K=4), True)):
        modes = []
        m = _stub_model(modes)
        MM.init_qwen_magcache(m, steps, kw.get("magcache_thresh", 0.06), kw.get("K", 2), 0.2, edit=edit)
        for _ in range(2 * steps):
            m(hidden_states=None, encoder_hidden_states=None, timestep=None, img_shapes=None, txt_seq_lens=None)
        assert [int(mo == MM.MC_MODE_SKIP) for mo, _ in modes] == g[f"{name}_skipped"].tolist(), name


def test_qwen_linspace_interp_matches_reference(golden):
    g, meta = golden
    probe = np.arange(11, dtype=np.float64) * 1.5
    for n, want in meta["nearest_interp"].items():
        np.testing.assert_array_equal(MM.qwen_nearest_interp(probe, int(n)), want)
    np.testing.assert_array_equal(meta["mag_ratios"]["qwen_image|steps9"], g["interp_mag_ratios"])


@pytest.mark.parametrize("shapes,txt", [([(1, 58, 104)], 40), ([(1, 58, 104), (1, 64, 64)], 17), ([(1, 5, 7)], 3)])
def test_qwen_rope_matches_restatement(shapes, txt):
    cos, sin = MM.qwen_rope(shapes, txt)
    img, tf = QR.QwenEmbedRope(10000, (16, 56, 56), scale_rope=True)([shapes], [txt])
    rc, rs = QR.complex_to_cos_sin(torch.cat([tf, img], 0))
    assert cos.shape == (txt + sum(f * h * w for f, h, w in shapes), 128)
    torch.testing.assert_close(cos, rc, rtol=0, atol=2e-6)
    torch.testing.assert_close(sin, rs, rtol=0, atol=2e-6)


def _restated_sigmas(n, seq_len, base_seq=256, max_seq=8192, base_shift=0.5, max_shift=0.9, terminal=0.02):
    # FlowMatchEulerDiscreteScheduler.set_timesteps(sigmas=linspace(1, 1/n, n), mu=calculate_shift(...)), restated in
    # its own steps: calculate_shift, _time_shift_exponential, stretch_shift_to_terminal, append 0
    m = (max_shift - base_shift) / (max_seq - base_seq)
    mu = seq_len * m + base_shift - m * base_seq
    s = torch.from_numpy(np.linspace(1.0, 1 / n, n)).float().double()
    s = np.exp(mu) / (np.exp(mu) + (1 / s - 1) ** 1.0)
    one = 1 - s
    s = 1 - one / (one[-1] / (1 - terminal))
    return np.concatenate([s.float().numpy(), [0.0]])


@pytest.mark.parametrize("steps,seq", [(50, 6032), (9, 48), (30, 4096 + 1024)])
def test_qwen_sigmas(steps, seq):
    sig, ts = qwen_image_sigmas(steps, seq)
    assert sig.shape == (steps + 1,) and ts.shape == (steps,)
    assert np.all(np.diff(sig) < 0) and sig[0] == pytest.approx(1.0) and sig[-1] == 0.0
    assert sig[-2] == pytest.approx(0.02, abs=1e-6)          # shift_terminal: the last nonzero sigma
    np.testing.assert_allclose(sig, _restated_sigmas(steps, seq), rtol=0, atol=1e-6)
    np.testing.assert_allclose(ts, sig[:-1] * 1000, rtol=1e-6)


def test_qwen_abi_declared():
    hdr = open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read()
    assert re.search(r"MC_FAMILY_QWEN\s*=\s*2", hdr) and _lib.MC_FAMILY_QWEN == 2
    assert "mc_mmdit_forward2(" in hdr and "mc_mmdit_forward2" in _lib.SIGNATURES
    hip = open(os.path.join(ROOT, "include", "magcache_hip.h")).read()
    for n in ("mc_op_cfg_norm_euler", "mc_op_rmsnorm_rows_bf16"):
        assert n + "(" in hip and n in _lib.SIGNATURES


def test_qwen_cli_parses_reference_flags():
    from magcache_amd import qwen_generate as QG
    a = QG._parse_args([])
    assert (a.sample_steps, a.true_cfg_scale, a.magcache_thresh, a.magcache_K, a.retention_ratio) == (50, 4.0, 0.06, 2, 0.2)
    assert a.use_magcache is True and a.magcache_calibration is False
    a = QG._parse_args(["--sample_steps", "20", "--magcache_calibration", "--edit"])
    assert a.sample_steps == 20 and a.magcache_calibration and a.edit

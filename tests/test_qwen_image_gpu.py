"""GPU parity of Qwen-Image / Qwen-Image-Edit on the MM-DiT engine (MC_FAMILY_QWEN, include/magcache_mmdit.h): one
full-width forward at the 16:9 image size vs the fp32 restatement (tests/qwen_image_ref.py) with prompts of different
lengths, the 100-call MagCache loop, calibration and Edit vs the golden of the reference's own functions
(tests/golden/qwen_image_golden.npz), the true-CFG step and txt_norm kernels, error paths."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd.sampler import cfg_norm_euler_, qwen_image_sigmas, sample_qwen_image  # noqa: E402

import qwen_image_ref as QR  # noqa: E402

DEV = "cuda:0"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


def record(cls):
    """(mode, branch) of every forward a shim class issues"""
    calls, base = [], cls.__mro__[1]._run

    def _run(self, *a):
        calls.append((a[-2], a[-1]))
        return base(self, *a)
    cls._run = _run
    return calls


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "qwen_image_golden.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    oracle = QR.init_synthetic_(QR.QwenImageTransformer2DModel(**cfg), seed=meta["weight_seed"], std=meta["weight_std"])
    t = lambda k: torch.from_numpy(g[k]).to(DEV)  # noqa: E731
    return g, meta, cfg, oracle, t


def _model(golden, img_tokens, calibration=False):
    g, meta, cfg, oracle, t = golden
    cls = type("QwenHIPUnderTest", (MM.QwenImageTransformer2DModelHIP,), {})
    m = cls(cfg, img_tokens, txt_len=int(g["prompt_embeds"].shape[1]), device=DEV, calibration=calibration)
    m.load_state_dict(oracle.state_dict())
    return m


def test_qwen_full_width_forward_vs_oracle():
    """3072 / 24 heads / FFN 12288 / txt_dim 3584, 2 double blocks, the 16:9 image (58 x 104 = 6032 tokens); the cond
    prompt (45 tokens) and then the shorter negative prompt (7) through ONE engine sized for 45: each equals the fp32
    restatement run at its exact, unpadded length.  Bar: 2e-2 relative L2 (the FLUX / HunyuanVideo forward bar)."""
    cfg = dict(QR.QWEN_IMAGE, num_layers=2)
    torch.manual_seed(0)
    with torch.device(DEV):
        oracle = QR.QwenImageTransformer2DModel(**cfg)
    QR.init_synthetic_(oracle, seed=11, std=0.02)
    shapes = [[(1, 58, 104)]]
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(1, 6032, 64, generator=g, device=DEV)
    pe = torch.randn(1, 45, 3584, generator=g, device=DEV)
    ne = torch.randn(1, 7, 3584, generator=g, device=DEV)
    t = torch.tensor([0.731], device=DEV)
    torch.backends.cuda.matmul.allow_tf32 = False
    with torch.no_grad():   # the fp32 restatement (torch, on the device only to keep the test short; fp32 math)
        want = [oracle(hidden_states=x, encoder_hidden_states=e, timestep=t, img_shapes=shapes, txt_seq_lens=[e.shape[1]],
                       return_dict=False)[0] for e in (pe, ne)]
    m = MM.QwenImageTransformer2DModelHIP(cfg, 6032, txt_len=45, device=DEV, calibration=False)
    m.load_state_dict(oracle.state_dict())
    del oracle
    got = [m(hidden_states=x, encoder_hidden_states=e, timestep=t, img_shapes=shapes, txt_seq_lens=[e.shape[1]],
             return_dict=False)[0] for e in (pe, ne)]
    errs = [rel_l2(a, b) for a, b in zip(got, want)]
    assert max(errs) < 2e-2, errs
    # 45 / 7 text keys beside 6032 image keys move the output by ~2e-3 at these weights (below the bf16 error): the
    # exact-length behaviour is pinned at toy size by the golden tests, where the text dominates
    assert rel_l2(want[0], want[1]) > 5e-4


def test_qwen_magcache_loop_vs_reference_golden(golden):
    """100 calls (50 steps, cond / uncond alternating, prompts of 37 and 5 tokens) through qwen_magcache_forward and the
    HIP true-CFG step: the reference's skip list, the recorded outputs and the final latent within tolerance."""
    g, meta, cfg, oracle, t = golden
    m = _model(golden, 48)
    MM.init_qwen_magcache(m, 50, meta["thresh"], meta["K"], meta["R"])
    calls = record(type(m))
    outs = {}
    idx = set(g["t2i_idx"].tolist())
    n = [0]

    def keep(model_out):
        if n[0] in idx:
            outs[n[0]] = model_out[0].float().cpu()
        n[0] += 1
    base = type(m).__call__

    def call(self, *a, **k):
        o = base(self, *a, **k)
        keep(o[0])
        return o
    type(m).__call__ = call
    x = sample_qwen_image(m, t("latent0"), t("prompt_embeds"), t("negative_prompt_embeds"), [[(1, 6, 8)]], 50,
                          meta["true_cfg_scale"])
    assert [int(mo == MM.MC_MODE_SKIP) for mo, _ in calls] == g["t2i_skipped"].tolist()
    assert [b for _, b in calls] == [i % 2 for i in range(100)]
    errs = [rel_l2(outs[c], g["t2i_outs"][k].astype(np.float32)) for k, c in enumerate(g["t2i_idx"].tolist())]
    assert max(errs) < 3e-2, errs
    assert rel_l2(x[0], g["t2i_final"]) < 3e-2
    assert m.cnt == 0


def test_qwen_residual_slots_are_per_branch(golden):
    """cond FULL, uncond FULL, then cond SKIP and uncond SKIP on the same inputs: each skip reproduces ITS branch's full
    output (a single slot would hand the cond call the uncond residual)."""
    g, meta, cfg, oracle, t = golden
    m = _model(golden, 48)
    e = m.engine
    e.reset()
    m.engine.set_rope(*MM.qwen_rope([(1, 6, 8)], m.txt_len))
    m._shapes_key = ((1, 6, 8),)
    x, pe, ne = t("latent0")[0], t("prompt_embeds")[0], t("negative_prompt_embeds")[0]
    full = [e.forward(x, 500.0, 0, emb, emb.shape[0], None, MM.MC_MODE_FULL, branch=b).clone() for b, emb in ((0, pe), (1, ne))]
    skip = [e.forward(x, 500.0, 0, emb, emb.shape[0], None, MM.MC_MODE_SKIP, branch=b).clone() for b, emb in ((0, pe), (1, ne))]
    assert rel_l2(full[0], full[1]) > 1e-2
    for b in (0, 1):
        assert float((skip[b] - full[b]).abs().max()) < 1e-4 * float(full[b].abs().max())
    assert not torch.equal(e.residual(0), e.residual(1))


def test_qwen_calibration_vs_reference_golden(golden):
    g, meta, cfg, oracle, t = golden
    want = meta["calib"]
    m = _model(golden, 48, calibration=True)
    MM.init_qwen_magcache(m, want["steps"], calibration=True)
    cls = type(m)
    with contextlib.redirect_stdout(io.StringIO()):
        sample_qwen_image(m, t("latent0"), t("prompt_embeds"), t("negative_prompt_embeds"), [[(1, 6, 8)]], want["steps"],
                          meta["true_cfg_scale"])
    assert len(cls.norm_ratio) == 2 * want["steps"] - 2
    np.testing.assert_allclose(cls.norm_ratio, want["norm_ratio"], rtol=0, atol=1e-3)
    np.testing.assert_allclose(cls.norm_std, want["norm_std"], rtol=0, atol=5e-4)
    np.testing.assert_allclose(cls.cos_dis, want["cos_dis"], rtol=0, atol=4e-4)


def test_qwen_edit_vs_reference_golden(golden):
    """Edit: 48 noisy + 16 reference-image tokens (frame 1 of the RoPE); the model output covers all 64, the sampler
    updates the first 48; interpolated Edit table, 12 steps."""
    g, meta, cfg, oracle, t = golden
    m = _model(golden, 64)
    assert m.engine.img_tokens == 48 + 16
    ed = meta["edit"]
    MM.init_qwen_magcache(m, ed["steps"], ed["thresh"], ed["K"], ed["R"], edit=True)
    calls = record(type(m))
    outs = []
    base = type(m).__call__

    def call(self, *a, **k):
        o = base(self, *a, **k)
        outs.append(o[0][0].float().cpu())
        return o
    type(m).__call__ = call
    x = sample_qwen_image(m, t("latent0"), t("prompt_embeds"), t("negative_prompt_embeds"), [[(1, 6, 8), (1, 4, 4)]],
                          ed["steps"], meta["true_cfg_scale"], image_latents=t("ref_latent"))
    assert [int(mo == MM.MC_MODE_SKIP) for mo, _ in calls] == g["edit_skipped"].tolist()
    assert outs[0].shape == (64, 64)
    errs = [rel_l2(o, g["edit_outs"][i].astype(np.float32)) for i, o in enumerate(outs)]
    assert max(errs) < 3e-2, errs
    assert x.shape == (1, 48, 64) and rel_l2(x[0], g["edit_final"]) < 3e-2


def test_qwen_interpolated_table_loop(golden):
    g, meta, cfg, oracle, t = golden
    m = _model(golden, 48)
    it = meta["interp"]
    MM.init_qwen_magcache(m, it["steps"], it["thresh"], it["K"], it["R"])
    np.testing.assert_array_equal(type(m).mag_ratios, g["interp_mag_ratios"])
    calls = record(type(m))
    x = sample_qwen_image(m, t("latent0"), t("prompt_embeds"), t("negative_prompt_embeds"), [[(1, 6, 8)]], it["steps"],
                          meta["true_cfg_scale"])
    assert [int(mo == MM.MC_MODE_SKIP) for mo, _ in calls] == g["interp_skipped"].tolist()
    assert rel_l2(x[0], g["interp_final"]) < 3e-2


def test_cfg_norm_euler_op():
    g = torch.Generator(device=DEV).manual_seed(3)
    rows, n, c = 300, 257, 64
    cond = torch.randn(rows, c, generator=g, device=DEV)
    unc = torch.randn(rows, c, generator=g, device=DEV)
    cond[5] = 0.0                                 # the zero-norm row: comb = 0 exactly (and |c| = 0)
    unc[5] = 0.0
    x = torch.randn(n, c, generator=g, device=DEV)
    want = QR.true_cfg_euler(x.clone(), cond, unc, 4.0, -0.0375)
    want[5] = x[5]                                # defined result: v = 0 (torch gives NaN there)
    got = x.clone()
    cfg_norm_euler_(got, cond, unc, 4.0, -0.0375)
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    # rows >= n of the predictions are not read, rows of x beyond n untouched
    big = torch.randn(n + 3, c, generator=g, device=DEV)
    keep = big.clone()
    cfg_norm_euler_(big[:n], cond, unc, 4.0, -0.0375)
    assert torch.equal(big[n:], keep[n:])


def test_rmsnorm_rows_bf16_op():
    import ctypes as C
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(4)
    rows, valid, d = 70, 37, 3584
    x = torch.randn(rows, d, generator=g, device=DEV) * 3
    w = 1 + 0.1 * torch.randn(d, generator=g, device=DEV)
    out = torch.full((rows, d), 7.0, device=DEV, dtype=torch.bfloat16)
    _lib.check(lib.mc_op_rmsnorm_rows_bf16(C.c_void_p(x.data_ptr()), d, C.c_void_p(w.data_ptr()), 1e-6,
                                           C.c_void_p(out.data_ptr()), d, valid, rows, d,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    xc, wc = x[:valid].cpu(), w.cpu()
    want = xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + 1e-6) * wc
    torch.testing.assert_close(out[:valid].float().cpu(), want, rtol=8e-3, atol=8e-3)
    assert not out[valid:].float().abs().any()


def test_qwen_errors(golden):
    g, meta, cfg, oracle, t = golden
    m = _model(golden, 48)
    e = m.engine
    x, pe = t("latent0")[0], t("prompt_embeds")[0]
    m.engine.set_rope(*MM.qwen_rope([(1, 6, 8)], m.txt_len))
    for bad in (0, m.txt_len + 1):
        with pytest.raises(_lib.MagCacheHipError, match="txt_valid"):
            e.forward(x, 500.0, 0, pe, bad, None, MM.MC_MODE_FULL, branch=0)
    with pytest.raises(_lib.MagCacheHipError, match="branch"):
        e.forward(x, 500.0, 0, pe, 10, None, MM.MC_MODE_FULL, branch=2)
    e.reset()
    with pytest.raises(_lib.MagCacheHipError, match="residual cache is empty"):
        e.forward(x, 500.0, 0, pe, 10, None, MM.MC_MODE_SKIP, branch=1)
    d = cfg["attention_head_dim"] * cfg["num_attention_heads"]
    args = (MM.MC_FAMILY_QWEN, d, cfg["num_attention_heads"], 2)
    with pytest.raises(_lib.MagCacheHipError, match="single-stream"):
        MM.MMDiTEngine(*args, 1, 64, 64, 256, 40, 0, 48, device=DEV)
    with pytest.raises(_lib.MagCacheHipError, match="one GPU"):
        MM.MMDiTEngine(*args, 0, 64, 64, 256, 40, 0, 48, device=DEV, sp_rank=0, sp_size=2)
    with pytest.raises(_lib.MagCacheHipError, match="pooled"):
        MM.MMDiTEngine(*args, 0, 64, 64, 256, 40, 768, 48, device=DEV)
    sd = dict(oracle.state_dict())
    del sd["transformer_blocks.1.txt_mlp.net.2.bias"]
    fresh = MM.QwenImageTransformer2DModelHIP(cfg, 48, txt_len=40, device=DEV, calibration=False)
    with pytest.raises(KeyError, match="txt_mlp.net.2.bias"):
        fresh.load_state_dict(sd)

"""Generate tests/golden/qwen_image_golden.npz by RUNNING THE REFERENCE'S OWN MagCache functions around the CPU
restatement of the Qwen-Image transformer (tests/qwen_image_ref.py).

    python tools/gen_golden_qwen.py          (needs the reference checkout: MAGCACHE_REFERENCE, default /root/reference)

MagCache4QwenImage/magcache_generate.py cannot be imported (it loads the diffusers pipeline at import time): the source
text of its `nearest_interp`, `init_magcache`, `init_magcache_calibration`, `magcache_calibration` and
`magcache_forward` definitions is read from the file and exec'd with stub globals (USE_PEFT_BACKEND = False, ...).
The same is done with MagCache4QwenImageEdit/magcache_generate.py for the Edit case.  The sampling loop around the
model is the pipeline's (cond then uncond per step, the norm-preserving true-CFG combine, the flow-Euler step) on the
Qwen-Image sigma schedule of magcache_amd.sampler.qwen_image_sigmas, all in fp32.

Cases (toy sizes, fp32; outputs of the recorded calls stored as fp16 to keep the file small):
  t2i      50 steps = 100 calls, cond / uncond prompts of different lengths, the Qwen-Image table (no interpolation)
  interp   9 steps: the table is re-interpolated per branch with the reference's linspace nearest_interp
  edit     Qwen-Image-Edit: noisy tokens + reference-image tokens, the Edit table, 12 steps (interpolated)
  calib    magcache_calibration statistics over 6 steps
  sched    skip lists of the reference rule for both tables at 50 steps and at 9 / 30 steps
"""
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MAGCACHE_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import qwen_image_ref as QR  # noqa: E402
from magcache_amd.mag_ratios import TABLES  # noqa: E402
from magcache_amd.sampler import qwen_image_sigmas  # noqa: E402

NAMES = ("nearest_interp", "init_magcache", "init_magcache_calibration", "magcache_calibration", "magcache_forward")


def reference_functions(script):
    path = os.path.join(REF, script)
    src = open(path).read().split("\n")

    def block(name):
        first = next(i for i, l in enumerate(src) if l.startswith(f"def {name}("))
        # the signature's closing ") -> ...:" line starts in column 0 too
        last = next(i for i in range(first + 1, len(src)) if src[i] and not src[i][0].isspace() and not src[i].startswith(")"))
        return "\n".join(src[first:last]), first + 1

    from typing import Any, Dict, List, Optional, Tuple, Union
    import torch.nn.functional as F

    class Transformer2DModelOutput:
        def __init__(self, sample):
            self.sample = sample

    g = dict(torch=torch, np=np, F=F, Any=Any, Dict=Dict, List=List, Optional=Optional, Tuple=Tuple, Union=Union,
             USE_PEFT_BACKEND=False, scale_lora_layers=None, unscale_lora_layers=None,
             Transformer2DModelOutput=Transformer2DModelOutput)
    for name in NAMES:
        code, line = block(name)
        exec(compile("\n" * (line - 1) + code, path, "exec"), g)
    return types.SimpleNamespace(**{k: g[k] for k in NAMES})


def fresh_model(cfg, seed, std):
    cls = type("PatchedQwenImage", (QR.QwenImageTransformer2DModel,), {})
    return cls, QR.init_synthetic_(cls(**cfg), seed=seed, std=std)


def run_loop(ref, cfg, steps, lat0, pe, ne, img_shapes, args, table, record, image_latents=None, calibration=False):
    """the pipeline loop around the reference-patched model; returns (skipped per call, recorded outputs, final latent,
    the class after the run)"""
    cls, model = fresh_model(cfg, 7, 0.04)
    if calibration:
        ref.init_magcache_calibration(model, args)
    else:
        ref.init_magcache(model, list(table[2:]), args)
    ran = []
    hook = model.transformer_blocks[0].register_forward_hook(lambda *a: ran.append(1))
    n = lat0.shape[1]
    sig, _ = qwen_image_sigmas(steps, n)
    x = lat0.clone()
    skipped, outs = [], {}
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        for i in range(steps):
            t = torch.tensor([float(sig[i]) * 1000.0])
            inp = x if image_latents is None else torch.cat([x, image_latents], dim=1)
            preds = []
            for j, emb in enumerate((pe, ne)):
                n0 = len(ran)
                o = model(hidden_states=inp, encoder_hidden_states=emb, timestep=t / 1000, img_shapes=img_shapes,
                          txt_seq_lens=[emb.shape[1]], return_dict=False)[0]
                c = 2 * i + j
                skipped.append(len(ran) == n0)
                if c in record:
                    outs[c] = o[0].numpy().copy()
                preds.append(o)
            x = QR.true_cfg_euler(x, preds[0], preds[1], args.true_cfg_scale, float(sig[i + 1] - sig[i]))
    hook.remove()
    return skipped, outs, x, model


def main():
    torch.manual_seed(0)
    ref = reference_functions("MagCache4QwenImage/magcache_generate.py")
    ref_edit = reference_functions("MagCache4QwenImageEdit/magcache_generate.py")
    cfg = QR.tiny_config(num_layers=2, heads=2, joint_attention_dim=256)
    g = torch.Generator().manual_seed(41)
    h2, w2, hr, wr = 6, 8, 4, 4                      # 48 noisy tokens; Edit: + 16 reference-image tokens
    lc, lu = 37, 5                                   # cond prompt vs the " " negative prompt: different lengths
    lat0 = torch.randn(1, h2 * w2, 64, generator=g)
    ref_lat = torch.randn(1, hr * wr, 64, generator=g)
    pe = torch.randn(1, lc, cfg["joint_attention_dim"], generator=g)
    ne = torch.randn(1, lu, cfg["joint_attention_dim"], generator=g)

    def args(steps, **kw):
        return types.SimpleNamespace(**dict(dict(sample_steps=steps, true_cfg_scale=4.0, magcache_thresh=0.06, magcache_K=2,
                                                 retention_ratio=0.2), **kw))

    out = dict(latent0=lat0.numpy(), ref_latent=ref_lat.numpy(), prompt_embeds=pe.numpy(), negative_prompt_embeds=ne.numpy())
    meta = dict(cfg={k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, h2=h2, w2=w2, hr=hr, wr=wr,
                weight_seed=7, weight_std=0.04, true_cfg_scale=4.0, thresh=0.06, K=2, R=0.2)
    t2i_shapes = [[(1, h2, w2)]]
    edit_shapes = [[(1, h2, w2), (1, hr, wr)]]
    # ---- t2i, 50 steps (100 calls)
    rec = set(range(0, 100, 7)) | {98, 99}
    sk, outs, x, cls = run_loop(ref, cfg, 50, lat0, pe, ne, t2i_shapes, args(50), TABLES["qwen_image"], rec)
    assert int(cls.cnt) == 0 and sum(sk) > 0, (int(cls.cnt), sum(sk))
    idx = sorted(outs)
    out.update(t2i_skipped=np.array(sk, np.int8), t2i_idx=np.array(idx), t2i_outs=np.stack([outs[i] for i in idx]).astype(np.float16),
               t2i_final=x[0].numpy())
    print("t2i skipped", sum(sk), "of", len(sk))
    # ---- interpolated table, 9 steps
    sk, outs, x, cls = run_loop(ref, cfg, 9, lat0, pe, ne, t2i_shapes, args(9, magcache_thresh=0.24, magcache_K=4),
                                TABLES["qwen_image"], set(range(18)))
    out.update(interp_skipped=np.array(sk, np.int8), interp_outs=np.stack([outs[i] for i in range(18)]).astype(np.float16),
               interp_final=x[0].numpy(), interp_mag_ratios=np.asarray(cls.mag_ratios, np.float64))
    meta["interp"] = dict(steps=9, thresh=0.24, K=4, R=0.2)
    print("interp skipped", [int(s) for s in sk])
    # ---- Edit: 12 steps, Edit table (interpolated), noisy + reference tokens
    sk, outs, x, cls = run_loop(ref_edit, cfg, 12, lat0, pe, ne, edit_shapes, args(12, magcache_thresh=0.24, magcache_K=4),
                                TABLES["qwen_image_edit"], set(range(24)), image_latents=ref_lat)
    out.update(edit_skipped=np.array(sk, np.int8), edit_outs=np.stack([outs[i] for i in range(24)]).astype(np.float16),
               edit_final=x[0].numpy())
    meta["edit"] = dict(steps=12, thresh=0.24, K=4, R=0.2)
    print("edit skipped", [int(s) for s in sk])
    # ---- calibration, 6 steps
    _, _, _, cls = run_loop(ref, cfg, 6, lat0, pe, ne, t2i_shapes, args(6), None, set(), calibration=True)
    meta["calib"] = dict(steps=6, norm_ratio=list(cls.norm_ratio), norm_std=list(cls.norm_std), cos_dis=list(cls.cos_dis))
    # ---- schedules of the reference rule (the decision never looks at the model output: a one-block model suffices)
    one = QR.tiny_config(num_layers=1, heads=2, joint_attention_dim=256)
    sched, interp = {}, {}
    for key, r in (("qwen_image", ref), ("qwen_image_edit", ref_edit)):
        for steps in (50, 9, 30):
            a = args(steps)
            sk, _, _, cls = run_loop(r, one, steps, lat0[:, :16], pe[:, :4], ne[:, :2], [[(1, 4, 4)]], a, TABLES[key], set())
            sched[f"{key}|steps{steps}"] = [int(s) for s in sk]
            interp[f"{key}|steps{steps}"] = np.asarray(cls.mag_ratios, np.float64).tolist()
    meta["sched"], meta["mag_ratios"] = sched, interp
    # the reference's own nearest_interp on a few lengths
    probe = np.arange(11, dtype=np.float64) * 1.5
    meta["nearest_interp"] = {str(n): ref.nearest_interp(probe, n).tolist() for n in (1, 2, 5, 11, 17, 40)}
    np.savez_compressed(os.path.join(GOLD, "qwen_image_golden.npz"), meta=json.dumps(meta), **out)
    print("  qwen_image_golden.npz", os.path.getsize(os.path.join(GOLD, "qwen_image_golden.npz")))


if __name__ == "__main__":
    main()

"""Generate tests/golden/flux_ip_adapter_golden.npz by RUNNING THE REFERENCE'S OWN magcache_forward / magcache_calibration
with joint_attention_kwargs["ip_adapter_image_embeds"] around the CPU FLUX restatement (oracle/flux_ref.py) carrying the
IP-Adapter modules of tests/flux_ip_adapter_ref.py.

    python tools/gen_golden_flux_ip_adapter.py     (needs the reference checkout: MAGCACHE_REFERENCE, default /root/reference)

The two functions are read from MagCache4FLUX/magcache_flux.py at run time and exec'd with stub globals, as
tools/gen_golden_flux_controlnet.py does; the model, its weights, the inputs and the sigma schedule are those of
tests/golden/flux_forward_golden.npz.  What the reference's code pins is that the key is popped, run through
self.encoder_hid_proj and handed to every block as ip_hidden_states; the block side is the helper's restatement.

Cases (toy FLUX: 2 double + 3 single blocks, 108 image tokens, fp32; outputs stored as fp16):
  one              adapter A (4 tokens per image), 1 image, scale 1: the MagCache loop
  two              adapters A and B (16 tokens per image, 2 images = 32 keys), per-block scales A (1.0, 0.5), B (0.0, 0.8)
  calib            magcache_calibration statistics of `one`
  last_double      the toy with num_single_layers = 0 and adapter A, one forward at t = 0.5
  with_controlnet  `one` plus the `each` samples of flux_controlnet_golden.npz, one forward at t = 0.5
The embeds are multiples of 1/16 (int8 numerators).  Asserted here and recorded in meta: every case moves the reference's own
output by more than 3 x LOOP_BAR (relative L2 against the same case without the key), and `two` differs from `one` by as much.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flux_ip_adapter_ref as IR  # noqa: E402
from magcache_amd.ip_adapter import normalise_scales  # noqa: E402
from magcache_amd.mag_ratios import TABLES  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402
from oracle.gen_golden_mmdit import fresh, reference_flux_functions  # noqa: E402

LOOP_BAR = 3e-2                        # tests/test_flux_controlnet_gpu.py
EMBED_DIM, CROSS_DIM = 64, 256
ADAPTERS = dict(A=dict(spec=(EMBED_DIM, CROSS_DIM, 4), seed=101, n_images=1),
                B=dict(spec=(EMBED_DIM, CROSS_DIM, 16), seed=202, n_images=2))
IP_STD = 0.012                          # synthetic IP weight scale: large enough for the margins asserted below
CASES = dict(one=dict(adapters=["A"], scale=1.0), two=dict(adapters=["A", "B"], scale=[[1.0, 0.5], [0.0, 0.8]]))
LAST_DOUBLE_SEED = 11


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    torch.manual_seed(0)
    ref = reference_flux_functions()
    base = np.load(os.path.join(GOLD, "flux_forward_golden.npz"))
    cn = np.load(os.path.join(GOLD, "flux_controlnet_golden.npz"))
    meta = json.loads(str(base["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    steps = meta["steps"]
    lat0, sig = torch.from_numpy(base["latent0"]), base["sigmas"]
    kw = dict(encoder_hidden_states=torch.from_numpy(base["ctx"]), pooled_projections=torch.from_numpy(base["pooled"]),
              img_ids=torch.from_numpy(base["img_ids"]), txt_ids=torch.from_numpy(base["txt_ids"]),
              guidance=torch.tensor([meta["guidance"]]), return_dict=False)
    g = torch.Generator().manual_seed(88)
    embeds_q = {k: torch.randn(a["n_images"], EMBED_DIM, generator=g).mul(16).round().clamp(-127, 127).to(torch.int8)
                for k, a in ADAPTERS.items()}

    def embeds(names):
        return [embeds_q[k].float()[None] / 16 for k in names]

    def patched(forward, case, cfg=cfg, seed=meta["weight_seed"]):
        cls = fresh(FR.FluxTransformer2DModel)
        model = FR.init_synthetic_(cls(**cfg), seed=seed, std=meta["weight_std"])
        names = CASES[case]["adapters"]
        IR.add_ip_adapters_(model, [ADAPTERS[k]["spec"] for k in names], [ADAPTERS[k]["seed"] for k in names], IP_STD)
        IR.set_ip_adapter_scale(model, normalise_scales(CASES[case]["scale"], len(names), cfg["num_layers"]))
        cls.forward = forward
        cls.cnt, cls.num_steps = 0, steps
        cls.norm_ratio, cls.norm_std, cls.cos_dis = [], [], []
        cls.mag_ratios = ref.nearest_interp(np.asarray(TABLES["flux_dev"]), steps)
        cls.K, cls.magcache_thresh, cls.retention_ratio = meta["K"], meta["thresh"], meta["R"]
        cls.accumulated_ratio, cls.accumulated_err, cls.accumulated_steps = 1, 0, 0
        return cls, model

    def loop(forward, case, n_calls, with_ip=True):
        cls, model = patched(forward, case)
        seen, ran, skipped, outs = [], [], [], []
        # the pinned part: encoder_hid_proj receives the popped list, every double block receives its result
        h1 = model.encoder_hid_proj.register_forward_hook(lambda m, a, out: seen.append(len(out)))
        h2 = model.transformer_blocks[0].register_forward_hook(lambda *a: ran.append(1))
        jak = dict(ip_adapter_image_embeds=embeds(CASES[case]["adapters"])) if with_ip else None
        x = lat0.clone()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            for i in range(n_calls):
                n0 = len(ran)
                o = model(hidden_states=x, timestep=torch.tensor([float(sig[i])]), joint_attention_kwargs=jak, **kw)[0]
                skipped.append(len(ran) == n0)
                outs.append(o[0].numpy().copy())
                x = x + float(sig[i + 1] - sig[i]) * o
        h1.remove()
        h2.remove()
        assert seen == ([len(CASES[case]["adapters"])] * n_calls if with_ip else [])
        assert jak is None or "ip_hidden_states" not in jak, "the reference works on a copy of the caller's dict"
        return cls, skipped, np.stack(outs)

    out, cases, loops = {}, {}, {}
    for name in ("one", "two"):
        cls, skipped, outs = loop(ref.magcache_forward, name, steps)
        assert cls.cnt == 0 and sum(skipped) > 0
        _, _, plain = loop(ref.magcache_forward, name, steps, with_ip=False)
        moved = rel(outs, plain)
        assert moved > 3 * LOOP_BAR, (name, moved)
        loops[name] = outs
        out[name + "_outs"] = outs.astype(np.float16)
        out[name + "_skipped"] = np.array(skipped, dtype=np.int8)
        cases[name] = dict(adapters=CASES[name]["adapters"], scale=CASES[name]["scale"], moved=round(moved, 4),
                           first_call_moved=round(rel(outs[0], plain[0]), 4),
                           same_skips_as_base=bool(skipped == [bool(s) for s in base["skipped"]]))
        print(name, "skipped", [int(s) for s in skipped], "moved the output by", moved, "first call", cases[name]["first_call_moved"])
    two_vs_one = rel(loops["two"], loops["one"])
    two_vs_one_first = rel(loops["two"][0], loops["one"][0])
    assert two_vs_one > 3 * LOOP_BAR and two_vs_one_first > 3 * LOOP_BAR, (two_vs_one, two_vs_one_first)
    assert cases["one"]["first_call_moved"] > 3 * LOOP_BAR and cases["two"]["first_call_moved"] > 3 * LOOP_BAR
    print("two vs one", two_vs_one, "first call", two_vs_one_first)

    cls, *_ = loop(ref.magcache_calibration, "one", steps - 1)
    calib = dict(norm_ratio=list(cls.norm_ratio), norm_std=list(cls.norm_std), cos_dis=list(cls.cos_dis))

    def single(case, cfg_, seed, jak, **extra):
        _, model = patched(ref.magcache_forward, case, cfg_, seed)
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            return model(hidden_states=lat0.clone(), timestep=torch.tensor([0.5]), joint_attention_kwargs=jak, **extra, **kw)[0][0].numpy().copy()

    cfg_ld = dict(cfg, num_single_layers=0)
    ld = single("one", cfg_ld, LAST_DOUBLE_SEED, dict(ip_adapter_image_embeds=embeds(["A"])))
    ld_moved = rel(ld, single("one", cfg_ld, LAST_DOUBLE_SEED, None))
    assert ld_moved > 3 * LOOP_BAR, ld_moved
    out["last_double_out"] = ld.astype(np.float16)

    cscale = json.loads(str(cn["meta"]))["sample_scale"]
    samples = dict(controlnet_block_samples=[torch.from_numpy(q).float()[None] * cscale for q in cn["double_q"]],
                   controlnet_single_block_samples=[torch.from_numpy(q).float()[None] * cscale for q in cn["single_q"]])
    wc = single("one", cfg, meta["weight_seed"], dict(ip_adapter_image_embeds=embeds(["A"])), **samples)
    wc_moved = rel(wc, single("one", cfg, meta["weight_seed"], None, **samples))
    assert wc_moved > 3 * LOOP_BAR, wc_moved
    out["with_controlnet_out"] = wc.astype(np.float16)
    print("last_double moved", ld_moved, "with_controlnet moved", wc_moved)

    info = dict(embed_scale=1 / 16, embed_dim=EMBED_DIM, cross_dim=CROSS_DIM, ip_std=IP_STD, loop_bar=LOOP_BAR,
                adapters={k: dict(spec=list(a["spec"]), seed=a["seed"], n_images=a["n_images"]) for k, a in ADAPTERS.items()},
                cases=cases, two_vs_one=round(two_vs_one, 4), two_vs_one_first_call=round(two_vs_one_first, 4), calib=calib,
                last_double=dict(weight_seed=LAST_DOUBLE_SEED, timestep=0.5, moved=round(ld_moved, 4)),
                with_controlnet=dict(timestep=0.5, moved=round(wc_moved, 4)))
    path = os.path.join(GOLD, "flux_ip_adapter_golden.npz")
    np.savez_compressed(path, meta=json.dumps(info), **{"embeds_%s_q" % k: v.numpy() for k, v in embeds_q.items()}, **out)
    print("  flux_ip_adapter_golden.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()

"""`python -m magcache_amd.qwen_generate` -- MagCache4QwenImage/magcache_generate.py (and MagCache4QwenImageEdit's) on the
HIP MM-DiT engine.  Same flags and defaults as the reference's `_parse_args` (:23-61):

    --sample_steps 50 --true_cfg_scale 4.0 --magcache_thresh 0.06 --magcache_K 2 --retention_ratio 0.2
    --use_magcache (default on) --magcache_calibration

What is outside the transformer and absent offline is declared, not faked: there is no Qwen2.5-VL text encoder and
no VAE in this repository.  So
  * the prompt embeddings come from `--prompt_embeds_file` / `--negative_prompt_embeds_file` (torch tensors
    [len, 3584]: the pipeline's encode_prompt output, template prefix dropped, unpadded), or -- without them -- are
    seeded synthetic stand-ins of the reference's two prompt lengths (a warning says so);
  * the transformer weights come from `--weights_file` (a diffusers state_dict saved with torch.save), or are seeded
    random weights of the Qwen-Image geometry (a warning says so);
  * Edit (`--edit`) takes the VAE latent of the reference image as `--image_latents_file` (packed [N_ref, 64]) or a
    synthetic stand-in of the reference's 1024 x 1024 area;
  * the result saved to `--save_file` is the final packed LATENT [N, 64] (fp32, torch.save) that the pipeline would
    unpack and decode with its VAE.
Use the Python API (magcache_amd.mmdit.QwenImageTransformer2DModelHIP + magcache_amd.sampler.sample_qwen_image) to
pass precomputed embeddings directly.
"""
import argparse
import logging
import sys

ASPECT_RATIOS = {"1:1": (1328, 1328), "16:9": (1664, 928), "9:16": (928, 1664), "4:3": (1472, 1104),
                 "3:4": (1104, 1472), "3:2": (1584, 1056), "2:3": (1056, 1584)}


def _parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate an image from a text prompt using Qwen Image with MagCache")
    p.add_argument("--sample_steps", type=int, default=50, help="The sampling steps.")
    p.add_argument("--true_cfg_scale", type=float, default=4.0, help="Classifier free guidance scale.")
    p.add_argument("--magcache_thresh", type=float, default=0.06, help="Upper bound of accumulated error for MagCache")
    p.add_argument("--retention_ratio", type=float, default=0.2, help="Retention ratio of unchanged steps for MagCache")
    p.add_argument("--magcache_K", type=int, default=2, help="Max skip steps for MagCache")
    p.add_argument("--use_magcache", action="store_true", default=True, help="Use MagCache for inference after calibration")
    p.add_argument("--magcache_calibration", action="store_true", default=False, help="Calibrate magnitude ratios for MagCache")
    # not in the reference's argparse (its pipeline owns these): the inputs that replace the absent encoder / VAE
    p.add_argument("--edit", action="store_true", default=False, help="Qwen-Image-Edit: reference-image tokens, Edit table")
    p.add_argument("--aspect_ratio", default="16:9", choices=sorted(ASPECT_RATIOS))
    p.add_argument("--prompt_embeds_file", default=None)
    p.add_argument("--negative_prompt_embeds_file", default=None)
    p.add_argument("--image_latents_file", default=None)
    p.add_argument("--weights_file", default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--save_file", default="qwen_image_latent.pt")
    return p.parse_args(argv)


def generate(args):
    import torch
    from magcache_amd import mmdit as MM
    from magcache_amd.sampler import sample_qwen_image

    log = logging.getLogger("qwen_generate")
    dev = "cuda:0"
    width, height = ASPECT_RATIOS[args.aspect_ratio] if not args.edit else (1024, 1024)
    h2, w2 = height // 16, width // 16
    shapes = [(1, h2, w2)]
    g = torch.Generator().manual_seed(args.seed)
    ref_lat = None
    if args.edit:
        ref_lat = (torch.load(args.image_latents_file) if args.image_latents_file else torch.randn(h2 * w2, 64, generator=g))
        ref_lat = ref_lat.reshape(1, -1, 64).float().to(dev)
        shapes.append((1, h2, w2))
        if ref_lat.shape[1] != h2 * w2:
            raise ValueError("--image_latents_file: the reference image must be packed at the output's latent grid here")
    if args.prompt_embeds_file:
        pe = torch.load(args.prompt_embeds_file).float().reshape(1, -1, 3584)
        ne = torch.load(args.negative_prompt_embeds_file).float().reshape(1, -1, 3584)
    else:
        log.warning("no Qwen2.5-VL text encoder offline: synthetic prompt embeddings (cond 120 tokens, negative 6)")
        pe, ne = torch.randn(1, 120, 3584, generator=g), torch.randn(1, 6, 3584, generator=g)
    img_tokens = sum(f * h * w for f, h, w in shapes)
    model = MM.QwenImageTransformer2DModelHIP(MM.QWEN_IMAGE, img_tokens, txt_len=max(pe.shape[1], ne.shape[1]), device=dev,
                                              calibration=args.magcache_calibration)
    if args.weights_file:
        model.load_state_dict(torch.load(args.weights_file, map_location="cpu"))
    else:
        log.warning("no checkpoint offline: seeded random Qwen-Image weights")
        from magcache_amd.qwen_bench import random_state_dict
        model.load_state_dict(random_state_dict(MM.QWEN_IMAGE, dev, seed=args.seed))
    if args.magcache_calibration or args.use_magcache:
        MM.init_qwen_magcache(model, args.sample_steps, args.magcache_thresh, args.magcache_K, args.retention_ratio,
                              calibration=args.magcache_calibration, edit=args.edit)
    lat = torch.randn(1, h2 * w2, 64, generator=g).to(dev)
    out = sample_qwen_image(model, lat, pe.to(dev), ne.to(dev), [shapes], args.sample_steps, args.true_cfg_scale,
                            image_latents=ref_lat)
    torch.save(out[0].cpu(), args.save_file)
    log.info("saved the final latent %s to %s", tuple(out.shape), args.save_file)
    return out


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(levelname)s: %(message)s", stream=sys.stdout)
    generate(_parse_args(argv))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Full-size MM-DiT measurements on one MI355X (BASELINE.json configs 0 and 2; parity-test configurations, not the
headline bench line):

    python tools/bench_mmdit.py flux      FLUX.1-dev 512x512, 28 steps: no-cache vs MagCache (thresh 0.24, K 5, R 0.1)
    python tools/bench_mmdit.py hunyuan   HunyuanVideo 720p 129 frames: full / skipped forward times, model TFLOP/s
    (a trailing `two_streams` runs the text half of every double block on a second HIP stream)
    python tools/bench_mmdit.py flux --controlnet 5,10
                                          FLUX.1-dev 1024x1024, one full forward with 5 double + 10 single random bf16
                                          ControlNet samples vs the same forward without, alternating, ms per forward
    python tools/bench_mmdit.py flux --regeometry 512x512,1024x1024
    python tools/bench_mmdit.py qwen --regeometry 1664x928,928x1664
                                          ONE engine (one copy of the weights) switched between the image sizes with
                                          MMDiTEngine.set_geometry, against a fresh engine per size: per size the full-forward
                                          time of both (alternating windows), the set_geometry time with and without reserve(),
                                          the workspace bytes, and the HBM the weights hold once (`--depth D,S`: fewer blocks)
    python tools/bench_mmdit.py flux --fp8_linear 0,2,3 [--size 1024x1024,512x512] [--depth D,S]
    python tools/bench_mmdit.py qwen --fp8_linear 0,2,3 [--size 1664x928]
                                          one engine per mc_mmdit_config.fp8_linear mode on the same weights and inputs, full
                                          forwards in alternating windows: ms per forward and the spread of the windows per mode,
                                          workspace bytes, distance of every mode's output from the first mode's
                                          `--mx_fp4` adds, per mode 2 | 3 of the list, an MXFP4 engine (option "mx_fp4": W4A4,
                                          opt-in) as "<mode>+mxfp4" and the same engine with fp8_fused_quant 0 (separate quantise
                                          passes instead of the fused FP4 producers) as "<mode>+mxfp4 separate";
                                          `--mx_fp6` adds an MXFP6 engine (option "mx_fp6": W6A6, opt-in, always separate
                                          quantise passes) as "<mode>+mxfp6"

    python tools/bench_mmdit.py flux --ip-adapter TOKENS[xIMAGES][,...] [--depth D,S]
                                          FLUX.1-dev 1024x1024, one full forward with one IP-Adapter per entry (768-wide embeds,
                                          cross_dim 4096, TOKENS per image, IMAGES images) against the same engine without
                                          the key, alternating windows; the set_ip_adapter_image wall time (projection,
                                          LayerNorm and the K|V of every double block) and the kernel and the add alone at
                                          the forward's shapes (mc_op_ip_attention, mc_op_add_rows)

Synthetic inputs, seeded random-init weights of the real architecture (no checkpoints offline).  One JSON line each.
Also checks the size-independent MagCache properties at full size: a skipped forward equals the final layer applied
to ori + cached residual, i.e. re-running a skip is idempotent and finite.
"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd._lib import load  # noqa: E402

DEV = "cuda:0"


def synth_load(model, names_shapes, seed=0, std=0.02):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for name, shape in names_shapes:
        if "norm" in name and name.endswith("weight") and len(shape) == 1:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g, device=DEV)
        else:
            t = std * torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)
        model.engine.set_weight(name, t.to(torch.bfloat16) if t.dim() > 1 and t.shape[0] > 64 else t)
    model.engine.load_weights({})          # raises if anything is missing


def flux_names(cfg):
    d = cfg["attention_head_dim"] * cfg["num_attention_heads"]
    out = [("x_embedder.weight", (d, cfg["in_channels"])), ("x_embedder.bias", (d,)),
           ("context_embedder.weight", (d, cfg["joint_attention_dim"])), ("context_embedder.bias", (d,)),
           ("norm_out.linear.weight", (2 * d, d)), ("norm_out.linear.bias", (2 * d,)),
           ("proj_out.weight", (cfg["in_channels"], d)), ("proj_out.bias", (cfg["in_channels"],))]
    for e, k in (("timestep_embedder", 256), ("guidance_embedder", 256), ("text_embedder", cfg["pooled_projection_dim"])):
        out += [(f"time_text_embed.{e}.linear_1.weight", (d, k)), (f"time_text_embed.{e}.linear_1.bias", (d,)),
                (f"time_text_embed.{e}.linear_2.weight", (d, d)), (f"time_text_embed.{e}.linear_2.bias", (d,))]

    def lin(p, n_out, n_in):
        return [(p + ".weight", (n_out, n_in)), (p + ".bias", (n_out,))]
    for i in range(cfg["num_layers"]):
        p = f"transformer_blocks.{i}."
        out += lin(p + "norm1.linear", 6 * d, d) + lin(p + "norm1_context.linear", 6 * d, d)
        for n in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"):
            out += lin(p + "attn." + n, d, d)
        out += [(p + f"attn.{n}.weight", (128,)) for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k")]
        for ff in ("ff", "ff_context"):
            out += lin(p + ff + ".net.0.proj", 4 * d, d) + lin(p + ff + ".net.2", d, 4 * d)
    for i in range(cfg["num_single_layers"]):
        p = f"single_transformer_blocks.{i}."
        out += lin(p + "norm.linear", 3 * d, d) + lin(p + "proj_mlp", 4 * d, d) + lin(p + "proj_out", d, 5 * d)
        for n in ("to_q", "to_k", "to_v"):
            out += lin(p + "attn." + n, d, d)
        out += [(p + "attn.norm_q.weight", (128,)), (p + "attn.norm_k.weight", (128,))]
    return out


def hunyuan_names(cfg):
    d, td, vd = cfg["hidden_size"], cfg["text_states_dim"], cfg["text_states_dim_2"]

    def lin(p, n_out, n_in):
        return [(p + ".weight", (n_out, n_in)), (p + ".bias", (n_out,))]
    out = [("img_in.proj.weight", (d, cfg["in_channels"], 1, 2, 2)), ("img_in.proj.bias", (d,))]
    out += lin("txt_in.input_embedder", d, td)
    for p, k in (("txt_in.t_embedder.mlp", 256), ("time_in.mlp", 256), ("guidance_in.mlp", 256)):
        out += lin(p + ".0", d, k) + lin(p + ".2", d, d)
    out += lin("txt_in.c_embedder.linear_1", d, td) + lin("txt_in.c_embedder.linear_2", d, d)
    out += lin("vector_in.in_layer", d, vd) + lin("vector_in.out_layer", d, d)
    for i in range(2):
        p = f"txt_in.individual_token_refiner.blocks.{i}."
        out += lin(p + "self_attn_qkv", 3 * d, d) + lin(p + "self_attn_proj", d, d) + lin(p + "mlp.fc1", 4 * d, d)
        out += lin(p + "mlp.fc2", d, 4 * d) + lin(p + "adaLN_modulation.1", 2 * d, d)
        out += [(p + "norm1.weight", (d,)), (p + "norm1.bias", (d,)), (p + "norm2.weight", (d,)), (p + "norm2.bias", (d,))]
    for i in range(cfg["mm_double_blocks_depth"]):
        for s in ("img", "txt"):
            p = f"double_blocks.{i}.{s}"
            out += lin(p + "_mod.linear", 6 * d, d) + lin(p + "_attn_qkv", 3 * d, d) + lin(p + "_attn_proj", d, d)
            out += lin(p + "_mlp.fc1", 4 * d, d) + lin(p + "_mlp.fc2", d, 4 * d)
            out += [(p + "_attn_q_norm.weight", (128,)), (p + "_attn_k_norm.weight", (128,))]
    for i in range(cfg["mm_single_blocks_depth"]):
        p = f"single_blocks.{i}."
        out += lin(p + "modulation.linear", 3 * d, d) + lin(p + "linear1", 7 * d, d) + lin(p + "linear2", d, 5 * d)
        out += [(p + "q_norm.weight", (128,)), (p + "k_norm.weight", (128,))]
    out += lin("final_layer.adaLN_modulation.1", 2 * d, d) + lin("final_layer.linear", 4 * cfg["out_channels"], d)
    return out


def mmdit_flops(d, n_double, n_single, li, lt, valid):
    s = li + lt
    attn = 4.0 * s * valid * d
    double = 2.0 * (li + lt) * d * d * (3 + 1 + 4 + 4) + attn
    single = 2.0 * s * d * d * (3 + 4 + 5) + attn
    return n_double * double + n_single * single


def timed(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


def bench_flux():
    cfg = MM.FLUX_DEV
    h2 = w2 = 32                      # 512x512 image: 64x64 latent, 2x2 packed -> 1024 tokens
    steps, txt_len = 28, 512
    cls = type("FluxBench", (MM.FluxTransformer2DModelHIP,), {})
    m = cls(cfg, h2 * w2, txt_len=txt_len, device=DEV, calibration=False)
    synth_load(m, flux_names(cfg))
    g = torch.Generator(device=DEV).manual_seed(42)
    lat0 = torch.randn(1, h2 * w2, 64, generator=g, device=DEV)
    ctx = torch.randn(1, txt_len, 4096, generator=g, device=DEV)
    pooled = torch.randn(1, 768, generator=g, device=DEV)
    ids = torch.zeros(h2, w2, 3, device=DEV)
    ids[..., 1] += torch.arange(h2, device=DEV)[:, None]
    ids[..., 2] += torch.arange(w2, device=DEV)[None, :]
    kw = dict(encoder_hidden_states=ctx, pooled_projections=pooled, img_ids=ids.reshape(-1, 3),
              txt_ids=torch.zeros(txt_len, 3, device=DEV), guidance=torch.tensor([3.5], device=DEV), return_dict=False)
    sig = np.linspace(1.0, 1.0 / steps, steps)
    sig = np.append(3.0 * sig / (1 + 2.0 * sig), 0.0)

    def run():
        x = lat0.clone()
        for i in range(steps):
            o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), **kw)[0]
            x = x + float(sig[i + 1] - sig[i]) * o
        return x
    run()                                                              # warm-up (no cache)
    t_plain, x_plain = timed(run)
    MM.init_flux_magcache(m, steps, 0.24, 5, 0.1)
    modes, base = [], MM.FluxTransformer2DModelHIP._run
    cls._run = lambda self, *a: (modes.append(a[-1]), base(self, *a))[1]
    t_mc, x_mc = timed(run)
    skipped = sum(int(mo == MM.MC_MODE_SKIP) for mo in modes)
    mse = float(((x_mc - x_plain) ** 2).mean())
    psnr = 10 * np.log10(float(x_plain.abs().max()) ** 2 / mse) if mse > 0 else 100.0
    fl = mmdit_flops(3072, 19, 38, h2 * w2, txt_len, h2 * w2 + txt_len)
    print(json.dumps({"config": "FLUX.1-dev 512x512, 28 steps (BASELINE.json config 0), synthetic weights/inputs",
                      "nocache_s": t_plain, "magcache_s": t_mc, "speedup": t_plain / t_mc, "forwards_skipped": skipped,
                      "steps_per_s_nocache": steps / t_plain, "steps_per_s_magcache": steps / t_mc,
                      "model_tflops_per_s_nocache": fl * steps / t_plain / 1e12, "latent_psnr_vs_nocache_db": psnr,
                      "finite": bool(torch.isfinite(x_mc).all())}))


def bench_flux_controlnet(n_double, n_single, rounds=7, per_round=4):
    """One FULL forward at FLUX.1-dev 1024x1024 (4096 image + 512 text tokens) with ControlNet samples and without, in
    alternating windows of `per_round` forwards after a warm-up of both; median and spread of the windows, host clock
    around a device synchronise."""
    cfg = MM.FLUX_DEV
    h2 = w2 = 64
    txt_len, d = 512, 3072
    cls = type("FluxControlNetBench", (MM.FluxTransformer2DModelHIP,), {})
    m = cls(cfg, h2 * w2, txt_len=txt_len, device=DEV, calibration=False)
    synth_load(m, flux_names(cfg))
    g = torch.Generator(device=DEV).manual_seed(42)
    lat = torch.randn(1, h2 * w2, 64, generator=g, device=DEV)
    ids = torch.zeros(h2, w2, 3, device=DEV)
    ids[..., 1] += torch.arange(h2, device=DEV)[:, None]
    ids[..., 2] += torch.arange(w2, device=DEV)[None, :]
    kw = dict(encoder_hidden_states=torch.randn(1, txt_len, 4096, generator=g, device=DEV),
              pooled_projections=torch.randn(1, 768, generator=g, device=DEV), img_ids=ids.reshape(-1, 3),
              txt_ids=torch.zeros(txt_len, 3, device=DEV), guidance=torch.tensor([3.5], device=DEV), return_dict=False)
    t = torch.tensor([0.5], device=DEV)
    double = [(0.05 * torch.randn(h2 * w2, d, generator=g, device=DEV)).bfloat16() for _ in range(n_double)]
    single = [(0.05 * torch.randn(h2 * w2, d, generator=g, device=DEV)).bfloat16() for _ in range(n_single)]
    cn = dict(controlnet_block_samples=double or None, controlnet_single_block_samples=single or None)
    without = lambda: m(hidden_states=lat, timestep=t, **kw)[0]
    with_cn = lambda: m(hidden_states=lat, timestep=t, **kw, **cn)[0]
    for f in (without, with_cn, without, with_cn):
        timed(f)
    ms = {"without": [], "with": []}
    for _ in range(rounds):
        ms["without"].append(timed(without, per_round)[0] * 1e3)
        ms["with"].append(timed(with_cn, per_round)[0] * 1e3)
    o_with, o_without = with_cn(), without()
    adds = (cfg["num_layers"] if double else 0) + (cfg["num_single_layers"] if single else 0)   # every block has a sample
    print(json.dumps({"config": f"FLUX.1-dev 1024x1024 full forward, {n_double} double + {n_single} single bf16 ControlNet samples "
                                f"({adds} add launches), synthetic weights/inputs",
                      "forward_ms_without": float(np.median(ms["without"])), "forward_ms_with": float(np.median(ms["with"])),
                      "windows_without_ms": [round(v, 3) for v in ms["without"]], "windows_with_ms": [round(v, 3) for v in ms["with"]],
                      "forwards_per_window": per_round, "finite": bool(torch.isfinite(o_with).all()),
                      "output_moved_rel_l2": float((o_with - o_without).norm() / o_without.norm())}))


def bench_flux_ip_adapter(specs, depth=None, rounds=7, per_round=4):
    """One FULL forward at FLUX.1-dev 1024x1024 with image prompts and without, on ONE engine, in alternating windows of
    `per_round` forwards after a warm-up of both; then the wall time of set_ip_adapter_image and, through the single-op
    entries at the forward's shapes, the attention launch and the add launch alone (100 launches each between two
    synchronises; operands of 25 to 75 MB each, so partly served by the last-level cache like in the forward)."""
    import ctypes as C
    from magcache_amd import _lib, ip_adapter as IP
    cfg = dict(MM.FLUX_DEV)
    if depth:
        cfg["num_layers"], cfg["num_single_layers"] = depth
    h2 = w2 = 64
    txt_len, d, heads, embed_dim, cross = 512, 3072, 24, 768, 4096
    n_img = h2 * w2
    cls = type("FluxIpAdapterBench", (MM.FluxTransformer2DModelHIP,), {})
    m = cls(cfg, n_img, txt_len=txt_len, device=DEV, calibration=False)
    synth_load(m, flux_names(cfg))
    g = torch.Generator(device=DEV).manual_seed(42)
    embeds = []
    for j, (tokens, images) in enumerate(specs):
        shapes = {n: None for n in IP.name_templates(cfg["num_layers"])}
        sd = {}
        for n in shapes:
            if "image_embeds.weight" in n:
                shape = (tokens * cross, embed_dim)
            elif "image_embeds.bias" in n:
                shape = (tokens * cross,)
            elif ".norm." in n:
                shape = (cross,)
            else:
                shape = (d, cross) if n.endswith("weight") else (d,)
            t = 0.02 * torch.randn(shape, generator=g, device=DEV)
            sd[n.format(j=0)] = (1.0 + t) if n.endswith("norm.weight") else (t.bfloat16() if len(shape) == 2 else t)
        m.load_ip_adapter(sd)
        embeds.append(torch.randn(1, images, embed_dim, generator=g, device=DEV))
    lat = torch.randn(1, n_img, 64, generator=g, device=DEV)
    ids = torch.zeros(h2, w2, 3, device=DEV)
    ids[..., 1] += torch.arange(h2, device=DEV)[:, None]
    ids[..., 2] += torch.arange(w2, device=DEV)[None, :]
    kw = dict(encoder_hidden_states=torch.randn(1, txt_len, 4096, generator=g, device=DEV),
              pooled_projections=torch.randn(1, 768, generator=g, device=DEV), img_ids=ids.reshape(-1, 3),
              txt_ids=torch.zeros(txt_len, 3, device=DEV), guidance=torch.tensor([3.5], device=DEV), return_dict=False)
    t = torch.tensor([0.5], device=DEV)
    joint = dict(ip_adapter_image_embeds=embeds)
    without = lambda: m(hidden_states=lat, timestep=t, **kw)[0]
    with_ip = lambda: m(hidden_states=lat, timestep=t, joint_attention_kwargs=joint, **kw)[0]
    for f in (without, with_ip, without, with_ip):
        timed(f)
    ms = {"without": [], "with": []}
    for _ in range(rounds):
        ms["without"].append(timed(without, per_round)[0] * 1e3)
        ms["with"].append(timed(with_ip, per_round)[0] * 1e3)
    o_with, o_without = with_ip(), without()
    # set_image: every adapter of the list into slot 1 (the forwards above used slot 0), wall time to completion
    e = m.engine
    set_ms = []
    for _ in range(5):
        set_ms.append(timed(lambda: [e.set_ip_adapter_image(j, 1, v[0]) for j, v in enumerate(embeds)])[0] * 1e3)
    # the two launches alone, at the forward's shapes
    lib = _lib.load()
    qkv = torch.randn(n_img, 3 * d, generator=g, device=DEV).bfloat16()
    wq = torch.ones(128, device=DEV)
    out = torch.empty(n_img, d, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(n_img, d, device=DEV)
    arr = (_lib.McIpKeys * len(specs))()
    caches = []
    for j, (tokens, images) in enumerate(specs):
        keys = tokens * images
        caches.append(torch.randn(keys, 2 * d, generator=g, device=DEV).bfloat16())
        arr[j] = _lib.McIpKeys(caches[-1].data_ptr(), 2 * d, keys, 1.0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    attn = lambda: _lib.check(lib.mc_op_ip_attention(C.c_void_p(qkv.data_ptr()), 3 * d, C.c_void_p(wq.data_ptr()), 1e-6, arr, len(specs),
                                                     C.c_void_p(out.data_ptr()), d, n_img, heads, stream()))
    add = lambda: _lib.check(lib.mc_op_add_rows(C.c_void_p(x.data_ptr()), d, C.c_void_p(out.data_ptr()), _lib.MC_BF16, None, 0, None, 0,
                                                n_img, d, stream()))
    for f in (attn, add):
        timed(f, 10)
    attn_us = [timed(attn, 100)[0] * 1e6 for _ in range(5)]
    add_us = [timed(add, 100)[0] * 1e6 for _ in range(5)]
    keys_total = sum(tk * im for tk, im in specs)
    bytes_attn = n_img * d * 2 * 2 + sum(tk * im for tk, im in specs) * 2 * d * 2      # q in, out; K|V once
    bytes_add = n_img * d * (2 + 4 + 4)                                                # bf16 source, fp32 read-modify-write
    print(json.dumps({"config": f"FLUX.1-dev 1024x1024 full forward ({cfg['num_layers']} double + {cfg['num_single_layers']} single blocks), "
                                f"IP-Adapters (tokens x images) {specs}, synthetic weights/inputs",
                      "forward_ms_without": float(np.median(ms["without"])), "forward_ms_with": float(np.median(ms["with"])),
                      "windows_without_ms": [round(v, 3) for v in ms["without"]], "windows_with_ms": [round(v, 3) for v in ms["with"]],
                      "forwards_per_window": per_round, "set_image_ms": [round(v, 3) for v in set_ms],
                      "ip_attention_us_per_launch": [round(v, 2) for v in attn_us], "add_rows_us_per_launch": [round(v, 2) for v in add_us],
                      "ip_attention_bytes": bytes_attn, "add_rows_bytes": bytes_add,
                      "ip_attention_flop": n_img * heads * keys_total * 512,
                      "finite": bool(torch.isfinite(o_with).all()),
                      "output_moved_rel_l2": float((o_with - o_without).norm() / o_without.norm())}))


def bench_hunyuan():
    cfg = MM.HUNYUAN_VIDEO
    grid, txt_len, n_valid = (33, 90, 160), 256, 77          # 720x1280, 129 frames -> latent 16 x 33 x 90 x 160
    cls = type("HunyuanBench", (MM.HYVideoDiffusionTransformerHIP,), {})
    m = cls(cfg, grid, txt_len=txt_len, device=DEV, calibration=False)
    synth_load(m, hunyuan_names(cfg))
    g = torch.Generator(device=DEV).manual_seed(42)
    x = torch.randn(1, 16, *grid, generator=g, device=DEV)
    txt = torch.randn(1, txt_len, 4096, generator=g, device=DEV)
    mask = torch.zeros(1, txt_len, dtype=torch.long, device=DEV)
    mask[0, :n_valid] = 1
    txt2 = torch.randn(1, 768, generator=g, device=DEV)
    li = m.img_tokens
    # hyvideo get_nd_rotary_pos_embed, theta 256, dims (16, 56, 56), built on the device (plumbing)
    axes = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=DEV) for n in (grid[0], grid[1] // 2, grid[2] // 2)], indexing="ij")
    cos, sin = [], []
    for pos, dim in zip(axes, (16, 56, 56)):
        fr = 1.0 / (256.0 ** (torch.arange(0, dim, 2, device=DEV).float() / dim))
        ang = torch.outer(pos.reshape(-1), fr)
        cos.append(ang.cos().repeat_interleave(2, dim=1))
        sin.append(ang.sin().repeat_interleave(2, dim=1))
    kw = dict(text_states=txt, text_mask=mask, text_states_2=txt2, freqs_cos=torch.cat(cos, 1), freqs_sin=torch.cat(sin, 1),
              guidance=torch.tensor([6000.0], device=DEV))
    t = torch.tensor([900.0], device=DEV)
    full = lambda: m(x, t, **kw)["x"]
    t_first, out0 = timed(full)
    t_full, out1 = timed(full)
    assert bool(torch.isfinite(out1).all()) and torch.equal(out0, out1)          # deterministic
    e = m.engine
    skip = lambda: e.forward(x[0], 900.0, 6000.0, txt[0], n_valid, txt2[0], mode=MM.MC_MODE_SKIP)
    t_skip, s0 = timed(skip)
    t_skip, s1 = timed(skip, 3)
    # skipped forward at the same inputs/timestep == the full forward it cached (x_out = ori + (x_out - ori))
    rel = float((s1 - out1[0]).norm() / out1[0].norm())
    fl = mmdit_flops(3072, 20, 40, li, txt_len, li + n_valid)
    print(json.dumps({"config": "HunyuanVideo 720p 129 frames (BASELINE.json config 2): 118800 image + 256 text tokens, 20+40 blocks",
                      "full_forward_s": t_full, "first_forward_s": t_first, "skipped_forward_ms": t_skip * 1e3,
                      "model_tflops_per_s": fl / t_full / 1e12, "model_pflop_per_forward": fl / 1e15,
                      "skip_equals_cached_full_rel_l2": rel, "idempotent": bool(torch.equal(s0, s1)),
                      "workspace_gb": e.workspace.numel() / 2 ** 30}))


def bench_regeometry(which, sizes, depth=None, rounds=7, per_round=4):
    """`sizes`: [(width, height)] in pixels; image tokens (H/16) * (W/16) for both families.  Engine-level forwards (the
    shims add host work only).  Windows of `per_round` full forwards alternate between a fresh engine created at the size
    and the one engine that is switched from size to size; host clock around a device synchronise."""
    from magcache_amd.qwen_bench import random_state_dict
    flux = which == "flux"
    cfg = dict(MM.FLUX_DEV if flux else MM.QWEN_IMAGE)
    if depth:
        cfg.update(num_layers=depth[0], **({"num_single_layers": depth[1]} if flux else {}))
    txt_len = 512
    grids = [(h // 16, w // 16) for w, h in sizes]

    def make(grid):
        free0 = torch.cuda.mem_get_info()[0]
        if flux:
            m = MM.FluxTransformer2DModelHIP(cfg, grid[0] * grid[1], txt_len=txt_len, device=DEV, calibration=False)
            synth_load(m, flux_names(cfg))
        else:
            m = MM.QwenImageTransformer2DModelHIP(cfg, grid[0] * grid[1], txt_len=txt_len, device=DEV, calibration=False)
            m.engine.load_weights(random_state_dict(cfg, DEV))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return m.engine, free0 - torch.cuda.mem_get_info()[0] - m.engine.workspace.numel()

    def inputs(grid):
        h2, w2 = grid
        g = torch.Generator(device=DEV).manual_seed(h2 * 1000 + w2)
        img = torch.randn(h2 * w2, 64, generator=g, device=DEV)
        txt = torch.randn(txt_len, cfg["joint_attention_dim"], generator=g, device=DEV)
        if flux:
            ids = torch.zeros(txt_len + h2 * w2, 3)
            ids[txt_len:, 1] = torch.arange(h2).repeat_interleave(w2)
            ids[txt_len:, 2] = torch.arange(w2).repeat(h2)
            return img, txt, torch.randn(768, generator=g, device=DEV), MM.flux_rope(ids)
        return img, txt, None, MM.qwen_rope([(1, h2, w2)], txt_len)

    def forward(e, inp):
        return lambda: e.forward(inp[0], 500.0, 3500.0, inp[1], txt_len, inp[2], branch=None if flux else 0)

    def switch(e, grid, inp):
        ptr = e.workspace.data_ptr()
        t_geo, _ = timed(lambda: e.set_geometry(grid[0] * grid[1], (0, 0, 0), txt_len))
        t_rope, _ = timed(lambda: e.set_rope(*inp[3]))
        return {"set_geometry_ms": t_geo * 1e3, "set_rope_ms": t_rope * 1e3, "reallocated": e.workspace.data_ptr() != ptr}

    order = sorted(range(len(grids)), key=lambda i: grids[i][0] * grids[i][1])
    one, weight_bytes = make(grids[order[0]])                  # created at the smallest size: every first switch grows
    data = {i: inputs(grids[i]) for i in range(len(grids))}
    no_reserve = {}
    for i in order[1:]:
        no_reserve["%dx%d" % sizes[i]] = switch(one, grids[i], data[i])
    one.reserve([(gr[0] * gr[1], (0, 0, 0), txt_len) for gr in grids])
    res = []
    for i in range(len(grids)):
        fresh, _ = make(grids[i])
        fresh.set_rope(*data[i][3])
        sw = switch(one, grids[i], data[i])
        f_fresh, f_one = forward(fresh, data[i]), forward(one, data[i])
        same = bool(torch.equal(f_fresh(), f_one()))
        for f in (f_fresh, f_one):
            timed(f, 2)
        ms = {"fresh": [], "switched": []}
        for _ in range(rounds):
            ms["fresh"].append(timed(f_fresh, per_round)[0] * 1e3)
            ms["switched"].append(timed(f_one, per_round)[0] * 1e3)
        res.append({"size": "%dx%d" % sizes[i], "img_tokens": grids[i][0] * grids[i][1],
                    "forward_ms_fresh": float(np.median(ms["fresh"])), "forward_ms_switched": float(np.median(ms["switched"])),
                    "windows_fresh_ms": [round(v, 3) for v in ms["fresh"]], "windows_switched_ms": [round(v, 3) for v in ms["switched"]],
                    "fresh_window_spread_ms": float(max(ms["fresh"]) - min(ms["fresh"])), "bitwise_equal_to_fresh": same,
                    "switch_with_reserve": sw, "workspace_bytes": one.geometry_bytes(grids[i][0] * grids[i][1], (0, 0, 0), txt_len),
                    "workspace_bytes_fresh_engine": fresh.workspace.numel() - 256})
        del fresh, f_fresh
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps({"config": f"{'FLUX.1-dev' if flux else 'Qwen-Image'} {cfg['num_layers']} double"
                                f"{' + %d single' % cfg['num_single_layers'] if flux else ''} blocks, one engine over "
                                f"{', '.join('%dx%d' % s for s in sizes)}, {txt_len} text tokens, synthetic weights/inputs",
                      "forwards_per_window": per_round, "weight_bytes_held_once": weight_bytes,
                      "weight_bytes_one_engine_per_size": weight_bytes * len(sizes), "reserved_workspace_bytes": one.ws.numel(),
                      "switch_without_reserve": no_reserve, "per_size": res}))


def bench_fp8(which, sizes, modes, depth=None, rounds=5, per_round=3, txt_len=512, mx_fp4=False, mx_fp6=False):
    """`sizes`: [(width, height)] in pixels; image tokens (H/16) * (W/16).  One engine per fp8_linear mode of `modes` (the same
    seeded weights: an fp8 engine quantises them as it takes them), switched from size to size with set_geometry; engine-level
    full forwards.  Per size, windows of `per_round` forwards alternate between the modes after a warm-up of each; host clock
    around a device synchronise.  One JSON line per size.  mx_fp4: the variants "<mode>+mxfp4" (an MXFP4 engine of mode 2 | 3) and
    "<mode>+mxfp4 separate" (the same engine under fp8_fused_quant 0) join the table, keyed by those labels; mx_fp6: the variant
    "<mode>+mxfp6" (an MXFP6 engine; its quantise passes are always separate)."""
    from magcache_amd._lib import check
    from magcache_amd.qwen_bench import random_state_dict
    lib = load()
    flux = which == "flux"
    cfg = dict(MM.FLUX_DEV if flux else MM.QWEN_IMAGE)
    if depth:
        cfg.update(num_layers=depth[0], **({"num_single_layers": depth[1]} if flux else {}))
    grids = [(h // 16, w // 16) for w, h in sizes]
    engines, fused = {}, {}
    variants = ([(mode, mode, False, False) for mode in modes] +
                [(f"{mode}+mxfp6", mode, False, True) for mode in modes if mx_fp6 and mode in (2, 3)] +
                [(f"{mode}+mxfp4", mode, True, False) for mode in modes if mx_fp4 and mode in (2, 3)])
    for label, mode, fp4, fp6 in variants:
        n0 = grids[0][0] * grids[0][1]
        if flux:
            m = MM.FluxTransformer2DModelHIP(cfg, n0, txt_len=txt_len, device=DEV, calibration=False, fp8_linear=mode, mx_fp4=fp4, mx_fp6=fp6)
            synth_load(m, flux_names(cfg))
        else:
            m = MM.QwenImageTransformer2DModelHIP(cfg, n0, txt_len=txt_len, device=DEV, calibration=False, fp8_linear=mode, mx_fp4=fp4, mx_fp6=fp6)
            m.engine.load_weights(random_state_dict(cfg, DEV))
        assert m.engine.mx_fp4 is fp4 and m.engine.mx_fp6 is fp6
        engines[label], fused[label] = m.engine, 1
        if fp4:
            engines[label + " separate"], fused[label + " separate"] = m.engine, 0
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    modes = list(engines)
    for size, (h2, w2) in zip(sizes, grids):
        g = torch.Generator(device=DEV).manual_seed(h2 * 1000 + w2)
        img = torch.randn(h2 * w2, 64, generator=g, device=DEV)
        txt = torch.randn(txt_len, cfg["joint_attention_dim"], generator=g, device=DEV)
        if flux:
            ids = torch.zeros(txt_len + h2 * w2, 3)
            ids[txt_len:, 1] = torch.arange(h2).repeat_interleave(w2)
            ids[txt_len:, 2] = torch.arange(w2).repeat(h2)
            vec, rope = torch.randn(768, generator=g, device=DEV), MM.flux_rope(ids)
        else:
            vec, rope = None, MM.qwen_rope([(1, h2, w2)], txt_len)
        for label, e in engines.items():
            if fused[label]:          # a "separate" variant is its fused twin's engine
                e.set_geometry(h2 * w2, (0, 0, 0), txt_len)
                e.set_rope(*rope)

        def forward(e, fq):
            check(lib.mc_set_option(b"fp8_fused_quant", fq))       # read by every launch of the forward; 1 is the default
            try:
                return e.forward(img, 500.0, 3500.0, txt, txt_len, vec, branch=None if flux else 0)
            finally:
                check(lib.mc_set_option(b"fp8_fused_quant", 1))
        fwd = {mode: (lambda e=e, fq=fused[mode]: forward(e, fq)) for mode, e in engines.items()}
        outs = {mode: timed(fwd[mode], 2)[1].clone() for mode in modes}
        ms = {mode: [] for mode in modes}
        for _ in range(rounds):
            for mode in modes:
                ms[mode].append(timed(fwd[mode], per_round)[0] * 1e3)
        base = outs[modes[0]]
        print(json.dumps({"config": f"{'FLUX.1-dev' if flux else 'Qwen-Image'} {cfg['num_layers']} double"
                                    f"{' + %d single' % cfg['num_single_layers'] if flux else ''} blocks, {size[0]}x{size[1]}: "
                                    f"{h2 * w2} image + {txt_len} text tokens, full forward, synthetic weights/inputs",
                          "forwards_per_window": per_round, "windows": rounds,
                          "per_mode": {str(mode): {"forward_ms": float(np.median(ms[mode])),
                                                   "window_spread_ms": float(max(ms[mode]) - min(ms[mode])),
                                                   "windows_ms": [round(v, 3) for v in ms[mode]],
                                                   "workspace_bytes": engines[mode].geometry_bytes(h2 * w2, (0, 0, 0), txt_len),
                                                   "finite": bool(torch.isfinite(outs[mode]).all()),
                                                   "rel_l2_vs_mode_%s" % modes[0]: float((outs[mode] - base).norm() / base.norm())}
                                       for mode in modes}}), flush=True)


if __name__ == "__main__":
    lib = load()
    which = sys.argv[1] if len(sys.argv) > 1 else "flux"
    if "two_streams" in sys.argv[2:]:      # text half of every double block on a second HIP stream
        from magcache_amd._lib import check
        check(lib.mc_set_option(b"mmdit_two_streams", 1))
        print("mmdit_two_streams = 1")
    if "--fp8_linear" in sys.argv[2:]:
        if which not in ("flux", "qwen"):
            sys.exit(f"--fp8_linear benches FLUX and Qwen-Image, not '{which}'")
        modes = [int(v) for v in sys.argv[sys.argv.index("--fp8_linear") + 1].split(",")]
        default = "1024x1024" if which == "flux" else "1664x928"
        sizes = [tuple(int(v) for v in g.split("x"))
                 for g in (sys.argv[sys.argv.index("--size") + 1] if "--size" in sys.argv else default).split(",")]
        depth = [int(v) for v in sys.argv[sys.argv.index("--depth") + 1].split(",")] if "--depth" in sys.argv else None
        bench_fp8(which, sizes, modes, depth, mx_fp4="--mx_fp4" in sys.argv[2:], mx_fp6="--mx_fp6" in sys.argv[2:])
    elif "--regeometry" in sys.argv[2:]:
        if which not in ("flux", "qwen"):
            sys.exit(f"--regeometry benches FLUX and Qwen-Image, not '{which}'")
        sizes = [tuple(int(v) for v in g.split("x")) for g in sys.argv[sys.argv.index("--regeometry") + 1].split(",")]
        depth = [int(v) for v in sys.argv[sys.argv.index("--depth") + 1].split(",")] if "--depth" in sys.argv else None
        bench_regeometry(which, sizes, depth)
    elif "--ip-adapter" in sys.argv[2:]:
        if which != "flux":
            sys.exit(f"--ip-adapter benches FLUX (IP-Adapters are a FLUX input), not '{which}'")
        specs = [tuple(int(v) for v in (e + "x1").split("x")[:2]) for e in sys.argv[sys.argv.index("--ip-adapter") + 1].split(",")]
        depth = [int(v) for v in sys.argv[sys.argv.index("--depth") + 1].split(",")] if "--depth" in sys.argv else None
        bench_flux_ip_adapter(specs, depth)
    elif "--controlnet" in sys.argv[2:]:
        if which != "flux":
            sys.exit(f"--controlnet benches FLUX (ControlNet residuals are a FLUX input), not '{which}'")
        n_d, n_s = (int(v) for v in sys.argv[sys.argv.index("--controlnet") + 1].split(","))
        bench_flux_controlnet(n_d, n_s)
    else:
        {"flux": bench_flux, "hunyuan": bench_hunyuan}[which]()

"""Seeded random Qwen-Image weights on the device (no checkpoint offline): the diffusers state_dict names and shapes of
QwenImageTransformer2DModel, generated block by block on the GPU so that the 20 B-parameter model needs no host copy."""
import torch


def qwen_weight_shapes(cfg):
    d = cfg["attention_head_dim"] * cfg["num_attention_heads"]
    td, cin, out = cfg["joint_attention_dim"], cfg["in_channels"], cfg["patch_size"] ** 2 * cfg["out_channels"]
    yield "img_in", (d, cin)
    yield "txt_norm.weight", (td,)
    yield "txt_in", (d, td)
    yield "time_text_embed.timestep_embedder.linear_1", (d, 256)
    yield "time_text_embed.timestep_embedder.linear_2", (d, d)
    for i in range(cfg["num_layers"]):
        p = f"transformer_blocks.{i}."
        for s in ("img_mod.1", "txt_mod.1"):
            yield p + s, (6 * d, d)
        for s in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"):
            yield p + "attn." + s, (d, d)
        for s in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            yield p + "attn." + s + ".weight", (128,)
        for s in ("img_mlp", "txt_mlp"):
            yield p + s + ".net.0.proj", (4 * d, d)
            yield p + s + ".net.2", (d, 4 * d)
    yield "norm_out.linear", (2 * d, d)
    yield "proj_out", (out, d)


def random_state_dict(cfg, device, seed=0, std=0.02):
    """generator of (name, tensor): Linear weights bf16 ~ N(0, std^2) and fp32 biases ~ N(0, std^2), norm weights
    1 + N(0, 0.1^2) -- tensors are produced lazily, one at a time"""
    g = torch.Generator(device=device).manual_seed(seed)

    def gen():
        for name, shape in qwen_weight_shapes(cfg):
            if len(shape) == 1:
                yield name, 1.0 + 0.1 * torch.randn(shape, generator=g, device=device)
            else:
                yield name + ".weight", (std * torch.randn(shape, generator=g, device=device)).to(torch.bfloat16)
                yield name + ".bias", std * torch.randn(shape[0], generator=g, device=device)
    return gen()

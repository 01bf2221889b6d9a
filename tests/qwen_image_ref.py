"""Test support (not product code): CPU PyTorch restatement of the Qwen-Image transformer (diffusers
`QwenImageTransformer2DModel`), the model MagCache4QwenImage/magcache_generate.py and MagCache4QwenImageEdit patch.

[UPSTREAM] The transformer is not in the reference tree: the scripts import it from huggingface/diffusers
(models/transformers/transformer_qwenimage.py: QwenTimestepProjEmbeddings, QwenEmbedRope, QwenImageTransformerBlock,
QwenDoubleStreamAttnProcessor2_0, QwenImageTransformer2DModel) and only replace `forward`.  This file restates the
published modules with the upstream state_dict names; it could not be checked against diffusers offline.  The pieces
Qwen-Image shares with FLUX.1 (joint attention with qk-RMSNorm and added text projections, GELU-tanh FeedForward,
AdaLayerNormContinuous, RMSNorm, TimestepEmbedding, pairwise RoPE) are imported from oracle/flux_ref.py.
It is anchored on the reference's call sites (MagCache4QwenImage/magcache_generate.py):
  img_in / timestep.to(dtype) / txt_norm / txt_in / time_text_embed(timestep, hidden_states)   :183-193
  pos_embed(img_shapes, txt_seq_lens, device=...)                                             :194
  transformer_blocks(hidden_states=, encoder_hidden_states=, encoder_hidden_states_mask=, temb=,
                     image_rotary_emb=, joint_attention_kwargs=)                              :222-239
  norm_out(hidden_states, temb); proj_out                                                     :247-248
tools/gen_golden_qwen.py executes the reference's own magcache_forward / magcache_calibration / init_magcache /
nearest_interp source around this model.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import flux_ref as FR

QWEN_IMAGE = dict(patch_size=2, in_channels=64, out_channels=16, num_layers=60, attention_head_dim=128,
                  num_attention_heads=24, joint_attention_dim=3584, guidance_embeds=False, axes_dims_rope=(16, 56, 56))


def tiny_config(num_layers=2, heads=2, joint_attention_dim=256):
    """Small geometry with the real head_dim (128), RoPE split and 64 packed channels, for CPU-sized parity runs."""
    return dict(QWEN_IMAGE, num_layers=num_layers, num_attention_heads=heads, joint_attention_dim=joint_attention_dim)


def timestep_proj(timesteps, dim=256, scale=1000.0, max_period=10000):
    """Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0, scale=1000): [cos | sin] of scale * t * f_i."""
    half = dim // 2
    exponent = -math.log(max_period) * torch.arange(half, dtype=torch.float32, device=timesteps.device) / half
    emb = scale * (timesteps[:, None].float() * torch.exp(exponent)[None, :])
    return torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1)


class QwenTimestepProjEmbeddings(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.timestep_embedder = FR.TimestepEmbedding(256, dim)

    def forward(self, timestep, hidden_states):
        return self.timestep_embedder(timestep_proj(timestep).to(hidden_states.dtype))


class QwenEmbedRope(nn.Module):
    """pos_freqs / neg_freqs: complex polar tables of positions 0..4095 / -4096..-1 per axis (fp32 angles);
    scale_rope: centred height / width positions; image idx at frame idx; text from max(h//2, w//2) on."""

    def __init__(self, theta=10000, axes_dim=(16, 56, 56), scale_rope=True):
        super().__init__()
        self.theta, self.axes_dim, self.scale_rope = theta, tuple(axes_dim), scale_rope
        pos, neg = torch.arange(4096), torch.arange(4096).flip(0) * -1 - 1
        self.pos_freqs = torch.cat([self.rope_params(pos, d) for d in self.axes_dim], dim=1)
        self.neg_freqs = torch.cat([self.rope_params(neg, d) for d in self.axes_dim], dim=1)

    def rope_params(self, index, dim):
        freqs = torch.outer(index, 1.0 / torch.pow(self.theta, torch.arange(0, dim, 2).to(torch.float32).div(dim)))
        return torch.polar(torch.ones_like(freqs), freqs)

    def _video_freqs(self, frame, height, width, idx):
        split = [x // 2 for x in self.axes_dim]
        fp, fn = self.pos_freqs.split(split, dim=1), self.neg_freqs.split(split, dim=1)
        ff = fp[0][idx:idx + frame].view(frame, 1, 1, -1).expand(frame, height, width, -1)
        fh = torch.cat([fn[1][-(height - height // 2):], fp[1][:height // 2]], dim=0).view(1, height, 1, -1).expand(frame, height, width, -1)
        fw = torch.cat([fn[2][-(width - width // 2):], fp[2][:width // 2]], dim=0).view(1, 1, width, -1).expand(frame, height, width, -1)
        return torch.cat([ff, fh, fw], dim=-1).reshape(frame * height * width, -1)

    def forward(self, video_fhw, txt_seq_lens, device=None):
        if isinstance(video_fhw, list) and len(video_fhw) and isinstance(video_fhw[0], list):
            video_fhw = video_fhw[0]
        if not isinstance(video_fhw, list):
            video_fhw = [video_fhw]
        vid, m = [], 0
        for idx, (f, h, w) in enumerate(video_fhw):
            vid.append(self._video_freqs(f, h, w, idx))
            m = max(h // 2, w // 2, m)
        n = max(txt_seq_lens)
        return torch.cat(vid, dim=0), self.pos_freqs[m:m + n]


def complex_to_cos_sin(freqs):
    """complex [n, 64] -> use_real (cos, sin) [n, 128], every frequency twice (what apply_rotary_emb pairs with)"""
    return (freqs.real.float().repeat_interleave(2, dim=1).contiguous(),
            freqs.imag.float().repeat_interleave(2, dim=1).contiguous())


class QwenImageTransformerBlock(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.img_mod = nn.Sequential(nn.SiLU(), nn.Linear(dim, 6 * dim))
        self.img_norm1 = nn.LayerNorm(dim, elementwise_affine=False, eps=1e-6)
        self.attn = FR.Attention(dim, heads, joint=True)
        self.img_norm2 = nn.LayerNorm(dim, elementwise_affine=False, eps=1e-6)
        self.img_mlp = FR.FeedForward(dim)
        self.txt_mod = nn.Sequential(nn.SiLU(), nn.Linear(dim, 6 * dim))
        self.txt_norm1 = nn.LayerNorm(dim, elementwise_affine=False, eps=1e-6)
        self.txt_norm2 = nn.LayerNorm(dim, elementwise_affine=False, eps=1e-6)
        self.txt_mlp = FR.FeedForward(dim)

    @staticmethod
    def _modulate(x, p):
        shift, scale, gate = p.chunk(3, dim=-1)
        return x * (1 + scale[:, None]) + shift[:, None], gate[:, None]

    def forward(self, hidden_states, encoder_hidden_states, encoder_hidden_states_mask, temb, image_rotary_emb,
                joint_attention_kwargs=None):
        img_mod1, img_mod2 = self.img_mod(temb).chunk(2, dim=-1)
        txt_mod1, txt_mod2 = self.txt_mod(temb).chunk(2, dim=-1)
        img_m, img_g1 = self._modulate(self.img_norm1(hidden_states), img_mod1)
        txt_m, txt_g1 = self._modulate(self.txt_norm1(encoder_hidden_states), txt_mod1)
        img_f, txt_f = image_rotary_emb
        n = encoder_hidden_states.shape[1]
        cos, sin = complex_to_cos_sin(torch.cat([txt_f[:n], img_f], dim=0))     # joint [text ; image] order
        img_attn, txt_attn = self.attn(img_m, txt_m, (cos, sin))
        hidden_states = hidden_states + img_g1 * img_attn
        encoder_hidden_states = encoder_hidden_states + txt_g1 * txt_attn
        img_m2, img_g2 = self._modulate(self.img_norm2(hidden_states), img_mod2)
        hidden_states = hidden_states + img_g2 * self.img_mlp(img_m2)
        txt_m2, txt_g2 = self._modulate(self.txt_norm2(encoder_hidden_states), txt_mod2)
        encoder_hidden_states = encoder_hidden_states + txt_g2 * self.txt_mlp(txt_m2)
        return encoder_hidden_states, hidden_states


class QwenImageTransformer2DModel(nn.Module):
    def __init__(self, patch_size=2, in_channels=64, out_channels=16, num_layers=60, attention_head_dim=128,
                 num_attention_heads=24, joint_attention_dim=3584, guidance_embeds=False, axes_dims_rope=(16, 56, 56)):
        super().__init__()
        dim = attention_head_dim * num_attention_heads
        self.inner_dim, self.out_channels = dim, out_channels
        self.pos_embed = QwenEmbedRope(10000, tuple(axes_dims_rope), scale_rope=True)
        self.time_text_embed = QwenTimestepProjEmbeddings(dim)
        self.txt_norm = FR.RMSNorm(joint_attention_dim, 1e-6)
        self.img_in = nn.Linear(in_channels, dim)
        self.txt_in = nn.Linear(joint_attention_dim, dim)
        self.transformer_blocks = nn.ModuleList([QwenImageTransformerBlock(dim, num_attention_heads) for _ in range(num_layers)])
        self.norm_out = FR.AdaLayerNormContinuous(dim)
        self.proj_out = nn.Linear(dim, patch_size * patch_size * out_channels)
        self.gradient_checkpointing = False

    def forward(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_mask=None, timestep=None,
                img_shapes=None, txt_seq_lens=None, guidance=None, attention_kwargs=None, return_dict=True):
        """upstream forward == the reference's magcache_forward without the cache (:183-248)"""
        hidden_states = self.img_in(hidden_states)
        timestep = timestep.to(hidden_states.dtype)
        encoder_hidden_states = self.txt_in(self.txt_norm(encoder_hidden_states))
        temb = self.time_text_embed(timestep, hidden_states)
        rope = self.pos_embed(img_shapes, txt_seq_lens, device=hidden_states.device)
        for block in self.transformer_blocks:
            encoder_hidden_states, hidden_states = block(hidden_states=hidden_states, encoder_hidden_states=encoder_hidden_states,
                                                         encoder_hidden_states_mask=encoder_hidden_states_mask, temb=temb,
                                                         image_rotary_emb=rope)
        out = self.proj_out(self.norm_out(hidden_states, temb))
        return (out,) if not return_dict else type("Out", (), {"sample": out})()


def init_synthetic_(model, seed=0, std=0.02):
    """Seeded synthetic weights (no checkpoint offline): FLUX's recipe (Linear ~ N(0, std^2), qk-norm weights
    1 + N(0, 0.1^2)) and the txt_norm weight 1 + N(0, 0.1^2)."""
    FR.init_synthetic_(model, seed=seed, std=std)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        model.txt_norm.weight.copy_(1.0 + 0.1 * torch.randn(model.txt_norm.weight.shape, generator=g))
    return model


def true_cfg_euler(x, cond, uncond, g, dt):
    """QwenImagePipeline true CFG (norm-preserving) + FlowMatchEulerDiscreteScheduler.step, fp32; cond / uncond may hold
    more rows than x (Edit): the first x.shape[-2] rows are used."""
    n = x.shape[-2]
    c, u = cond[..., :n, :].float(), uncond[..., :n, :].float()
    comb = u + g * (c - u)
    v = comb * (torch.norm(c, dim=-1, keepdim=True) / torch.norm(comb, dim=-1, keepdim=True))
    return x + dt * v

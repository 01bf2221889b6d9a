"""TEST INFRASTRUCTURE -- the IP-Adapter side of the FLUX transformer as a CPU PyTorch restatement on top of oracle/flux_ref.py.

The one place where upstream's IP-Adapter arithmetic and names are written down for the tests and the golden generator
(tools/gen_golden_flux_ip_adapter.py).  Restated from diffusers (not on this machine, not in the reference checkout):
  models/embeddings.py             ImageProjection, MultiIPAdapterImageProjection
  models/attention_processor.py    FluxIPAdapterJointAttnProcessor2_0
  models/transformers/transformer_flux.py  FluxTransformerBlock.forward (the `len(attention_outputs) == 3` branch)
  loaders/ip_adapter.py, loaders/transformer_flux.py  FluxIPAdapterMixin.load_ip_adapter / set_ip_adapter_scale and the names
                                   the converted weights get
PINNED by the reference's own code (MagCache4FLUX/magcache_flux.py:108-111, :321-324, run by the generator): the forward pops
joint_attention_kwargs["ip_adapter_image_embeds"], applies self.encoder_hid_proj to it and hands the result to every block as
joint_attention_kwargs["ip_hidden_states"].  UNPINNED, like the rest of the block: everything below that.

  projection   adapter j: image_embeds_j [batch, n_images, embed_dim] -> Linear(embed_dim, T * cross_dim) per image, reshaped to
               T rows of cross_dim, affine LayerNorm(cross_dim) (eps 1e-5) -> [batch, n_images, T, cross_dim]
  attention    double blocks only.  ip_query = the image stream's q after norm_q, BEFORE RoPE.  Per adapter j:
               K_j = to_k_ip_j(h_j), V_j = to_v_ip_j(h_j) (bias; all n_images * T rows; heads of 128; no RoPE, no mask),
               ip_out = sum_j scale_j * softmax(ip_query K_j^T / sqrt(128)) V_j  -- no output projection, no gate
  placement    hidden += gate_msa * attn; hidden += gate_mlp * ff(...); hidden += ip_out  (then the block's ControlNet sample,
               which the model's forward adds after the block returns)
State-dict names after load_ip_adapter (adapter j, double block i):
  encoder_hid_proj.image_projection_layers.{j}.image_embeds.{weight,bias}   [T * cross_dim, embed_dim]
  encoder_hid_proj.image_projection_layers.{j}.norm.{weight,bias}           [cross_dim]
  transformer_blocks.{i}.attn.processor.to_k_ip.{j}.{weight,bias}           [dim, cross_dim]
  transformer_blocks.{i}.attn.processor.to_v_ip.{j}.{weight,bias}           [dim, cross_dim]
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import flux_ref as FR


class ImageProjection(nn.Module):
    def __init__(self, embed_dim, cross_dim, num_image_text_embeds):
        super().__init__()
        self.num_image_text_embeds = num_image_text_embeds
        self.image_embeds = nn.Linear(embed_dim, num_image_text_embeds * cross_dim)
        self.norm = nn.LayerNorm(cross_dim)

    def forward(self, image_embeds):
        b = image_embeds.shape[0]
        h = self.image_embeds(image_embeds.to(self.image_embeds.weight.dtype))
        return self.norm(h.reshape(b, self.num_image_text_embeds, -1))


class MultiIPAdapterImageProjection(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.image_projection_layers = nn.ModuleList(layers)

    def forward(self, image_embeds):
        if not isinstance(image_embeds, (list, tuple)):
            image_embeds = [image_embeds.unsqueeze(1)]
        assert len(image_embeds) == len(self.image_projection_layers)
        out = []
        for e, layer in zip(image_embeds, self.image_projection_layers):
            b, n = e.shape[0], e.shape[1]
            h = layer(e.reshape((b * n,) + e.shape[2:]))
            out.append(h.reshape((b, n) + h.shape[1:]))
        return out


class IPAttention(FR.Attention):
    """FR.Attention with FluxIPAdapterJointAttnProcessor2_0: a third result, the IP attention of the image stream"""

    def forward(self, hidden, encoder=None, rope=None, ip_hidden_states=None):
        q, k, v = self._heads(self.to_q(hidden)), self._heads(self.to_k(hidden)), self._heads(self.to_v(hidden))
        q, k = self.norm_q(q), self.norm_k(k)
        ip_query = q                                         # after norm_q, before the text rows are joined and before RoPE
        eq = self.norm_added_q(self._heads(self.add_q_proj(encoder)))
        ek = self.norm_added_k(self._heads(self.add_k_proj(encoder)))
        ev = self._heads(self.add_v_proj(encoder))
        q, k, v = torch.cat([eq, q], dim=2), torch.cat([ek, k], dim=2), torch.cat([ev, v], dim=2)
        if rope is not None:
            q, k = FR.apply_rotary_emb(q, *rope), FR.apply_rotary_emb(k, *rope)
        o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).flatten(2).to(q.dtype)
        n = encoder.shape[1]
        out, c_out = self.to_out[0](o[:, n:]), self.to_add_out(o[:, :n])
        if ip_hidden_states is None:
            return out, c_out
        ip_out = torch.zeros_like(hidden)
        b = hidden.shape[0]
        for h, scale, to_k, to_v in zip(ip_hidden_states, self.processor.scale, self.processor.to_k_ip, self.processor.to_v_ip):
            ik = to_k(h).view(b, -1, self.heads, 128).transpose(1, 2)          # [b, n_images, T, c] -> all n_images * T keys
            iv = to_v(h).view(b, -1, self.heads, 128).transpose(1, 2)
            a = F.scaled_dot_product_attention(ip_query, ik, iv).transpose(1, 2).reshape(b, -1, self.heads * 128)
            ip_out = ip_out + scale * a.to(ip_query.dtype)
        return out, c_out, ip_out


class IPFluxTransformerBlock(FR.FluxTransformerBlock):
    def forward(self, hidden_states, encoder_hidden_states, temb, image_rotary_emb, joint_attention_kwargs=None):
        ip = (joint_attention_kwargs or {}).get("ip_hidden_states")
        nh, gate_msa, shift_mlp, scale_mlp, gate_mlp = self.norm1(hidden_states, temb)
        ne, c_gate_msa, c_shift_mlp, c_scale_mlp, c_gate_mlp = self.norm1_context(encoder_hidden_states, temb)
        res = self.attn(nh, ne, image_rotary_emb, ip_hidden_states=ip)
        attn, c_attn = res[0], res[1]
        hidden_states = hidden_states + gate_msa.unsqueeze(1) * attn
        nh = self.norm2(hidden_states) * (1 + scale_mlp[:, None]) + shift_mlp[:, None]
        hidden_states = hidden_states + gate_mlp.unsqueeze(1) * self.ff(nh)
        if len(res) == 3:
            hidden_states = hidden_states + res[2]
        encoder_hidden_states = encoder_hidden_states + c_gate_msa.unsqueeze(1) * c_attn
        ne = self.norm2_context(encoder_hidden_states) * (1 + c_scale_mlp[:, None]) + c_shift_mlp[:, None]
        encoder_hidden_states = encoder_hidden_states + c_gate_mlp.unsqueeze(1) * self.ff_context(ne)
        return encoder_hidden_states, hidden_states


def add_ip_adapters_(model, specs, seeds, std):
    """load_ip_adapter on a FR.FluxTransformer2DModel whose own weights are already set: specs = [(embed_dim, cross_dim, T)]
    per adapter, adapter j with seeded synthetic weights of its own (seeds[j]; the same seed gives the same adapter in any
    model with the same widths and depth).  Linear weights ~ N(0, std^2) -- to_k_ip N(0, (8 std)^2), so that the scores spread
    by about one and the softmax is not flat --, biases a quarter of that, LayerNorm weight 1 + N(0, 0.1^2), bias N(0, 0.1^2).
    Scales start at 1.0."""
    dim = model.inner_dim
    layers = []
    per_block = [([], []) for _ in model.transformer_blocks]
    with torch.no_grad():
        for (embed_dim, cross_dim, tokens), seed in zip(specs, seeds):
            g = torch.Generator().manual_seed(seed)

            def lin(n_in, n_out, std=std):
                m = nn.Linear(n_in, n_out)
                m.weight.copy_(std * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(std / 4 * torch.randn(m.bias.shape, generator=g))
                return m
            p = ImageProjection(embed_dim, cross_dim, tokens)
            p.image_embeds = lin(embed_dim, tokens * cross_dim)
            p.norm.weight.copy_(1.0 + 0.1 * torch.randn(cross_dim, generator=g))
            p.norm.bias.copy_(0.1 * torch.randn(cross_dim, generator=g))
            layers.append(p)
            for ks, vs in per_block:
                ks.append(lin(cross_dim, dim, 8 * std))
                vs.append(lin(cross_dim, dim))
    model.encoder_hid_proj = MultiIPAdapterImageProjection(layers)
    for block, (ks, vs) in zip(model.transformer_blocks, per_block):
        block.__class__ = IPFluxTransformerBlock
        block.attn.__class__ = IPAttention
        proc = nn.Module()
        proc.to_k_ip, proc.to_v_ip = nn.ModuleList(ks), nn.ModuleList(vs)
        proc.scale = [1.0] * len(ks)
        block.attn.processor = proc
    return model


def set_ip_adapter_scale(model, scales):
    """scales [n_adapters][n_double] (magcache_amd.ip_adapter.normalise_scales): block i's processor reads scales[j][i]"""
    for i, block in enumerate(model.transformer_blocks):
        block.attn.processor.scale = [float(s[i]) for s in scales]


def adapter_state_dict(model, j):
    """adapter j's weights under their names in the loaded model (the second spelling of ip_adapter.parse_state_dict)"""
    pre = ("encoder_hid_proj.image_projection_layers.%d." % j,)
    mid = (".attn.processor.to_k_ip.%d." % j, ".attn.processor.to_v_ip.%d." % j)
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(pre) or any(m in k for m in mid)}


def checkpoint_state_dict(model, j):
    """the same adapter as an adapter FILE holds it: {"image_proj": {...}, "ip_adapter": {"<i>.to_k_ip.weight", ...}}"""
    p = model.encoder_hid_proj.image_projection_layers[j]
    image_proj = {"proj.weight": p.image_embeds.weight, "proj.bias": p.image_embeds.bias, "norm.weight": p.norm.weight,
                  "norm.bias": p.norm.bias}
    ip = {}
    for i, block in enumerate(model.transformer_blocks):
        for kv in ("k", "v"):
            m = getattr(block.attn.processor, "to_%s_ip" % kv)[j]
            ip["%d.to_%s_ip.weight" % (i, kv)], ip["%d.to_%s_ip.bias" % (i, kv)] = m.weight, m.bias
    return {"image_proj": {k: v.detach().clone() for k, v in image_proj.items()}, "ip_adapter": {k: v.detach().clone() for k, v in ip.items()}}


def base_state_dict(model):
    """the transformer's own weights (what FluxTransformer2DModelHIP.load_state_dict takes)"""
    return {k: v for k, v in model.state_dict().items() if not k.startswith("encoder_hid_proj.") and ".attn.processor." not in k}


def plain_forward(model, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                  joint_attention_kwargs=None, controlnet_block_samples=None, controlnet_single_block_samples=None):
    """upstream's forward (the reference's magcache_forward without the cache) with the IP-Adapter and ControlNet arguments"""
    h, e, temb, rope = model.pre_blocks(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance)
    kw = dict(joint_attention_kwargs or {})
    if "ip_adapter_image_embeds" in kw:
        kw["ip_hidden_states"] = model.encoder_hid_proj(kw.pop("ip_adapter_image_embeds"))
    n = len(model.transformer_blocks)
    for i, block in enumerate(model.transformer_blocks):
        e, h = block(h, e, temb, rope, joint_attention_kwargs=kw)
        if controlnet_block_samples:
            h = h + controlnet_block_samples[i // int(math.ceil(n / len(controlnet_block_samples)))]
    n_txt, n = e.shape[1], len(model.single_transformer_blocks)
    h = torch.cat([e, h], dim=1)
    for i, block in enumerate(model.single_transformer_blocks):
        h = block(h, temb, rope)
        if controlnet_single_block_samples:
            h[:, n_txt:] = h[:, n_txt:] + controlnet_single_block_samples[i // int(math.ceil(n / len(controlnet_single_block_samples)))]
    return model.post_blocks(h[:, n_txt:], temb)

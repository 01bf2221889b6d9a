"""FLUX IP-Adapters on the MM-DiT engine, the host side: the names of an adapter's weights, reading an adapter state dict,
the scale forms of diffusers' set_ip_adapter_scale, the checks on joint_attention_kwargs["ip_adapter_image_embeds"] and the
two image slots of the engine (the positive and the negative image prompt of a true-CFG pipeline alternate call by call; the
K|V of every double block are computed once per tensor, not per forward).  Nothing here touches the device: the engine is
whatever object has set_ip_adapter_image / select_ip_adapter (tests/test_flux_ip_adapter_cpu.py drives it with a fake)."""
import re

import torch

MAX_ADAPTERS, MAX_KEYS = 4, 256       # MC_IP_MAX_ADAPTERS, MC_IP_MAX_KEYS of include/magcache_hip.h

# the names diffusers gives the weights of adapter j after FluxIPAdapterMixin.load_ip_adapter (mc_mmdit_ip_adapter_add)
PROJ = "encoder_hid_proj.image_projection_layers.{j}."
ATTN = "transformer_blocks.{i}.attn.processor."


def name_templates(n_double):
    """every name an adapter registers in the engine, its index still open as "{j}", in a fixed order"""
    names = [PROJ + "image_embeds.weight", PROJ + "image_embeds.bias", PROJ + "norm.weight", PROJ + "norm.bias"]
    for i in range(n_double):
        a = ATTN.replace("{i}", str(i))
        names += [a + "to_k_ip.{j}.weight", a + "to_k_ip.{j}.bias", a + "to_v_ip.{j}.weight", a + "to_v_ip.{j}.bias"]
    return names


def weight_names(j, n_double):
    return [n.format(j=j) for n in name_templates(n_double)]


_CKPT_PROJ = {"proj.weight": "image_embeds.weight", "proj.bias": "image_embeds.bias", "norm.weight": "norm.weight",
              "norm.bias": "norm.bias"}


def _flatten(sd):
    flat = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{kk}": vv for kk, vv in _flatten(v).items()})
        else:
            flat[k] = v
    return flat


def parse_state_dict(sd, n_double, tokens_per_image=None):
    """One adapter's state dict -> dict(embed_dim, cross_dim, tokens, weights, unknown): `weights` maps the engine names with
    "{j}" still open (format them with the adapter's index) to tensors.  Two spellings are read:
      * the adapter file's: {"image_proj": {"proj.weight", "proj.bias", "norm.weight", "norm.bias"},
        "ip_adapter": {"<i>.to_k_ip.weight", "<i>.to_k_ip.bias", "<i>.to_v_ip.weight", "<i>.to_v_ip.bias"}} with <i> counting
        the double blocks, nested as diffusers loads it or flattened with dots;
      * the module names of a loaded diffusers model (weight_names above) for ONE adapter index, whatever it is there.
    Shapes give embed_dim, cross_dim and tokens per image (image_embeds.weight is [tokens * cross_dim, embed_dim]);
    `tokens_per_image`, when given, must agree.  `unknown`: keys that are no IP-Adapter weight.  ValueError for a missing
    weight, inconsistent shapes or more than one adapter index."""
    flat = _flatten(sd)
    w, unknown, seen = {}, [], set()
    pat_proj = re.compile(r"^encoder_hid_proj\.image_projection_layers\.(\d+)\.(image_embeds|norm)\.(weight|bias)$")
    pat_attn = re.compile(r"^transformer_blocks\.(\d+)\.attn\.processor\.to_([kv])_ip\.(\d+)\.(weight|bias)$")
    pat_ckpt = re.compile(r"^ip_adapter\.(\d+)\.to_([kv])_ip\.(weight|bias)$")
    for k, v in flat.items():
        m = pat_proj.match(k)
        if m:
            seen.add(int(m.group(1)))
            w[PROJ + f"{m.group(2)}.{m.group(3)}"] = v
            continue
        m = pat_attn.match(k)
        if m:
            seen.add(int(m.group(3)))
            w[ATTN.replace("{i}", m.group(1)) + f"to_{m.group(2)}_ip.{{j}}.{m.group(4)}"] = v
            continue
        m = pat_ckpt.match(k)
        if m:
            w[ATTN.replace("{i}", m.group(1)) + f"to_{m.group(2)}_ip.{{j}}.{m.group(3)}"] = v
            continue
        if k.startswith("image_proj.") and k[len("image_proj."):] in _CKPT_PROJ:
            w[PROJ + _CKPT_PROJ[k[len("image_proj."):]]] = v
            continue
        unknown.append(k)
    if len(seen) > 1:
        raise ValueError(f"IP-Adapter state dict holds adapters {sorted(seen)}: load one adapter per call")
    want = name_templates(n_double)
    missing = [n for n in want if n not in w]
    if missing:
        raise ValueError(f"IP-Adapter state dict: {len(missing)} weights missing for {n_double} double blocks, e.g. {missing[:3]}")
    extra = sorted(set(w) - set(want))
    if extra:
        raise ValueError(f"IP-Adapter state dict has weights for blocks the model does not have, e.g. {extra[:3]}")
    proj = w[PROJ + "image_embeds.weight"]
    k0 = w[ATTN.replace("{i}", "0") + "to_k_ip.{j}.weight"]
    if proj.dim() != 2 or k0.dim() != 2:
        raise ValueError("IP-Adapter weights must be matrices")
    embed_dim, cross_dim = int(proj.shape[1]), int(k0.shape[1])
    if cross_dim <= 0 or proj.shape[0] % cross_dim:
        raise ValueError(f"image_embeds.weight {tuple(proj.shape)} is no multiple of cross_dim {cross_dim}")
    tokens = int(proj.shape[0]) // cross_dim
    if tokens_per_image is not None and int(tokens_per_image) != tokens:
        raise ValueError(f"tokens_per_image {tokens_per_image}, but image_embeds.weight {tuple(proj.shape)} / cross_dim {cross_dim} = {tokens}")
    return dict(embed_dim=embed_dim, cross_dim=cross_dim, tokens=tokens, weights={n: w[n] for n in want}, unknown=unknown)


def normalise_scales(scale, n_adapters, n_double):
    """diffusers' set_ip_adapter_scale forms -> [n_adapters][n_double] floats: a number (every adapter, every block), a list
    with one entry per adapter, each a number or a list of n_double numbers."""
    if n_adapters < 1:
        raise ValueError("no IP-Adapter is loaded (load_ip_adapter)")
    if not isinstance(scale, (list, tuple)):
        scale = [scale] * n_adapters
    if len(scale) != n_adapters:
        raise ValueError(f"{len(scale)} scales for {n_adapters} IP-Adapters")
    out = []
    for s in scale:
        if isinstance(s, (list, tuple)):
            if len(s) != n_double:
                raise ValueError(f"{len(s)} per-block scales for {n_double} double blocks")
            out.append([float(v) for v in s])
        else:
            out.append([float(s)] * n_double)
    return out


def check_embeds(embeds, adapters):
    """joint_attention_kwargs["ip_adapter_image_embeds"] against the loaded adapters ([(embed_dim, tokens)]): a list with one
    [1, n_images, embed_dim] or [n_images, embed_dim] floating-point tensor per adapter.  Returns the [n_images, embed_dim]
    views; ValueError before anything is set."""
    if not adapters:
        raise ValueError("ip_adapter_image_embeds were passed but no IP-Adapter is loaded: call load_ip_adapter first")
    if torch.is_tensor(embeds) or not isinstance(embeds, (list, tuple)):
        raise ValueError("ip_adapter_image_embeds must be a list with one tensor per IP-Adapter")
    if len(embeds) != len(adapters):
        raise ValueError(f"{len(embeds)} ip_adapter_image_embeds for {len(adapters)} loaded IP-Adapters")
    out = []
    for j, (t, (embed_dim, tokens)) in enumerate(zip(embeds, adapters)):
        if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"ip_adapter_image_embeds[{j}] must be a float32, bfloat16 or float16 tensor")
        v = t[0] if t.dim() == 3 and t.shape[0] == 1 else t
        if v.dim() != 2 or v.shape[1] != embed_dim or v.shape[0] < 1:
            raise ValueError(f"ip_adapter_image_embeds[{j}] is {tuple(t.shape)}: expected [1, n_images, {embed_dim}] or [n_images, {embed_dim}]")
        if v.shape[0] * tokens > MAX_KEYS:
            raise ValueError(f"ip_adapter_image_embeds[{j}]: {v.shape[0]} images of {tokens} tokens are more than {MAX_KEYS} keys")
        out.append(v)
    return out


class ImageSlots:
    """Which of the engine's two image slots holds which list of embeds tensors (model._tensor_key: identity and version
    counter, no content compare and no device sync).  use() selects the slot of the call's embeds, computing it first where
    neither slot has them: a slot that holds the same storage with older contents is computed again in place, otherwise the slot
    used least recently is replaced."""

    def __init__(self):
        self.keys = [None, None]
        self.lru = 0

    def forget(self):
        self.keys = [None, None]
        self.lru = 0

    def use(self, engine, embeds):
        from .model import _same_tensor, _tensor_key
        for slot, key in enumerate(self.keys):
            if key is not None and len(key) == len(embeds) and all(_same_tensor(k, t) for k, t in zip(key, embeds)):
                engine.select_ip_adapter(slot)
                self.lru = 1 - slot
                return slot
        slot = self.lru
        for i, key in enumerate(self.keys):           # the same storage with other contents (an in-place write): its own slot again
            if key is not None and len(key) == len(embeds) and all(k[0].data_ptr() == t.data_ptr() and k[0].shape == t.shape
                                                                   for k, t in zip(key, embeds)):
                slot = i
        self.keys[slot] = None                     # a failure below leaves the slot unclaimed
        for j, t in enumerate(embeds):
            engine.set_ip_adapter_image(j, slot, t)
        self.keys[slot] = [_tensor_key(t) for t in embeds]
        engine.select_ip_adapter(slot)
        self.lru = 1 - slot
        return slot

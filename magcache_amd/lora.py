"""LoRA state dicts -> the weight names of the engines.  Pure Python: no GPU, no library.  The MM-DiT engine's reader comes
first; the Wan engine's (parse_wan_lora_state_dict, wan_lora_target_names) is at the end of the file.

An adapter file names the MODULE it wraps; the engine names WEIGHTS, by their upstream state_dict names
(mc_mmdit_set_weight), and takes an adapter pair per such name (mc_mmdit_lora_set) -- also where it stores several upstream
matrices as one (q | k | v, the stacked modulation matrix): `transformer_blocks.3.attn.to_q` addresses its rows of the
fused matrix by its own name.  So the mapping is `<module>` -> `<module>.weight`, and what is left to do here is to read
the spellings adapter files come in:

    <module>.lora_A.weight / <module>.lora_B.weight                      PEFT
    <module>.lora_A.<adapter>.weight / <module>.lora_B.<adapter>.weight  PEFT, inside a model with named adapters
    <module>.lora.down.weight / <module>.lora.up.weight                  the older diffusers spelling
    <module>.alpha                                                       optional, any spelling: factor = alpha / rank

lora_A / down is [rank, in_features], lora_B / up is [out_features, rank].
"""
import re

_PAIR = re.compile(r"^(?P<module>.+)\.(?:lora_(?P<ab>[AB])(?:\.[^.]+)?|lora\.(?P<du>down|up))\.weight$")
_ALPHA = re.compile(r"^(?P<module>.+)\.alpha$")


def parse_lora_state_dict(sd, prefix="transformer."):
    """{target weight name: (down [rank, in], up [out, rank], alpha or None)} of a LoRA state dict.

    prefix: pipeline-level files put the transformer's modules under "transformer." next to other components
    ("text_encoder."): where any key carries the prefix, the keys that carry it are the adapter (prefix removed) and the
    others are another component's; where none does, every key is taken as it is.  Within the keys taken, one that is no
    half of a pair and no alpha of one raises ValueError, as does a pair whose ranks differ."""
    keys = list(sd.keys())
    if prefix and any(k.startswith(prefix) for k in keys):
        keys = [k for k in keys if k.startswith(prefix)]
        strip = len(prefix)
    else:
        strip = 0
    down, up, alpha, orphans = {}, {}, {}, []
    for key in keys:
        name = key[strip:]
        m = _PAIR.match(name)
        if m:
            is_down = m.group("ab") == "A" or m.group("du") == "down"
            half = down if is_down else up
            if m.group("module") in half:
                raise ValueError(f"LoRA state dict: '{key}' repeats a matrix of '{m.group('module')}' (several adapters in one "
                                 "state dict: load them one by one)")
            half[m.group("module")] = sd[key]
            continue
        m = _ALPHA.match(name)
        if m:
            alpha[m.group("module")] = sd[key]
            continue
        orphans.append(key)
    orphans += [f"{m} (down without up)" for m in down if m not in up]
    orphans += [f"{m} (up without down)" for m in up if m not in down]
    orphans += [f"{m}.alpha (no pair)" for m in alpha if m not in down and m not in up]
    if orphans:
        raise ValueError(f"LoRA state dict: {len(orphans)} keys belong to no down / up pair, e.g. {sorted(orphans)[:5]}")
    out = {}
    for module, d in down.items():
        u = up[module]
        if len(d.shape) != 2 or len(u.shape) != 2 or d.shape[0] != u.shape[1]:
            raise ValueError(f"LoRA pair of '{module}': down {tuple(d.shape)} and up {tuple(u.shape)} share no rank")
        a = alpha.get(module)
        out[module + ".weight"] = (d, u, None if a is None else float(a))
    return out


def lora_factor(down, alpha):
    """alpha / rank of a pair; 1 where the file carries no alpha"""
    return 1.0 if alpha is None else float(alpha) / int(down.shape[0])


def lora_target_names(family, n_double, n_single=0, refiner_depth=0):
    """The weight names of an MM-DiT engine that take an adapter, by family ("flux", "hunyuan", "qwen"): every bf16 matrix
    of a GEMM -- the block Linears (the parts of a fused matrix under their own names), the modulation Linears, the
    embedders' MLPs and the text embedder.  Not among them: the fp32 head (proj_out / final_layer.linear), the image
    embedder where its input width is padded, norm weights and biases."""
    names = []

    def add(prefix, modules):
        names.extend(f"{prefix}{m}.weight" for m in modules)
    if family in ("flux", "qwen"):
        flux = family == "flux"
        add("", ["context_embedder" if flux else "txt_in",
                 "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2"])
        if flux:
            add("time_text_embed.", ["guidance_embedder.linear_1", "guidance_embedder.linear_2", "text_embedder.linear_1",
                                     "text_embedder.linear_2"])
        ff, ffc = ("ff", "ff_context") if flux else ("img_mlp", "txt_mlp")
        for i in range(n_double):
            add(f"transformer_blocks.{i}.", (["norm1.linear", "norm1_context.linear"] if flux else ["img_mod.1", "txt_mod.1"]) + [
                "attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj",
                "attn.to_add_out", f"{ff}.net.0.proj", f"{ff}.net.2", f"{ffc}.net.0.proj", f"{ffc}.net.2"])
        for i in range(n_single):
            add(f"single_transformer_blocks.{i}.", ["norm.linear", "attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp", "proj_out"])
        add("", ["norm_out.linear"])
    elif family == "hunyuan":
        add("", ["txt_in.input_embedder", "time_in.mlp.0", "time_in.mlp.2", "guidance_in.mlp.0", "guidance_in.mlp.2",
                 "vector_in.in_layer", "vector_in.out_layer", "txt_in.t_embedder.mlp.0", "txt_in.t_embedder.mlp.2",
                 "txt_in.c_embedder.linear_1", "txt_in.c_embedder.linear_2"])
        for i in range(refiner_depth):
            add(f"txt_in.individual_token_refiner.blocks.{i}.", ["self_attn_qkv", "self_attn_proj", "mlp.fc1", "mlp.fc2",
                                                                 "adaLN_modulation.1"])
        for i in range(n_double):
            for s in ("img", "txt"):
                add(f"double_blocks.{i}.{s}", ["_mod.linear", "_attn_qkv", "_attn_proj", "_mlp.fc1", "_mlp.fc2"])
        for i in range(n_single):
            add(f"single_blocks.{i}.", ["modulation.linear", "linear1", "linear2"])
        add("", ["final_layer.adaLN_modulation.1"])
    else:
        raise ValueError(f"unknown family '{family}'")
    return names


# ------------------------------------------------------------------------------------------------ Wan
_WAN_PREFIXES = ("model.diffusion_model.", "diffusion_model.", "transformer.")   # longest first
_WAN_PAIR = re.compile(r"^(?P<module>.+)\.(?:lora_(?P<ab>[AB])(?:\.[^.]+)?|lora\.(?P<du>down|up)|lora_(?P<du2>down|up))\.weight$")
_WAN_DELTA = re.compile(r"^(?P<module>.+)\.(?P<kind>diff|diff_b|diff_m)$")
# diffusers' WanTransformer3DModel module names -> upstream WanModel's, inside a block ...
_WAN_BLOCK_TABLE = {
    "attn1.to_q": "self_attn.q", "attn1.to_k": "self_attn.k", "attn1.to_v": "self_attn.v", "attn1.to_out.0": "self_attn.o",
    "attn1.norm_q": "self_attn.norm_q", "attn1.norm_k": "self_attn.norm_k",
    "attn2.to_q": "cross_attn.q", "attn2.to_k": "cross_attn.k", "attn2.to_v": "cross_attn.v", "attn2.to_out.0": "cross_attn.o",
    "attn2.norm_q": "cross_attn.norm_q", "attn2.norm_k": "cross_attn.norm_k",
    "attn2.add_k_proj": "cross_attn.k_img", "attn2.add_v_proj": "cross_attn.v_img", "attn2.norm_added_k": "cross_attn.norm_k_img",
    "ffn.net.0.proj": "ffn.0", "ffn.net.2": "ffn.2", "norm2": "norm3", "scale_shift_table": "modulation",
}
# ... and outside the blocks
_WAN_TOP_TABLE = {
    "condition_embedder.time_embedder.linear_1": "time_embedding.0", "condition_embedder.time_embedder.linear_2": "time_embedding.2",
    "condition_embedder.time_proj": "time_projection.1",
    "condition_embedder.text_embedder.linear_1": "text_embedding.0", "condition_embedder.text_embedder.linear_2": "text_embedding.2",
    "proj_out": "head.head", "scale_shift_table": "head.modulation",
}
_WAN_BLOCK = re.compile(r"^(?P<block>(?:vace_)?blocks\.\d+)\.(?P<rest>.+)$")


def _wan_module(module):
    """an adapter file's module name as upstream WanModel spells it (diffusers' names through the tables, others as given)"""
    m = _WAN_BLOCK.match(module)
    if m:
        return m.group("block") + "." + _WAN_BLOCK_TABLE.get(m.group("rest"), m.group("rest"))
    return _WAN_TOP_TABLE.get(module, module)


def parse_wan_lora_state_dict(sd):
    """{target: ("pair", down [rank, in], up [out, rank], alpha or None) | ("delta", tensor)} of a Wan adapter state dict,
    keyed by upstream WanModel parameter names ("blocks.3.self_attn.q.weight", "blocks.3.modulation", "head.modulation"):
    the names mc_lora_set / mc_lora_set_delta take.

    Read: the pair spellings of parse_lora_state_dict plus <module>.lora_down.weight / <module>.lora_up.weight; one of the
    prefixes "model.diffusion_model.", "diffusion_model.", "transformer." (where any key carries one, the keys that carry it
    are the adapter and the others another component's); the additive spellings of the ComfyUI family, <module>.diff
    (-> <module>.weight), <module>.diff_b (-> <module>.bias) and <block>.diff_m (-> <block>.modulation; "head.diff_m" ->
    "head.modulation"); and diffusers' WanTransformer3DModel module names, mapped to upstream's by _WAN_BLOCK_TABLE /
    _WAN_TOP_TABLE.  The delta spellings and the tables are written from knowledge of those projects: neither an adapter
    file nor a copy of diffusers was at hand to check them against.

    ValueError for a key that is none of these, half a pair, an alpha without a pair, a pair whose ranks differ, and a
    matrix or parameter that two keys address."""
    keys = list(sd.keys())
    strip = 0
    for prefix in _WAN_PREFIXES:
        if any(k.startswith(prefix) for k in keys):
            keys = [k for k in keys if k.startswith(prefix)]
            strip = len(prefix)
            break
    down, up, alpha, delta, orphans = {}, {}, {}, {}, []
    for key in keys:
        name = key[strip:]
        m = _WAN_PAIR.match(name)
        if m:
            module = _wan_module(m.group("module"))
            is_down = m.group("ab") == "A" or "down" in (m.group("du"), m.group("du2"))
            half = down if is_down else up
            if module in half:
                raise ValueError(f"LoRA state dict: '{key}' repeats a matrix of '{module}' (several adapters in one state "
                                 "dict: load them one by one)")
            half[module] = sd[key]
            continue
        m = _ALPHA.match(name)
        if m:
            alpha[_wan_module(m.group("module"))] = sd[key]
            continue
        m = _WAN_DELTA.match(name)
        if m:
            module, kind = _wan_module(m.group("module")), m.group("kind")
            if kind == "diff_m":
                target = module + ".modulation"
            elif module.endswith("modulation"):     # diffusers' scale_shift_table is a parameter, not a module
                target = module
            else:
                target = module + (".bias" if kind == "diff_b" else ".weight")
            if target in delta:
                raise ValueError(f"LoRA state dict: '{key}' repeats the delta of '{target}'")
            delta[target] = sd[key]
            continue
        orphans.append(key)
    orphans += [f"{m} (down without up)" for m in down if m not in up]
    orphans += [f"{m} (up without down)" for m in up if m not in down]
    orphans += [f"{m}.alpha (no pair)" for m in alpha if m not in down and m not in up]
    if orphans:
        raise ValueError(f"LoRA state dict: {len(orphans)} keys belong to no down / up pair and are no delta, e.g. {sorted(orphans)[:5]}")
    out = {}
    for module, d in down.items():
        u = up[module]
        if len(d.shape) != 2 or len(u.shape) != 2 or d.shape[0] != u.shape[1]:
            raise ValueError(f"LoRA pair of '{module}': down {tuple(d.shape)} and up {tuple(u.shape)} share no rank")
        a = alpha.get(module)
        out[module + ".weight"] = ("pair", d, u, None if a is None else float(a))
    for target, t in delta.items():
        if target in out:
            raise ValueError(f"LoRA state dict: '{target}' has a low-rank pair and a delta")
        out[target] = ("delta", t)
    return out


def wan_lora_target_names(cfg):
    """Every parameter name of a Wan engine built from `cfg` that takes a low-rank pair (the matrices: "....weight" of a
    Linear, bf16 in the blocks and embedders, fp32 for time_embedding, time_projection and head.head) or an additive delta
    (biases, norm weights, modulation tables, the fp32 matrices): the engine's whole state dict minus the patch embedders'
    weights, which take neither."""
    from .engine import weight_names
    return [n for n, _ in weight_names(cfg) if n not in ("patch_embedding.weight", "vace_patch_embedding.weight")]

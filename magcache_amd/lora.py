"""LoRA state dicts -> the weight names of the engines.  Pure Python: no GPU, no library.  The MM-DiT engine's reader comes
first, then the Wan engine's (parse_wan_lora_state_dict, wan_lora_target_names at the end of the file); between them the
readers both engines load files through, which add DoRA, LoKr and LoHa to what those two read (parse_adapter_state_dict,
parse_wan_adapter_state_dict).

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


# ------------------------------------------------------------------------------------------------ DoRA, LoKr, LoHa
# The readers both engines use (adapters.LoraHost._lora_entries, engine.Engine._lora_entries).  They read everything the two
# readers above read -- through them, so a plain LoRA file gives exactly their entries -- and three more kinds of key, each
# also with a trailing ".<adapter>" infix:
#
#   <module>.lora_magnitude_vector[.<adapter>][.weight]  | <module>.dora_scale     DoRA magnitude, [out] or [out, 1]
#   <module>.lokr_w1 | .lokr_w1_a @ .lokr_w1_b,  <module>.lokr_w2 | .lokr_w2_a @ .lokr_w2_b      LoKr: kron(w1, w2)
#   <module>.hada_w1_a [out, r], .hada_w1_b [r, in], .hada_w2_a, .hada_w2_b        LoHa: (w1_a w1_b) * (w2_a w2_b)
#   <module>.alpha                                                                 optional, as for pairs
#
# Entries, next to the pair / delta entries of the reader above:
#   ("kron", w1, w2, factor)                    w1, w2: a tensor, or the tuple (a, b) of a factorised half (a @ b is the half)
#   ("hada", w1_a, w1_b, w2_a, w2_b, factor)
#   ("dora", inner, magnitude [out])            inner: ("pair", down, up, alpha) or one of the two above
# Refused (ValueError): lokr_t2 / hada_t1 / hada_t2 (Tucker / conv forms), a per-input-column magnitude [1, in], a magnitude
# on a module that has no term, two spellings of one tensor, halves that share no rank, half a LoKr / LoHa set, LoKr and LoHa
# (or one of them and a pair) on one module.  Whether kron(w1, w2) has the weight's shape only the engine can say
# (mc_lora_set_kron: MC_EINVAL).  Key names and the three rules below are LyCORIS's and PEFT's as remembered: [UPSTREAM] in
# INTEGRATION.md.
_MAGNITUDE = re.compile(r"^(?P<module>.+)\.(?:lora_magnitude_vector(?:\.[^.]+)?(?:\.weight)?|dora_scale(?:\.[^.]+)?)$")
_KIND = re.compile(r"^(?P<module>.+)\.(?P<what>lokr_w[12](?:_[ab])?|lokr_t2|hada_w[12]_[ab]|hada_t[12])(?:\.[^.]+)?$")
_TUCKER = ("lokr_t2", "hada_t1", "hada_t2")


def dora_magnitude(module, t):
    """[UPSTREAM] the magnitude of a module as a 1-D [out] tensor: PEFT stores [out], LyCORIS's dora_scale [out, 1]"""
    shape = tuple(t.shape)
    if len(shape) == 1:
        return t
    if len(shape) == 2 and shape[1] == 1:
        return t.reshape(shape[0])
    if len(shape) == 2 and shape[0] == 1:
        raise ValueError(f"DoRA magnitude of '{module}' is {shape}: one value per input column (LyCORIS's per-input-column "
                         "variant), which is not supported; the engines take one value per output row")
    raise ValueError(f"DoRA magnitude of '{module}' is {shape}, expected [out] or [out, 1]")


def lokr_factor(alpha, rank):
    """[UPSTREAM] alpha / rank where a half is factorised (rank: its inner dimension), 1 where both halves are full (rank None)
    or the file carries no alpha"""
    return 1.0 if alpha is None or rank is None else float(alpha) / int(rank)


def loha_factor(alpha, rank):
    """[UPSTREAM] alpha / rank; 1 where the file carries no alpha"""
    return 1.0 if alpha is None else float(alpha) / int(rank)


def _lokr_half(module, parts, n):
    """(half, rank or None): lokr_w<n>, or (lokr_w<n>_a, lokr_w<n>_b)"""
    full, a, b = (parts.get(f"lokr_w{n}{s}") for s in ("", "_a", "_b"))
    if full is not None and (a is not None or b is not None):
        raise ValueError(f"LoKr of '{module}': lokr_w{n} repeats what lokr_w{n}_a / lokr_w{n}_b spell (two spellings of one tensor)")
    if full is not None:
        if len(full.shape) != 2:
            raise ValueError(f"LoKr of '{module}': lokr_w{n} is {tuple(full.shape)}, not a matrix (conv forms are not supported)")
        return full, None
    if a is None or b is None:
        raise ValueError(f"LoKr of '{module}': keys belong to no complete set (lokr_w{n}, or lokr_w{n}_a and lokr_w{n}_b, is missing)")
    if len(a.shape) != 2 or len(b.shape) != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"LoKr of '{module}': lokr_w{n}_a {tuple(a.shape)} and lokr_w{n}_b {tuple(b.shape)} share no rank")
    return (a, b), int(a.shape[1])


def _kind_entry(module, parts, alpha):
    lokr = any(k.startswith("lokr") for k in parts)
    if lokr and any(k.startswith("hada") for k in parts):
        raise ValueError(f"adapter state dict: '{module}' has LoKr and LoHa keys")
    if lokr:
        (w1, rank1), (w2, rank2) = _lokr_half(module, parts, 1), _lokr_half(module, parts, 2)
        if rank1 is not None and rank2 is not None and rank1 != rank2:
            raise ValueError(f"LoKr of '{module}': the factorised halves share no rank ({rank1} and {rank2})")
        return ("kron", w1, w2, lokr_factor(alpha, rank2 if rank2 is not None else rank1))
    names = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")
    missing = [n for n in names if n not in parts]
    if missing:
        raise ValueError(f"LoHa of '{module}': keys belong to no complete set ({missing} missing)")
    w1a, w1b, w2a, w2b = (parts[n] for n in names)
    if any(len(t.shape) != 2 for t in (w1a, w1b, w2a, w2b)):
        raise ValueError(f"LoHa of '{module}': the factors are matrices (conv forms are not supported)")
    rank = int(w1a.shape[1])
    if w1b.shape[0] != rank or w2a.shape[1] != rank or w2b.shape[0] != rank or w1a.shape[0] != w2a.shape[0] or w1b.shape[1] != w2b.shape[1]:
        raise ValueError(f"LoHa of '{module}': {[tuple(t.shape) for t in (w1a, w1b, w2a, w2b)]} share no rank")
    return ("hada", w1a, w1b, w2a, w2b, loha_factor(alpha, rank))


def _parse_adapter(items, old_reader, module_of, tag_pair):
    """items: [(name with the file's prefix removed, key as the file has it, tensor)].  The keys of the three new kinds are taken
    out, the rest goes through `old_reader`; module_of: a file's module name -> the engine's; tag_pair: an entry of the old
    reader -> the ("pair", ...) form a "dora" entry holds."""
    rest, parts, mags = {}, {}, {}
    for name, key, t in items:
        m = _MAGNITUDE.match(name)
        if m:
            module = module_of(m.group("module"))
            if module in mags:
                raise ValueError(f"adapter state dict: '{key}' repeats the magnitude of '{module}' (two spellings of one tensor)")
            mags[module] = t
            continue
        m = _KIND.match(name)
        if m:
            module, what = module_of(m.group("module")), m.group("what")
            if what in _TUCKER:
                raise ValueError(f"adapter state dict: '{key}' is a Tucker / conv factor ({what}), which is not supported")
            if what in parts.setdefault(module, {}):
                raise ValueError(f"adapter state dict: '{key}' repeats {what} of '{module}' (two spellings of one tensor)")
            parts[module][what] = t
            continue
        rest[name] = t
    alpha = {}
    for name in list(rest):
        m = _ALPHA.match(name)
        if m and module_of(m.group("module")) in parts:
            alpha[module_of(m.group("module"))] = float(rest.pop(name))
    out = dict(old_reader(rest))
    for module, p in parts.items():
        target = module + ".weight"
        if target in out:
            raise ValueError(f"adapter state dict: '{target}' has two kinds of term in one file")
        out[target] = _kind_entry(module, p, alpha.get(module))
    for module, t in mags.items():
        target = module + ".weight"
        if target not in out or (isinstance(out[target][0], str) and out[target][0] == "delta"):
            raise ValueError(f"adapter state dict: '{module}' has a DoRA magnitude and no term (a magnitude with no term is no adapter)")
        out[target] = ("dora", tag_pair(out[target]), dora_magnitude(module, t))
    return out


def parse_adapter_state_dict(sd, prefix="transformer."):
    """parse_lora_state_dict plus DoRA, LoKr and LoHa (the comment above): {target weight name: entry}, a plain pair as the
    3-tuple (down, up, alpha) of parse_lora_state_dict -- on a plain LoRA file exactly its result."""
    keys = list(sd.keys())
    strip = 0
    if prefix and any(k.startswith(prefix) for k in keys):
        keys = [k for k in keys if k.startswith(prefix)]
        strip = len(prefix)
    return _parse_adapter([(k[strip:], k, sd[k]) for k in keys], lambda rest: parse_lora_state_dict(rest, prefix=None),
                          lambda module: module, lambda e: e if isinstance(e[0], str) else ("pair",) + tuple(e))


def parse_wan_adapter_state_dict(sd):
    """parse_wan_lora_state_dict plus DoRA, LoKr and LoHa on the bf16 matrices: on a plain Wan adapter file exactly its result"""
    keys = list(sd.keys())
    strip = 0
    for prefix in _WAN_PREFIXES:
        if any(k.startswith(prefix) for k in keys):
            keys = [k for k in keys if k.startswith(prefix)]
            strip = len(prefix)
            break
    return _parse_adapter([(k[strip:], k, sd[k]) for k in keys], parse_wan_lora_state_dict, _wan_module, lambda e: e)


def wan_lora_target_names(cfg):
    """Every parameter name of a Wan engine built from `cfg` that takes a low-rank pair (the matrices: "....weight" of a
    Linear, bf16 in the blocks and embedders, fp32 for time_embedding, time_projection and head.head) or an additive delta
    (biases, norm weights, modulation tables, the fp32 matrices): the engine's whole state dict minus the patch embedders'
    weights, which take neither."""
    from .engine import weight_names
    return [n for n, _ in weight_names(cfg) if n not in ("patch_embedding.weight", "vace_patch_embedding.weight")]

"""FLUX.1 and HunyuanVideo on the HIP MM-DiT engine (include/magcache_mmdit.h), behind the reference's monkey-patch
surfaces:

    FluxTransformer2DModel.forward = magcache_forward            MagCache4FLUX/magcache_flux.py:445
      + class attributes cnt, num_steps, mag_ratios, K, magcache_thresh, retention_ratio, accumulated_ratio,
        accumulated_err, accumulated_steps, previous_residual     (:452-470)
    HYVideoDiffusionTransformer.forward = magcache_forward        MagCache4HunyuanVideo/magcache_sample_video.py:325
      + cnt, num_steps, magcache_thresh, K, retention_ratio, mag_ratios, accumulated_*, residual_cache  (:305-328)
    QwenImageTransformer2DModel.forward = magcache_forward        MagCache4QwenImage/magcache_generate.py:64
      + cnt, num_steps, magcache_thresh, K, retention_ratio, accumulated_{err,steps,ratio}[2], residual_cache[2],
        mag_ratios                                                (:63-83; MagCache4QwenImageEdit: the same functions)

`FluxTransformer2DModelHIP` / `HYVideoDiffusionTransformerHIP` stand where the upstream model objects stand (same
forward signatures and return types), `flux_magcache_forward` / `hunyuan_magcache_forward` and the two
`*_magcache_calibration` functions are drop-ins for the reference functions of the same names: same arguments, same
class-attribute names and meaning, same decision arithmetic on the host (scalar state, `<=`, FLUX's retention
rounding and its never-skipped step) -- and everything between the arguments and the return value is ONE call into the
HIP engine.  No compute happens in torch here.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import (MC_F32, MC_BF16, MC_FAMILY_FLUX, MC_FAMILY_HUNYUAN, MC_FAMILY_QWEN, MC_MODE_CALIB, MC_MODE_FULL,
                   MC_MODE_SKIP, McMmditConfig, check)
from . import ip_adapter as IP
from . import rule
from .adapters import EngineHost, LoraModel, _ptr, _stream
from .mag_ratios import TABLES
from .model import nearest_interp
from .parallel import SP_OVERLAP

FLUX_DEV = dict(in_channels=64, num_layers=19, num_single_layers=38, attention_head_dim=128, num_attention_heads=24,
                joint_attention_dim=4096, pooled_projection_dim=768, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
HUNYUAN_VIDEO = dict(patch_size=(1, 2, 2), in_channels=16, out_channels=16, hidden_size=3072, heads_num=24,
                     mm_double_blocks_depth=20, mm_single_blocks_depth=40, rope_dim_list=(16, 56, 56),
                     text_states_dim=4096, text_states_dim_2=768, guidance_embed=True)


def _f32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class MMDiTEngine(EngineHost):
    """One MM-DiT engine on one device.  PyTorch-ROCm owns the workspace and the stream, the library the rest.  The
    workspace, set_weight / load_weights, buffer and destruction are adapters.EngineHost's; load_lora / set_adapters /
    set_lora_call_scale / unload_lora / apply_lora / lora_info (adapters merged into the weights on the device,
    mc_mmdit_lora_*; magcache_amd/lora.py reads the files) adapters.LoraHost's."""
    _abi = "mc_mmdit_"

    def __init__(self, family, dim, num_heads, n_double, n_single, in_channels, out_channels, txt_dim, txt_len, vec_dim,
                 img_tokens, latent_grid=(0, 0, 0), refiner_depth=0, calibration=False, device="cuda:0", sp_rank=0,
                 sp_size=1, fp8_linear=0, mx_fp4=False, mx_fp6=False):
        """fp8_linear: 0 bf16 Linears; 2 / 3 the opt-in MX fp8 modes of mc_mmdit_config.fp8_linear (one GPU, dim >= 512).
        mx_fp4: with fp8_linear 2 | 3 those Linears are MXFP4 (W4A4) instead -- much coarser, an opt-in speed /
        quality experiment, never a default; dim a multiple of 256.  The process-wide option "mx_fp4" is set around the create
        call only and put back; the engine keeps what it read (self.mx_fp4).
        mx_fp6: the same latch for MXFP6 (W6A6, e2m3 elements; activations always quantised by separate passes); self.mx_fp6.
        Asking for both is refused by the library."""
        if not torch.cuda.is_available():
            raise RuntimeError("magcache_amd.MMDiTEngine needs a ROCm device; there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.family, self.dim, self.img_tokens, self.txt_len = family, dim, img_tokens, txt_len
        self.out_channels, self.latent_grid = out_channels, tuple(latent_grid)
        self.sp_rank, self.sp_size, self.n_blocks = sp_rank, sp_size, n_double + n_single
        self.fp8_linear = int(fp8_linear)
        self.tokens_per_rank = img_tokens // sp_size
        c = McMmditConfig(family=family, dim=dim, num_heads=num_heads, n_double=n_double, n_single=n_single,
                          in_channels=in_channels, out_channels=out_channels, txt_dim=txt_dim, txt_len=txt_len,
                          vec_dim=vec_dim, img_tokens=img_tokens, latent_f=latent_grid[0], latent_h=latent_grid[1],
                          latent_w=latent_grid[2], refiner_depth=refiner_depth, calibration=int(calibration),
                          sp_rank=sp_rank, sp_size=sp_size, fp8_linear=int(fp8_linear))

        def create():
            h = C.c_void_p()
            check(self.lib.mc_mmdit_create_sized(C.byref(c), C.sizeof(c), C.byref(h)))
            return h
        self._create_latching(create, {"mx_fp4": mx_fp4, "mx_fp6": mx_fp6}, "mc_mmdit_")
        self._bind(self.lib.mc_mmdit_workspace_bytes(self.h))
        self._rope_key = None
        self._controlnet = None
        self._ip = []                 # loaded IP-Adapters: (embed_dim, tokens per image)
        self._ip_keep = {}            # (adapter, slot) -> the staged embeds the last set_ip_adapter_image launched on
        self._lora_init()

    def geometry_bytes(self, img_tokens, latent_grid=(0, 0, 0), txt_len=None):
        """workspace bytes the geometry would need (mc_mmdit_geometry_bytes); the engine is not changed"""
        n = C.c_size_t()
        f, h, w = (int(v) for v in latent_grid)
        check(self.lib.mc_mmdit_geometry_bytes(self.h, int(img_tokens), f, h, w,
                                               int(self.txt_len if txt_len is None else txt_len), C.byref(n)))
        return n.value

    def reserve(self, geometries):
        """Size the workspace once for every geometry of the list -- (img_tokens, latent_grid, txt_len) tuples, or dicts
        with those keys; latent_grid and txt_len may be left out as in set_geometry -- so that set_geometry among them
        allocates nothing.  The maximum of their needs, not the need of the largest: the plan is not monotone in the token
        count.  A workspace that has to grow is rebound, which forgets the residual caches like set_geometry does."""
        need = self.ws.numel()
        for g in geometries:
            need = max(need, self.geometry_bytes(**g) if isinstance(g, dict) else self.geometry_bytes(*g))
        self._grow(need)
        return need

    def set_geometry(self, img_tokens, latent_grid=(0, 0, 0), txt_len=None):
        """Change the token geometry of the engine between forwards (mc_mmdit_set_geometry): image tokens, the
        HunyuanVideo latent grid, the text length (None: unchanged).  The weights stay; the workspace stays too when the new
        plan fits it (see reserve), else a larger one is allocated.  The residual caches, the calibration statistics, the
        RoPE table and the ControlNet samples are forgotten, and views handed out earlier by buffer() / residual() are
        invalid: they point into the old plan."""
        txt_len = int(self.txt_len if txt_len is None else txt_len)
        grid = tuple(int(v) for v in latent_grid)
        self._grow(self.geometry_bytes(img_tokens, grid, txt_len))
        check(self.lib.mc_mmdit_set_geometry(self.h, int(img_tokens), grid[0], grid[1], grid[2], txt_len))
        self.img_tokens, self.txt_len, self.latent_grid = int(img_tokens), txt_len, grid
        self.tokens_per_rank = self.img_tokens // self.sp_size
        self._rope_key = None
        self._controlnet = None

    def residual(self, branch=None):
        """fp32 [img_tokens / sp_size, dim] view of the cached residual (reference previous_residual / residual_cache);
        `branch` 0 / 1: that CFG branch's cache (Qwen-Image), None: the branch of the last forward."""
        name = "residual" if branch is None else f"residual_b{int(branch)}"
        return self.buffer(name, torch.float32).view(-1, self.dim)[:self.tokens_per_rank]

    def set_rope(self, cos, sin):
        """upstream use_real tables [n, 128]; uploaded only when the tensors change (constant over a sample).  The
        check is by tensor identity + version counter (model._tensor_key), not by content: no device sync per call."""
        from .model import _same_tensor, _tensor_key
        k = self._rope_key
        if k is not None and _same_tensor(k[0], cos) and _same_tensor(k[1], sin):
            return
        key = (_tensor_key(cos), _tensor_key(sin))
        cos, sin = _f32(cos, self.device), _f32(sin, self.device)
        assert cos.shape == sin.shape and cos.shape[1] == 128, f"RoPE tables {tuple(cos.shape)}"
        check(self.lib.mc_mmdit_set_rope(self.h, _ptr(cos), _ptr(sin), cos.shape[0], _stream()))
        torch.cuda.current_stream().synchronize()
        self._rope_key = key

    def set_controlnet(self, double=None, single=None, blocks_repeat=False):
        """FLUX ControlNet residuals (upstream controlnet_block_samples / controlnet_single_block_samples /
        controlnet_blocks_repeat) for every following full or calibration forward; both None clears them.  Each sample is
        [1, img_tokens, dim] or [img_tokens, dim], all bf16 or all fp32.  The engine reads the tensors in place during the
        forwards, so they are kept alive here until the next call."""
        double = list(double) if double is not None else []
        single = list(single) if single is not None else []
        if not double and not single:
            if self._controlnet is not None:
                check(self.lib.mc_mmdit_set_controlnet(self.h, None, 0, None, 0, MC_F32, 0))
                self._controlnet = None
            return
        dtypes = {t.dtype for t in double + single}
        if len(dtypes) != 1 or next(iter(dtypes)) not in (torch.float32, torch.bfloat16):
            raise ValueError(f"ControlNet samples must all be fp32 or all be bf16, got {sorted(map(str, dtypes))}")

        def rows(t):
            if t.dim() == 3 and t.shape[0] == 1:
                t = t[0]
            if tuple(t.shape) != (self.img_tokens, self.dim):
                raise ValueError(f"ControlNet sample {tuple(t.shape)}: expected [{self.img_tokens}, {self.dim}]")
            return t.detach().to(self.device).contiguous()
        keep = ([rows(t) for t in double], [rows(t) for t in single])
        lists = [(C.c_void_p * len(k))(*[t.data_ptr() for t in k]) for k in keep]
        check(self.lib.mc_mmdit_set_controlnet(self.h, lists[0], len(keep[0]), lists[1], len(keep[1]),
                                               MC_F32 if dtypes == {torch.float32} else MC_BF16, int(bool(blocks_repeat))))
        self._controlnet = keep

    # ---- FLUX IP-Adapters (mc_mmdit_ip_adapter_*; magcache_amd/ip_adapter.py reads the files and keeps the slots)
    def add_ip_adapter(self, embed_dim, cross_dim, tokens_per_image):
        """register one more adapter; its weights are then set by name (ip_adapter.weight_names).  Returns its index."""
        j = C.c_int(-1)
        check(self.lib.mc_mmdit_ip_adapter_add(self.h, int(embed_dim), int(cross_dim), int(tokens_per_image), C.byref(j)))
        self._ip.append((int(embed_dim), int(tokens_per_image)))
        return j.value

    def set_ip_adapter_image(self, adapter, slot, embeds):
        """the image prompt of `adapter` in slot 0 / 1: embeds [n_images, embed_dim] -> projection, LayerNorm and the K|V of
        every double block, once (None: empty the slot).  Not a per-forward call."""
        if embeds is None:
            check(self.lib.mc_mmdit_ip_adapter_set_image(self.h, int(adapter), int(slot), None, 0, _stream()))
            self._ip_keep.pop((adapter, slot), None)
            return
        t = _f32(embeds, self.device)
        if t.dim() != 2:
            raise ValueError(f"IP-Adapter image embeds {tuple(t.shape)}: expected [n_images, embed_dim]")
        if 0 <= adapter < len(self._ip) and t.shape[1] != self._ip[adapter][0]:
            raise ValueError(f"IP-Adapter {adapter} image embeds {tuple(t.shape)}: embed_dim is {self._ip[adapter][0]}")
        check(self.lib.mc_mmdit_ip_adapter_set_image(self.h, int(adapter), int(slot), _ptr(t), t.shape[0], _stream()))
        self._ip_keep[(adapter, slot)] = t      # the launches are asynchronous

    def set_ip_adapter_scale(self, adapter, scales):
        """a number (every double block) or one number per double block; launch arguments of the following forwards"""
        v = [float(scales)] if not isinstance(scales, (list, tuple)) else [float(x) for x in scales]
        check(self.lib.mc_mmdit_ip_adapter_scale(self.h, int(adapter), (C.c_float * len(v))(*v), len(v)))

    def select_ip_adapter(self, slot):
        """the image slot the following forwards read: 0, 1 or -1 / None for none"""
        check(self.lib.mc_mmdit_ip_adapter_select(self.h, -1 if slot is None else int(slot)))

    def clear_ip_adapter(self):
        check(self.lib.mc_mmdit_ip_adapter_clear(self.h))
        self._ip, self._ip_keep = [], {}

    def forward(self, img, timestep, guidance, txt, txt_valid, vec, mode=MC_MODE_FULL, out=None, branch=None):
        """`branch` (None = the one-slot mc_mmdit_forward): the CFG branch of mc_mmdit_forward2 (Qwen-Image 0 / 1).
        `vec` None: no pooled vector (Qwen-Image)."""
        img, txt = _f32(img, self.device), _f32(txt, self.device)
        vec = _f32(vec, self.device) if vec is not None else None
        if out is None:
            shape = (self.out_channels,) + self.latent_grid if self.family == MC_FAMILY_HUNYUAN else (self.img_tokens, self.out_channels)
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        vp = _ptr(vec) if vec is not None else C.c_void_p(0)
        if branch is None:
            check(self.lib.mc_mmdit_forward(self.h, _ptr(img), float(timestep), float(guidance), _ptr(txt), int(txt_valid),
                                            vp, mode, _ptr(out), _stream()))
        else:
            check(self.lib.mc_mmdit_forward2(self.h, _ptr(img), float(timestep), float(guidance), _ptr(txt), int(txt_valid),
                                             vp, mode, int(branch), _ptr(out), _stream()))
        return out

    # ---- the same forward in phases (sequence parallel; see MMDiTSequenceParallel)
    def begin(self, img, timestep, guidance, txt, txt_valid, vec, mode):
        img, txt, vec = _f32(img, self.device), _f32(txt, self.device), _f32(vec, self.device)
        self._keep = (img, txt, vec)          # the launches are asynchronous: keep the staging tensors alive
        check(self.lib.mc_mmdit_begin(self.h, _ptr(img), float(timestep), float(guidance), _ptr(txt), int(txt_valid),
                                      _ptr(vec), mode, _stream()))

    def block_pre(self, blk):
        check(self.lib.mc_mmdit_block_pre(self.h, blk, _stream()))

    def block_attn_local(self, blk):
        check(self.lib.mc_mmdit_block_attn_local(self.h, blk, _stream()))

    def block_post(self, blk):
        check(self.lib.mc_mmdit_block_post(self.h, blk, _stream()))

    def end(self, out=None):
        check(self.lib.mc_mmdit_end(self.h, _ptr(out) if out is not None else C.c_void_p(0), _stream()))

    def unpatchify(self, tokens, out):
        check(self.lib.mc_mmdit_unpatchify(self.h, _ptr(tokens), _ptr(out), _stream()))

    def calib_stats(self):
        out = (C.c_float * 3)()
        check(self.lib.mc_mmdit_calib_stats(self.h, out, _stream()))
        return float(out[0]), float(out[1]), float(out[2])

    def reset(self):
        check(self.lib.mc_mmdit_state_reset(self.h))


class MMDiTSequenceParallel:
    """Sequence-parallel MM-DiT forward: the IMAGE tokens are sharded across the ranks of `group` (contiguous chunks,
    global RoPE positions), the text tokens and the conditioning are replicated, and the only data-path collective is
    the per-block all-gather of the image K|V rows ("kv_gather", RCCL over xGMI through torch.distributed).  Each rank
    then attends its queries over all image shards and over the text keys and merges the two partial softmaxes by their
    log-sum-exp inside the attention kernel (local image shard + text keys first, while the gather is in flight; the
    remote shards after it).  The MagCache residual cache and skip path are shard-local; the decision
    is host arithmetic on identical state, so all ranks take the same branch."""

    def __init__(self, engine, group=None):
        import torch.distributed as dist
        self.dist, self.e, self.group = dist, engine, group
        self.P, self.rank = engine.sp_size, engine.sp_rank
        assert dist.is_initialized() and dist.get_world_size(group) == self.P
        self.inplace = dist.get_backend(group) == "nccl"
        if self.inplace:
            from .parallel import inplace_gather_selftest
            self.inplace = inplace_gather_selftest(self.P, self.rank, group, engine.device)
        self.kv = engine.buffer("kv_gather", torch.bfloat16).view(self.P, -1)
        self.Lr = engine.tokens_per_rank
        hy = engine.family == MC_FAMILY_HUNYUAN
        self.cols = 64 if hy else engine.out_channels
        self.full = torch.empty(engine.img_tokens, self.cols, dtype=torch.float32, device=engine.device)

    def _gather(self, full, mine, async_op=False):
        if self.inplace:
            return self.dist.all_gather_into_tensor(full.view(-1), mine.reshape(-1), group=self.group, async_op=async_op)
        else:
            parts = [torch.empty_like(mine) for _ in range(self.P)]
            self.dist.all_gather(parts, mine.contiguous(), group=self.group)
            for r, p_ in enumerate(parts):
                full.view(self.P, -1)[r].copy_(p_.reshape(-1))

    def forward(self, img, timestep, guidance, txt, txt_valid, vec, mode):
        """FLUX ControlNet samples are state of the rank's engine, not an argument: MMDiTEngine.set_controlnet ahead of
        this call (the FLUX shims do it), with the FULL [img_tokens, dim] tensors on every rank; block_post adds this
        rank's rows of them.
        FLUX IP-Adapters likewise: the adapters, the image prompt of each slot and the selection belong to the rank's
        engine (load_ip_adapter on every rank's model; the shims set and select the image ahead of this call).  The keys
        of an image prompt are replicated, every rank attends its own image rows over them, and nothing is gathered."""
        e = self.e
        e.begin(img, timestep, guidance, txt, txt_valid, vec, mode)
        if mode != MC_MODE_SKIP:
            for blk in range(e.n_blocks):
                e.block_pre(blk)
                # RCCL: asynchronous gather on its own stream, overlapped with the attention over the local image
                # shard and the text keys; block_post then attends the remote shards and merges
                work = self._gather(self.kv, self.kv[self.rank].clone() if not self.inplace else self.kv[self.rank],
                                    async_op=True)
                if work is not None and not SP_OVERLAP:
                    work.wait()
                    work = None
                e.block_attn_local(blk)
                if work is not None:
                    work.wait()
                e.block_post(blk)
        if e.family == MC_FAMILY_HUNYUAN:
            e.end(None)
            local = e.buffer("head_tokens", torch.float32).view(-1, 64)[:self.Lr]
            self._gather(self.full, local)
            out = torch.empty((e.out_channels,) + e.latent_grid, dtype=torch.float32, device=e.device)
            e.unpatchify(self.full, out)
            return out
        local = torch.empty(self.Lr, self.cols, dtype=torch.float32, device=e.device)
        e.end(local)
        self._gather(self.full, local)
        return self.full.clone()


def _engine_forward(model, img, t, g, txt, txt_valid, vec, mode):
    e = model.engine
    if e.sp_size > 1:
        if getattr(model, "_sp", None) is None:
            model._sp = MMDiTSequenceParallel(e, group=model.sp_group)
        return model._sp.forward(img, t, g, txt, txt_valid, vec, mode)
    return e.forward(img, t, g, txt, txt_valid, vec, mode)


def _dispatch(self, *args, **kwargs):
    return type(self).forward(self, *args, **kwargs)


class _LoraMethods(LoraModel):
    """the adapter calls of MMDiTEngine on the model objects (adapters.LoraModel); an MM-DiT adapter file's names carry a prefix"""

    def load_lora(self, sd, adapter="default", scale=1.0, strict=True, prefix="transformer."):
        return self.engine.load_lora(sd, adapter=adapter, scale=scale, strict=strict, prefix=prefix)


def _lora_call_scale(model, kwargs):
    """joint_attention_kwargs / attention_kwargs["scale"] of a call, as scale_lora_layers reads it (magcache_flux.py:62-67,
    magcache_generate.py:107-113): the call's factor on every loaded adapter, 1.0 without the key.  Without adapters the key
    is ignored (upstream warns and ignores it too)."""
    e = model.engine
    if getattr(e, "_lora", None):
        e.set_lora_call_scale(1.0 if not kwargs or kwargs.get("scale") is None else kwargs["scale"])


def _shim_set_geometry(model, img_tokens, latent_grid, txt_len, fresh):
    """dynamic_geometry: a call whose shapes differ from the engine's geometry switches the engine first and starts the
    MagCache state of a new sample, as init_*_magcache would (`fresh`: the family's rule.fresh_state).  Only between samples:
    the reference cannot change shapes in the middle of one either (its cached residual has the old shape)."""
    cnt = int(getattr(model, "cnt", 0))
    if cnt != 0:
        raise ValueError(f"geometry change in the middle of a sample (cnt = {cnt}): {model.img_tokens} image / "
                         f"{model.txt_len} text tokens -> {img_tokens} / {txt_len}")
    model.engine.set_geometry(img_tokens, latent_grid, txt_len)
    model.img_tokens, model.txt_len = img_tokens, txt_len
    if hasattr(model, "cnt"):
        for k, v in fresh.items():
            if hasattr(model, k):
                setattr(model, k, v)


# ============================================================================================== FLUX
def flux_rope(ids, axes_dim=(16, 56, 56), theta=10000.0):
    """diffusers FluxPosEmbed(ids): host float64 angles -> fp32 (cos, sin) [S, 128], each frequency twice."""
    ids = np.asarray(ids.detach().cpu().double().numpy() if torch.is_tensor(ids) else ids, dtype=np.float64)
    cos, sin = [], []
    for i, dim in enumerate(axes_dim):
        freqs = 1.0 / (theta ** (np.arange(0, dim, 2, dtype=np.float64) / dim))
        ang = np.outer(ids[:, i], freqs)
        cos.append(np.repeat(np.cos(ang), 2, axis=1))
        sin.append(np.repeat(np.sin(ang), 2, axis=1))
    return (torch.from_numpy(np.concatenate(cos, 1).astype(np.float32)), torch.from_numpy(np.concatenate(sin, 1).astype(np.float32)))


class FluxTransformer2DModelHIP(_LoraMethods):
    """Stands where diffusers' FluxTransformer2DModel stands.  One (image tokens, text length) geometry per instance, unless
    dynamic_geometry=True: then every call may bring its own (MMDiTEngine.set_geometry)."""
    dynamic_geometry = False

    def __init__(self, cfg, img_tokens, txt_len=512, device="cuda:0", calibration=True, engine=None, sp_rank=0,
                 sp_size=1, sp_group=None, dynamic_geometry=False, fp8_linear=0, mx_fp4=False, mx_fp6=False):
        self.config = SimpleNamespace(**cfg)
        self.cfg = dict(cfg)
        dim = cfg["attention_head_dim"] * cfg["num_attention_heads"]
        assert cfg["attention_head_dim"] == 128 and cfg.get("guidance_embeds", True)
        self.inner_dim, self.img_tokens, self.txt_len = dim, img_tokens, txt_len
        self.dynamic_geometry = dynamic_geometry
        self.engine = engine or MMDiTEngine(MC_FAMILY_FLUX, dim, cfg["num_attention_heads"], cfg["num_layers"],
                                            cfg["num_single_layers"], cfg["in_channels"], cfg["in_channels"],
                                            cfg["joint_attention_dim"], txt_len, cfg["pooled_projection_dim"], img_tokens,
                                            calibration=calibration, device=device, sp_rank=sp_rank, sp_size=sp_size,
                                            fp8_linear=fp8_linear, mx_fp4=mx_fp4, mx_fp6=mx_fp6)
        self.device = self.engine.device
        self.sp_group = sp_group
        self._ids_key = None

    def load_state_dict(self, sd):
        self.engine.load_weights(sd)
        return self

    # ---- IP-Adapters (diffusers FluxIPAdapterMixin)
    def load_ip_adapter(self, state_dict, tokens_per_image=None, strict=True):
        """Load ONE IP-Adapter (the spellings ip_adapter.parse_state_dict reads); a second call loads a second adapter, and the
        list in joint_attention_kwargs["ip_adapter_image_embeds"] then has one tensor per adapter in that order.  embed_dim,
        cross_dim and the tokens per image come from the shapes.  Keys that are no IP-Adapter weight raise under `strict` and
        are returned otherwise, like load_lora's.  Scales start at 1.0 (set_ip_adapter_scale)."""
        a = IP.parse_state_dict(state_dict, self.cfg["num_layers"], tokens_per_image)
        if a["unknown"] and strict:
            raise ValueError(f"IP-Adapter state dict has {len(a['unknown'])} keys that are no IP-Adapter weight, e.g. {a['unknown'][:3]}")
        e = self.engine
        if len(e._ip) >= IP.MAX_ADAPTERS:
            raise ValueError(f"at most {IP.MAX_ADAPTERS} IP-Adapters")
        j = e.add_ip_adapter(a["embed_dim"], a["cross_dim"], a["tokens"])
        for name, t in a["weights"].items():
            e.set_weight(name.format(j=j), t)
        self._ip_slots().forget()
        return a["unknown"]

    def set_ip_adapter_scale(self, scale):
        """diffusers' set_ip_adapter_scale: a number, a list with one entry per adapter, each a number or a list with one
        number per double block.  Costs nothing: the scales are arguments of the next forward's launches."""
        for j, s in enumerate(IP.normalise_scales(scale, len(self.engine._ip), self.cfg["num_layers"])):
            self.engine.set_ip_adapter_scale(j, s)

    def unload_ip_adapter(self):
        self.engine.clear_ip_adapter()
        self._ip_slots().forget()

    def _ip_slots(self):
        if getattr(self, "_ip_image_slots", None) is None:
            self._ip_image_slots = IP.ImageSlots()
        return self._ip_image_slots

    def _geometry(self, hidden_states, encoder_hidden_states):
        """dynamic_geometry: follow the call's image tokens / text length (the RoPE comes from the call's ids as always)"""
        if not self.dynamic_geometry or hidden_states.dim() != 3:
            return
        li, lt = int(hidden_states.shape[1]), int(encoder_hidden_states.shape[1])
        if (li, lt) != (self.img_tokens, self.txt_len):
            _shim_set_geometry(self, li, (0, 0, 0), lt, rule.fresh_state("flux", None))
            self._ids_key = None

    def _run(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, mode):
        assert hidden_states.dim() == 3 and hidden_states.shape[0] == 1, "one sample per call, as the FLUX pipeline does"
        assert hidden_states.shape[1] == self.img_tokens and encoder_hidden_states.shape[1] == self.txt_len
        if guidance is None:
            raise ValueError("FLUX.1-dev is guidance distilled: `guidance` is required")
        # timestep.to(hidden_states.dtype) * 1000 (:303-305): in the reference's bf16 pipeline this rounds the
        # timestep to bf16 twice; the same arithmetic runs here on the caller's dtype
        t = float((timestep.to(hidden_states.dtype) * 1000).reshape(-1)[0])
        g = float((guidance.to(hidden_states.dtype) * 1000).reshape(-1)[0])
        if txt_ids.ndim == 3:
            txt_ids = txt_ids[0]
        if img_ids.ndim == 3:
            img_ids = img_ids[0]
        from .model import _same_tensor, _tensor_key
        k = self._ids_key
        if k is None or not (_same_tensor(k[0], txt_ids) and _same_tensor(k[1], img_ids)):   # identity, no device sync
            ids = torch.cat((txt_ids, img_ids), dim=0).to(self.device, torch.float32)
            self._rope_tables = flux_rope(ids, tuple(self.cfg["axes_dims_rope"]))
            self.engine.set_rope(*self._rope_tables)
            self._ids_key = (_tensor_key(txt_ids), _tensor_key(img_ids))
        out = _engine_forward(self, hidden_states[0], t, g, encoder_hidden_states[0], self.txt_len, pooled_projections[0], mode)
        return out.unsqueeze(0).to(hidden_states.dtype)

    __call__ = _dispatch


def controlnet_sample_index(block, n_blocks, n_samples, blocks_repeat=False):
    """The list index the reference's forward reads for block `block` of n_blocks (magcache_flux.py:376-384, :418-422:
    block // int(ceil(n_blocks / n_samples)), or block % n_samples under controlnet_blocks_repeat, a rule of the double
    blocks only), as the engine computes it; ValueError where the engine refuses the pair."""
    k = _lib.load().mc_mmdit_controlnet_index(int(n_blocks), int(n_samples), int(block), int(bool(blocks_repeat)))
    if k < 0:
        raise ValueError(f"{n_samples} ControlNet samples do not fit {n_blocks} blocks (block {block})")
    return k


def _flux_set_controlnet(model, double, single, blocks_repeat, hidden_states=None, encoder_hidden_states=None):
    """the forward's ControlNet arguments -> the engine, ahead of the forward; a call without samples clears what an earlier
    call set (and touches nothing when there is nothing to clear).  The engine takes the call's geometry first
    (dynamic_geometry): the samples are checked against it."""
    if hidden_states is not None:
        model._geometry(hidden_states, encoder_hidden_states)
    e = model.engine
    if double is not None or single is not None or getattr(e, "_controlnet", None) is not None:
        e.set_controlnet(double, single, blocks_repeat)


def _flux_set_ip_adapter(model, kwargs):
    """joint_attention_kwargs["ip_adapter_image_embeds"] of a call (magcache_flux.py:108-111, :321-324) -> the engine, ahead
    of the forward: the list is checked against the loaded adapters, the slot that holds these tensors is selected (computed
    first where neither slot does); a call without the key selects none.  The key without a loaded adapter is an error --
    it used to be dropped without a word."""
    e = model.engine
    if kwargs is None or "ip_adapter_image_embeds" not in kwargs:
        if getattr(e, "_ip", None):
            e.select_ip_adapter(None)
        return
    embeds = IP.check_embeds(kwargs["ip_adapter_image_embeds"], getattr(e, "_ip", []))
    model._ip_slots().use(e, embeds)


def _flux_output(output, return_dict):
    return SimpleNamespace(sample=output) if return_dict else (output,)


def flux_plain_forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None,
                       img_ids=None, txt_ids=None, guidance=None, joint_attention_kwargs=None,
                       controlnet_block_samples=None, controlnet_single_block_samples=None, return_dict=True,
                       controlnet_blocks_repeat=False, **_):
    _lora_call_scale(self, joint_attention_kwargs)
    _flux_set_ip_adapter(self, joint_attention_kwargs)
    _flux_set_controlnet(self, controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat,
                         hidden_states, encoder_hidden_states)
    out = self._run(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, MC_MODE_FULL)
    return _flux_output(out, return_dict)


FluxTransformer2DModelHIP.forward = flux_plain_forward


def flux_magcache_forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None,
                          img_ids=None, txt_ids=None, guidance=None, joint_attention_kwargs=None,
                          controlnet_block_samples=None, controlnet_single_block_samples=None, return_dict=True,
                          controlnet_blocks_repeat=False):
    """Drop-in for MagCache4FLUX/magcache_flux.py magcache_forward (:234-445)."""
    _lora_call_scale(self, joint_attention_kwargs)
    _flux_set_ip_adapter(self, joint_attention_kwargs)
    _flux_set_controlnet(self, controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat,
                         hidden_states, encoder_hidden_states)
    _, skip_forward = rule.decide(self, "flux")      # :333-344: int(R n + 0.5), `<=`, step 11 of 28 never skipped
    out = self._run(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                    MC_MODE_SKIP if skip_forward else MC_MODE_FULL)
    rule.store_residual(self, "flux", 0, self.engine.residual())
    rule.advance(self, "flux")                                                              # :434-438
    return _flux_output(out, return_dict)


def flux_magcache_calibration(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None,
                              img_ids=None, txt_ids=None, guidance=None, joint_attention_kwargs=None,
                              controlnet_block_samples=None, controlnet_single_block_samples=None, return_dict=True,
                              controlnet_blocks_repeat=False):
    """Drop-in for magcache_flux.py magcache_calibration (:37-232)."""
    _lora_call_scale(self, joint_attention_kwargs)
    _flux_set_ip_adapter(self, joint_attention_kwargs)
    _flux_set_controlnet(self, controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat,
                         hidden_states, encoder_hidden_states)
    out = self._run(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, MC_MODE_CALIB)
    stats = rule.calibrate(self, "flux", 0, self.engine.calib_stats, self.engine.residual)   # :199-207
    _print_calibration(self, stats, self.cnt >= self.num_steps - 1)
    if rule.advance(self, "flux", reset=False):                                             # :219-223
        self.norm_ratio = []
        self.norm_std = []
        self.cos_dis = []
    return _flux_output(out, return_dict)


def _print_calibration(self, stats, last):
    """what the FLUX and HunyuanVideo calibration forwards print: the call's statistics, the three lists at the end"""
    if stats:
        print(f"time: {self.cnt}, norm_ratio: {stats[0]}, norm_std: {stats[1]}, cos_dis: {stats[2]}")
    if last:
        print("norm ratio")
        print(self.norm_ratio)
        print("norm std")
        print(self.norm_std)
        print("cos_dis")
        print(self.cos_dis)


def init_flux_magcache(model, num_inference_steps=28, magcache_thresh=0.24, K=5, retention_ratio=0.1, mag_ratios=None,
                       calibration=False):
    """The reference's patch site (magcache_flux.py:445-470) on the model's CLASS."""
    cls = model.__class__
    cls.forward = flux_magcache_calibration if calibration else flux_magcache_forward
    rule.init_state(cls, "flux", calibration)
    cls.num_steps = num_inference_steps
    table = np.asarray(TABLES["flux_dev"] if mag_ratios is None else mag_ratios, dtype=np.float64)
    if len(table) != num_inference_steps:
        table = nearest_interp(table, num_inference_steps)
    cls.mag_ratios = table
    cls.K = K
    cls.magcache_thresh = magcache_thresh
    cls.retention_ratio = retention_ratio
    model.engine.reset()
    return model


# ============================================================================================== HunyuanVideo
class HYVideoDiffusionTransformerHIP(_LoraMethods):
    """Stands where hyvideo's HYVideoDiffusionTransformer stands.  One latent grid / text length per instance, unless
    dynamic_geometry=True: then every call may bring its own (MMDiTEngine.set_geometry)."""
    dynamic_geometry = False

    def __init__(self, cfg, latent_grid, txt_len=256, device="cuda:0", calibration=True, engine=None, sp_rank=0,
                 sp_size=1, sp_group=None, dynamic_geometry=False, fp8_linear=0, mx_fp4=False, mx_fp6=False):
        self.cfg = dict(cfg)
        self.sp_group = sp_group
        self.dynamic_geometry = dynamic_geometry
        self.patch_size = tuple(cfg.get("patch_size", (1, 2, 2)))
        assert self.patch_size == (1, 2, 2)
        self.hidden_size, self.heads_num = cfg["hidden_size"], cfg["heads_num"]
        self.guidance_embed = cfg.get("guidance_embed", True)
        self.text_projection, self.use_attention_mask = "single_refiner", True
        self.latent_grid, self.txt_len = tuple(latent_grid), txt_len
        F_, H_, W_ = self.latent_grid
        self.img_tokens = F_ * (H_ // 2) * (W_ // 2)
        self.engine = engine or MMDiTEngine(MC_FAMILY_HUNYUAN, cfg["hidden_size"], cfg["heads_num"],
                                            cfg["mm_double_blocks_depth"], cfg["mm_single_blocks_depth"], cfg["in_channels"],
                                            cfg["out_channels"], cfg["text_states_dim"], txt_len, cfg["text_states_dim_2"],
                                            self.img_tokens, latent_grid=self.latent_grid, refiner_depth=2,
                                            calibration=calibration, device=device, sp_rank=sp_rank, sp_size=sp_size,
                                            fp8_linear=fp8_linear, mx_fp4=mx_fp4, mx_fp6=mx_fp6)
        self.device = self.engine.device

    def load_state_dict(self, sd):
        self.engine.load_weights(sd)
        return self

    def _geometry(self, x, text_states):
        """dynamic_geometry: follow the call's latent grid / text length (the RoPE tables come with every call)"""
        if not self.dynamic_geometry or x.dim() != 5:
            return
        grid, lt = tuple(int(v) for v in x.shape[2:]), int(text_states.shape[1])
        if (grid, lt) != (self.latent_grid, self.txt_len):
            _shim_set_geometry(self, grid[0] * (grid[1] // 2) * (grid[2] // 2), grid, lt, rule.fresh_state("hunyuan", None))
            self.latent_grid = grid

    def _run(self, x, t, text_states, text_mask, text_states_2, freqs_cos, freqs_sin, guidance, mode):
        assert x.dim() == 5 and x.shape[0] == 1, "one sample per call, as the HunyuanVideo sampler does"
        assert tuple(x.shape[2:]) == self.latent_grid and text_states.shape[1] == self.txt_len
        if self.guidance_embed and guidance is None:
            raise ValueError("Didn't get guidance strength for guidance distilled model.")   # :60-63
        assert freqs_cos is not None and freqs_sin is not None
        m = text_mask[0].to(torch.bool)
        n_valid = int(m.sum())
        assert n_valid > 0 and bool(m[:n_valid].all()), "text_mask must be a prefix mask (tokenizer right padding)"
        self.engine.set_rope(freqs_cos, freqs_sin)
        out = _engine_forward(self, x[0], float(t.reshape(-1)[0]), float(guidance.reshape(-1)[0]), text_states[0], n_valid,
                              text_states_2[0], mode)
        return out.unsqueeze(0).to(x.dtype)

    __call__ = _dispatch


def _hy_output(img, return_dict):
    return {"x": img} if return_dict else img


def hunyuan_plain_forward(self, x, t, text_states=None, text_mask=None, text_states_2=None, freqs_cos=None,
                          freqs_sin=None, guidance=None, return_dict=True):
    self._geometry(x, text_states)
    return _hy_output(self._run(x, t, text_states, text_mask, text_states_2, freqs_cos, freqs_sin, guidance, MC_MODE_FULL),
                      return_dict)


HYVideoDiffusionTransformerHIP.forward = hunyuan_plain_forward


def hunyuan_magcache_forward(self, x, t, text_states=None, text_mask=None, text_states_2=None, freqs_cos=None,
                             freqs_sin=None, guidance=None, return_dict=True):
    """Drop-in for MagCache4HunyuanVideo/magcache_sample_video.py magcache_forward (:29-160)."""
    self._geometry(x, text_states)
    _, skip_forward = rule.decide(self, "hunyuan")                                           # :91-102
    img = self._run(x, t, text_states, text_mask, text_states_2, freqs_cos, freqs_sin, guidance,
                    MC_MODE_SKIP if skip_forward else MC_MODE_FULL)
    rule.store_residual(self, "hunyuan", 0, self.engine.residual())
    rule.advance(self, "hunyuan")                                                            # :149-153
    return _hy_output(img, return_dict)


def hunyuan_magcache_calibration(self, x, t, text_states=None, text_mask=None, text_states_2=None, freqs_cos=None,
                                 freqs_sin=None, guidance=None, return_dict=True):
    """Drop-in for magcache_sample_video.py magcache_calibration (:162-281)."""
    self._geometry(x, text_states)
    img = self._run(x, t, text_states, text_mask, text_states_2, freqs_cos, freqs_sin, guidance, MC_MODE_CALIB)
    stats = rule.calibrate(self, "hunyuan", 0, self.engine.calib_stats, self.engine.residual)
    _print_calibration(self, stats, self.cnt >= 49)                                          # :263 (hard-coded upstream)
    self.cnt += 1                                                                            # never wraps, as upstream
    return _hy_output(img, return_dict)


def init_hunyuan_magcache(model, infer_steps=50, magcache_thresh=0.24, K=6, retention_ratio=0.2, video_height=720,
                          mag_ratios=None, calibration=False):
    """The reference's patch site (magcache_sample_video.py:300-328) on the model's CLASS."""
    cls = model.__class__
    rule.init_state(cls, "hunyuan", calibration)
    cls.num_steps = infer_steps
    cls.magcache_thresh = magcache_thresh
    cls.K = K
    if mag_ratios is None:
        mag_ratios = TABLES["hunyuan_720p" if video_height == 720 else "hunyuan_540p"]
    table = np.asarray(mag_ratios, dtype=np.float64)
    if len(table) != infer_steps:
        table = nearest_interp(table, infer_steps)
    cls.mag_ratios = table
    cls.retention_ratio = retention_ratio
    cls.forward = hunyuan_magcache_calibration if calibration else hunyuan_magcache_forward
    model.engine.reset()
    return model


# ============================================================================================== Qwen-Image (-Edit)
QWEN_IMAGE = dict(patch_size=2, in_channels=64, out_channels=16, num_layers=60, attention_head_dim=128,
                  num_attention_heads=24, joint_attention_dim=3584, guidance_embeds=False, axes_dims_rope=(16, 56, 56))


def qwen_nearest_interp(original, target_length):
    """MagCache4QwenImage/magcache_generate.py nearest_interp (:14-21): the np.linspace form, per CFG branch."""
    original = np.asarray(original)
    if len(original) == target_length:
        return original.copy()
    return original[np.round(np.linspace(0, len(original) - 1, target_length)).astype(int)]


def qwen_rope(img_shapes, max_txt_len, axes_dim=(16, 56, 56), theta=10000.0):
    """[UPSTREAM] diffusers QwenEmbedRope(theta=10000, axes_dim=(16, 56, 56), scale_rope=True) as fp32 use_real tables
    (cos, sin) [max_txt_len + sum(f*h*w), 128], rows [text ; image 0 ; image 1 ...], every frequency twice.
    Image `idx` (0 = the noisy latent, 1 = Qwen-Image-Edit's reference image) has frame positions idx + f and centred
    row / column positions y - (h - h//2), x - (w - w//2); text token j sits at max(h//2, w//2) over the images + j on
    all three axes.  Angles are fp32 products position * theta^(-2i/dim), as upstream's rope_params computes them."""
    ids, m = [], 0
    for idx, (f, h, w) in enumerate(img_shapes):
        fi, yi, xi = np.meshgrid(np.arange(f) + idx, np.arange(h) - (h - h // 2), np.arange(w) - (w - w // 2), indexing="ij")
        ids.append(np.stack([fi.ravel(), yi.ravel(), xi.ravel()], 1))
        m = max(m, h // 2, w // 2)
    t = np.arange(max_txt_len) + m
    ids = np.concatenate([np.stack([t, t, t], 1)] + ids, 0)
    cos, sin = [], []
    for i, dim in enumerate(axes_dim):
        freqs = (1.0 / torch.pow(torch.tensor(theta), torch.arange(0, dim, 2, dtype=torch.float32) / dim)).float()
        ang = torch.outer(torch.from_numpy(ids[:, i]).float(), freqs)
        cos.append(ang.cos().repeat_interleave(2, dim=1))
        sin.append(ang.sin().repeat_interleave(2, dim=1))
    return torch.cat(cos, 1).contiguous(), torch.cat(sin, 1).contiguous()


class QwenImageTransformer2DModelHIP(_LoraMethods):
    """Stands where diffusers' QwenImageTransformer2DModel stands (Qwen-Image and Qwen-Image-Edit: the same transformer;
    Edit's image tokens are the noisy latent's followed by the reference image's).  One (image tokens, longest prompt)
    geometry per instance; every call may carry a shorter prompt (cond vs the " " negative prompt, unpadded).  The two
    CFG branches keep their own residual cache in the engine (mc_mmdit_forward2).  dynamic_geometry=True: the image
    tokens follow the call and txt_len grows with the longest prompt seen (MMDiTEngine.set_geometry)."""
    dynamic_geometry = False

    def __init__(self, cfg, img_tokens, txt_len=1024, device="cuda:0", calibration=True, engine=None, sp_size=1,
                 dynamic_geometry=False, fp8_linear=0, mx_fp4=False, mx_fp6=False):
        self.config = SimpleNamespace(**cfg)
        self.cfg = dict(cfg)
        self.dynamic_geometry = dynamic_geometry
        dim = cfg["attention_head_dim"] * cfg["num_attention_heads"]
        assert cfg["attention_head_dim"] == 128 and not cfg.get("guidance_embeds", False)
        out = cfg["patch_size"] ** 2 * cfg["out_channels"]
        self.inner_dim, self.img_tokens, self.txt_len, self.out_features = dim, img_tokens, txt_len, out
        self.engine = engine or MMDiTEngine(MC_FAMILY_QWEN, dim, cfg["num_attention_heads"], cfg["num_layers"], 0,
                                            cfg["in_channels"], out, cfg["joint_attention_dim"], txt_len, 0, img_tokens,
                                            calibration=calibration, device=device, sp_size=sp_size, fp8_linear=fp8_linear, mx_fp4=mx_fp4, mx_fp6=mx_fp6)
        self.device = self.engine.device
        self._shapes_key = None

    def load_state_dict(self, sd):
        """diffusers state_dict names (img_in, txt_norm, txt_in, time_text_embed.timestep_embedder, transformer_blocks.{i}.*,
        norm_out.linear, proj_out); a missing name raises KeyError."""
        self.engine.load_weights(sd)
        return self

    @staticmethod
    def _images(img_shapes):
        # pipeline form: [[(1, h, w)]] per batch entry (Edit: [[(1, h, w), (1, h_ref, w_ref)]]); a bare [(1, h, w)] too
        shapes = img_shapes[0] if isinstance(img_shapes[0], list) else img_shapes
        return [tuple(int(v) for v in s) for s in shapes]

    def _geometry(self, hidden_states, encoder_hidden_states, txt_seq_lens):
        """dynamic_geometry: follow the call's image tokens; txt_len stays the MAXIMUM, so only a prompt longer than it
        changes the geometry (a shorter one is this call's txt_valid, as always)"""
        if not self.dynamic_geometry or hidden_states.dim() != 3:
            return
        li = int(hidden_states.shape[1])
        n = int(txt_seq_lens[0]) if txt_seq_lens is not None else int(encoder_hidden_states.shape[1])
        if li != self.img_tokens or n > self.txt_len:
            _shim_set_geometry(self, li, (0, 0, 0), max(n, self.txt_len), rule.fresh_state("qwen", None))
            self._shapes_key = None

    def _run(self, hidden_states, encoder_hidden_states, timestep, img_shapes, txt_seq_lens, mode, branch):
        assert hidden_states.dim() == 3 and hidden_states.shape[0] == 1, "one sample per call, as the Qwen-Image pipeline does"
        assert hidden_states.shape[1] == self.img_tokens, (tuple(hidden_states.shape), self.img_tokens)
        shapes = self._images(img_shapes)
        assert sum(f * h * w for f, h, w in shapes) == self.img_tokens, ("img_shapes do not cover the image tokens", shapes)
        n = int(txt_seq_lens[0]) if txt_seq_lens is not None else int(encoder_hidden_states.shape[1])
        if not 0 < n <= min(self.txt_len, encoder_hidden_states.shape[1]):
            raise ValueError(f"text length {n} outside (0, {self.txt_len}]")
        # timestep.to(hidden_states.dtype) (:184); Timesteps(scale=1000) of the upstream embedding: the sinusoid of t * 1000
        t = float(timestep.to(hidden_states.dtype).reshape(-1)[0]) * 1000.0
        key = tuple(shapes)
        if key != self._shapes_key:
            self.engine.set_rope(*qwen_rope(shapes, self.txt_len, tuple(self.cfg["axes_dims_rope"])))
            self._shapes_key = key
        out = self.engine.forward(hidden_states[0], t, 0.0, encoder_hidden_states[0, :n], n, None, mode, branch=branch)
        return out.unsqueeze(0).to(hidden_states.dtype)

    __call__ = _dispatch


def qwen_plain_forward(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_mask=None, timestep=None,
                       img_shapes=None, txt_seq_lens=None, guidance=None, attention_kwargs=None, return_dict=True, **_):
    _lora_call_scale(self, attention_kwargs)
    self._geometry(hidden_states, encoder_hidden_states, txt_seq_lens)
    out = self._run(hidden_states, encoder_hidden_states, timestep, img_shapes, txt_seq_lens, MC_MODE_FULL, 0)
    return _flux_output(out, return_dict)


QwenImageTransformer2DModelHIP.forward = qwen_plain_forward


def qwen_magcache_forward(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_mask=None, timestep=None,
                          img_shapes=None, txt_seq_lens=None, guidance=None, attention_kwargs=None, return_dict=True):
    """Drop-in for MagCache4QwenImage/magcache_generate.py magcache_forward (:173-253): calls alternate cond / uncond
    (branch cnt % 2), strict `<`, and the accumulators are NOT reset when cnt wraps."""
    _lora_call_scale(self, attention_kwargs)
    self._geometry(hidden_states, encoder_hidden_states, txt_seq_lens)
    b, skip_forward = rule.decide(self, "qwen")                                              # :205-219
    out = self._run(hidden_states, encoder_hidden_states, timestep, img_shapes, txt_seq_lens,
                    MC_MODE_SKIP if skip_forward else MC_MODE_FULL, b)
    rule.store_residual(self, "qwen", b, self.engine.residual(b))                             # :242
    rule.advance(self, "qwen")
    return _flux_output(out, return_dict)


def qwen_magcache_calibration(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_mask=None,
                              timestep=None, img_shapes=None, txt_seq_lens=None, guidance=None, attention_kwargs=None,
                              return_dict=True):
    """Drop-in for magcache_generate.py magcache_calibration (:94-171): statistics against the same branch's previous
    residual from the third call on."""
    _lora_call_scale(self, attention_kwargs)
    self._geometry(hidden_states, encoder_hidden_states, txt_seq_lens)
    cnt = int(self.cnt)
    b = cnt % 2
    out = self._run(hidden_states, encoder_hidden_states, timestep, img_shapes, txt_seq_lens, MC_MODE_CALIB, b)
    stats = rule.calibrate(self, "qwen", b, self.engine.calib_stats, lambda: self.engine.residual(b))   # :140
    if stats:
        print(f"Step {cnt}: norm_ratio={stats[0]:.5f}, norm_std={stats[1]:.5f}, cos_dis={stats[2]:.5f}")
    if rule.advance(self, "qwen"):                                                            # :156-161
        print("\nCalibration Results:")
        print("norm_ratio:", self.norm_ratio)
        print("norm_std:", self.norm_std)
        print("cos_dis:", self.cos_dis)
    return _flux_output(out, return_dict)


def init_qwen_magcache(model, sample_steps=50, magcache_thresh=0.06, K=2, retention_ratio=0.2, mag_ratios=None,
                       calibration=False, edit=False):
    """The reference's patch site on the model's CLASS: init_magcache (:63-83) / init_magcache_calibration (:85-92).
    `mag_ratios` is the reference's list WITHOUT the two leading 1.0 pads (default: the Qwen-Image or -Edit table)."""
    cls = model.__class__
    rule.init_state(cls, "qwen", calibration)
    cls.num_steps = sample_steps * 2
    if calibration:
        cls.forward = qwen_magcache_calibration
    else:
        cls.forward = qwen_magcache_forward
        cls.split_step = None
        cls.mode = "t2v"
        cls.magcache_thresh = magcache_thresh
        cls.K = K
        cls.retention_ratio = retention_ratio
        if mag_ratios is None:
            mag_ratios = list(TABLES["qwen_image_edit" if edit else "qwen_image"][2:])
        table = np.array([1.0] * 2 + list(mag_ratios))
        if len(table) != sample_steps * 2:                                                  # :77-83
            con = qwen_nearest_interp(table[0::2], sample_steps)
            ucon = qwen_nearest_interp(table[1::2], sample_steps)
            table = np.concatenate([con.reshape(-1, 1), ucon.reshape(-1, 1)], axis=1).flatten()
        cls.mag_ratios = table
    model.engine.reset()
    return model

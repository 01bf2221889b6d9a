"""The adapter bookkeeping both engines' Python wrappers share: load / set_adapters / per-call scale / unload / apply / info
over the C calls of one weight store (mc_mmdit_lora_* for MMDiTEngine, mc_lora_* for the Wan Engine).  The class that mixes
this in has `lib`, `h` and `device`, names its C calls' prefix in `_lora_abi` and reads an adapter file in `_lora_entries`."""
import ctypes as C

import torch

from . import _lib
from ._lib import MC_BF16, MC_F32, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


_CLASS_DEFAULT = object()     # load_lora(prefix=...): the class's _lora_prefix


class LoraHost:
    _lora_abi = "mc_mmdit_lora_"
    _lora_prefix = "transformer."       # default `prefix` of load_lora

    def _lora_init(self):
        self._lora = {}           # adapter -> the scale set_adapters / load_lora gave it
        self._lora_call = 1.0     # the per-call factor on top of it (the shims' joint_attention_kwargs["scale"])

    def _lora_fn(self, name):
        return getattr(self.lib, self._lora_abi + name)

    def _lora_entries(self, sd, prefix):
        """{target: ("pair", down, up, alpha) | ("delta", tensor)} of an adapter state dict"""
        from .lora import parse_lora_state_dict
        return {t: ("pair",) + p for t, p in parse_lora_state_dict(sd, prefix=prefix).items()}

    def _lora_set(self, adapter, target, entry):
        """one entry into the store; the status of the C call"""
        from .lora import lora_factor
        if entry[0] == "delta":
            t = entry[1].detach().to(device=self.device, dtype=torch.float32).contiguous()
            st = self._lora_fn("set_delta")(self.h, adapter.encode(), target.encode(), _ptr(t), t.numel(), MC_F32, _stream())
        else:
            _, down, up, alpha = entry
            dt = torch.bfloat16 if down.dtype == torch.bfloat16 and up.dtype == torch.bfloat16 else torch.float32
            d = down.detach().to(device=self.device, dtype=dt).contiguous()
            u = up.detach().to(device=self.device, dtype=dt).contiguous()
            st = self._lora_fn("set")(self.h, adapter.encode(), target.encode(), _ptr(d), (C.c_int64 * 2)(*d.shape), _ptr(u),
                                      (C.c_int64 * 2)(*u.shape), MC_BF16 if dt == torch.bfloat16 else MC_F32,
                                      lora_factor(down, alpha), _stream())
        torch.cuda.current_stream().synchronize()      # the operands are read by launches on the stream
        return st

    def load_lora(self, sd, adapter="default", scale=1.0, strict=True, prefix=_CLASS_DEFAULT):
        """Load a LoRA state dict (the spellings magcache_amd/lora.py reads) as `adapter` at `scale` and merge it.  A target
        the engine takes no adapter on (an unknown name, an fp32 head or a padded embedder where the engine refuses them, wrong
        shapes) raises under `strict` -- the engine is then as before the call --, and is skipped otherwise: the skipped
        weight names are returned.  Loading a known adapter again replaces the entries it brings."""
        entries = self._lora_entries(sd, self._lora_prefix if prefix is _CLASS_DEFAULT else prefix)
        known, skipped, done = adapter in self._lora, [], 0
        for target, entry in entries.items():
            st = self._lora_set(adapter, target, entry)
            if st == _lib.MC_OK:
                done += 1
            elif st == _lib.MC_EINVAL and not strict:
                skipped.append(target)
            else:
                msg = self.lib.mc_last_error().decode()
                if done and not known:
                    self.unload_lora(adapter, _known=True)
                elif done:
                    self.apply_lora()
                raise _lib.MagCacheHipError(st, msg)
        if done or known:
            self._lora[adapter] = float(scale)
            check(self._lora_fn("scale")(self.h, adapter.encode(), float(scale) * self._lora_call))
        self.apply_lora()
        return skipped

    def set_adapters(self, names, scales=None):
        """diffusers' set_adapters: the adapters of `names` (a name or a list) are active at `scales` (a number, a list, None
        = 1.0), every other loaded adapter is off (scale 0, its pairs kept); merged at once."""
        names = [names] if isinstance(names, str) else list(names)
        scales = [1.0 if scales is None else scales] * len(names) if not isinstance(scales, (list, tuple)) else list(scales)
        if len(scales) != len(names):
            raise ValueError(f"{len(names)} adapters, {len(scales)} scales")
        unknown = [n for n in names if n not in self._lora]
        if unknown:
            raise KeyError(f"unknown adapters {unknown}; loaded: {sorted(self._lora)}")
        want = {n: 0.0 for n in self._lora}
        want.update({n: float(s) for n, s in zip(names, scales)})
        self._lora = want
        self._push_lora_scales()

    def _push_lora_scales(self):
        for n, s in self._lora.items():
            check(self._lora_fn("scale")(self.h, n.encode(), s * self._lora_call))
        self.apply_lora()

    def set_lora_call_scale(self, scale):
        """The factor of one call on every adapter's scale -- what scale_lora_layers(model, lora_scale) does at the top of
        the reference forwards and unscale_lora_layers undoes at their end.  Nothing happens without adapters or while the
        factor stays what it is; else every adapter is rescaled and the weights are merged again."""
        scale = float(scale)
        if not self._lora or scale == self._lora_call:
            return
        self._lora_call = scale
        self._push_lora_scales()

    def unload_lora(self, adapter=None, _known=False):
        """remove one adapter, or all of them (None): the weights it touched are the loaded ones again, bit for bit"""
        if adapter is not None and adapter not in self._lora and not _known:
            raise KeyError(f"unknown adapter '{adapter}'; loaded: {sorted(self._lora)}")
        check(self._lora_fn("remove")(self.h, adapter.encode() if adapter is not None else None))
        if adapter is None:
            self._lora = {}
        else:
            self._lora.pop(adapter, None)
        if not self._lora:
            self._lora_call = 1.0
        self.apply_lora()

    def apply_lora(self):
        """merge what changed (the engine's *_lora_apply): after set_weight on a weight an adapter touches; the other calls
        here apply by themselves"""
        check(self._lora_fn("apply")(self.h, _stream()))
        torch.cuda.current_stream().synchronize()

    def lora_info(self):
        a, n, b = C.c_int(), C.c_int(), C.c_size_t()
        check(self._lora_fn("info")(self.h, C.byref(a), C.byref(n), C.byref(b)))
        return dict(adapters=a.value, linears=n.value, base_bytes=b.value, scales=dict(self._lora), call_scale=self._lora_call)

"""What both engines' Python wrappers share, over the C calls of one prefix (`_abi`: mc_ for the Wan Engine, mc_mmdit_ for
MMDiTEngine).  EngineHost: the workspace PyTorch owns and the engine is bound to, weights in, buffers out, destruction.
LoraHost: the adapter bookkeeping -- load / set_adapters / per-call scale / unload / apply / info -- over the <_abi>lora_*
calls of the weight store; the class that mixes it in has `lib`, `h` and `device` and reads an adapter file in
`_lora_entries`.  LoraModel: the adapter calls of the engine on the model objects."""
import ctypes as C

import torch

from . import _lib
from ._lib import MC_BF16, MC_F32, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_CLASS_DEFAULT = object()     # load_lora(prefix=...): the class's _lora_prefix


class _LoraAbi:
    """`_lora_abi`, derived from the class's `_abi`; readable on the class as on an instance"""

    def __get__(self, obj, cls):
        return cls._abi + "lora_"


class LoraHost:
    _abi = "mc_mmdit_"
    _lora_abi = _LoraAbi()
    _lora_prefix = "transformer."       # default `prefix` of load_lora

    def _lora_init(self):
        self._lora = {}           # adapter -> the scale set_adapters / load_lora gave it
        self._lora_call = 1.0     # the per-call factor on top of it (the shims' joint_attention_kwargs["scale"])

    def _lora_fn(self, name):
        return getattr(self.lib, self._lora_abi + name)

    def _lora_entries(self, sd, prefix):
        """{target: ("pair", down, up, alpha) | ("delta", tensor) | ("kron", ...) | ("hada", ...) | ("dora", inner, magnitude)} of
        an adapter state dict (lora.py says what the last three hold)"""
        from .lora import parse_adapter_state_dict
        return {t: e if isinstance(e[0], str) else ("pair",) + tuple(e) for t, e in parse_adapter_state_dict(sd, prefix=prefix).items()}

    def _f32(self, t):
        """a tensor, or the (a, b) of a factorised half multiplied out, as contiguous fp32 on the device"""
        if isinstance(t, tuple):
            a, b = (x.detach().to(device=self.device, dtype=torch.float32) for x in t)
            return (a @ b).contiguous()
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _lora_set(self, adapter, target, entry):
        """one entry into the store; the status of the C call.  A "dora" entry is its magnitude (which meets every refusal of
        the target first), then its term: the status of the first call that fails; self._lora_half says that the magnitude
        went in and the term did not, which load_lora never leaves behind."""
        from .lora import lora_factor
        self._lora_half = False
        if entry[0] == "dora":
            g = self._f32(entry[2])
            st = self._lora_fn("set_magnitude")(self.h, adapter.encode(), target.encode(), _ptr(g), g.numel(), MC_F32, _stream())
            torch.cuda.current_stream().synchronize()
            if st != _lib.MC_OK:
                return st
            st = self._lora_set(adapter, target, entry[1])
            self._lora_half = st != _lib.MC_OK
            return st
        elif entry[0] == "kron":
            w1, w2 = self._f32(entry[1]), self._f32(entry[2])
            st = self._lora_fn("set_kron")(self.h, adapter.encode(), target.encode(), _ptr(w1), (C.c_int64 * 2)(*w1.shape), _ptr(w2),
                                           (C.c_int64 * 2)(*w2.shape), MC_F32, float(entry[3]), _stream())
        elif entry[0] == "hada":
            u1, d1, u2, d2 = (self._f32(t) for t in entry[1:5])
            st = self._lora_fn("set_hada")(self.h, adapter.encode(), target.encode(), _ptr(u1), (C.c_int64 * 2)(*u1.shape), _ptr(d1),
                                           (C.c_int64 * 2)(*d1.shape), _ptr(u2), _ptr(d2), MC_F32, float(entry[5]), _stream())
        elif entry[0] == "delta":
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
            elif st == _lib.MC_EINVAL and not strict and not self._lora_half:
                skipped.append(target)
            else:     # also half a DoRA entry under strict=False: a magnitude without its term is not skipped, it is undone
                msg = self.lib.mc_last_error().decode()
                done += self._lora_half
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


# the options that select an engine's MX element format at create time (csrc/ops.h: MxInfo::option); none set: e4m3
MX_FORMAT_OPTIONS = ("mx_fp4", "mx_fp6")


class EngineHost(LoraHost):
    """An engine handle `h` of `lib` on `device`, bound to a workspace tensor.  The subclass creates the handle, says in
    _rebound() what its Python side holds that the engine forgot with the old binding and in _release() what goes before
    the handle is destroyed, and keeps the geometry calls: their arguments differ."""

    def _fn(self, name):
        return getattr(self.lib, self._abi + name)

    def _rebound(self):
        pass

    def _release(self):
        pass

    def _create_latching(self, create, requests, query_prefix):
        """Run create() (which makes the handle and returns it) with the process-wide element-format options (MX_FORMAT_OPTIONS) set
        around that call only.  requests: {"mx_fp4": bool, "mx_fp6": bool}; for each option an explicit request wins, otherwise the
        process-wide value (MAGCACHE_HIP_OPTIONS=mx_fp6=1) stands; the previous values are put back.  The engine keeps what it
        read: self.mx_fp4 / self.mx_fp6 = <query_prefix>mx_fp4 / _mx_fp6 (handle).  Both options at 1 is the library's MC_EINVAL."""
        prev = {}
        for name in MX_FORMAT_OPTIONS:
            v = C.c_int(0)
            check(self.lib.mc_get_option(name.encode(), C.byref(v)))
            prev[name] = v.value
        try:
            for name in MX_FORMAT_OPTIONS:
                check(self.lib.mc_set_option(name.encode(), 1 if requests.get(name) else prev[name]))
            self.h = create()
        finally:
            for name in MX_FORMAT_OPTIONS:
                self.lib.mc_set_option(name.encode(), prev[name])
        for name in MX_FORMAT_OPTIONS:   # self.mx_fp4, self.mx_fp6
            setattr(self, name, bool(getattr(self.lib, query_prefix + name)(self.h)))

    def _bind(self, nbytes):
        """a zeroed workspace of `nbytes` (at least the current plan), bound with <_abi>set_workspace; the tensor it replaces
        is let go after a device synchronise (forwards in flight may still use it)"""
        workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-workspace.data_ptr()) % 256
        ws = workspace[off:off + nbytes]
        # finite, deterministic scratch: padded rows feed MFMAs (0 * NaN would poison valid rows)
        ws.zero_()
        torch.cuda.synchronize(self.device)
        check(self._fn("set_workspace")(self.h, _ptr(ws), nbytes))
        self.workspace, self.ws = workspace, ws
        self._rebound()               # the engine forgot them with everything else that belonged to the old binding

    def _grow(self, need):
        """rebind when the workspace is smaller than `need` (reserve, set_geometry)"""
        if need > self.ws.numel():
            self._bind(need)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize(self.device)
                self._release()
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    def set_weight(self, name, tensor):
        t = tensor.detach()
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        t = t.to(self.device).contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        dt = MC_F32 if t.dtype == torch.float32 else MC_BF16
        st = self._fn("set_weight")(self.h, name.encode(), _ptr(t), dt, shape, t.dim(), _stream())
        if st != 0 and dt == MC_BF16 and b"must be given as fp32" in self.lib.mc_last_error():
            # fp32 slots (biases, norm weights, modulation, time MLP, head): a state_dict converted with
            # .to(bfloat16) (upstream convert_model_dtype) still loads, widened exactly
            t = t.float()
            st = self._fn("set_weight")(self.h, name.encode(), _ptr(t), MC_F32, shape, t.dim(), _stream())
        check(st)
        torch.cuda.current_stream().synchronize()  # t may be freed by the caller right after

    def load_weights(self, named_tensors):
        items = named_tensors.items() if hasattr(named_tensors, "items") else named_tensors
        for name, t in items:
            self.set_weight(name, t)
        buf = C.create_string_buffer(4096)
        n = self._fn("weights_missing")(self.h, buf, 4096)
        if n:
            raise KeyError(f"{n} weights missing, e.g.: {buf.value.decode().split()[:5]}")

    def buffer(self, name, dtype=torch.uint8):
        off, nb = C.c_size_t(), C.c_size_t()
        check(self._fn("buffer_info")(self.h, name.encode(), C.byref(off), C.byref(nb)))
        return self.ws[off.value:off.value + nb.value].view(dtype)


class LoraModel:
    """the adapter calls of the model's engine on the model object; _lora_call is where a model does more than delegate"""

    def _lora_call(self, name, *args, **kw):
        return getattr(self.engine, name)(*args, **kw)

    def load_lora(self, sd, adapter="default", scale=1.0, strict=True):
        """Load an adapter state dict (the spellings the engine's _lora_entries reads) as `adapter` at `scale` and merge it;
        returns the names skipped under strict=False."""
        return self._lora_call("load_lora", sd, adapter=adapter, scale=scale, strict=strict)

    def set_adapters(self, names, scales=None):
        return self._lora_call("set_adapters", names, scales)

    def unload_lora(self, adapter=None):
        return self._lora_call("unload_lora", adapter)

    def apply_lora(self):
        return self._lora_call("apply_lora")

    def lora_info(self):
        return self.engine.lora_info()

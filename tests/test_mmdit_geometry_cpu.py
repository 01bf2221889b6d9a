"""CPU: the per-call geometry entry points of the MM-DiT engine are declared, exported and bound with matching signatures, and
the shims keep their fixed geometry unless asked (no GPU, no compute calls)."""
import ctypes as C
import inspect
import os
import re

from magcache_amd import _lib
from magcache_amd import mmdit as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int": C.c_int, "size_t*": C.POINTER(C.c_size_t), "mc_mmdit*": C.c_void_p, "const mc_mmdit*": C.c_void_p}


def test_geometry_symbols_in_header_exports_and_ctypes():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("mc_mmdit_set_geometry", "mc_mmdit_geometry_bytes"):
        m = re.search(r"mc_status\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in magcache_mmdit.h"
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter name
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C_TYPES[t] for t in types], (name, types)
    assert [re.sub(r"\s+", " ", p).strip().split()[-1] for p in
            re.search(r"mc_mmdit_set_geometry\s*\(([^)]*)\)", hdr).group(1).split(",")] == \
        ["e", "img_tokens", "latent_f", "latent_h", "latent_w", "txt_len"]


def test_dynamic_geometry_is_opt_in_on_every_shim():
    for cls in (MM.FluxTransformer2DModelHIP, MM.HYVideoDiffusionTransformerHIP, MM.QwenImageTransformer2DModelHIP):
        assert inspect.signature(cls.__init__).parameters["dynamic_geometry"].default is False
    for name in ("set_geometry", "reserve", "geometry_bytes"):
        assert callable(getattr(MM.MMDiTEngine, name))
    p = inspect.signature(MM.MMDiTEngine.set_geometry).parameters
    assert list(p) == ["self", "img_tokens", "latent_grid", "txt_len"]
    assert p["latent_grid"].default == (0, 0, 0) and p["txt_len"].default is None

"""CPU: the per-call latent grid of the Wan engine -- its entry points are declared, exported and bound with matching
signatures, the shim keeps its fixed grid unless asked, and the per-axis RoPE values expand to the host table bit for bit
(both are host calls: no GPU, no compute calls)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from magcache_amd import _lib
from magcache_amd import engine as E
from magcache_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int": C.c_int, "size_t*": C.POINTER(C.c_size_t), "mc_engine*": C.c_void_p, "const mc_engine*": C.c_void_p,
           "float*": C.c_void_p, "const float*": C.c_void_p, "mc_stream": C.c_void_p}
N_T, N_HW = 22, 21      # complex pairs of head_dim 128 that turn with the frame / the height / the width index


def test_geometry_symbols_in_header_exports_and_ctypes():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magcache_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    names = {}
    for name in ("mc_geometry_bytes", "mc_set_geometry", "mc_op_rope_axes", "mc_op_rope_expand"):
        m = re.search(r"mc_status\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in magcache_hip.h"
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]      # drop the parameter name
        names[name] = [p.split()[-1].lstrip("*") for p in params]
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C_TYPES[t] for t in types], (name, types)
    assert names["mc_set_geometry"] == ["e", "latent_f", "latent_h", "latent_w"]
    assert names["mc_geometry_bytes"] == ["e", "latent_f", "latent_h", "latent_w", "bytes"]
    assert names["mc_op_rope_axes"] == ["F", "Hp", "Wp", "axes_host", "n_floats"]
    assert names["mc_op_rope_expand"] == ["axes_dev", "F", "Hp", "Wp", "tok0", "n_tok", "n_rows", "cs_dev", "stream"]
    assert b"0.7" in lib.mc_version()


def test_dynamic_geometry_is_opt_in():
    assert inspect.signature(M.WanModelHIP.__init__).parameters["dynamic_geometry"].default is False
    assert M.WanModelHIP.dynamic_geometry is False
    for name in ("set_geometry", "reserve", "geometry_bytes", "_bind"):
        assert callable(getattr(E.Engine, name))
    assert list(inspect.signature(E.Engine.set_geometry).parameters) == ["self", "latent_grid"]


def rope_axes(F, Hp, Wp):
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.mc_op_rope_axes(F, Hp, Wp, None, C.byref(n)))          # NULL: the count only
    assert n.value == 2 * (F * N_T + Hp * N_HW + Wp * N_HW)
    axes = np.full(n.value, np.nan, dtype=np.float32)
    n2 = C.c_size_t()
    _lib.check(lib.mc_op_rope_axes(F, Hp, Wp, axes.ctypes.data_as(C.c_void_p), C.byref(n2)))
    assert n2.value == n.value
    return axes


def rope_table(F, Hp, Wp, tok0, n_tok):
    cs = np.full((n_tok, 64, 2), np.nan, dtype=np.float32)
    _lib.check(_lib.load().mc_op_rope_table(F, Hp, Wp, tok0, n_tok, cs.ctypes.data_as(C.c_void_p)))
    return cs


def expand_numpy(axes, F, Hp, Wp, tok0, n_tok, n_rows):
    """what mc_op_rope_expand computes: a copy of the axis pairs per token, the identity elsewhere"""
    af = axes[:2 * F * N_T].reshape(F, N_T, 2)
    ah = axes[2 * F * N_T:2 * (F * N_T + Hp * N_HW)].reshape(Hp, N_HW, 2)
    aw = axes[2 * (F * N_T + Hp * N_HW):].reshape(Wp, N_HW, 2)
    cs = np.empty((n_rows, 64, 2), dtype=np.float32)
    cs[:, :, 0], cs[:, :, 1] = 1.0, 0.0
    tok = tok0 + np.arange(n_tok)
    ok = tok < F * Hp * Wp
    f, h, w = tok[ok] // (Hp * Wp), tok[ok] % (Hp * Wp) // Wp, tok[ok] % Wp
    cs[:n_tok][ok] = np.concatenate([af[f], ah[h], aw[w]], axis=1)
    return cs


@pytest.mark.parametrize("F,Hp,Wp,tok0,n_tok", [(1, 1, 1, 0, 1), (3, 5, 7, 0, 105), (3, 5, 7, 37, 50), (3, 5, 7, 90, 40),
                                                (5, 30, 52, 0, 7800)])
def test_axes_expand_to_the_host_table_bitwise(F, Hp, Wp, tok0, n_tok):
    axes = rope_axes(F, Hp, Wp)
    assert np.isfinite(axes).all()
    got = expand_numpy(axes, F, Hp, Wp, tok0, n_tok, n_tok + 3)
    want = rope_table(F, Hp, Wp, tok0, n_tok)
    assert np.array_equal(got[:n_tok].view(np.int32), want.view(np.int32))
    assert (got[n_tok:, :, 0] == 1).all() and (got[n_tok:, :, 1] == 0).all()


def test_rope_axes_refuses_bad_arguments():
    lib = _lib.load()
    n = C.c_size_t()
    for args in ((0, 1, 1), (1, 0, 1), (1, 1, -2)):
        assert lib.mc_op_rope_axes(*args, None, C.byref(n)) == _lib.MC_EINVAL
    assert lib.mc_op_rope_axes(1, 1, 1, None, None) == _lib.MC_EINVAL

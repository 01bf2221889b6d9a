"""CPU: the predicted tile mask's entry points are declared, exported and bound with matching signatures, and
generate.py --sparse_attention parses topmass:MASS beside decay[:DENSE[:SINK]] (host code only: no GPU, no compute calls)."""
import ctypes as C
import os
import re

import pytest

from magcache_amd import _lib
from magcache_amd.generate import parse_sparse_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "size_t": C.c_size_t, "int*": C.POINTER(C.c_int),
           "float*": C.POINTER(C.c_float), "mc_engine*": C.c_void_p, "const mc_engine*": C.c_void_p, "const void*": C.c_void_p,
           "void*": C.c_void_p, "uint32_t*": C.c_void_p, "mc_stream": C.c_void_p}


@pytest.mark.parametrize("name", ["mc_set_attention_tile_mass", "mc_engine_attention_tile_mass", "mc_read_attention_tile_mask",
                                  "mc_op_attention_tile_predict_scratch", "mc_op_attention_tile_predict"])
def test_symbol_in_header_exports_and_ctypes(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magcache_hip.h")).read(), flags=re.S)
    m = re.search(r"(mc_status|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in magcache_hip.h"
    types = [re.sub(r"\s*\w+$", "", re.sub(r"\s+", " ", p).strip()).replace(" *", "*") for p in m.group(2).split(",")]
    assert hasattr(_lib.load(), name), f"{name} is not exported"
    res, args = _lib.SIGNATURES[name]
    assert res is (C.c_int if m.group(1) == "mc_status" else C.c_size_t) and args == [C_TYPES[t] for t in types], (name, types)


@pytest.mark.parametrize("spec,want", [
    ("topmass:0.9", ("topmass", 0.9)), ("topmass:1", ("topmass", 1.0)), ("decay", ("decay", 1, 1)), ("decay:2:3", ("decay", 2, 3)),
    ("topmass", None), ("topmass:0", None), ("topmass:1.5", None), ("topmass:x", None), ("topmass:0.5:1", None), ("decay:1:2:3", None),
    ("decay:a", None), ("radial", None)])
def test_sparse_attention_parser(spec, want):
    if want is not None:
        assert parse_sparse_attention(spec) == want
        return
    with pytest.raises(ValueError, match="sparse_attention"):
        parse_sparse_attention(spec)

"""No GPU: the C ABI and Python surface of mc_mmdit_config.fp8_linear, and the fake-quant oracle that
tests/test_mmdit_fp8_gpu.py measures the fp8 engines against."""
import ctypes as C
import os
import re

from magcache_amd import _lib

import mmdit_fp8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_create_sized():
    text = open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read()
    assert re.search(r"mc_status\s+mc_mmdit_create_sized\s*\(\s*const\s+mc_mmdit_config\s*\*\s*cfg,\s*size_t\s+cfg_bytes,\s*mc_mmdit\s*\*\*\s*out\s*\)",
                     text)
    struct = text[text.index("typedef struct {"):text.index("} mc_mmdit_config;")]
    fields = re.findall(r"\bint\s+([a-z0-9_, ]+);", struct)
    assert fields[-1].strip() == "fp8_linear"
    assert "mc_mmdit_create_sized" in _lib.SIGNATURES
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mc_mmdit_create_sized") and hasattr(lib, "mc_mmdit_create")


def test_config_struct_grew_by_one_int_at_its_end():
    names = [n for n, _ in _lib.McMmditConfig._fields_]
    assert names[-1] == "fp8_linear" and names[-2] == "sp_size"
    assert C.sizeof(_lib.McMmditConfig) == 18 * 4 + 4
    assert _lib.McMmditConfig.fp8_linear.offset == 18 * 4
    assert _lib.McMmditConfig().fp8_linear == 0


def test_fake_quant_oracle_moves_the_flux_toy_by_a_meaningful_amount():
    """more than the bf16 oracle's 1.2e-2 and at most 7e-2: the 8e-2 bar of the GPU test then leaves room for the engine's
    bf16 rounding and no more"""
    fam, geo = R.Flux, R.FLUX_ODD
    for mode, n_linears in ((2, 28), (3, 34)):
        assert len(R.fake_quant(fam.oracle(), mode)[1]) == n_linears
        plain, fq = R.references(fam, geo, mode)
        err = R.rel_l2(fq, plain)
        print(f"FLUX toy, fake-quant oracle of mode {mode} vs the plain fp32 oracle: {err:.3e}")
        assert 1e-2 < err < 7e-2

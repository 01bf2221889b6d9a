"""No GPU: the C ABI and Python surface of the MM-DiT engine's option "mx_fp4", and the FP4 fake-quant oracle that
tests/test_mmdit_mxfp4_gpu.py measures the MXFP4 engines against."""
import ctypes as C
import inspect
import os
import re

import pytest

from magcache_amd import _lib

import mmdit_fp8_ref as R
import mmdit_mxfp4_ref as R4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"flux_odd": (R.Flux, R.FLUX_ODD), "flux_exact": (R.Flux, R.FLUX_EXACT), "hunyuan": (R.Hunyuan, R.HUNYUAN_GEO),
         "qwen": (R.Qwen, R.QWEN_GEO), "qwen_edit": (R.Qwen, R.QWEN_EDIT_GEO)}


def test_header_declares_library_exports_and_signatures_list_the_query():
    text = open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read()
    assert re.search(r"\bint\s+mc_mmdit_mx_fp4\s*\(\s*const\s+mc_mmdit\s*\*\s*e\s*\)\s*;", text)
    assert _lib.SIGNATURES["mc_mmdit_mx_fp4"] == (C.c_int, [C.c_void_p])
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mc_mmdit_mx_fp4")
    fn = lib.mc_mmdit_mx_fp4
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    assert fn(None) == 0   # no engine, no MXFP4


def test_config_struct_did_not_grow():
    names = [n for n, _ in _lib.McMmditConfig._fields_]
    assert names[-1] == "fp8_linear" and "mx_fp4" not in names
    assert C.sizeof(_lib.McMmditConfig) == 18 * 4 + 4
    text = open(os.path.join(ROOT, "include", "magcache_mmdit.h")).read()
    struct = text[text.index("typedef struct {"):text.index("} mc_mmdit_config;")]
    assert re.findall(r"\bint\s+([a-z0-9_, ]+);", struct)[-1].strip() == "fp8_linear"


def test_the_option_message_names_no_engine_and_the_epilogue_enumerator_is_appended():
    lib = _lib.load()
    assert lib.mc_set_option(b"mx_fp4", 2) == _lib.MC_EINVAL
    msg = lib.mc_last_error().decode()
    assert "mx_fp4" in msg and "Wan engine" not in msg
    ops = open(os.path.join(ROOT, "magcache_amd", "csrc", "ops.h")).read()
    enum = ops[ops.index("enum GemmEpi {"):ops.index("struct GemmParams")]
    vals = {k: int(v) for k, v in re.findall(r"\b(EPI_[A-Z0-9_]+)\s*=\s*(\d+)", enum)}
    assert vals["EPI_GELU_MXFP4"] == max(vals.values()) and vals["EPI_GELU_MXFP8"] == 8 and vals["EPI_GELU_BF16"] == 1
    assert len(set(vals.values())) == len(vals)
    assert re.findall(r"\b(EPI_[A-Z0-9_]+)\s*=", enum)[-1] == "EPI_GELU_MXFP4"


def test_python_surface_takes_the_keyword_and_shares_one_latch():
    from magcache_amd import adapters, engine, mmdit
    for cls in (mmdit.MMDiTEngine, mmdit.FluxTransformer2DModelHIP, mmdit.HYVideoDiffusionTransformerHIP,
                mmdit.QwenImageTransformer2DModelHIP, engine.Engine):
        assert inspect.signature(cls.__init__).parameters["mx_fp4"].default is False, cls
    # the set / create / put back sequence exists once, in the base both engine classes derive from
    assert issubclass(mmdit.MMDiTEngine, adapters.EngineHost) and issubclass(engine.Engine, adapters.EngineHost)
    # (over the tuple of element-format options, which names this one)
    for mod in (engine, mmdit):
        assert "mc_set_option(" not in inspect.getsource(mod)
    assert "mx_fp4" in adapters.MX_FORMAT_OPTIONS
    latch = inspect.getsource(adapters.EngineHost._create_latching)
    assert latch.count("mc_set_option(") == 2 and latch.count("in MX_FORMAT_OPTIONS") == 4   # get, set, put back, query
    assert inspect.getsource(adapters.EngineHost).count("mc_set_option(") == 2


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_fp4_fake_quant_oracle_is_at_the_expected_distance(case, mode):
    fam, geo = CASES[case]
    assert R4.picked_names(fam.oracle(), mode) == R.fake_quant(fam.oracle(), mode)[1]
    for b in fam.branches:
        plain, fq = R4.references(fam, geo, mode, b)
        q = R.rel_l2(fq, plain)
        print(f"{case} branch {b} mode {mode}: FP4 fake-quant oracle vs the plain fp32 oracle {q:.3e}")
        assert R4.Q_BAND[0] <= q <= R4.Q_BAND[1]

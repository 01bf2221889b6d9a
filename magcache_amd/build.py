"""Build libmagcache_hip.so (HIP kernels + C-ABI engine) for gfx950 with hipcc, in-tree.

`python -m magcache_amd.build` or `magcache_amd.build.build()`.  The .so lands next to this file so
that it travels with the repo snapshot to the GPU box; nothing is JIT-compiled at import time.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmagcache_hip.so")
SOURCES = ["gemm_bf16.hip", "gemm_bf16_v2.hip", "gemm_fp8_big.hip", "gemm_mxfp8.hip", "gemm_mxfp4.hip", "gemm_mxfp6.hip", "attention_v3.hip", "attention_v5.hip", "ip_attention.hip", "elementwise.hip",
           "magcache_ops.hip", "lora_merge.hip", "adapter_merge.hip", "host.cpp", "engine.cpp", "mmdit_engine.cpp", "ops_capi.cpp", "rule.cpp", "sp_rccl.cpp"]
# the attention kernel's hand-interleaved VALU stream must stay scalar: the SLP vectoriser packs the row-sum
# adds into v_pk_add_f32 and moves them out of the MFMA shadow
EXTRA_FLAGS = {"attention_v3.hip": ["-fno-slp-vectorize"]}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
OBJDIR = os.path.join(CSRC, "build")


# The test-only reference build: the same objects + gemm_bf16_big.hip (rounds 1-3's 8-wave 256 x 256 GEMM), with the
# dispatcher compiled with MC_WITH_REF_GEMM so that gemm_kernel = 2 selects it (mc_set_option asks the dispatcher,
# mc::gemm_bf16_big_linked(), whether it may).  It is the independent implementation the parity tests compare gemm_bf16_v2
# with bit for bit (tests/hip_ops.py: ref_lib()); the product never loads it.  Lives under tests/ and travels to the GPU box
# like the shipped library.
# test_ops.cpp adds the mc_test_* entry points (thin wrappers around the launchers of ops.h that the shipped C ABI has no
# single-op call for: tests/test_tokenwise_ops_gpu.py).  Only REF_RECOMPILED is compiled a second time: every other object --
# the engines, elementwise.hip.o and gemm_mxfp8.hip.o among them -- is the very file the shipped library links, so a test that
# calls a launcher through the reference library runs the shipped machine code.
REF_LIB = os.path.join(HERE, "..", "tests", "_ref", "libmagcache_hip_ref.so")
REF_RECOMPILED = ["gemm_bf16.hip"]     # the one translation unit that tests MC_WITH_REF_GEMM
REF_EXTRA = ["gemm_bf16_big.hip", "test_ops.cpp"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _headers():
    hs = [os.path.join(CSRC, h) for h in ("common.h", "ops.h", "host.h", "gemm_epilogue.h", "attention_v5_body.inc",
                                          "attention_v5_clobbers.inc", "attention_v5_config.h", "gemm_v2_body.inc",
                                          "gemm_v2_clobbers.inc", "gemm_v2_config.h", "quant.h", "gemm_pipe8.h")]
    return hs + [os.path.join(HERE, "..", "include", "magcache_hip.h"), os.path.join(HERE, "..", "include", "magcache_mmdit.h")]


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _compile(src, obj, extra_flags, force, verbose):
    """csrc/<src> -> obj, if obj is older than the source or a header"""
    sp = os.path.join(CSRC, src)
    if force or _stale(obj, [sp] + _headers()):
        _run([HIPCC] + FLAGS + extra_flags + EXTRA_FLAGS.get(src, []) + (["-x", "hip"] if src.endswith(".cpp") else []) +
             ["-c", sp, "-o", obj], verbose)


def _link(target, objs, force, verbose):
    """objs -> target, linked under a temporary name and renamed into place: the linker removes its output file before it
    writes it, and a process that looks for the library meanwhile (a test run beside a build) must not find it missing"""
    if force or _stale(target, objs):
        tmp = target + ".linking"
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs + ["-ldl"], verbose)
        os.replace(tmp, target)


def build(force=False, verbose=False):
    os.makedirs(OBJDIR, exist_ok=True)
    objs = [os.path.join(OBJDIR, src + ".o") for src in SOURCES]
    for src, obj in zip(SOURCES, objs):
        _compile(src, obj, [], force, verbose)
    _link(LIB, objs, force, verbose)
    return LIB


def build_ref(force=False, verbose=False):
    """tests/_ref/libmagcache_hip_ref.so (see REF_LIB above); builds the shipped library first and reuses its objects"""
    build(force=force, verbose=verbose)
    os.makedirs(os.path.dirname(REF_LIB), exist_ok=True)
    objs = []
    for src in SOURCES + REF_EXTRA:
        special = src in REF_RECOMPILED or src in REF_EXTRA
        objs.append(os.path.join(OBJDIR, ("ref_" if special else "") + src + ".o"))
        if special:
            _compile(src, objs[-1], ["-DMC_WITH_REF_GEMM"], force, verbose)
    _link(REF_LIB, objs, force, verbose)
    return os.path.abspath(REF_LIB)


if __name__ == "__main__":
    # both libraries, always: a reference build older than the shipped one lacks its newest symbols and every test that
    # binds it fails (tests/test_host_logic.py::test_reference_library_is_current catches that on CPU)
    print(build_ref(force="--force" in sys.argv, verbose=True))
    print(LIB)

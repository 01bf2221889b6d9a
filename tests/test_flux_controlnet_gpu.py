"""ControlNet residuals in the FLUX forward of the MM-DiT engine (mc_mmdit_set_controlnet, mc_op_add_rows): the add kernel
alone, the MagCache loop and the calibration through the shims against the golden produced by the reference's own
magcache_forward / magcache_calibration with samples (tools/gen_golden_flux_controlnet.py), the residual capture when a
sample lands on the last block, neutrality, the phase path and two sequence-parallel ranks, error behaviour.  The toy FLUX
geometry, weights and inputs are those of tests/test_mmdit_gpu.py's `flux` fixture."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402

from hip_ops import P, S  # noqa: E402

DEV = "cuda:0"
# the bars of tests/test_mmdit_gpu.py: test_flux_magcache_loop_vs_reference_golden (per-call relative L2),
# test_flux_calibration_vs_reference_golden (norm_ratio, norm_std, cos_dis) and the sequence-parallel test
LOOP_BAR, CALIB_BARS, SP_BAR = 3e-2, (1e-3, 5e-4, 4e-4), 4e-3


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


def dev(t):
    return t.to(DEV)


def hip_model(cfg, meta, oracle, name, **kw):
    cls = type(name, (MM.FluxTransformer2DModelHIP,), {})
    m = cls(cfg, meta["h2"] * meta["w2"], txt_len=meta["txt_len"], device=DEV, **kw)
    m.load_state_dict(oracle.state_dict())
    return m


@pytest.fixture(scope="module")
def flux(golden_dir):
    g = np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))
    cn = np.load(os.path.join(golden_dir, "flux_controlnet_golden.npz"))
    meta, cmeta = json.loads(str(g["meta"])), json.loads(str(cn["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    oracle = FR.init_synthetic_(FR.FluxTransformer2DModel(**cfg), seed=meta["weight_seed"], std=meta["weight_std"])
    m = hip_model(cfg, meta, oracle, "FluxHIPControlNet", calibration=True)
    kw = {k: dev(v) for k, v in dict(
        encoder_hidden_states=torch.from_numpy(g["ctx"]), pooled_projections=torch.from_numpy(g["pooled"]),
        img_ids=torch.from_numpy(g["img_ids"]), txt_ids=torch.from_numpy(g["txt_ids"]),
        guidance=torch.tensor([meta["guidance"]])).items()}
    scale = cmeta["sample_scale"]
    double = [dev(torch.from_numpy(q).float() * scale)[None] for q in cn["double_q"]]     # [1, img_tokens, dim] fp32
    single = [dev(torch.from_numpy(q).float() * scale)[None] for q in cn["single_q"]]
    return dict(g=g, cn=cn, meta=meta, cmeta=cmeta, cfg=cfg, oracle=oracle, m=m, kw=kw, double=double, single=single,
                x=dev(torch.from_numpy(g["latent0"]).clone()), t=torch.tensor([0.5], device=DEV))


def plain(f, m=None, **cn):
    m = m or f["m"]
    return m(hidden_states=f["x"], timestep=f["t"], return_dict=False, **f["kw"], **cn)[0].clone()


# ----------------------------------------------------------------------------- 1. the kernel alone
def add_rows(x, s, r, x0, rows, dim):
    lib = _lib.load()
    return lib.mc_op_add_rows(P(x), x.stride(0), P(s), _lib.MC_BF16 if s.dtype == torch.bfloat16 else _lib.MC_F32,
                              P(r), r.stride(0) if r is not None else 0, P(x0), x0.stride(0) if x0 is not None else 0,
                              rows, dim, S())


@pytest.mark.parametrize("second", ["none", "add", "capture"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dim", [512, 3072])
@pytest.mark.parametrize("rows", [1, 255, 257])
def test_add_rows_is_bitwise_x_plus_sample(rows, dim, dtype, second):
    """x[r, :] += s[r, :] is ONE fp32 add of an exactly widened sample: bitwise torch's x + s.float().  The row range sits
    inside a poisoned buffer with a leading dimension larger than dim: rows outside it and the columns past dim keep their
    bits.  Second destination: R += s, or (x0 given) R = x_new - x0 -- the residual capture after the add."""
    g = torch.Generator(device=DEV).manual_seed(rows * 7 + dim)
    ld = dim + 8
    buf = torch.randn(rows + 2, ld, generator=g, device=DEV)
    rbuf = torch.randn(rows + 2, ld + 4, generator=g, device=DEV)
    s = torch.randn(rows, dim, generator=g, device=DEV).to(dtype)
    x0 = torch.randn(rows, dim, generator=g, device=DEV).bfloat16()
    want, rwant = buf.clone(), rbuf.clone()
    want[1:1 + rows, :dim] += s.float()
    if second == "add":
        rwant[1:1 + rows, :dim] += s.float()
    elif second == "capture":
        rwant[1:1 + rows, :dim] = want[1:1 + rows, :dim] - x0.float()
    st = add_rows(buf[1:], s, rbuf[1:] if second != "none" else None, x0 if second == "capture" else None, rows, dim)
    assert st == _lib.MC_OK, _lib.load().mc_last_error()
    assert torch.equal(buf, want)
    assert torch.equal(rbuf, rwant)


def test_add_rows_refuses_misaligned_pointers_and_ragged_widths():
    lib = _lib.load()
    x = torch.zeros(4, 64, device=DEV)
    s = torch.zeros(4, 64, device=DEV)
    sb = torch.zeros(4, 72, device=DEV, dtype=torch.bfloat16)
    assert add_rows(x, s, None, None, 4, 64) == _lib.MC_OK
    assert add_rows(x.view(-1)[1:65].view(1, 64), s, None, None, 1, 64) == _lib.MC_EINVAL       # x + 4 bytes
    assert add_rows(x, s.view(-1)[1:65].view(1, 64), None, None, 1, 64) == _lib.MC_EINVAL       # sample + 4 bytes
    assert add_rows(x, sb.view(-1)[4:68].view(1, 64), None, None, 1, 64) == _lib.MC_EINVAL      # bf16 sample + 8 bytes
    assert add_rows(x, s, x.view(-1)[2:66].view(1, 64), None, 1, 64) == _lib.MC_EINVAL          # R + 8 bytes
    assert add_rows(x, s, None, None, 4, 12) == _lib.MC_EINVAL                                  # dim = 12
    assert b"add_rows" in lib.mc_last_error()
    torch.cuda.synchronize()
    assert not bool(x.any())                                                                    # nothing ran


# ----------------------------------------------------------------------------- 2. / 3. the loops against the golden
def record_modes(cls):
    modes, base = [], cls.__mro__[1]._run

    def _run(self, *a):
        modes.append(a[-1])
        return base(self, *a)
    cls._run = _run
    return modes


def case_samples(f, name, dtype):
    c = f["cmeta"]["cases"][name]
    return dict(controlnet_block_samples=[t.to(dtype) for t in f["double"][:c["n_double_samples"]]],
                controlnet_single_block_samples=[t.to(dtype) for t in f["single"][:c["n_single_samples"]]],
                controlnet_blocks_repeat=c["blocks_repeat"])


@pytest.mark.parametrize("name,dtype", [("each", torch.float32), ("repeat", torch.bfloat16)])
def test_flux_magcache_loop_with_controlnet_vs_reference_golden(flux, name, dtype):
    """flux_magcache_forward with samples vs the reference's own magcache_forward with the same samples: the skip schedule
    of the golden, every call under the bar of test_flux_magcache_loop_vs_reference_golden.  `each`: a sample per block
    (the last block too); `repeat`: controlnet_blocks_repeat with n - 1 samples (2 for the 3 single blocks).  The samples
    are multiples of 1/64: the bf16 and the fp32 form are the same numbers."""
    f = flux
    m, g, cn, meta = f["m"], f["g"], f["cn"], f["meta"]
    steps = meta["steps"]
    MM.init_flux_magcache(m, steps, meta["thresh"], meta["K"], meta["R"])
    cls = type(m)
    kwc = case_samples(f, name, dtype)
    x, sig = f["x"].clone(), g["sigmas"]
    modes, errs = record_modes(cls), []
    try:
        for i in range(steps):
            o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), return_dict=False, **f["kw"], **kwc)[0]
            errs.append(rel_l2(o[0], cn[name + "_outs"][i].astype(np.float32)))
            x = x + float(sig[i + 1] - sig[i]) * o
        print(name, "per-call relative L2 vs the golden:", ["%.2e" % e for e in errs])
        assert cls.cnt == 0 and cls.accumulated_steps == 0
        assert [int(mo == MM.MC_MODE_SKIP) for mo in modes] == cn[name + "_skipped"].tolist() == g["skipped"].tolist()
        assert max(errs) < LOOP_BAR, errs
    finally:
        del cls._run
        if "previous_residual" in m.__dict__:
            del m.previous_residual
        cls.forward = MM.flux_plain_forward
        m.engine.set_controlnet()


def test_flux_calibration_with_controlnet_vs_reference_golden(flux):
    f = flux
    m, g, meta, want = f["m"], f["g"], f["meta"], f["cmeta"]["calib"]
    steps = meta["steps"]
    MM.init_flux_magcache(m, steps, calibration=True)
    cls = type(m)
    kwc = case_samples(f, "each", torch.float32)
    x, sig = f["x"].clone(), g["sigmas"]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for i in range(steps - 1):
                o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), return_dict=False, **f["kw"], **kwc)[0]
                x = x + float(sig[i + 1] - sig[i]) * o
        assert len(cls.norm_ratio) == steps - 2
        for k, bar in zip(("norm_ratio", "norm_std", "cos_dis"), CALIB_BARS):
            print(k, "max difference from the golden: %.2e" % float(np.abs(np.array(getattr(cls, k)) - np.array(want[k])).max()))
        for k, bar in zip(("norm_ratio", "norm_std", "cos_dis"), CALIB_BARS):
            np.testing.assert_allclose(getattr(cls, k), want[k], rtol=0, atol=bar)
        # the statistics are those of the run WITH samples: the plain golden's differ by far more than the bar
        assert np.abs(np.array(want["norm_ratio"]) - np.array(meta["calib"]["norm_ratio"])).max() > 10 * CALIB_BARS[0]
    finally:
        if "previous_residual" in m.__dict__:
            del m.previous_residual
        cls.forward = MM.flux_plain_forward
        cls.cnt = 0
        m.engine.set_controlnet()


# ----------------------------------------------------------------------------- 4. the residual capture
def stream_rows(m):
    """(x, x0) image rows of the engine's residual stream after a forward: fp32 and bf16 [img_tokens, dim]"""
    e = m.engine
    r0 = m.txt_len                                         # FLUX row order: [text ; image]
    x = e.buffer("x", torch.float32).view(-1, e.dim)[r0:r0 + e.img_tokens]
    x0 = e.buffer("x0", torch.bfloat16).view(-1, e.dim)[r0:r0 + e.img_tokens]
    return x, x0


def check_capture(f, m, cn):
    e = m.engine
    e.reset()
    a = plain(f, m, **cn)
    x, x0 = stream_rows(m)
    assert torch.equal(e.residual(), x - x0.float()), "cached residual != x_final - x0"
    args = (f["x"][0], 500.0, float(f["meta"]["guidance"]) * 1000, f["kw"]["encoder_hidden_states"][0], m.txt_len,
            f["kw"]["pooled_projections"][0])
    full = e.forward(*args, mode=MM.MC_MODE_FULL).clone()
    assert torch.equal(full, a[0])
    skip = e.forward(*args, mode=MM.MC_MODE_SKIP).clone()
    assert rel_l2(skip, full) < 1e-5                       # ori + cached residual, re-associated in fp32
    # without the sample the residual is another one: the capture really contains it
    r_with = e.residual().clone()
    plain(f, m)
    assert rel_l2(e.residual(), r_with) > 1e-2


def test_residual_capture_includes_a_sample_on_the_last_single_block(flux):
    """The reference takes hidden_states - ori after the last block's ControlNet add.  The engine captures the residual in
    the last block's output GEMM, before an add could run, so with a sample on the last block the add launch captures
    instead: engine.residual() is bitwise x_final - x0, and a skipped forward adds exactly that."""
    f = flux
    assert f["cmeta"]["cases"]["each"]["single_index"][-1] == len(f["single"]) - 1
    try:
        check_capture(f, f["m"], dict(controlnet_single_block_samples=f["single"]))
    finally:
        f["m"].engine.set_controlnet()


def test_residual_capture_includes_a_sample_on_the_last_double_block(flux):
    """the same on a model without single blocks (the capture of the merged double-block MLP-out launch)"""
    f = flux
    cfg = dict(f["cfg"], num_single_layers=0)
    oracle = FR.init_synthetic_(FR.FluxTransformer2DModel(**cfg), seed=11, std=f["meta"]["weight_std"])
    m = hip_model(cfg, f["meta"], oracle, "FluxHIPDoubleOnly", calibration=False)
    check_capture(f, m, dict(controlnet_block_samples=[t.bfloat16() for t in f["double"]]))
    with pytest.raises(_lib.MagCacheHipError):             # no single blocks: a single sample has no block
        m.engine.set_controlnet(None, f["single"][:1])


# ----------------------------------------------------------------------------- 5. / 6. neutrality, effect
def test_zero_samples_and_cleared_samples_change_no_bit(flux):
    f = flux
    m = f["m"]
    ref = plain(f)
    r_ref = m.engine.residual().clone()
    zeros = dict(controlnet_block_samples=[torch.zeros_like(t) for t in f["double"]],
                 controlnet_single_block_samples=[torch.zeros_like(t) for t in f["single"]])
    assert torch.equal(plain(f, **zeros), ref)
    assert torch.equal(m.engine.residual(), r_ref)
    moved = plain(f, controlnet_block_samples=f["double"], controlnet_single_block_samples=f["single"])
    assert not torch.equal(moved, ref)
    assert torch.equal(plain(f), ref)                      # set, then cleared by the next call without samples
    m.engine.set_controlnet(f["double"], f["single"])
    m.engine.set_controlnet()
    assert torch.equal(plain(f), ref)


def test_samples_move_the_output(flux):
    """double samples and single samples each change the output by more than the loop's tolerance (on a build without the
    feature the arguments were refused or dropped).  With one sample per double block the repeat flag selects the same
    samples and changes nothing; test_blocks_repeat_selects_other_samples_than_the_plain_rule is where it matters."""
    f = flux
    ref = plain(f)
    d = plain(f, controlnet_block_samples=f["double"])
    s = plain(f, controlnet_single_block_samples=f["single"][:2])
    both = plain(f, controlnet_block_samples=f["double"], controlnet_single_block_samples=f["single"])
    for o in (d, s, both):
        assert rel_l2(o, ref) > LOOP_BAR
    assert rel_l2(both, d) > LOOP_BAR and rel_l2(both, s) > LOOP_BAR
    # [a, b] on two double blocks: repeat keeps i % 2 = (0, 1) = i // 1, one sample per block either way ...
    assert torch.equal(plain(f, controlnet_block_samples=f["double"], controlnet_blocks_repeat=True), d)
    # ... and [img_tokens, dim] is accepted like [1, img_tokens, dim], bf16 like fp32 (the samples are bf16 numbers)
    assert torch.equal(plain(f, controlnet_block_samples=[t[0].bfloat16() for t in f["double"]]), d)
    f["m"].engine.set_controlnet()


def test_blocks_repeat_selects_other_samples_than_the_plain_rule(flux):
    """controlnet_blocks_repeat with a sample count that does not divide the number of double blocks: four double blocks
    and samples [a, b, c].  Repeat reads a, b, c, a (i % 3), the plain rule a, a, b, b (i // ceil(4 / 3)).  The forward
    with repeat is bitwise the plain-rule forward with [a, b, c, a], under the loop's bar from the reference's own
    forward with the same arguments (golden `repeat4`), and further than the bar from the plain-rule forward with
    [a, b, c] -- which the reference's two outputs are apart by 0.24."""
    f = flux
    r4 = f["cmeta"]["repeat4"]
    cfg = dict(f["cfg"], num_layers=r4["num_layers"])
    oracle = FR.init_synthetic_(FR.FluxTransformer2DModel(**cfg), seed=r4["weight_seed"], std=f["meta"]["weight_std"])
    m = hip_model(cfg, f["meta"], oracle, "FluxHIPFourDouble", calibration=False)
    a, b, c = f["double"][0], f["double"][1], f["single"][0]
    assert r4["n_double_samples"] == 3 and r4["timestep"] == 0.5
    rep = plain(f, m, controlnet_block_samples=[a, b, c], controlnet_blocks_repeat=True)
    assert torch.equal(rep, plain(f, m, controlnet_block_samples=[a, b, c, a]))
    assert torch.equal(rep, plain(f, m, controlnet_block_samples=[a, b, c, a], controlnet_blocks_repeat=True))
    err = rel_l2(rep[0], f["cn"]["repeat4_out"].astype(np.float32))
    print("repeat4 relative L2 vs the golden: %.2e" % err)
    assert err < LOOP_BAR
    no_rep = plain(f, m, controlnet_block_samples=[a, b, c])
    assert rel_l2(no_rep, rep) > LOOP_BAR
    assert torch.equal(no_rep, plain(f, m, controlnet_block_samples=[a, a, b, b]))
    # the flag is a rule of the double blocks only: single samples keep i // ceil(3 / 2) = 0, 0, 1 with it
    s2 = f["single"][:2]
    assert torch.equal(plain(f, m, controlnet_single_block_samples=s2, controlnet_blocks_repeat=True),
                       plain(f, m, controlnet_single_block_samples=[s2[0], s2[0], s2[1]]))


# ----------------------------------------------------------------------------- 7. phase path, shards
def engine_args(f):
    return (f["x"][0], 500.0, float(f["meta"]["guidance"]) * 1000, f["kw"]["encoder_hidden_states"][0], f["meta"]["txt_len"],
            f["kw"]["pooled_projections"][0])


def test_phase_path_with_samples_equals_the_forward(flux):
    f = flux
    m, e = f["m"], f["m"].engine
    ref = plain(f, controlnet_block_samples=f["double"], controlnet_single_block_samples=f["single"])[0]
    try:
        e.set_controlnet(f["double"], f["single"])
        e.begin(*engine_args(f), MM.MC_MODE_FULL)
        with pytest.raises(_lib.MagCacheHipError):         # the lists are fixed for the forward in progress
            e.set_controlnet()
        for blk in range(e.n_blocks):
            e.block_pre(blk)
            e.block_post(blk)
        out = torch.empty_like(ref)
        e.end(out)
        assert torch.equal(out, ref)
        x, x0 = stream_rows(m)
        assert torch.equal(e.residual(), x - x0.float())
    finally:
        e.set_controlnet()


def test_two_sequence_parallel_ranks_read_their_rows_of_the_samples(flux):
    """two ranks of a sequence-parallel engine in one process (copies between the two "kv_gather" buffers play the
    all-gather): every rank adds rows [rank, rank + 1) * img_tokens / 2 of the FULL samples; its output rows equal the
    one-rank result under the bar of test_mmdit_sequence_parallel_ranks_on_one_gpu."""
    f = flux
    cn = (f["double"], f["single"])
    ref = plain(f, controlnet_block_samples=cn[0], controlnet_single_block_samples=cn[1])[0]
    f["m"].engine.set_controlnet()
    no_cn = plain(f)[0]
    ids = torch.cat((f["kw"]["txt_ids"], f["kw"]["img_ids"]), dim=0).float()
    ranks = []
    for r in range(2):
        m = hip_model(f["cfg"], f["meta"], f["oracle"], "FluxHIPSP%d" % r, calibration=False, sp_rank=r, sp_size=2)
        m.engine.set_rope(*MM.flux_rope(ids, tuple(f["cfg"]["axes_dims_rope"])))
        m.engine.set_controlnet(*cn)
        ranks.append(m.engine)
    kv = [e.buffer("kv_gather", torch.bfloat16).view(2, -1) for e in ranks]
    for e in ranks:
        e.begin(*engine_args(f), MM.MC_MODE_FULL)
    for blk in range(ranks[0].n_blocks):
        for e in ranks:
            e.block_pre(blk)
        kv[0][1].copy_(kv[1][1])
        kv[1][0].copy_(kv[0][0])
        for e in ranks:
            e.block_post(blk)
    n = ranks[0].tokens_per_rank
    for r, e in enumerate(ranks):
        out = torch.empty(n, ref.shape[1], dtype=torch.float32, device=DEV)
        e.end(out)
        err = rel_l2(out, ref[r * n:(r + 1) * n])
        print("rank", r, "relative L2 vs one rank: %.2e" % err)
        assert err < SP_BAR
        assert rel_l2(out, no_cn[r * n:(r + 1) * n]) > LOOP_BAR


# ----------------------------------------------------------------------------- 8. errors
def test_controlnet_errors(flux):
    f = flux
    m, e = f["m"], f["m"].engine
    ref = plain(f)
    # another family refuses the call
    hy = MM.MMDiTEngine(_lib.MC_FAMILY_HUNYUAN, 256, 2, 1, 1, 16, 16, 256, 32, 128, 96, latent_grid=(2, 12, 16),
                        refiner_depth=2, device=DEV)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        hy.set_controlnet([torch.zeros(96, 256, device=DEV)])
    assert ex.value.status == _lib.MC_EINVAL and "FLUX" in str(ex.value)
    # more samples than blocks: refused when they are set
    with pytest.raises(_lib.MagCacheHipError) as ex:
        e.set_controlnet(f["double"] + f["double"][:1])
    assert ex.value.status == _lib.MC_EINVAL
    with pytest.raises(_lib.MagCacheHipError):
        e.set_controlnet(None, f["single"] + f["single"][:1])
    # wrong shape, mixed dtypes, an unsupported dtype: raised in Python, through the shim's arguments too
    with pytest.raises(ValueError):
        e.set_controlnet([f["double"][0][:, :50]])
    with pytest.raises(ValueError):
        e.set_controlnet([f["double"][0].transpose(1, 2)])
    with pytest.raises(ValueError):
        plain(f, controlnet_block_samples=[f["double"][0], f["double"][1].bfloat16()])
    with pytest.raises(ValueError):
        plain(f, controlnet_block_samples=f["double"][:1], controlnet_single_block_samples=[f["single"][0].bfloat16()])
    with pytest.raises(ValueError):
        e.set_controlnet([f["double"][0].half()])
    # a misaligned sample pointer is refused by the engine, not faulted on
    lib = _lib.load()
    t = torch.zeros(e.img_tokens * e.dim + 4, device=DEV)
    arr = (C.c_void_p * 1)(t.data_ptr() + 4)
    assert lib.mc_mmdit_set_controlnet(e.h, arr, 1, None, 0, _lib.MC_F32, 0) == _lib.MC_EINVAL
    assert lib.mc_mmdit_set_controlnet(e.h, arr, 1, None, 0, 7, 0) == _lib.MC_EINVAL
    # none of the refused calls left anything set
    assert torch.equal(plain(f), ref)

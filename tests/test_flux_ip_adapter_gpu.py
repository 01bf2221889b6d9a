"""FLUX IP-Adapters on the MM-DiT engine (mc_mmdit_ip_adapter_*, mc_op_ip_attention; the kernel alone:
tests/test_ip_attention_gpu.py): the MagCache loop and the calibration through the shims against the golden produced by the
reference's own magcache_forward / magcache_calibration with joint_attention_kwargs["ip_adapter_image_embeds"]
(tools/gen_golden_flux_ip_adapter.py), neutrality, the K|V cache of the two image slots, scales, the residual capture on a
model without single blocks, ControlNet samples on top, the phase path, two sequence-parallel ranks, a geometry switch, MX fp8
Linears and the errors.  Toy FLUX geometry, weights and inputs: tests/test_flux_controlnet_gpu.py's, whose bars apply."""
import contextlib
import copy
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

import flux_ip_adapter_ref as IR  # noqa: E402
from test_flux_controlnet_gpu import CALIB_BARS, LOOP_BAR, SP_BAR, rel_l2, stream_rows  # noqa: E402

DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


def oracle_with(f, adapters, cfg=None, seed=None):
    """the CPU model with the named adapters ("A", "B" of the golden's meta) loaded"""
    o = FR.init_synthetic_(FR.FluxTransformer2DModel(**(cfg or f["cfg"])), seed=f["meta"]["weight_seed"] if seed is None else seed,
                           std=f["meta"]["weight_std"])
    ad = f["imeta"]["adapters"]
    return IR.add_ip_adapters_(o, [tuple(ad[k]["spec"]) for k in adapters], [ad[k]["seed"] for k in adapters], f["imeta"]["ip_std"])


def hip_model(f, name, adapters=("A",), scale=None, cfg=None, seed=None, img_tokens=None, txt_len=None, **kw):
    """a FluxTransformer2DModelHIP of a class of its own with the adapters loaded, one in each spelling load_ip_adapter reads"""
    o = oracle_with(f, adapters, cfg, seed)
    cls = type(name, (MM.FluxTransformer2DModelHIP,), {})
    m = cls(cfg or f["cfg"], img_tokens or f["meta"]["h2"] * f["meta"]["w2"], txt_len=txt_len or f["meta"]["txt_len"], device=DEV, **kw)
    m.load_state_dict(IR.base_state_dict(o))
    for j in range(len(adapters)):
        assert m.load_ip_adapter(IR.adapter_state_dict(o, j) if j % 2 else IR.checkpoint_state_dict(o, j)) == []
    if scale is not None:
        m.set_ip_adapter_scale(scale)
    m.set_image_calls = record_set_image(m)
    return m


def record_set_image(m):
    calls, e = [], m.engine
    inner = e.set_ip_adapter_image

    def set_ip_adapter_image(adapter, slot, embeds):
        calls.append((adapter, slot))
        return inner(adapter, slot, embeds)
    e.set_ip_adapter_image = set_ip_adapter_image
    return calls


@pytest.fixture(scope="module")
def flux(golden_dir):
    g = np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))
    ip = np.load(os.path.join(golden_dir, "flux_ip_adapter_golden.npz"))
    cn = np.load(os.path.join(golden_dir, "flux_controlnet_golden.npz"))
    meta, imeta = json.loads(str(g["meta"])), json.loads(str(ip["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    kw = {k: dev(v) for k, v in dict(
        encoder_hidden_states=torch.from_numpy(g["ctx"]), pooled_projections=torch.from_numpy(g["pooled"]),
        img_ids=torch.from_numpy(g["img_ids"]), txt_ids=torch.from_numpy(g["txt_ids"]),
        guidance=torch.tensor([meta["guidance"]])).items()}
    emb = {k: dev(torch.from_numpy(ip["embeds_%s_q" % k]).float() * imeta["embed_scale"])[None] for k in imeta["adapters"]}
    cscale = json.loads(str(cn["meta"]))["sample_scale"]
    f = dict(g=g, ip=ip, meta=meta, imeta=imeta, cfg=cfg, kw=kw, emb=emb, x=dev(torch.from_numpy(g["latent0"]).clone()),
             t=torch.tensor([0.5], device=DEV),
             double=[dev(torch.from_numpy(q).float() * cscale)[None] for q in cn["double_q"]],
             single=[dev(torch.from_numpy(q).float() * cscale)[None] for q in cn["single_q"]])
    f["one"] = hip_model(f, "FluxHIPIpOne", ("A",), calibration=True)
    f["two"] = hip_model(f, "FluxHIPIpTwo", ("A", "B"), scale=imeta["cases"]["two"]["scale"], calibration=False)
    return f


def jak(f, names=("A",)):
    return dict(ip_adapter_image_embeds=[f["emb"][k] for k in names])


def plain(f, m, joint=None, x=None, t=None, **extra):
    kw = dict(f["kw"], **extra)
    return m(hidden_states=f["x"] if x is None else x, timestep=f["t"] if t is None else t, return_dict=False,
             joint_attention_kwargs=joint, **kw)[0].clone()


def engine_args(f):
    return (f["x"][0], 500.0, float(f["meta"]["guidance"]) * 1000, f["kw"]["encoder_hidden_states"][0], f["meta"]["txt_len"],
            f["kw"]["pooled_projections"][0])


# ----------------------------------------------------------------------------- the loops against the golden
def record_modes(cls):
    modes, base = [], cls.__mro__[1]._run

    def _run(self, *a):
        modes.append(a[-1])
        return base(self, *a)
    cls._run = _run
    return modes


@pytest.mark.parametrize("name", ["one", "two"])
def test_flux_magcache_loop_with_ip_adapter_vs_reference_golden(flux, name):
    """flux_magcache_forward with image embeds vs the reference's own magcache_forward with the same embeds: the golden's skip
    schedule, every call under the bar of the plain loop, cnt wrapped; K|V computed once per adapter for the whole sample."""
    f = flux
    m, g, ip, meta = f[name], f["g"], f["ip"], f["meta"]
    steps = meta["steps"]
    MM.init_flux_magcache(m, steps, meta["thresh"], meta["K"], meta["R"])
    cls = type(m)
    joint = jak(f, f["imeta"]["cases"][name]["adapters"])
    x, sig = f["x"].clone(), g["sigmas"]
    modes, errs = record_modes(cls), []
    del m.set_image_calls[:]
    m._ip_slots().forget()
    try:
        for i in range(steps):
            o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), return_dict=False, joint_attention_kwargs=joint,
                  **f["kw"])[0]
            errs.append(rel_l2(o[0], ip[name + "_outs"][i].astype(np.float32)))
            x = x + float(sig[i + 1] - sig[i]) * o
        print(name, "per-call relative L2 vs the golden:", ["%.2e" % e for e in errs])
        assert cls.cnt == 0 and cls.accumulated_steps == 0
        assert [int(mo == MM.MC_MODE_SKIP) for mo in modes] == ip[name + "_skipped"].tolist()
        assert max(errs) < LOOP_BAR, errs
        assert len(m.set_image_calls) == len(joint["ip_adapter_image_embeds"])
    finally:
        del cls._run
        if "previous_residual" in m.__dict__:
            del m.previous_residual
        cls.forward = MM.flux_plain_forward


def test_flux_calibration_with_ip_adapter_vs_reference_golden(flux):
    f = flux
    m, g, meta, want = f["one"], f["g"], f["meta"], f["imeta"]["calib"]
    steps = meta["steps"]
    MM.init_flux_magcache(m, steps, calibration=True)
    cls = type(m)
    x, sig = f["x"].clone(), g["sigmas"]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for i in range(steps - 1):
                o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), return_dict=False,
                      joint_attention_kwargs=jak(f), **f["kw"])[0]
                x = x + float(sig[i + 1] - sig[i]) * o
        assert len(cls.norm_ratio) == steps - 2
        for k, bar in zip(("norm_ratio", "norm_std", "cos_dis"), CALIB_BARS):
            print(k, "max difference from the golden: %.2e" % float(np.abs(np.array(getattr(cls, k)) - np.array(want[k])).max()))
        for k, bar in zip(("norm_ratio", "norm_std", "cos_dis"), CALIB_BARS):
            np.testing.assert_allclose(getattr(cls, k), want[k], rtol=0, atol=bar)
        # the statistics are those of the run WITH the image prompt: the plain golden's differ by far more than the bar
        assert np.abs(np.array(want["norm_ratio"]) - np.array(meta["calib"]["norm_ratio"])).max() > 10 * CALIB_BARS[0]
    finally:
        if "previous_residual" in m.__dict__:
            del m.previous_residual
        cls.forward = MM.flux_plain_forward
        cls.cnt = 0


# ----------------------------------------------------------------------------- the key no longer vanishes; neutrality
def test_the_key_moves_the_output(flux):
    f = flux
    no_ip = plain(f, f["one"])
    one = plain(f, f["one"], jak(f))
    two = plain(f, f["two"], jak(f, ("A", "B")))
    assert rel_l2(one, no_ip) > LOOP_BAR and rel_l2(two, no_ip) > LOOP_BAR
    assert rel_l2(two, one) > LOOP_BAR
    # [n_images, embed_dim] is accepted like [1, n_images, embed_dim], bf16 like fp32 (the embeds are multiples of 1/16)
    assert torch.equal(plain(f, f["one"], dict(ip_adapter_image_embeds=[f["emb"]["A"][0].bfloat16()])), one)
    # the engine's own weights are those of the model without adapters: without the key the plain golden's first call
    assert rel_l2(plain(f, f["two"], t=torch.tensor([float(f["g"]["sigmas"][0])], device=DEV))[0],
                  f["g"]["outs"][0]) < LOOP_BAR


def test_neutrality_is_bitwise(flux):
    """scale 0 on every adapter, a call without the key after one with it, and unload_ip_adapter: the forward without the key,
    bit for bit, the cached residual included"""
    f = flux
    m = hip_model(f, "FluxHIPIpNeutral", ("A", "B"), calibration=False)
    base = hip_model(f, "FluxHIPIpNone", (), calibration=False)
    ref = plain(f, base)
    r_ref = base.engine.residual().clone()
    both = jak(f, ("A", "B"))
    moved = plain(f, m, both)
    assert rel_l2(moved, ref) > LOOP_BAR
    m.set_ip_adapter_scale(0.0)
    assert torch.equal(plain(f, m, both), ref) and torch.equal(m.engine.residual(), r_ref)
    m.set_ip_adapter_scale([1.0, [0.0, 0.0]])
    assert not torch.equal(plain(f, m, both), ref)
    assert torch.equal(plain(f, m), ref) and torch.equal(m.engine.residual(), r_ref)       # the key is gone again
    assert torch.equal(plain(f, m, {"scale": 1.0}), ref)
    m.set_ip_adapter_scale(1.0)
    assert torch.equal(plain(f, m, both), moved)
    m.unload_ip_adapter()
    assert torch.equal(plain(f, m), ref) and torch.equal(m.engine.residual(), r_ref)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        plain(f, m, both)
    # and an adapter loaded after the unload is adapter 0 again
    o = oracle_with(f, ("A",))
    m.load_ip_adapter(IR.adapter_state_dict(o, 0))
    assert torch.equal(plain(f, m, jak(f)), plain(f, f["one"], jak(f)))


# ----------------------------------------------------------------------------- K|V caching, scales
def test_kv_is_computed_once_per_embeds_tensor(flux):
    f = flux
    m = f["one"]
    a, b = f["emb"]["A"].clone(), (f["emb"]["A"] * 0.5).clone()
    m._ip_slots().forget()
    del m.set_image_calls[:]
    outs = [plain(f, m, dict(ip_adapter_image_embeds=[t])) for t in (a, b, a, b, a, b)]
    assert len(m.set_image_calls) == 2 and {s for _, s in m.set_image_calls} == {0, 1}
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[5]) and not torch.equal(outs[0], outs[1])
    a.mul_(2.0)                                            # an in-place write: that slot is computed once more
    changed = plain(f, m, dict(ip_adapter_image_embeds=[a]))
    assert len(m.set_image_calls) == 3 and not torch.equal(changed, outs[0])
    assert torch.equal(plain(f, m, dict(ip_adapter_image_embeds=[b])), outs[1]) and len(m.set_image_calls) == 3


def test_a_scale_change_costs_no_kv_and_equals_a_fresh_model(flux):
    f = flux
    m = f["two"]
    joint = jak(f, ("A", "B"))
    scales = [[0.25, -0.5], 0.75]
    try:
        plain(f, m, joint)
        n = len(m.set_image_calls)
        m.set_ip_adapter_scale(scales)
        got = plain(f, m, joint)
        assert len(m.set_image_calls) == n
        fresh = hip_model(f, "FluxHIPIpFreshScale", ("A", "B"), scale=scales, calibration=False)
        assert torch.equal(got, plain(f, fresh, joint))
    finally:
        m.set_ip_adapter_scale(f["imeta"]["cases"]["two"]["scale"])


# ----------------------------------------------------------------------------- capture on the last double block, ControlNet
def check_capture(f, m, joint, **cn):
    e = m.engine
    e.reset()
    a = plain(f, m, joint, **cn)
    x, x0 = stream_rows(m)
    assert torch.equal(e.residual(), x - x0.float()), "cached residual != x_final - x0"
    full = e.forward(*engine_args(f), mode=MM.MC_MODE_FULL).clone()
    assert torch.equal(full, a[0])
    skip = e.forward(*engine_args(f), mode=MM.MC_MODE_SKIP).clone()
    assert rel_l2(skip, full) < 1e-5                       # ori + cached residual, re-associated in fp32
    return a


def test_last_double_block_captures_after_the_ip_add(flux):
    """no single blocks: the IP add is the last thing that touches x, so its launch takes the residual (bitwise x - x0), a
    skipped forward reproduces the full one, and the output is the reference's"""
    f = flux
    ld = f["imeta"]["last_double"]
    cfg = dict(f["cfg"], num_single_layers=0)
    m = hip_model(f, "FluxHIPIpDoubleOnly", ("A",), cfg=cfg, seed=ld["weight_seed"], calibration=False)
    a = check_capture(f, m, jak(f))
    err = rel_l2(a[0], f["ip"]["last_double_out"].astype(np.float32))
    print("last_double relative L2 vs the golden: %.2e" % err)
    assert err < LOOP_BAR
    r_ip = m.engine.residual().clone()
    plain(f, m)
    assert rel_l2(m.engine.residual(), r_ip) > 1e-2        # the capture really contains the IP contribution
    # a ControlNet sample on the last double block comes after the IP add and captures instead
    try:
        check_capture(f, m, jak(f), controlnet_block_samples=f["double"])
    finally:
        m.engine.set_controlnet()


def test_ip_adapter_with_controlnet_samples(flux):
    f = flux
    m = f["one"]
    try:
        a = check_capture(f, m, jak(f), controlnet_block_samples=f["double"], controlnet_single_block_samples=f["single"])
        err = rel_l2(a[0], f["ip"]["with_controlnet_out"].astype(np.float32))
        print("with_controlnet relative L2 vs the golden: %.2e" % err)
        assert err < LOOP_BAR
    finally:
        m.engine.set_controlnet()


# ----------------------------------------------------------------------------- phase path, shards
def test_phase_path_equals_the_forward_and_fixes_the_state(flux):
    f = flux
    m, e = f["two"], f["two"].engine
    ref = plain(f, m, jak(f, ("A", "B")))[0]
    e.begin(*engine_args(f), MM.MC_MODE_FULL)
    t = torch.zeros(1, f["imeta"]["embed_dim"], device=DEV)
    for call in (lambda: e.set_ip_adapter_scale(0, 0.5), lambda: e.select_ip_adapter(None), lambda: e.set_ip_adapter_image(0, 0, t),
                 lambda: e.add_ip_adapter(64, 256, 4), lambda: e.clear_ip_adapter()):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            call()
        assert ex.value.status == _lib.MC_ESTATE
    for blk in range(e.n_blocks):
        e.block_pre(blk)
        e.block_post(blk)
    out = torch.empty_like(ref)
    e.end(out)
    assert torch.equal(out, ref)
    assert len(e._ip) == 2


def test_two_sequence_parallel_ranks_attend_their_own_rows(flux):
    """two ranks of a sequence-parallel engine in one process (copies between the two "kv_gather" buffers play the all-gather):
    the image prompt's keys are replicated, every rank attends its own image rows"""
    f = flux
    ref = plain(f, f["one"], jak(f))[0]
    no_ip = plain(f, f["one"])[0]
    ids = torch.cat((f["kw"]["txt_ids"], f["kw"]["img_ids"]), dim=0).float()
    ranks = []
    for r in range(2):
        m = hip_model(f, "FluxHIPIpSP%d" % r, ("A",), calibration=False, sp_rank=r, sp_size=2)
        m.engine.set_rope(*MM.flux_rope(ids, tuple(f["cfg"]["axes_dims_rope"])))
        m.engine.set_ip_adapter_image(0, 1, f["emb"]["A"][0])
        m.engine.select_ip_adapter(1)
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
        assert rel_l2(out, no_ip[r * n:(r + 1) * n]) > LOOP_BAR


# ----------------------------------------------------------------------------- geometry, fp8
def test_a_geometry_switch_keeps_the_image_prompt(flux):
    """dynamic_geometry: the adapters, the slot's K|V, the scales and the selection depend on no token geometry.  After a switch
    from 108 image tokens (3 row tiles of the kernel and 12 rows) to 8 x 20 = 160 with 40 text tokens the forward is bitwise
    that of a model created there with the same image, and nothing is computed again."""
    f = flux
    h2, w2, lt = 8, 20, 40
    g = torch.Generator().manual_seed(4)
    x2 = dev(torch.randn(1, h2 * w2, f["cfg"]["in_channels"], generator=g))
    kw2 = dict(encoder_hidden_states=f["kw"]["encoder_hidden_states"][:, :lt].contiguous(), img_ids=dev(FR.prepare_latent_image_ids(h2, w2)),
               txt_ids=f["kw"]["txt_ids"][:lt].contiguous())
    scales = [[0.5, 1.5]]
    m = hip_model(f, "FluxHIPIpDynamic", ("A",), scale=scales, calibration=False, dynamic_geometry=True)
    joint = jak(f)
    first = plain(f, m, joint)
    assert torch.equal(first, plain(f, hip_model(f, "FluxHIPIpStatic", ("A",), scale=scales, calibration=False), joint))
    assert len(m.set_image_calls) == 1
    got = plain(f, m, joint, x=x2, **kw2)
    assert m.engine.img_tokens == h2 * w2 and len(m.set_image_calls) == 1
    fresh = hip_model(f, "FluxHIPIpAtSecond", ("A",), scale=scales, calibration=False, img_tokens=h2 * w2, txt_len=lt)
    assert torch.equal(got, plain(f, fresh, joint, x=x2, **kw2))
    assert rel_l2(got, plain(f, fresh, x=x2, **kw2)) > LOOP_BAR
    assert torch.equal(plain(f, m, joint), first) and len(m.set_image_calls) == 1           # and back


def test_mx_fp8_linears_with_an_ip_adapter():
    """fp8_linear = 2 (one range at a time): the forward with an image prompt against the bf16 engine's with the same prompt,
    under the bar tests/test_mmdit_fp8_gpu.py holds that mode to"""
    import mmdit_fp8_ref as R
    from test_mmdit_fp8_gpu import FP8_BAR
    fam, geo = R.Flux, R.FLUX_ODD
    o = IR.add_ip_adapters_(copy.deepcopy(fam.oracle()), [(64, 256, 4)], [101], 0.012)
    inp = fam.inputs(geo)
    g = torch.Generator().manual_seed(6)
    emb = dev(torch.randn(3, 64, generator=g))
    outs = {}
    for mode in (0, 2):
        args, extra = fam.engine_args(geo)
        e = MM.MMDiTEngine(*args, calibration=False, device=DEV, fp8_linear=mode, **extra)
        e.load_weights(IR.base_state_dict(o))
        j = e.add_ip_adapter(64, 256, 4)
        for name, t in IR.adapter_state_dict(o, 0).items():
            e.set_weight(name, t)
        e.set_rope(*inp.rope)
        run = lambda: e.forward(dev(inp.img), 500.0, inp.guidance, dev(inp.txt[0]), inp.valid[0], dev(inp.vec), mode=MM.MC_MODE_FULL).clone()  # noqa: E731
        outs[mode, "plain"] = run()
        e.set_ip_adapter_image(j, 0, emb)
        e.select_ip_adapter(0)
        outs[mode, "ip"] = run()
    err = rel_l2(outs[2, "ip"], outs[0, "ip"])
    print("fp8_linear 2 with an image prompt vs bf16 with it: %.3e (without: %.3e)" % (err, rel_l2(outs[2, "plain"], outs[0, "plain"])))
    assert err < FP8_BAR
    assert rel_l2(outs[2, "ip"], outs[2, "plain"]) > 3e-2 and rel_l2(outs[0, "ip"], outs[0, "plain"]) > 3e-2


# ----------------------------------------------------------------------------- errors
def test_ip_adapter_errors(flux):
    f = flux
    m, e = f["one"], f["one"].engine
    lib = _lib.load()
    ref, ref_ip = plain(f, m), plain(f, m, jak(f))
    # another family refuses every call
    hy = MM.MMDiTEngine(_lib.MC_FAMILY_HUNYUAN, 256, 2, 1, 1, 16, 16, 256, 32, 128, 96, latent_grid=(2, 12, 16),
                        refiner_depth=2, device=DEV)
    for call in (lambda: hy.add_ip_adapter(64, 256, 4), lambda: hy.select_ip_adapter(0), lambda: hy.clear_ip_adapter(),
                 lambda: hy.set_ip_adapter_scale(0, 1.0), lambda: hy.set_ip_adapter_image(0, 0, torch.zeros(1, 64, device=DEV))):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            call()
        assert ex.value.status == _lib.MC_EINVAL and "FLUX" in str(ex.value)
    # the key without a loaded adapter: an error that names the remedy, no longer a silent text-only result
    none = hip_model(f, "FluxHIPIpUnloaded", (), calibration=False)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        plain(f, none, jak(f))
    # wrong list length, shape, dtype: raised before anything is set
    n_calls = len(m.set_image_calls)
    a = f["emb"]["A"]
    for bad in ([a, a], [], a, [a[:, :, :32]], [a[0, 0]], [a.double()], [a.long()], [a.expand(1, 65, 64)]):
        with pytest.raises(ValueError):
            plain(f, m, dict(ip_adapter_image_embeds=bad))
    assert len(m.set_image_calls) == n_calls
    # more images than 256 keys of 4 tokens: refused by the raw call as well
    t = torch.zeros(65, 64, device=DEV)
    assert lib.mc_mmdit_ip_adapter_set_image(e.h, 0, 0, C.c_void_p(t.data_ptr()), 65, None) == _lib.MC_EINVAL
    # a misaligned embeds pointer, a slot or an adapter that does not exist, a bad scale count
    assert lib.mc_mmdit_ip_adapter_set_image(e.h, 0, 0, C.c_void_p(t.data_ptr() + 4), 1, None) == _lib.MC_EINVAL
    assert lib.mc_mmdit_ip_adapter_set_image(e.h, 0, 2, C.c_void_p(t.data_ptr()), 1, None) == _lib.MC_EINVAL
    assert lib.mc_mmdit_ip_adapter_set_image(e.h, 1, 0, C.c_void_p(t.data_ptr()), 1, None) == _lib.MC_EINVAL
    assert lib.mc_mmdit_ip_adapter_select(e.h, 2) == _lib.MC_EINVAL
    assert lib.mc_mmdit_ip_adapter_scale(e.h, 0, (C.c_float * 3)(1, 1, 1), 3) == _lib.MC_EINVAL
    with pytest.raises(ValueError):
        m.set_ip_adapter_scale([1.0, 1.0])
    with pytest.raises(ValueError):
        m.set_ip_adapter_scale([[1.0, 1.0, 1.0]])
    # a state dict that misses a weight, holds a stranger (strict), or two adapters
    sd = IR.adapter_state_dict(oracle_with(f, ("A", "B")), 1)
    with pytest.raises(ValueError):
        m.load_ip_adapter({k: v for k, v in sd.items() if "to_v_ip" not in k or "blocks.1" not in k})
    with pytest.raises(ValueError):
        m.load_ip_adapter(dict(sd, stranger=torch.zeros(1)))
    with pytest.raises(ValueError):
        m.load_ip_adapter(sd, tokens_per_image=4)
    assert len(e._ip) == 1
    # a fifth adapter
    five = hip_model(f, "FluxHIPIpFive", ("A", "B", "A", "B"), calibration=False)
    with pytest.raises(ValueError):
        five.load_ip_adapter(sd)
    idx = C.c_int(-1)
    assert lib.mc_mmdit_ip_adapter_add(five.engine.h, 64, 256, 4, C.byref(idx)) == _lib.MC_EINVAL and idx.value == -1
    assert lib.mc_mmdit_ip_adapter_add(e.h, 64, 200, 4, C.byref(idx)) == _lib.MC_EINVAL          # no LayerNorm width
    assert lib.mc_mmdit_ip_adapter_add(e.h, 60, 256, 4, C.byref(idx)) == _lib.MC_EINVAL
    assert lib.mc_mmdit_ip_adapter_add(e.h, 64, 256, 257, C.byref(idx)) == _lib.MC_EINVAL
    # none of the refused calls left anything behind
    assert torch.equal(plain(f, m), ref) and torch.equal(plain(f, m, jak(f)), ref_ip)

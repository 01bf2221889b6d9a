"""GPU: DoRA, LoKr and LoHa adapters on both engines, loaded through load_lora from state dicts, on the tiny FLUX and Wan
engines of test_mmdit_lora_gpu.py / test_wan_lora_gpu.py.

The yardstick is a second engine whose weights were merged on the CPU by the float64 oracle (tests/adapter_kinds_ref.py) and
rounded to bf16.  LoKr, LoHa and pair terms are dyadic here (entries in {-1, -1/2, 0, 1/2, 1} * 2^e, power-of-two factors), so
their fp32 merge has ONE value, the oracle's, and the two forwards must agree BIT FOR BIT -- the bar the existing LoRA engine
tests set for this comparison.  A DoRA weight goes through a square root and a division, so it may differ from the rounded
oracle by one bf16 value on at most 1e-3 of its elements (test_adapter_merge_gpu.py).  Such a perturbation, about
sqrt(1e-3) * 2^-8 = 1.2e-4 of a touched weight's norm, re-rounds a fraction of the bf16 activations behind it by 2^-9 each; over
the few layers of these engines that stays below DORA_TOL = 2e-3 of the output's norm, and the adapters move the output by far
more, which every DoRA case asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adapter_kinds_ref as AR  # noqa: E402
import mmdit_fp8_ref as R8  # noqa: E402
import test_wan_lora_gpu as TW  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from test_mmdit_lora_gpu import dev, flux, lora_sd, merged_state_dict, rel_l2, same_bits  # noqa: E402,F401  (flux: a fixture)

DEV = "cuda:0"
EINVAL, ESTATE = _lib.MC_EINVAL, _lib.MC_ESTATE
DORA_TOL = 2e-3
KINDS = ["lokr", "lokr_factorised", "loha", "dora", "dora_lokr"]
FLUX_TARGETS = ["transformer_blocks.0.attn.to_q",            # one part of the fused q | k | v
                "transformer_blocks.1.ff.net.0.proj",
                "single_transformer_blocks.0.proj_mlp"]      # the last part of the single block's fused [q; k; v; mlp]
WAN_TARGETS = ["blocks.0.self_attn.q", "blocks.1.cross_attn.k", "blocks.0.ffn.0", "text_embedding.0"]


def make_adapter(sd, modules, kind, seed, prefix):
    """(adapter state dict, spec) with one entry of `kind` per module, shaped after sd[<module>.weight].
    spec: {target: (oracle terms without their multiplier, factor, magnitude or None)}"""
    g = torch.Generator().manual_seed(seed)
    lsd, spec = {}, {}
    for m in modules:
        W = sd[m + ".weight"]
        rows, k = W.shape[0], W.numel() // W.shape[0]
        mag = None
        if kind in ("lokr", "lokr_factorised", "dora_lokr"):
            s1, s2 = AR.kron_shapes(rows, k)
            w1 = AR.dyadic(s1, g, -3)
            if kind == "lokr_factorised":                      # w2 = a @ b of rank 2, alpha 4: factor 2
                a, b = AR.dyadic((s2[0], 2), g, -2), AR.dyadic((2, s2[1]), g, -2)
                keys, term, factor = AR.lokr_keys(m, w1, (a, b), alpha=4.0), ("kron", w1, a @ b), 2.0
            else:                                              # both halves full: factor 1 whatever alpha says
                w2 = AR.dyadic(s2, g, -3)
                keys, term, factor = AR.lokr_keys(m, w1, w2, alpha=16.0), ("kron", w1, w2), 1.0
        elif kind == "loha":                                   # rank 4, alpha 2: factor 1/2
            ops = [AR.dyadic(s, g, -2) for s in ((rows, 4), (4, k), (rows, 4), (4, k))]
            keys, term, factor = AR.loha_keys(m, *ops, alpha=2.0, infix=".default"), ("hada",) + tuple(ops), 0.5
        else:                                                  # "dora": a rank-4 pair, alpha 8: factor 2
            a, b = AR.dyadic((4, k), g, -5), AR.dyadic((rows, 4), g, -5)
            keys, term, factor = AR.pair_keys(m, a, b, alpha=8.0), ("pair", a, b), 2.0
        if kind.startswith("dora"):                            # not the row norm: every row changes its length
            mag = W.detach().float().cpu().reshape(rows, k).bfloat16().float().norm(dim=1) * (0.5 + torch.rand(rows, generator=g))
            keys.update(AR.magnitude_keys(m, mag, ".lora_magnitude_vector" if kind == "dora" else ".dora_scale", column=kind != "dora"))
        lsd.update({prefix + key: v for key, v in keys.items()})
        spec[m + ".weight"] = (term, factor, mag)
    return lsd, spec


def oracle_merged(sd, adapters, device=None):
    """sd with every touched weight rebuilt by the float64 oracle from its bf16 value and rounded to bf16; adapters:
    [(spec, scale)] in load order.  A magnitude is live while its adapter's scale is not 0."""
    out = dict(sd)
    for target in {t for spec, _ in adapters for t in spec}:
        W = sd[target].detach()
        Wb = W.cpu().reshape(W.shape[0], -1).bfloat16()
        terms, mag = [], None
        for spec, scale in adapters:
            if target not in spec or scale == 0.0:
                continue
            term, factor, g = spec[target]
            terms.append(term + (AR.multiplier(scale, factor),))
            mag = g if g is not None else mag
        new = AR.to_bf16(AR.merged_weight(Wb, terms, mag)) if terms or mag is not None else Wb
        out[target] = new.reshape(W.shape).to(device or W.device)
    return out


def pair_spec(lsd, prefix="transformer."):
    """the spec of a plain LoRA state dict of lora_sd()"""
    from magcache_amd.lora import lora_factor, parse_lora_state_dict
    return {t: (("pair", a.float(), b.float()), lora_factor(a, alpha), None) for t, (a, b, alpha) in parse_lora_state_dict(lsd, prefix).items()}


def agree(got, want, exact, what):
    if exact:
        assert same_bits(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} elements differ"
    else:
        err = rel_l2(got, want)
        print(f"{what}: rel. L2 distance to the oracle-merged engine {err:.3e}")
        assert err < DORA_TOL, (what, err)


# ----------------------------------------------------------------------------------------------------------- FLUX
@pytest.mark.parametrize("kind", KINDS)
def test_flux_every_kind_parity_rescale_and_off_states(flux, kind):
    lsd, spec = make_adapter(flux.sd, FLUX_TARGETS, kind, seed=31, prefix="transformer.")
    exact = not kind.startswith("dora")
    m = flux.make()
    base = flux.run(m).clone()
    assert m.load_lora(lsd, adapter="a") == []
    info = m.lora_info()
    assert info["adapters"] == 1 and info["linears"] == 3 and info["base_bytes"] > 0
    got = flux.run(m).clone()
    agree(got, flux.run(flux.make(oracle_merged(flux.sd, [(spec, 1.0)]))), exact, f"flux {kind} at scale 1")
    moved = rel_l2(got, base)
    print(f"flux {kind}: the adapter moves the output by {moved:.3e}")
    # bit-exact cases cannot pass on an ignored adapter once the outputs differ at all; a case with a tolerance must move far more
    assert not same_bits(got, base) and (exact or moved > 10 * DORA_TOL), moved
    # a new scale re-merges from the pristine weight
    m.set_adapters("a", 0.5)
    half = flux.run(m).clone()
    agree(half, flux.run(flux.make(oracle_merged(flux.sd, [(spec, 0.5)]))), exact, f"flux {kind} at scale 0.5")
    assert not same_bits(half, got)
    if not exact:
        # ... and recomputes the norm: W + 0.5 (W_dora(1) - W), half the delta merge, is another weight
        one = oracle_merged(flux.sd, [(spec, 1.0)])
        lin = {t: (0.5 * (one[t].double() + flux.sd[t].bfloat16().double())).float().bfloat16() for t in spec}
        linear = flux.run(flux.make(dict(flux.sd, **lin)))
        assert rel_l2(half, linear) > 10 * DORA_TOL, rel_l2(half, linear)
    # scale 0: the term and the magnitude are both left out, the pristine rows come back (the copies stay)
    m.set_adapters("a", 0.0)
    assert same_bits(flux.run(m), base) and m.lora_info()["base_bytes"] > 0
    m.set_adapters("a", 1.0)
    assert same_bits(flux.run(m), got)
    m.unload_lora()
    info = m.lora_info()
    assert same_bits(flux.run(m), base) and info["adapters"] == 0 and info["linears"] == 0 and info["base_bytes"] == 0


def test_flux_lora_plus_lokr_on_one_weight_and_pairs_alone_keep_their_merge(flux):
    shared = ["transformer_blocks.0.attn.to_q", "single_transformer_blocks.1.proj_out"]
    la = lora_sd(flux.sd, shared, 4, seed=1, alpha=8)
    lb, spec_b = make_adapter(flux.sd, shared, "lokr", seed=32, prefix="transformer.")
    lc, spec_c = make_adapter(flux.sd, shared[:1], "loha", seed=33, prefix="transformer.")
    m = flux.make()
    assert m.load_lora(la, adapter="a") == [] and m.load_lora(lb, adapter="b", scale=2.0) == [] and m.load_lora(lc, adapter="c") == []
    assert m.lora_info()["adapters"] == 3
    got = flux.run(m).clone()
    want = flux.run(flux.make(oracle_merged(flux.sd, [(pair_spec(la), 1.0), (spec_b, 2.0), (spec_c, 1.0)])))
    assert same_bits(got, want)
    # the other kinds off: the weight has live pairs only and is the existing merge's, bit for bit
    m.set_adapters("a")
    only_a = flux.run(m).clone()
    assert same_bits(only_a, flux.run(flux.make(merged_state_dict(flux.sd, [(la, 1.0)])))) and not same_bits(only_a, got)
    # all kinds count towards the limit of terms per weight: a, b, c hold three of the eight on to_q
    name = b"transformer_blocks.0.attn.to_q.weight"
    rows, k = flux.sd["transformer_blocks.0.attn.to_q.weight"].shape
    (r1, c1), (r2, c2) = AR.kron_shapes(rows, k)
    w1, w2 = torch.zeros(r1, c1, device=DEV), torch.zeros(r2, c2, device=DEV)
    e = m.engine

    def set_kron(adapter):
        return e.lib.mc_mmdit_lora_set_kron(e.h, adapter, name, MM._ptr(w1), (MM.C.c_int64 * 2)(r1, c1), MM._ptr(w2),
                                            (MM.C.c_int64 * 2)(r2, c2), _lib.MC_F32, 1.0, None)
    for i in range(5):
        assert set_kron(b"x%d" % i) == _lib.MC_OK
    assert set_kron(b"x5") == EINVAL and b"more than 8" in e.lib.mc_last_error()
    assert set_kron(b"b") == _lib.MC_OK                                                # the same (adapter, weight, kind) replaces
    # the change waits for its apply: a forward is refused until then
    with pytest.raises(_lib.MagCacheHipError) as ex:
        flux.run(m)
    assert ex.value.status == ESTATE and "mc_mmdit_lora_apply" in str(ex.value)
    m.unload_lora()
    assert m.lora_info()["base_bytes"] == 0


def test_flux_bf16_operands_through_the_c_calls_are_widened_exactly(flux):
    """load_lora hands fp32 operands over; the C calls also take bf16, which the dyadic values fit exactly"""
    lh, spec_h = make_adapter(flux.sd, FLUX_TARGETS[:1], "loha", seed=39, prefix="transformer.")
    lk, spec_k = make_adapter(flux.sd, FLUX_TARGETS[1:2], "dora_lokr", seed=40, prefix="transformer.")
    m = flux.make()
    assert m.load_lora(dict(lh, **lk), adapter="a") == []
    want = flux.run(m).clone()
    m2 = flux.make()
    e = m2.engine

    def b16(t):
        return t.to(DEV).bfloat16().contiguous()

    def shape(t):
        return (MM.C.c_int64 * 2)(*t.shape)
    (target, (term, factor, _)), = spec_h.items()
    u1, d1, u2, d2 = (b16(t) for t in term[1:])
    _lib.check(e.lib.mc_mmdit_lora_set_hada(e.h, b"a", target.encode(), MM._ptr(u1), shape(u1), MM._ptr(d1), shape(d1), MM._ptr(u2),
                                            MM._ptr(d2), _lib.MC_BF16, factor, None))
    (target, (term, factor, mag)), = spec_k.items()
    w1, w2 = b16(term[1]), b16(term[2])
    _lib.check(e.lib.mc_mmdit_lora_set_kron(e.h, b"a", target.encode(), MM._ptr(w1), shape(w1), MM._ptr(w2), shape(w2), _lib.MC_BF16,
                                            factor, None))
    g = mag.to(DEV).float().contiguous()        # a magnitude is no bf16 value: fp32
    _lib.check(e.lib.mc_mmdit_lora_set_magnitude(e.h, b"a", target.encode(), MM._ptr(g), g.numel(), _lib.MC_F32, None))
    torch.cuda.synchronize()
    m2.apply_lora()
    assert same_bits(flux.run(m2), want)


def test_flux_two_magnitudes_refused_targets_and_state(flux):
    m = flux.make()
    e = m.engine
    la, spec_a = make_adapter(flux.sd, FLUX_TARGETS[:1], "dora", seed=34, prefix="transformer.")
    lb, _ = make_adapter(flux.sd, FLUX_TARGETS[:2], "dora_lokr", seed=35, prefix="transformer.")
    assert m.load_lora(la, adapter="first") == []
    with_a = flux.run(m).clone()

    def status_of(lsd, **kw):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            m.load_lora(lsd, **kw)
        return ex.value.status, str(ex.value)
    # a second adapter's magnitude on a weight that carries one
    st, msg = status_of(lb, adapter="second")
    assert st == EINVAL and "'first'" in msg and "'second'" in msg and "attn.to_q.weight" in msg
    assert m.lora_info()["adapters"] == 1 and same_bits(flux.run(m), with_a)           # the strict load left nothing behind
    # the same adapter's again replaces it
    assert m.load_lora(la, adapter="first") == [] and same_bits(flux.run(m), with_a)
    # refused targets: the fp32 head for every kind, a shape that does not factor
    rows, k = flux.sd["proj_out.weight"].shape
    for kind in ("lokr", "loha", "dora"):
        st, msg = status_of(make_adapter(flux.sd, ["proj_out"], kind, seed=36, prefix="transformer.")[0], adapter="x")
        assert st == EINVAL and "proj_out.weight" in msg, (kind, msg)
    rows, k = flux.sd[FLUX_TARGETS[0] + ".weight"].shape
    bad = {"transformer." + key: v for key, v in AR.lokr_keys(FLUX_TARGETS[0], torch.zeros(3, 8), torch.zeros(rows // 4, k // 8)).items()}
    st, msg = status_of(bad, adapter="x")
    assert st == EINVAL and "no factorisation" in msg and "attn.to_q.weight" in msg
    bad_loha = {"transformer." + key: v for key, v in
                AR.loha_keys(FLUX_TARGETS[0], torch.zeros(rows, 4), torch.zeros(4, k // 2), torch.zeros(rows, 4), torch.zeros(4, k // 2)).items()}
    assert status_of(bad_loha, adapter="x")[0] == EINVAL
    assert m.lora_info()["adapters"] == 1 and same_bits(flux.run(m), with_a)
    # strict=False skips what the engine refuses and says so
    mixed = dict(make_adapter(flux.sd, ["proj_out"], "lokr", seed=37, prefix="transformer.")[0],
                 **make_adapter(flux.sd, FLUX_TARGETS[1:2], "lokr", seed=38, prefix="transformer.")[0])
    assert m.load_lora(mixed, adapter="mixed", strict=False) == ["proj_out.weight"]
    assert m.lora_info()["adapters"] == 2 and not same_bits(flux.run(m), with_a)
    # a padded image embedder takes none of the kinds (in_channels 16 -> K padded to 64)
    small = MM.MMDiTEngine(_lib.MC_FAMILY_FLUX, 256, 2, 1, 1, 16, 16, 256, 64, 128, 64, device=DEV)
    for keys in (AR.lokr_keys("x_embedder", torch.zeros(4, 4), torch.zeros(64, 4)),
                 AR.loha_keys("x_embedder", torch.zeros(256, 2), torch.zeros(2, 16), torch.zeros(256, 2), torch.zeros(2, 16))):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            small.load_lora(keys)
        assert ex.value.status == EINVAL and "x_embedder.weight" in str(ex.value)
    # inside begin .. end every new call is refused
    kw = flux.kw
    e.begin(dev(flux.x[0]), 500.0, 4000.0, dev(kw["encoder_hidden_states"][0]), flux.meta["txt_len"], dev(kw["pooled_projections"][0]),
            MM.MC_MODE_FULL)
    z = torch.zeros(rows, device=DEV)
    name = (FLUX_TARGETS[0] + ".weight").encode()
    two = (MM.C.c_int64 * 2)(1, 1)
    assert e.lib.mc_mmdit_lora_set_magnitude(e.h, b"first", name, MM._ptr(z), rows, _lib.MC_F32, None) == ESTATE
    assert e.lib.mc_mmdit_lora_set_kron(e.h, b"first", name, MM._ptr(z), two, MM._ptr(z), two, _lib.MC_F32, 1.0, None) == ESTATE
    assert e.lib.mc_mmdit_lora_set_hada(e.h, b"first", name, MM._ptr(z), two, MM._ptr(z), two, MM._ptr(z), MM._ptr(z), _lib.MC_F32, 1.0,
                                        None) == ESTATE
    for blk in range(e.n_blocks):
        e.block_pre(blk)
        e.block_post(blk)
    e.end(torch.empty(e.img_tokens, e.out_channels, device=DEV))
    torch.cuda.synchronize()
    m.unload_lora()
    assert m.lora_info()["base_bytes"] == 0


def test_flux_mx_copy_follows_the_merge():
    """width 512, fp8_linear = 2: q|k|v, MLP-in and the single block's linear1 run on their MX copies, so the identity holds only
    if exactly the touched rows were requantised from the merged rows"""
    fam, geo = R8.Flux, R8.FLUX_ODD
    sd = {k: v.detach() for k, v in fam.oracle().state_dict().items()}
    args, extra = fam.engine_args(geo)
    inp = fam.inputs(geo)

    def make(weights):
        e = MM.MMDiTEngine(*args, calibration=False, device=DEV, fp8_linear=2, **extra)
        e.load_weights(weights)
        e.set_rope(*inp.rope)
        return e

    def run(e):
        return e.forward(dev(inp.img), 500.0, inp.guidance, dev(inp.txt[0]), inp.valid[0], dev(inp.vec)).clone()
    targets = ["transformer_blocks.0.attn.to_k", "transformer_blocks.0.ff.net.0.proj", "single_transformer_blocks.0.proj_mlp"]
    la, spec_a = make_adapter(sd, targets, "lokr", seed=41, prefix="transformer.")
    lb, spec_b = make_adapter(sd, targets[:2], "loha", seed=42, prefix="transformer.")
    e = make(sd)
    base = run(e)
    assert e.load_lora(la, adapter="a") == [] and e.load_lora(lb, adapter="b", scale=-2.0) == []
    got = run(e)
    assert same_bits(got, run(make(oracle_merged(sd, [(spec_a, 1.0), (spec_b, -2.0)]))))
    assert not same_bits(got, base) and bool(torch.isfinite(got).all())
    e.unload_lora()                                            # ... and requantised back
    assert same_bits(run(e), base)


# ----------------------------------------------------------------------------------------------------------- Wan
OUTPUTS = (0, 1, 4, 5)     # of test_wan_lora_gpu.trace(): FULL forwards, their residual slots, SKIP forwards, the slots again


def floats(trace):
    return [t.view(torch.float32) for t in trace]


@pytest.mark.parametrize("kind", ["lokr", "loha", "dora"])
def test_wan_every_kind_parity_rescale_and_off_states(kind):
    cfg = TW.CFG
    wd = TW.weights(cfg)
    lsd, spec = make_adapter(wd, WAN_TARGETS, kind, seed=51, prefix="diffusion_model.")
    exact = kind != "dora"
    A = TW.make_engine(cfg, wd)
    plain = TW.trace(A)
    assert A.load_lora(lsd, adapter="a") == []
    assert A.lora_info()["adapters"] == 1 and A.lora_info()["base_bytes"] > 0
    for scale in (1.0, 0.5):
        A.set_adapters("a", scale)
        got = TW.trace(A)
        want = TW.trace(TW.make_engine(cfg, oracle_merged(wd, [(spec, scale)])))
        if exact:
            TW.assert_same(got, want, f"wan {kind} at scale {scale} vs oracle-merged weights")
        else:
            # the forward outputs (FULL and SKIP, both branches); the residual slots are differences of hidden states, a
            # fraction of their norm, to which the reasoning behind DORA_TOL does not apply: they are printed only
            for i, (a, b) in enumerate(zip(floats(got), floats(want))):
                if i in OUTPUTS:
                    agree(a, b, False, f"wan {kind} at scale {scale}, output {i}")
                else:
                    print(f"wan {kind} at scale {scale}, residual slot {i}: rel. L2 distance {rel_l2(a, b):.3e}")
        moved = rel_l2(floats(got)[0], floats(plain)[0])
        print(f"wan {kind} at scale {scale}: the adapter moves the output by {moved:.3e}")
        assert not torch.equal(got[0], plain[0]) and (exact or moved > 10 * DORA_TOL), moved
    A.set_adapters("a", 0.0)
    TW.assert_same(TW.trace(A), plain, "scale 0")
    A.unload_lora()
    TW.assert_same(TW.trace(A), plain, "after unload_lora")
    info = A.lora_info()
    assert info["adapters"] == 0 and info["linears"] == 0 and info["base_bytes"] == 0


def test_wan_refused_targets_and_two_magnitudes():
    cfg = TW.CFG
    wd = TW.weights(cfg)
    A = TW.make_engine(cfg, wd)
    plain = TW.trace(A)
    # the fp32 matrices take pairs at most; the patch embedder nothing
    for module in ("time_embedding.0", "time_projection.1", "head.head"):
        for kind in ("lokr", "loha"):
            with pytest.raises(_lib.MagCacheHipError) as ex:
                A.load_lora(make_adapter(wd, [module], kind, seed=52, prefix="diffusion_model.")[0], adapter="x")
            assert ex.value.status == EINVAL and module + ".weight" in str(ex.value), (module, kind)
    rows = wd["time_embedding.0.weight"].shape[0]
    z = torch.zeros(rows, device=DEV)
    assert A.lib.mc_lora_set_magnitude(A.h, b"x", b"time_embedding.0.weight", MM._ptr(z), rows, _lib.MC_F32, None) == EINVAL
    assert b"time_embedding.0.weight" in A.lib.mc_last_error()
    pe = wd["patch_embedding.weight"]
    keys = AR.lokr_keys("patch_embedding", torch.zeros(1, 1), torch.zeros(pe.shape[0], pe.numel() // pe.shape[0]))
    with pytest.raises(_lib.MagCacheHipError) as ex:
        A.load_lora(keys, adapter="x")
    assert ex.value.status == EINVAL and "patch_embedding.weight" in str(ex.value)
    assert A.load_lora(make_adapter(wd, ["time_embedding.0", "blocks.0.ffn.0"], "lokr", seed=53, prefix="")[0], adapter="y",
                       strict=False) == ["time_embedding.0.weight"]
    A.unload_lora()
    # two magnitudes on one weight
    la, _ = make_adapter(wd, WAN_TARGETS[:1], "dora", seed=54, prefix="diffusion_model.")
    lb, _ = make_adapter(wd, WAN_TARGETS[:1], "dora_lokr", seed=55, prefix="diffusion_model.")
    assert A.load_lora(la, adapter="first") == []
    with pytest.raises(_lib.MagCacheHipError) as ex:
        A.load_lora(lb, adapter="second")
    assert ex.value.status == EINVAL and "'first'" in str(ex.value) and "'second'" in str(ex.value)
    A.unload_lora()
    TW.assert_same(TW.trace(A), plain, "after the refusals")
    assert A.lora_info()["base_bytes"] == 0

"""GPU: LoRA adapters on the MM-DiT engine (mc_mmdit_lora_*), merged into the weights on the device.

The bar for the merge is identity: an engine with adapters loaded must compute, bit for bit, what a second engine computes
whose weights were merged on the host by the kernel's formula, W_eff = bf16(bf16(W) + sum_j m_j (B_j A_j)) with m_j = scale_j *
alpha_j / rank_j.  With dyadic adapters (entries in {-1, -1/2, 0, 1/2, 1} * 2^-5, power-of-two multipliers) B A and the sum over
adapters are exact in fp32 in any order, so the host formula has ONE value and the engine (deterministic by default) must hit
it -- in bf16 and, at width 512, with the MX fp8 copies requantised.  Random adapters are held to the fp32 oracle with the
bars of test_flux_forward_vs_oracle.  Toy FLUX / HunyuanVideo / Qwen-Image fixtures from tests/golden, as test_mmdit_gpu.py
and test_qwen_image_gpu.py build them."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd.lora import lora_factor, lora_target_names, parse_lora_state_dict  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402
from oracle import hunyuan_ref as HR  # noqa: E402

import mmdit_fp8_ref as R8  # noqa: E402
import qwen_image_ref as QR  # noqa: E402

DEV = "cuda:0"
EINVAL, ESTATE = _lib.MC_EINVAL, _lib.MC_ESTATE


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


def dev(t):
    return t.to(DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def acts(got, base_out):
    """The identity tests compare with an engine whose WEIGHTS differ from the adapter-free ones, so they cannot pass on ignored
    adapters once the two outputs differ at all; the dyadic deltas are small by construction (rank 4 of entries <= 2^-5 against
    weights of std 0.04), so no size is asked of the difference here -- test 3 asks 1e-2 of its random adapters."""
    return not same_bits(got, base_out) and bool(torch.isfinite(got).all())


def fresh_flux_magcache(m, meta):
    """init_flux_magcache, and the per-sample attributes the forward assigned through `self` (they shadow the class's) dropped"""
    for k in ("cnt", "accumulated_ratio", "accumulated_steps", "accumulated_err", "previous_residual"):
        m.__dict__.pop(k, None)
    MM.init_flux_magcache(m, meta["steps"], meta["thresh"], meta["K"], meta["R"])


def plain_flux(m):
    for k in ("cnt", "accumulated_ratio", "accumulated_steps", "accumulated_err", "previous_residual"):
        m.__dict__.pop(k, None)
    type(m).forward = MM.flux_plain_forward
    type(m).cnt = 0


# ----------------------------------------------------------------------------- adapters and host merges
def lora_sd(sd, modules, rank, seed, alpha=None, dyadic=True, std=0.05, prefix="transformer."):
    """a PEFT-style state dict with one pair per module of `modules`, shaped after sd[<module>.weight]; the values are exact
    in bf16 either way, so the engine's bf16 copies hold what the host merge uses"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m in modules:
        n_out, k_in = sd[m + ".weight"].shape
        if dyadic:
            a = torch.randint(-2, 3, (rank, k_in), generator=g).float() / 2 * 2.0 ** -5
            b = torch.randint(-2, 3, (n_out, rank), generator=g).float() / 2 * 2.0 ** -5
        else:
            a = (torch.randn(rank, k_in, generator=g) * std).bfloat16().float()
            b = (torch.randn(n_out, rank, generator=g) * std).bfloat16().float()
        out[f"{prefix}{m}.lora_A.weight"], out[f"{prefix}{m}.lora_B.weight"] = a, b
        if alpha is not None:
            out[f"{prefix}{m}.alpha"] = torch.tensor(float(alpha))
    return out


def merged_state_dict(sd, loras, engine_bits=True):
    """sd with W + sum_j m_j (B_j A_j) on every target of `loras` = [(lora state dict, scale)], in load order.
    engine_bits: the kernel's arithmetic on the engine's bf16 weight, rounded to bf16 once; else plain fp32 (for the oracle)."""
    terms = {}
    for lsd, scale in loras:
        for target, (a, b, alpha) in parse_lora_state_dict(lsd).items():
            m = float(np.float32(np.float32(scale) * np.float32(lora_factor(a, alpha))))
            terms.setdefault(target, []).append((a.float(), b.float(), m))
    out = dict(sd)
    for target, ts in terms.items():
        delta = None
        for a, b, m in ts:
            d = m * (b @ a)
            delta = d if delta is None else delta + d
        w = sd[target].detach()
        out[target] = (w.bfloat16().float() + delta).bfloat16() if engine_bits else w.float() + delta
    return out


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def flux(golden_dir):
    g = np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    oracle = FR.init_synthetic_(FR.FluxTransformer2DModel(**cfg), seed=meta["weight_seed"], std=meta["weight_std"])
    sd = {k: v.detach() for k, v in oracle.state_dict().items()}
    kw = dict(encoder_hidden_states=torch.from_numpy(g["ctx"]), pooled_projections=torch.from_numpy(g["pooled"]),
              img_ids=torch.from_numpy(g["img_ids"]), txt_ids=torch.from_numpy(g["txt_ids"]), guidance=torch.tensor([4.0]))
    x, t = torch.from_numpy(g["latent0"]), torch.tensor([0.5])

    def make(weights=sd, **extra):
        cls = type("FluxLoraUnderTest", (MM.FluxTransformer2DModelHIP,), {})
        m = cls(cfg, meta["h2"] * meta["w2"], txt_len=meta["txt_len"], device=DEV, calibration=True, **extra)
        return m.load_state_dict(weights)

    def run(m, **over):
        return m(hidden_states=dev(x), timestep=dev(t), return_dict=False, **{k: dev(v) for k, v in kw.items()}, **over)[0]
    return SimpleNamespace(g=g, meta=meta, cfg=cfg, oracle=oracle, sd=sd, kw=kw, x=x, t=t, make=make, run=run)


FLUX_TARGETS = ["transformer_blocks.0.attn.to_q",            # one part of the fused q | k | v
                "transformer_blocks.0.attn.to_out.0", "transformer_blocks.1.ff.net.0.proj", "transformer_blocks.1.ff_context.net.2",
                "single_transformer_blocks.0.proj_mlp",      # the last part of the single block's fused [q; k; v; mlp]
                "single_transformer_blocks.1.proj_out", "transformer_blocks.0.norm1.linear"]   # a part of the stacked modulation matrix
FLUX_OVERLAP = ["transformer_blocks.0.attn.to_q", "single_transformer_blocks.1.proj_out"]


def flux_loras(sd):
    """adapter "a": rank 4, alpha 8 (factor 2) on every kind of Linear; adapter "b": rank 24, alpha 12 (factor 1/2) overlapping on two"""
    return lora_sd(sd, FLUX_TARGETS, 4, seed=1, alpha=8), lora_sd(sd, FLUX_OVERLAP, 24, seed=2, alpha=12)


@pytest.fixture(scope="module")
def flux_lora_model(flux):
    """one engine with the two dyadic adapters loaded: a at scale 1, b at scale 2"""
    m = flux.make()
    base_out = flux.run(m).clone()
    la, lb = flux_loras(flux.sd)
    assert m.load_lora(la, adapter="a") == [] and m.load_lora(lb, adapter="b", scale=2.0) == []
    return m, base_out, la, lb


# ----------------------------------------------------------------------------- 1. identity with host-merged weights
def test_flux_adapters_equal_host_merged_weights_bitwise(flux, flux_lora_model):
    m, base_out, la, lb = flux_lora_model
    info = m.lora_info()
    assert info["adapters"] == 2 and info["scales"] == {"a": 1.0, "b": 2.0}
    # base copies: q|k|v, to_out, ff.net.0.proj, ff_context.net.2, the single [q;k;v;mlp] of block 0, proj_out of block 1, the modulation matrix
    assert info["linears"] == 7 and info["base_bytes"] > 0
    got = flux.run(m)
    ref = flux.make(merged_state_dict(flux.sd, [(la, 1.0), (lb, 2.0)]))
    want = flux.run(ref)
    assert same_bits(got, want)
    assert acts(got, base_out)


def test_hunyuan_adapters_equal_host_merged_weights_bitwise(golden_dir):
    g = np.load(os.path.join(golden_dir, "hunyuan_forward_golden.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = dict(meta["cfg"], patch_size=tuple(meta["cfg"]["patch_size"]), rope_dim_list=tuple(meta["cfg"]["rope_dim_list"]))
    oracle = HR.init_synthetic_(HR.HYVideoDiffusionTransformer(**cfg), seed=meta["weight_seed"], std=meta["weight_std"])
    sd = {k: v.detach() for k, v in oracle.state_dict().items()}
    kw = dict(text_states=torch.from_numpy(g["txt"]), text_mask=torch.from_numpy(g["mask"]),
              text_states_2=torch.from_numpy(g["txt2"]), freqs_cos=torch.from_numpy(g["cos"]),
              freqs_sin=torch.from_numpy(g["sin"]), guidance=torch.tensor([meta["guidance"]]))
    x, t = torch.from_numpy(g["latent0"]), torch.tensor([500.0])

    def make(weights):
        m = MM.HYVideoDiffusionTransformerHIP(cfg, tuple(meta["grid"]), txt_len=meta["txt_len"], device=DEV, calibration=False)
        return m.load_state_dict(weights)

    def run(m):
        return m(dev(x), dev(t), **{k: dev(v) for k, v in kw.items()})["x"]
    targets = ["single_blocks.0.linear1", "txt_in.individual_token_refiner.blocks.0.mlp.fc1", "double_blocks.1.img_attn_proj"]
    la = lora_sd(sd, targets, 4, seed=3, alpha=4)
    lb = lora_sd(sd, targets[:1], 130, seed=4, alpha=65)
    m = make(sd)
    base_out = run(m).clone()
    assert m.load_lora(la, adapter="a", scale=2.0) == [] and m.load_lora(lb, adapter="b") == []
    got = run(m)
    assert same_bits(got, run(make(merged_state_dict(sd, [(la, 2.0), (lb, 1.0)]))))
    assert acts(got, base_out)
    # the permuted fp32 head takes no adapter
    with pytest.raises(_lib.MagCacheHipError) as ex:
        m.load_lora(lora_sd(sd, ["final_layer.linear"], 4, seed=5))
    assert ex.value.status == EINVAL and "final_layer.linear.weight" in str(ex.value)
    assert same_bits(run(m), got)


@pytest.fixture(scope="module")
def qwen(golden_dir):
    g = np.load(os.path.join(golden_dir, "qwen_image_golden.npz"))
    meta = json.loads(str(g["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    oracle = QR.init_synthetic_(QR.QwenImageTransformer2DModel(**cfg), seed=meta["weight_seed"], std=meta["weight_std"])
    sd = {k: v.detach() for k, v in oracle.state_dict().items()}
    x, pe = torch.from_numpy(g["latent0"]).to(DEV), torch.from_numpy(g["prompt_embeds"]).to(DEV)
    shapes = [[(1, meta["h2"], meta["w2"])]]

    def make(weights=sd):
        m = MM.QwenImageTransformer2DModelHIP(cfg, x.shape[1], txt_len=pe.shape[1], device=DEV, calibration=False)
        return m.load_state_dict(weights)

    def run(m, **over):
        return m(hidden_states=x, encoder_hidden_states=pe, timestep=torch.tensor([0.5], device=DEV), img_shapes=shapes,
                 txt_seq_lens=[pe.shape[1]], return_dict=False, **over)[0]
    return SimpleNamespace(sd=sd, make=make, run=run)


QWEN_TARGETS = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.add_k_proj", "transformer_blocks.0.attn.to_out.0",
                "transformer_blocks.1.img_mlp.net.0.proj", "transformer_blocks.1.txt_mlp.net.2", "transformer_blocks.1.img_mod.1"]


def test_qwen_adapters_equal_host_merged_weights_bitwise_and_scale_per_call(qwen):
    la = lora_sd(qwen.sd, QWEN_TARGETS, 4, seed=6, alpha=8)
    lb = lora_sd(qwen.sd, QWEN_TARGETS[:1], 24, seed=7, alpha=12)
    m = qwen.make()
    base_out = qwen.run(m).clone()
    assert m.load_lora(la, adapter="a") == [] and m.load_lora(lb, adapter="b", scale=2.0) == []
    got = qwen.run(m).clone()
    assert same_bits(got, qwen.run(qwen.make(merged_state_dict(qwen.sd, [(la, 1.0), (lb, 2.0)]))))
    assert acts(got, base_out)
    # attention_kwargs["scale"], as scale_lora_layers reads it: this call's factor on every adapter
    half = qwen.run(m, attention_kwargs={"scale": 0.5}).clone()
    assert m.lora_info()["call_scale"] == 0.5
    assert same_bits(qwen.run(m), got) and m.lora_info()["call_scale"] == 1.0          # a call without the key is back at 1
    m.set_adapters(["a", "b"], [0.5, 1.0])
    assert same_bits(qwen.run(m), half)
    assert not same_bits(half, got)
    m.unload_lora()
    assert same_bits(qwen.run(m), base_out) and m.lora_info()["base_bytes"] == 0


# ----------------------------------------------------------------------------- 2. the same identity with MX fp8 Linears
def test_flux_fp8_linear_2_adapters_equal_host_merged_weights_bitwise():
    """width 512, fp8_linear = 2: q|k|v, MLP-in, MLP-out and the single block's linear1 run on their e4m3 copies, so the identity
    holds only if the copy and the block scales of exactly the touched rows were requantised from the merged rows."""
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
    targets = ["transformer_blocks.0.attn.to_k", "transformer_blocks.1.attn.add_q_proj", "transformer_blocks.0.ff.net.0.proj",
               "transformer_blocks.1.ff_context.net.2", "single_transformer_blocks.0.proj_mlp", "single_transformer_blocks.1.attn.to_v",
               "transformer_blocks.1.attn.to_out.0"]      # the last one stays bf16 in mode 2
    la = lora_sd(sd, targets, 4, seed=8, alpha=8)
    lb = lora_sd(sd, targets[:2], 24, seed=9, alpha=12)
    e = make(sd)
    base_out = run(e)
    assert e.load_lora(la, adapter="a") == [] and e.load_lora(lb, adapter="b", scale=-2.0) == []
    got = run(e)
    assert same_bits(got, run(make(merged_state_dict(sd, [(la, 1.0), (lb, -2.0)]))))
    assert acts(got, base_out)
    e.unload_lora()                                        # ... and requantised back
    assert same_bits(run(e), base_out)


# ----------------------------------------------------------------------------- 3. random adapters against the fp32 oracle
def test_flux_random_adapters_vs_fp32_oracle(flux):
    """the bars of test_flux_forward_vs_oracle, with W + s B A in the oracles' state dicts"""
    targets = FLUX_TARGETS + ["transformer_blocks.1.attn.add_k_proj", "single_transformer_blocks.2.attn.to_v"]
    la = lora_sd(flux.sd, targets, 16, seed=10, alpha=16, dyadic=False, std=0.1)
    lb = lora_sd(flux.sd, FLUX_OVERLAP, 130, seed=11, dyadic=False, std=0.03)
    loras = [(la, 0.8), (lb, -1.3)]
    merged = merged_state_dict(flux.sd, loras, engine_bits=False)
    kw, x, t = flux.kw, flux.x, flux.t
    with torch.no_grad():
        o32 = FR.FluxTransformer2DModel(**flux.cfg)
        o32.load_state_dict(merged)
        ref32 = o32(hidden_states=x, timestep=t, **kw)[0]
        obf = FR.FluxTransformer2DModel(**flux.cfg)
        obf.load_state_dict(merged)
        obf = obf.bfloat16()
        refbf = obf(hidden_states=x.bfloat16(), timestep=t.bfloat16(),
                    **{k: (v.bfloat16() if v.is_floating_point() and "ids" not in k else v) for k, v in kw.items()})[0].float()
        plain32 = flux.oracle(hidden_states=x, timestep=t, **kw)[0]
    m = flux.make()
    plain = flux.run(m).clone()
    m.load_lora(la, adapter="a", scale=0.8)
    m.load_lora(lb, adapter="b", scale=-1.3)
    got = flux.run(m)
    e_hip, e_bf = rel_l2(got, ref32), rel_l2(refbf, ref32)
    print(f"flux lora vs fp32 oracle: e_hip {e_hip:.3e}, e_bf {e_bf:.3e}; adapters move the output by {rel_l2(got, plain):.3e} "
          f"(oracle: {rel_l2(ref32, plain32):.3e})")
    assert e_hip < 2 * e_bf + 1e-3, (e_hip, e_bf)
    assert e_hip < 2e-2, e_hip
    assert rel_l2(got, plain) > 1e-2, "the test would pass on ignored adapters"


# ----------------------------------------------------------------------------- 4. reversibility
def test_flux_unload_scale_zero_and_set_weight(flux):
    m = flux.make()
    before = flux.run(m).clone()
    la, lb = flux_loras(flux.sd)
    m.load_lora(la, adapter="a")
    m.load_lora(lb, adapter="b", scale=2.0)
    with_both = flux.run(m).clone()
    assert not same_bits(with_both, before)
    # scale 0 on every adapter: the base rows come back bit for bit (the copies stay: the adapters are still loaded)
    m.set_adapters(["a", "b"], [0.0, 0.0])
    assert same_bits(flux.run(m), before) and m.lora_info()["base_bytes"] > 0
    # only "a" active = a fresh engine with "a" alone
    m.set_adapters("a")
    only_a = flux.run(m).clone()
    assert same_bits(only_a, flux.run(flux.make(merged_state_dict(flux.sd, [(la, 1.0)]))))
    m.set_adapters(["a", "b"], [1.0, 2.0])
    assert same_bits(flux.run(m), with_both)
    # set_weight on a touched weight goes to the pristine copy: a forward is refused until the apply, which merges the new weight
    name = "transformer_blocks.0.attn.to_q.weight"
    new_w = (flux.sd[name] * 1.5).contiguous()
    m.engine.set_weight(name, new_w)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        flux.run(m)
    assert ex.value.status == ESTATE and "mc_mmdit_lora_apply" in str(ex.value)
    m.apply_lora()
    sd2 = dict(flux.sd, **{name: new_w})
    assert same_bits(flux.run(m), flux.run(flux.make(merged_state_dict(sd2, [(la, 1.0), (lb, 2.0)]))))
    # unload one, then all: the loaded weights again (with the new to_q), no copy left
    m.unload_lora("b")
    assert same_bits(flux.run(m), flux.run(flux.make(merged_state_dict(sd2, [(la, 1.0)]))))
    m.unload_lora()
    info = m.lora_info()
    assert info["adapters"] == 0 and info["linears"] == 0 and info["base_bytes"] == 0
    m.engine.set_weight(name, flux.sd[name])
    assert same_bits(flux.run(m), before)


# ----------------------------------------------------------------------------- 5. scale per call (FLUX shim)
def test_flux_joint_attention_kwargs_scale(flux, flux_lora_model):
    m, base_out, la, lb = flux_lora_model
    try:
        fresh_flux_magcache(m, flux.meta)                              # every call below is step 0 of a sample: a full forward
        at_one = flux.run(m).clone()
        fresh_flux_magcache(m, flux.meta)
        half = flux.run(m, joint_attention_kwargs={"scale": 0.5}).clone()
        assert m.lora_info()["call_scale"] == 0.5 and not same_bits(half, at_one)
        fresh_flux_magcache(m, flux.meta)
        assert same_bits(flux.run(m), at_one) and m.lora_info()["call_scale"] == 1.0     # without the key: back at scale 1
        m.set_adapters(["a", "b"], [0.5 * 1.0, 0.5 * 2.0])
        fresh_flux_magcache(m, flux.meta)
        assert same_bits(flux.run(m), half)
        assert m.cnt == 1
        # without adapters the key is ignored, as before
        plain = flux.make()
        assert same_bits(flux.run(plain, joint_attention_kwargs={"scale": 0.5}), base_out)
        assert plain.lora_info() == dict(adapters=0, linears=0, base_bytes=0, scales={}, call_scale=1.0)
    finally:
        m.set_adapters(["a", "b"], [1.0, 2.0])
        plain_flux(m)


# ----------------------------------------------------------------------------- 6. MagCache loop with an adapter loaded
def test_flux_magcache_loop_with_adapters_keeps_the_skip_pattern(flux, flux_lora_model):
    """the decision sequence depends on the table alone; the residual cache survives an apply in the middle of a sample (a skipped
    step follows it)"""
    m, base_out, la, lb = flux_lora_model
    g, meta = flux.g, flux.meta
    steps = meta["steps"]
    skipped = g["skipped"].tolist()
    change_at = next(i for i in range(1, steps) if skipped[i])        # the apply happens right before a skipped step
    fresh_flux_magcache(m, meta)
    cls = type(m)
    modes, base_run = [], cls.__mro__[1]._run

    def _run(self, *a):
        modes.append(a[-1])
        return base_run(self, *a)
    cls._run = _run
    try:
        x = dev(torch.from_numpy(g["latent0"]).clone())
        sig = g["sigmas"]
        kwd = {k: dev(v) for k, v in dict(flux.kw, guidance=torch.tensor([meta["guidance"]])).items()}
        for i in range(steps):
            extra = {}
            if i >= change_at:
                extra = dict(joint_attention_kwargs={"scale": 0.5})
            if i == change_at:
                kept = m.engine.residual().clone()
            o = m(hidden_states=x, timestep=torch.tensor([float(sig[i])], device=DEV), return_dict=False, **kwd, **extra)[0]
            if i == change_at:
                assert m.lora_info()["call_scale"] == 0.5 and same_bits(m.engine.residual(), kept)
            assert bool(torch.isfinite(o).all())
            x = x + float(sig[i + 1] - sig[i]) * o
        assert [int(mo == MM.MC_MODE_SKIP) for mo in modes] == skipped
        assert cls.cnt == 0
    finally:
        del cls._run
        plain_flux(m)
        m.engine.set_lora_call_scale(1.0)


# ----------------------------------------------------------------------------- 7. errors
def test_lora_errors_leave_the_engine_usable(flux):
    m = flux.make()
    e = m.engine
    before = flux.run(m).clone()
    sd = flux.sd
    good = lora_sd(sd, ["transformer_blocks.0.attn.to_q"], 4, seed=20)

    def status_of(lsd, **kw):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            m.load_lora(lsd, **kw)
        return ex.value.status, str(ex.value)
    # an unknown target; the fp32 GEMV matrix of the head; wrong row count of `up`; wrong in_features of `down`
    st, msg = status_of({"transformer.transformer_blocks.9.attn.to_q.lora_A.weight": torch.zeros(4, 256),
                         "transformer.transformer_blocks.9.attn.to_q.lora_B.weight": torch.zeros(256, 4)})
    assert st == EINVAL and "transformer_blocks.9.attn.to_q.weight" in msg
    st, msg = status_of(lora_sd(sd, ["proj_out"], 4, seed=21))
    assert st == EINVAL and "proj_out.weight" in msg
    bad_up = dict(good)
    bad_up["transformer.transformer_blocks.0.attn.to_q.lora_B.weight"] = torch.zeros(255, 4)
    st, msg = status_of(bad_up)
    assert st == EINVAL and "attn.to_q.weight" in msg
    bad_down = dict(good)
    bad_down["transformer.transformer_blocks.0.attn.to_q.lora_A.weight"] = torch.zeros(4, 128)
    assert status_of(bad_down)[0] == EINVAL
    # a strict load that fails half way leaves nothing behind
    st, msg = status_of(dict(good, **lora_sd(sd, ["proj_out"], 4, seed=22)))
    assert st == EINVAL and m.lora_info()["adapters"] == 0 and m.lora_info()["base_bytes"] == 0
    assert same_bits(flux.run(m), before)
    # strict=False skips what the engine refuses and says so
    mixed = dict(good, **lora_sd(sd, ["proj_out", "x_embedder"], 4, seed=23))
    skipped = m.load_lora(mixed, adapter="mixed", strict=False)
    assert skipped == ["proj_out.weight"]          # x_embedder is [dim, 64] here, unpadded: a plain bf16 Linear
    assert m.lora_info()["adapters"] == 1 and not same_bits(flux.run(m), before)
    # an unknown adapter name
    with pytest.raises(KeyError):
        m.set_adapters("nope")
    lib, h = e.lib, e.h
    assert lib.mc_mmdit_lora_scale(h, b"nope", 1.0) == EINVAL and lib.mc_mmdit_lora_remove(h, b"nope") == EINVAL
    # a change that waits for its apply refuses the forward; inside begin .. end every lora call is refused
    _lib.check(lib.mc_mmdit_lora_scale(h, b"mixed", 0.5))
    with pytest.raises(_lib.MagCacheHipError) as ex:
        flux.run(m)
    assert ex.value.status == ESTATE and "mc_mmdit_lora_apply" in str(ex.value)
    m.apply_lora()
    kw = flux.kw
    e.begin(dev(flux.x[0]), 500.0, 4000.0, dev(kw["encoder_hidden_states"][0]), flux.meta["txt_len"], dev(kw["pooled_projections"][0]),
            MM.MC_MODE_FULL)
    assert lib.mc_mmdit_lora_scale(h, b"mixed", 1.0) == ESTATE
    assert lib.mc_mmdit_lora_remove(h, None) == ESTATE
    assert lib.mc_mmdit_lora_apply(h, None) == ESTATE
    d = torch.zeros(4, 256, device=DEV)
    shape = (MM.C.c_int64 * 2)(4, 256)
    assert lib.mc_mmdit_lora_set(h, b"x", b"transformer_blocks.0.attn.to_q.weight", MM._ptr(d), shape, MM._ptr(d.t().contiguous()),
                                 (MM.C.c_int64 * 2)(256, 4), _lib.MC_F32, 1.0, None) == ESTATE
    for blk in range(e.n_blocks):
        e.block_pre(blk)
        e.block_post(blk)
    out = torch.empty(e.img_tokens, e.out_channels, device=DEV)
    e.end(out)
    torch.cuda.synchronize()
    m.unload_lora()
    assert same_bits(flux.run(m), before)
    # a padded image embedder takes no adapter (in_channels 16 -> K padded to 64); no weights needed to be told so
    small = MM.MMDiTEngine(_lib.MC_FAMILY_FLUX, 256, 2, 1, 1, 16, 16, 256, 64, 128, 64, device=DEV)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        small.load_lora({"x_embedder.lora_A.weight": torch.zeros(4, 16), "x_embedder.lora_B.weight": torch.zeros(256, 4)})
    assert ex.value.status == EINVAL and "x_embedder.weight" in str(ex.value)
    # every name lora_target_names lists is one the engine takes
    for name in lora_target_names("flux", 1, 1):
        st = small.lib.mc_mmdit_lora_set(small.h, b"t", name.encode(), MM._ptr(d), (MM.C.c_int64 * 2)(1, 4), MM._ptr(d),
                                         (MM.C.c_int64 * 2)(4, 1), _lib.MC_F32, 1.0, None)
        assert st == EINVAL and b"elements" in small.lib.mc_last_error(), (name, small.lib.mc_last_error())   # known and plain: only the counts are off

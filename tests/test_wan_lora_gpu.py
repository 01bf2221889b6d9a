"""GPU: LoRA adapters on the Wan engine (mc_lora_*; Engine / WanModelHIP.load_lora & co.), on tiny shapes.

The yardstick of most cases is BITWISE: an engine with adapters must equal an engine that was given, through plain set_weight,
the weights the merge ops (mc_op_lora_merge, mc_op_lora_merge_f32, mc_op_param_delta) build from the same operands on the
host's side -- outputs, captured residuals and skipped forwards.  One case holds the merged engine to the fp32 oracle run on
W + dW, with the tolerance test_forward_vs_oracle uses, which the adapter-free engine must miss."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd import model as M  # noqa: E402
from magcache_amd.engine import MC_MODE_FULL, MC_MODE_SKIP, Engine, synthetic_weights  # noqa: E402
from magcache_amd.lora import lora_factor  # noqa: E402
from oracle import wan_dit_ref as W  # noqa: E402

DEV = "cuda:0"
GRID = (2, 16, 16)
L = GRID[0] * (GRID[1] // 2) * (GRID[2] // 2)
EINVAL, ESTATE = _lib.MC_EINVAL, _lib.MC_ESTATE
CFG = W.tiny_config(num_layers=2, num_heads=2, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64)
CFG_I2V = W.tiny_config(num_layers=2, num_heads=2, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64, i2v=True)
CFG_VACE = dict(W.tiny_config(num_layers=3), model_type="vace", vace_layers=[0, 2], vace_in_dim=16)

PAIRS = ["blocks.0.self_attn.q", "blocks.0.self_attn.k", "blocks.0.self_attn.v", "blocks.0.self_attn.o",
         "blocks.1.cross_attn.q", "blocks.1.cross_attn.k", "blocks.1.cross_attn.v", "blocks.1.cross_attn.o",
         "blocks.0.ffn.0", "blocks.1.ffn.2", "text_embedding.0",
         "time_embedding.0", "time_projection.1", "head.head"]                       # the last three are fp32 matrices
DELTAS = ["blocks.0.self_attn.q.bias", "blocks.1.self_attn.norm_q.weight", "blocks.0.modulation", "head.modulation"]


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().clone().contiguous().view(torch.int32).cpu()


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _weights(cfg_json):
    cfg = json.loads(cfg_json)
    return {n: t for n, t in synthetic_weights(cfg, seed=0, std=0.05, device=DEV)}


def weights(cfg):
    return dict(_weights(json.dumps(cfg, sort_keys=True)))


def adapter(wd, pairs, deltas, rank, alpha, seed, std=0.1, delta_std=0.05):
    """{target: ("pair", down, up, alpha) | ("delta", tensor)} with bf16-representable fp32 values, as adapter files carry"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for module in pairs:
        w = wd[module + ".weight"]
        rows, k = w.shape[0], w.numel() // w.shape[0]
        down = (torch.randn(rank, k, generator=g, device=DEV) * std).bfloat16().float()
        up = (torch.randn(rows, rank, generator=g, device=DEV) * std).bfloat16().float()
        out[module + ".weight"] = ("pair", down, up, alpha)
    for name in deltas:
        out[name] = ("delta", torch.randn(wd[name].shape, generator=g, device=DEV) * delta_std)
    return out


def as_state_dict(entries, prefix="diffusion_model."):
    """the entries as a ComfyUI-style adapter file spells them"""
    sd = {}
    for target, e in entries.items():
        if e[0] == "pair":
            module = target[:-len(".weight")]
            sd[prefix + module + ".lora_down.weight"], sd[prefix + module + ".lora_up.weight"] = e[1], e[2]
            if e[3] is not None:
                sd[prefix + module + ".alpha"] = torch.tensor(float(e[3]))
        elif target.endswith(".modulation"):
            sd[prefix + target[:-len(".modulation")] + ".diff_m"] = e[1]
        elif target.endswith(".bias"):
            sd[prefix + target[:-len(".bias")] + ".diff_b"] = e[1]
        else:
            sd[prefix + target[:-len(".weight")] + ".diff"] = e[1]
    return sd


FP32_MATRICES = ("time_embedding.0.weight", "time_embedding.2.weight", "time_projection.1.weight", "head.head.weight")


def host_merged(wd, loras):
    """wd with every touched parameter rebuilt by the merge ops: loras = [(entries, scale)] in load order.  bf16 matrices come
    back as bf16 (what the engine keeps), fp32 parameters as fp32."""
    lib = _lib.load()
    out = dict(wd)
    for target in {t for entries, _ in loras for t in entries if t in wd}:
        w = wd[target]
        terms, dl, ds, keep = [], [], [], []
        for entries, scale in loras:
            e = entries.get(target)
            if e is None:
                continue
            if e[0] == "pair":
                d, u = e[1].bfloat16().contiguous(), e[2].bfloat16().contiguous()
                keep += [d, u]
                terms.append(_lib.McLoraTerm(d.data_ptr(), u.data_ptr(), d.shape[0],
                                             float(np.float32(scale) * np.float32(lora_factor(e[1], e[3])))))
            else:
                dl.append(e[1].float().contiguous())
                ds.append(float(scale))
        if terms:
            rows, k = w.shape[0], w.numel() // w.shape[0]
            arr = (_lib.McLoraTerm * len(terms))(*terms)
            if target in FP32_MATRICES:
                new = w.float().clone().contiguous()
                _lib.check(lib.mc_op_lora_merge_f32(ptr(new), k, ptr(new), k, rows, k, arr, len(terms), None, 0, stream()))
            else:
                new = w.bfloat16().contiguous()
                _lib.check(lib.mc_op_lora_merge(ptr(new), k, ptr(new), k, rows, k, arr, len(terms), None, 0, stream()))
        else:
            new = w.float().clone().contiguous()
        if dl:
            pa = (C.c_void_p * len(dl))(*[d.data_ptr() for d in dl])
            _lib.check(lib.mc_op_param_delta(ptr(new), ptr(new), new.numel(), pa, (C.c_float * len(ds))(*ds), len(dl), stream()))
        torch.cuda.synchronize()
        out[target] = new
    return out


def make_engine(cfg, wd, grid=GRID):
    e = Engine(cfg, grid, device=DEV, n_branches=2, calibration=True)
    e.load_weights(wd)
    return e


def load(e, entries, name, scale=1.0, **kw):
    return e.load_lora(as_state_dict(entries), adapter=name, scale=scale, **kw)


@functools.lru_cache(maxsize=None)
def inputs(in_dim=16, text_dim=128):
    g = torch.Generator(device=DEV).manual_seed(11)
    lat = torch.randn(in_dim, *GRID, generator=g, device=DEV)
    ctx = [torch.randn(n, text_dim, generator=g, device=DEV) for n in (64, 37)]
    return lat, ctx


def trace(e, cached=False):
    """FULL forwards of both branches, their residual slots, SKIP forwards on another latent"""
    lat, ctx = inputs(e.cfg["in_dim"], e.cfg["text_dim"])
    t = torch.tensor([640.0], device=DEV)
    if cached:
        for b in (0, 1):
            e.set_context(b, ctx[b])
    seen = []
    for mode, x in ((MC_MODE_FULL, lat), (MC_MODE_SKIP, lat * 0.9 + 0.05)):
        for b in (0, 1):
            if cached:
                e.use_context(b)
            seen.append(bits(e.forward(x, t, None if cached else ctx[b], branch=b, mode=mode)))
        seen += [bits(e.residual(b)) for b in (0, 1)]
    return seen


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: item {i} differs in {int((a != b).sum())} of {a.numel()} words"


def two_adapters(wd, pairs=PAIRS, deltas=DELTAS):
    a = adapter(wd, pairs, deltas, rank=4, alpha=8.0, seed=1)
    b = adapter(wd, pairs[::2] + ["time_embedding.2"], deltas[1:] + ["time_embedding.0.weight"], rank=17, alpha=None, seed=2, std=0.06)
    return a, b


# ---------------------------------------------------------------------------------------------------- 1, 5
@pytest.mark.parametrize("fp8", [0, 1, 2], ids=["bf16", "fp8_rows", "fp8_mx"])
def test_adapters_equal_host_merged_weights_bitwise(fp8):
    """two adapters at different scales, pairs on bf16 and fp32 matrices, deltas on a fused bias, a norm weight and both
    modulation tables; FULL and SKIP forwards and the captured residuals.  With fp8_linear the equality shows that the rows
    an adapter touched were requantised."""
    cfg = CFG if not fp8 else dict(W.tiny_config(num_layers=2, num_heads=4, ffn_dim=512, text_len=64, text_dim=128, freq_dim=64),
                                   fp8_linear=fp8)
    wd = weights(cfg)
    a, b = two_adapters(wd)
    A = make_engine(cfg, wd)
    plain = trace(A)
    assert load(A, a, "a", 0.8) == [] and load(A, b, "b", -1.3) == []
    info = A.lora_info()
    assert info["adapters"] == 2 and info["base_bytes"] > 0
    got = trace(A)
    B = make_engine(cfg, host_merged(wd, [(a, 0.8), (b, -1.3)]))
    assert_same(got, trace(B), f"adapters vs host-merged weights (fp8_linear {fp8})")
    assert not torch.equal(got[0], plain[0])
    # the cached-context path reads the merged cross-attention K|V too
    assert_same(trace(A, cached=True), got, "cached contexts after the merge")
    # unloaded: every touched parameter (and its quantised rows) is the loaded one again, and the copies are gone
    A.unload_lora()
    assert_same(trace(A), plain, "after unload_lora")
    info = A.lora_info()
    assert info["adapters"] == 0 and info["linears"] == 0 and info["base_bytes"] == 0


# ---------------------------------------------------------------------------------------------------- 2
def test_adapters_against_the_fp32_oracle():
    oracle = W.init_synthetic_(W.WanModel(**CFG), seed=0, std=0.05)
    sd = {k: v.clone() for k, v in oracle.state_dict().items()}
    wd = {k: v.to(DEV) for k, v in sd.items()}
    a, b = two_adapters(wd)
    scales = (0.8, -1.3)
    merged = dict(sd)
    for entries, s in zip((a, b), scales):
        for target, e in entries.items():
            if e[0] == "pair":
                dw = s * lora_factor(e[1], e[3]) * (e[2].double() @ e[1].double())
            else:
                dw = s * e[1].double()
            merged[target] = (merged[target].double() + dw.cpu().reshape(merged[target].shape)).float()
    oracle.load_state_dict(merged)
    g = torch.Generator().manual_seed(3)
    lat, ctx = torch.randn(16, *GRID, generator=g), torch.randn(21, CFG["text_dim"], generator=g)
    t = torch.tensor([500.0])
    ref_ac = oracle.forward([lat], t, [ctx], L, autocast=True)[0]
    oracle.set_fp32_attention(True)
    ref_32 = oracle.forward([lat], t, [ctx], L, autocast=False)[0]
    oracle.set_fp32_attention(False)
    e = make_engine(CFG, wd)
    tt = torch.tensor([500.0], device=DEV)
    free = e.forward(lat.to(DEV), tt, ctx.to(DEV)).clone()
    load(e, a, "a", scales[0])
    load(e, b, "b", scales[1])
    got = e.forward(lat.to(DEV), tt, ctx.to(DEV))
    e_hip, e_ac, e_free = rel_l2(got, ref_32), rel_l2(ref_ac, ref_32), rel_l2(free, ref_32)
    print(f"adapters vs fp32 oracle on W + dW: engine {e_hip:.3e}, autocast oracle {e_ac:.3e}, adapter-free engine {e_free:.3e}; "
          f"engine vs autocast oracle {rel_l2(got, ref_ac):.3e}")
    assert e_hip < 2 * e_ac + 1e-3, (e_hip, e_ac)                     # test_forward_vs_oracle's bars
    assert rel_l2(got, ref_ac) < 2e-2
    assert e_free >= 2 * e_ac + 1e-3 and rel_l2(free, ref_ac) >= 2e-2, "a no-op merge would pass: the adapters are too small"


# ---------------------------------------------------------------------------------------------------- 3
def _model(cfg, wd, forward=M.plain_forward):
    cls = type("WanModelHIPLora", (M.WanModelHIP,), {"forward": forward})
    m = cls(cfg, GRID, device=DEV, calibration=False)
    m.engine.load_weights(wd)
    return m


def test_stale_text_context_is_refused_and_uploaded_again():
    wd = weights(CFG)
    a = adapter(wd, ["blocks.0.cross_attn.k", "text_embedding.2"], [], rank=4, alpha=None, seed=5)
    lat, ctx = inputs()
    t = torch.tensor([300.0], device=DEV)
    m = _model(CFG, wd)
    before = bits(m([lat], t=t, context=[ctx[0]], seq_len=L)[0])
    assert m._ctx_keys[0] is not None
    m.load_lora(as_state_dict(a), adapter="a")
    assert m._ctx_keys == [None, None]
    with pytest.raises(_lib.MagCacheHipError) as ex:                  # the engine's slot went with the merge
        m.engine.use_context(0)
    assert ex.value.status == ESTATE
    with pytest.raises(_lib.MagCacheHipError) as ex:
        m.engine.forward(lat, t, None)
    assert ex.value.status == ESTATE and "context" in str(ex.value)
    got = bits(m([lat], t=t, context=[ctx[0]], seq_len=L)[0])          # the shim uploads again on its own
    fresh = _model(CFG, host_merged(wd, [(a, 1.0)]))
    assert torch.equal(got, bits(fresh([lat], t=t, context=[ctx[0]], seq_len=L)[0])) and not torch.equal(got, before)


def test_stale_clip_context_is_refused_and_uploaded_again():
    wd = weights(CFG_I2V)
    a = adapter(wd, ["img_emb.proj.1", "blocks.1.cross_attn.k_img"], [], rank=4, alpha=None, seed=6)
    g = torch.Generator(device=DEV).manual_seed(12)
    lat, y = torch.randn(16, *GRID, generator=g, device=DEV), torch.randn(20, *GRID, generator=g, device=DEV)
    clip = torch.randn(257, CFG_I2V["clip_dim"], generator=g, device=DEV)
    ctx = torch.randn(40, CFG_I2V["text_dim"], generator=g, device=DEV)
    t = torch.tensor([300.0], device=DEV)
    kw = dict(t=t, context=[ctx], seq_len=L, clip_fea=clip, y=[y])
    m = _model(CFG_I2V, wd)
    before = bits(m([lat], **kw)[0])
    m.load_lora(as_state_dict(a), adapter="a")
    assert m._clip_key is None
    with pytest.raises(_lib.MagCacheHipError) as ex:
        m.engine.forward(torch.cat([lat, y]), t, ctx)
    assert ex.value.status == ESTATE and "mc_set_clip_fea" in str(ex.value)
    got = bits(m([lat], **kw)[0])
    fresh = _model(CFG_I2V, host_merged(wd, [(a, 1.0)]))
    assert torch.equal(got, bits(fresh([lat], **kw)[0])) and not torch.equal(got, before)


def test_stale_vace_context_is_refused_and_uploaded_again():
    wd = weights(CFG_VACE)
    a = adapter(wd, ["vace_blocks.0.before_proj", "vace_blocks.1.after_proj"], [], rank=4, alpha=None, seed=7)
    g = torch.Generator(device=DEV).manual_seed(13)
    lat = torch.randn(16, *GRID, generator=g, device=DEV)
    vace = torch.randn(CFG_VACE["vace_in_dim"], *GRID, generator=g, device=DEV)
    ctx = torch.randn(40, CFG_VACE["text_dim"], generator=g, device=DEV)
    t = torch.tensor([300.0], device=DEV)
    kw = dict(t=t, vace_context=[vace], context=[ctx], seq_len=L, vace_context_scale=0.75)
    m = _model(CFG_VACE, wd, forward=M.vace_plain_forward)
    before = bits(m([lat], **kw)[0])
    m.load_lora(as_state_dict(a), adapter="a")
    assert m._vace_key is None
    with pytest.raises(_lib.MagCacheHipError) as ex:
        m.engine.forward(lat, t, ctx)
    assert ex.value.status == ESTATE and "mc_set_vace_context" in str(ex.value)
    got = bits(m([lat], **kw)[0])
    fresh = _model(CFG_VACE, host_merged(wd, [(a, 1.0)]), forward=M.vace_plain_forward)
    assert torch.equal(got, bits(fresh([lat], **kw)[0])) and not torch.equal(got, before)


def test_pair_front_is_not_continued_across_a_merge():
    """a declared CFG pair before and after a merge: the adapter calls are refused inside the pair (the kept front stays what
    it is), and the pair after the merge equals the pair of an engine built with the merged weights"""
    wd = weights(CFG)
    a = adapter(wd, ["blocks.0.self_attn.q", "time_embedding.0"], ["blocks.0.modulation"], rank=4, alpha=None, seed=8)
    lat, ctx = inputs()
    t = torch.tensor([450.0], device=DEV)

    def pair(e):
        e.pair_begin()
        out = [bits(e.forward(lat, t, ctx[b], branch=b)) for b in (0, 1)]
        e.pair_end()
        return out
    e = make_engine(CFG, wd)
    e.pair_begin()
    first = bits(e.forward(lat, t, ctx[0], branch=0))                  # the front is kept now
    name, entry = next(iter(a.items()))
    assert e._lora_set("a", name, entry) == ESTATE and b"mc_pair_begin" in e.lib.mc_last_error()
    assert e.lib.mc_lora_apply(e.h, stream()) == ESTATE
    second = bits(e.forward(lat, t, ctx[1], branch=1))
    e.pair_end()
    load(e, a, "a")
    fresh = make_engine(CFG, host_merged(wd, [(a, 1.0)]))
    want = pair(fresh)
    assert_same(pair(e), want, "the pair after the merge")
    assert not torch.equal(first, want[0]) and not torch.equal(second, want[1])


# ---------------------------------------------------------------------------------------------------- 4
def test_unload_scale_zero_set_adapters_and_set_weight():
    wd = weights(CFG)
    a, b = two_adapters(wd)
    e = make_engine(CFG, wd)
    plain = trace(e)
    load(e, a, "a", 0.8)
    load(e, b, "b", -1.3)
    both = trace(e)
    e.set_adapters("a", 0.8)                                           # b off, its terms kept
    only_a = trace(e)
    assert_same(only_a, trace(make_engine(CFG, host_merged(wd, [(a, 0.8)]))), "set_adapters('a')")
    e.set_adapters(["a", "b"], [0.0, 0.0])                             # scale 0 equals unloaded
    assert_same(trace(e), plain, "both adapters at scale 0")
    e.set_adapters(["a", "b"], [0.8, -1.3])
    assert_same(trace(e), both, "both adapters back")
    # set_weight on a touched fp32 matrix (and a touched fp32 vector) lands in the base; the live values follow the apply
    new_w = wd["time_embedding.0.weight"] * 1.5
    new_m = wd["blocks.0.modulation"] + 0.01
    e.set_weight("time_embedding.0.weight", new_w)
    e.set_weight("blocks.0.modulation", new_m)
    with pytest.raises(_lib.MagCacheHipError) as ex:
        trace(e)
    assert ex.value.status == ESTATE and "mc_lora_apply" in str(ex.value)
    e.apply_lora()
    wd2 = dict(wd, **{"time_embedding.0.weight": new_w, "blocks.0.modulation": new_m})
    assert_same(trace(e), trace(make_engine(CFG, host_merged(wd2, [(a, 0.8), (b, -1.3)]))), "set_weight into the base")
    e.unload_lora("b")
    assert_same(trace(e), trace(make_engine(CFG, host_merged(wd2, [(a, 0.8)]))), "unload_lora('b')")
    e.unload_lora()
    assert_same(trace(e), trace(make_engine(CFG, wd2)), "unload_lora()")
    info = e.lora_info()
    assert info["adapters"] == 0 and info["linears"] == 0 and info["base_bytes"] == 0


# ---------------------------------------------------------------------------------------------------- 6
def test_captured_forward_stays_valid_and_launch_counts_do_not_change():
    wd = weights(CFG)
    a, _ = two_adapters(wd)
    e = make_engine(CFG, wd)
    lat, ctx = inputs()
    x = lat.clone()
    t = torch.tensor([700.0], device=DEV)
    e.set_context(0, ctx[0])
    out = torch.empty_like(e.forward(x, t, None, 0, MC_MODE_FULL))      # warm-up
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        e.forward(x, t, None, 0, MC_MODE_FULL, out=out)

    def counts():
        e.profile(2)
        e.forward(x, t, None, 0, MC_MODE_FULL)
        n = {k: v[1] for k, v in e.profile_read_classes().items()}
        e.profile(0)
        return n
    without = counts()
    load(e, a, "a", 0.8)
    e.set_context(0, ctx[0])                                            # outside the graph: the merge invalidated the slot
    x.copy_(lat * 0.5 + 0.1)
    t.fill_(333.0)
    gr.replay()
    torch.cuda.synchronize()
    replayed = bits(out)
    eager = bits(e.forward(x, t, None, 0, MC_MODE_FULL))
    assert torch.equal(replayed, eager)
    B = make_engine(CFG, host_merged(wd, [(a, 0.8)]))
    assert torch.equal(eager, bits(B.forward(x, t, ctx[0], 0, MC_MODE_FULL)))
    assert counts() == without and sum(without.values()) > 0


# ---------------------------------------------------------------------------------------------------- 7
def test_errors_leave_the_engine_usable():
    wd = weights(CFG)
    a = adapter(wd, ["blocks.0.self_attn.q", "head.head"], ["blocks.0.modulation"], rank=4, alpha=None, seed=9)
    e = make_engine(CFG, wd)
    load(e, a, "a")
    want = trace(make_engine(CFG, host_merged(wd, [(a, 1.0)])))
    assert_same(trace(e), want, "before the errors")
    d = wd["blocks.0.self_attn.q.weight"].shape[0]
    pair = lambda rows, k, r=4: ("pair", torch.zeros(r, k, device=DEV), torch.zeros(rows, r, device=DEV), None)   # noqa: E731
    cases = [("no.such.weight", pair(d, d), "unknown"),
             ("patch_embedding.weight", pair(d, 64), "patch_embedding.weight"),
             ("blocks.0.self_attn.q.weight", ("delta", torch.zeros(d, d, device=DEV)), "blocks.0.self_attn.q.weight"),   # a delta on a bf16 matrix
             ("blocks.0.self_attn.q.weight", pair(d, d + 8), "elements"),
             ("time_embedding.0.weight", pair(d + 1, CFG["freq_dim"]), "elements"),
             ("blocks.0.modulation", ("delta", torch.zeros(5 * d, device=DEV)), "elements"),
             ("blocks.0.modulation", pair(6, d), "blocks.0.modulation")]       # a pair on a table that is no matrix
    for target, entry, word in cases:
        assert e._lora_set("x", target, entry) == EINVAL, target
        assert word in e.lib.mc_last_error().decode(), (target, e.lib.mc_last_error())
        assert_same(trace(e), want, f"after the refusal on {target}")
    # strict loading leaves the engine as before; strict=False skips and names what it skipped
    bad = dict(as_state_dict(adapter(wd, ["blocks.1.ffn.0"], [], rank=4, alpha=None, seed=10)),
               **{"diffusion_model.blocks.1.self_attn.v.diff": torch.zeros(d, d)})
    with pytest.raises(_lib.MagCacheHipError):
        e.load_lora(bad, adapter="bad")
    assert e.lora_info()["adapters"] == 1
    assert_same(trace(e), want, "after a failed strict load")
    assert e.load_lora(bad, adapter="bad", strict=False, scale=0.0) == ["blocks.1.self_attn.v.weight"]
    e.unload_lora("bad")
    # a ninth adapter on one slot, for pairs and for deltas
    for i in range(_lib.MC_LORA_MAX_TERMS - 1):
        assert e._lora_set(f"n{i}", "head.head.weight", a["head.head.weight"]) == _lib.MC_OK
        assert e._lora_set(f"n{i}", "blocks.0.modulation", a["blocks.0.modulation"]) == _lib.MC_OK
    assert e._lora_set("ninth", "head.head.weight", a["head.head.weight"]) == EINVAL
    assert e._lora_set("ninth", "blocks.0.modulation", a["blocks.0.modulation"]) == EINVAL
    # a change that waits for its apply
    lat, ctx = inputs()
    for call in (lambda: e.forward(lat, 500.0, ctx[0]), lambda: e.set_context(0, ctx[0])):
        with pytest.raises(_lib.MagCacheHipError) as ex:
            call()
        assert ex.value.status == ESTATE and "mc_lora_apply" in str(ex.value)
    for i in range(_lib.MC_LORA_MAX_TERMS - 1):
        _lib.check(e.lib.mc_lora_remove(e.h, f"n{i}".encode()))
    e.apply_lora()
    assert_same(trace(e), want, "after the pending change was taken back and applied")


# ---------------------------------------------------------------------------------------------------- 8
def test_mmdit_engine_still_refuses_its_fp32_head():
    small = MM.MMDiTEngine(_lib.MC_FAMILY_FLUX, 256, 2, 1, 1, 16, 16, 256, 64, 128, 64, device=DEV)
    down, up = torch.zeros(4, 256, device=DEV), torch.zeros(64, 4, device=DEV)
    st = small.lib.mc_mmdit_lora_set(small.h, b"a", b"proj_out.weight", ptr(down), (C.c_int64 * 2)(*down.shape), ptr(up),
                                     (C.c_int64 * 2)(*up.shape), _lib.MC_F32, 1.0, stream())
    assert st == EINVAL and b"proj_out.weight" in small.lib.mc_last_error()
    assert small.lora_info()["adapters"] == 0


# ---------------------------------------------------------------------------------------------------- 9
def test_generate_lora_file_flag(tmp_path, monkeypatch):
    """python -m magcache_amd.generate --lora_file PATH:SCALE (5 frames, 4 steps): differs from the run without the flag and
    equals the run whose weights were merged on the host's side with the merge ops"""
    from safetensors.torch import save_file
    from magcache_amd import engine as E
    from magcache_amd import generate as G
    cfg = E.WAN_T2V_1_3B
    shapes = dict(E.weight_names(cfg))
    stand_in = {n: torch.empty(shapes[n], device="meta") for n in
                ("blocks.0.self_attn.q.weight", "blocks.29.ffn.2.weight", "time_projection.1.weight", "head.head.weight",
                 "blocks.3.modulation", "blocks.0.cross_attn.k.bias")}
    a = adapter(stand_in, ["blocks.0.self_attn.q", "blocks.29.ffn.2", "time_projection.1", "head.head"],
                ["blocks.3.modulation", "blocks.0.cross_attn.k.bias"], rank=8, alpha=16.0, seed=21, std=0.05, delta_std=0.02)
    path = tmp_path / "style.safetensors"
    save_file({k: v.cpu().contiguous() for k, v in as_state_dict(a).items()}, str(path))
    common = ["--task", "t2v-1.3B", "--size", "832*480", "--frame_num", "5", "--sample_steps", "4", "--base_seed", "42",
              "--sample_solver", "euler", "--prompt", "a cat boxing"]

    def run(extra, name):
        try:
            return G.generate(G._parse_args(common + extra + ["--save_file", str(tmp_path / name)])).cpu()
        finally:
            M.WanModelHIP.forward = M.plain_forward
    plain = run([], "plain.pt")
    with_lora = run(["--lora_file", f"{path}:0.5"], "lora.pt")
    original = E.synthetic_weights

    def merged_weights(cfg_, **kw):
        for name, t in original(cfg_, **kw):
            yield name, (host_merged({name: t}, [(a, 0.5)])[name] if name in a else t)
    monkeypatch.setattr(E, "synthetic_weights", merged_weights)
    host = run([], "host.pt")
    assert bool(torch.isfinite(with_lora).all()) and not torch.equal(with_lora, plain)
    assert torch.equal(with_lora, host)
    assert G._lora_spec("/a/b.safetensors") == ("/a/b.safetensors", 1.0) and G._lora_spec("x:y/z.safetensors:-2") == ("x:y/z.safetensors", -2.0)

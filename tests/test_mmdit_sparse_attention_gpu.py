"""GPU: tile-sparse joint attention on the MM-DiT engine (mc_mmdit_set_attention_tile_mask / _mass; csrc/attention_joint.hip).
Toy FLUX ([text ; image], 64 + 288 rows) and toy HunyuanVideo ([image ; text], 324 + 32 rows of which 23 text rows are valid: the
boundary row 324 lies inside query tile 2 and key tile 5), both 4 x 8 tiles.  The oracle runs the same element mask -- the rule
of include/magcache_mmdit.h -- in its joint SDPA, from the first sparse block on.
Predicted mode runs at mass 0.5, as on the Wan engine: the toy weights give near-flat pooled attention, and the test asserts that
the density of the mask read back is strictly between 0 and 1 (measured: 0.556 over the valid tiles in both families; static masks:
e_hip 4.5e-3 .. 4.6e-3 against e_bf 8.1e-3 .. 8.4e-3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_cases as A  # noqa: E402
import hip_ops as H  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd import mmdit as MM  # noqa: E402
from magcache_amd.sparse_masks import pack_tile_mask  # noqa: E402
from oracle import flux_ref as FR  # noqa: E402
from oracle import hunyuan_ref as HR  # noqa: E402
from test_mmdit_geometry_gpu import DEV, FULL, Flux, Hunyuan, Qwen, flux_calls, fwd, hunyuan_calls  # noqa: E402

MASS = 0.5
SCALE = float(torch.tensor(1.0) / torch.sqrt(torch.tensor(128.0)))      # the engine's kAttnScale
# family: (helper class, geometry, shim class, calls, oracle module, oracle class, seed, rows: S, valid keys, txt0, Lt, valid text, blocks)
FAMS = {"flux": (Flux, (288, 64), MM.FluxTransformer2DModelHIP, flux_calls, FR, "FluxTransformer2DModel", 3, (352, 352, 0, 64, 64, 4)),
        "hunyuan": (Hunyuan, ((6, 12, 18), 32), MM.HYVideoDiffusionTransformerHIP, hunyuan_calls, HR, "HYVideoDiffusionTransformer", 4,
                    (356, 347, 324, 32, 23, 3))}


def make_mask(mh, ones=False):
    """bool [mh, 4, 8]: a seeded random half of the tiles, another per head, the diagonal forced"""
    m = torch.rand(mh, 4, 8, generator=torch.Generator().manual_seed(7)) < 0.5
    return m | (torch.arange(8)[None, :] // 2 == torch.arange(4)[:, None]) | ones


def element_mask(fam, mask):
    """the rule on elements: bool [mh, valid, valid]"""
    S, valid, txt0, lt, tv, _ = FAMS[fam][7]
    i = torch.arange(512)
    qdense = (i // 128 >= txt0 // 128) & (i // 128 < (txt0 + lt + 127) // 128)
    kalways = (i // 64 >= txt0 // 64) & (i // 64 < (txt0 + tv + 63) // 64)
    return (mask[:, i // 128][:, :, i // 64] | qdense[None, :, None] | kalways[None, None, :])[:, :valid, :valid]


class MaskedF:
    """torch.nn.functional for an oracle module, its joint SDPA under an element mask from joint call `first` on (one joint call
    per block, in forward order; the HunyuanVideo token refiner's shorter SDPA passes through)"""
    def __init__(self, elem, first):
        self.elem, self.first, self.calls = elem, first, 0

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def scaled_dot_product_attention(self, q, k, v):
        joint = q.shape[-2] == self.elem.shape[-1]
        self.calls += int(joint)
        masked = joint and self.calls > self.first
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=self.elem[None] if masked else None)


def oracle_out(fam, call, bf16, monkeypatch, elem, first):
    _, _, _, _, mod, cls, seed, _ = FAMS[fam]
    model = mod.init_synthetic_(getattr(mod, cls)(**FAMS[fam][0].cfg), seed=seed, std=0.05)
    kw = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in call.items()}
    if bf16:
        model = model.bfloat16()
        keep = ("img_ids", "txt_ids", "text_mask", "freqs_cos", "freqs_sin", "t", "guidance") if fam == "hunyuan" else ("img_ids", "txt_ids")
        kw = {k: (v.bfloat16() if torch.is_tensor(v) and v.is_floating_point() and k not in keep else v) for k, v in kw.items()}
    monkeypatch.setattr(mod, "F", MaskedF(elem, first))
    with torch.no_grad():
        return model(**kw)[0].float()


def shim(fam, **kw):
    helper, geo, cls = FAMS[fam][:3]
    m = type(cls.__name__ + "Sparse", (cls,), {})(helper.cfg, geo[0], txt_len=geo[1], device=DEV, calibration=False, **kw)
    return m.load_state_dict(helper.sd())


def engine(fam, **kw):
    helper, geo = FAMS[fam][:2]
    e = helper.engine(geo, **kw)
    inp = helper.inputs(geo)
    e.set_rope(*inp.rope)
    return e, inp


@pytest.mark.parametrize("mh,dense_blocks", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("fam", list(FAMS))
def test_engine_vs_masked_oracle(fam, mh, dense_blocks, monkeypatch):
    mask, call = make_mask(mh), FAMS[fam][3](FAMS[fam][1])[1]
    m = shim(fam, attention_tile_mask=lambda nqt, nkt, geo: make_mask(mh)[:, :nqt, :nkt], sparse_dense_blocks=dense_blocks)
    st = m.engine.attention_tile_state
    assert (st["mode"], st["mask_heads"], st["nqt"], st["nkt"], st["dense_blocks"]) == ("static", mh, 4, 8, dense_blocks)
    assert 0 < st["density"] < 1
    got, elem = m(**call)[0].cpu(), element_mask(fam, mask)
    ref_32 = oracle_out(fam, call, False, monkeypatch, elem, dense_blocks)
    e_hip, e_bf = A.rel_l2(got, ref_32), A.rel_l2(oracle_out(fam, call, True, monkeypatch, elem, dense_blocks), ref_32)
    print(f"{fam} density {st['density']:.3f}: e_hip {e_hip:.3e} e_bf {e_bf:.3e}")
    assert e_hip < 2 * e_bf + 1e-3 and e_hip < 2e-2, (e_hip, e_bf)


@pytest.mark.parametrize("fam", list(FAMS))
def test_ones_off_and_dense_blocks_are_the_dense_engine(fam):
    never, inp = engine(fam)
    want, (e, _) = fwd(never, inp, FULL), engine(fam)
    e.set_attention_tile_mask(make_mask(2))
    assert not torch.equal(fwd(e, inp, FULL), want)
    e.set_attention_tile_mask(make_mask(1, ones=True))       # all bits set: plain attention, another kernel's summation order
    A.accept(fwd(e, inp, FULL), want.double())
    e.set_attention_tile_mask(make_mask(2), dense_blocks=FAMS[fam][7][5])   # every block stays dense
    assert torch.equal(fwd(e, inp, FULL), want)
    e.set_attention_tile_mask(None)
    assert e.attention_tile_state is None and torch.equal(fwd(e, inp, FULL), want)


@pytest.mark.parametrize("fam", list(FAMS))
def test_predicted_mask_is_the_predictors_and_replays_as_a_static_mask(fam):
    """only the last block sparse, so that one mask describes the forward"""
    S, valid, _, _, _, nb = FAMS[fam][7]
    e, inp = engine(fam)
    e.set_attention_tile_mass(MASS, dense_blocks=nb - 1)
    st = e.attention_tile_state
    assert st["mode"] == "predicted" and st["mass"] == pytest.approx(MASS) and st["density"] is None and st["mask_heads"] == 2
    out = torch.empty_like(fwd(e, inp, FULL))
    e.begin(inp.img, 500.0, inp.guidance, inp.txt[0], inp.valid[0], inp.vec, FULL)
    for blk in range(nb):
        e.block_pre(blk)
        if blk == nb - 1:
            qkv = e.buffer("qkv", torch.bfloat16)[:512 * 768].view(512, 768).clone()
        e.block_post(blk)
    e.end(out)
    torch.cuda.synchronize()
    mask = e.read_attention_tile_mask()
    assert mask.shape == (2, 4, 8) and 0.0 < float(mask[:, :(S + 127) // 128, :(valid + 63) // 64].double().mean()) < 1.0
    bits = torch.zeros(2, 4, 1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(H.L().mc_op_attention_tile_predict_scratch(512, 2, 512), dtype=torch.uint8, device=DEV)
    k = qkv[:, 256:]
    _lib.check(H.L().mc_op_attention_tile_predict(H.P(qkv), qkv.stride(0), H.P(k), k.stride(0), 512, 2, 512, valid, SCALE, MASS,
                                                  H.P(bits), H.P(scratch), H.S()))
    torch.cuda.synchronize()
    assert torch.equal(bits.cpu(), pack_tile_mask(mask))
    e.set_attention_tile_mass(0)
    e.set_attention_tile_mask(mask, dense_blocks=nb - 1)
    assert torch.equal(fwd(e, inp, FULL), out)


@pytest.mark.parametrize("what,status,names", [
    ("sequence parallel", _lib.MC_EINVAL, "sequence parallel"), ("wrong sizes", _lib.MC_EINVAL, "4 x 8"),
    ("mass 1.5", _lib.MC_EINVAL, "mass"), ("dense -1", _lib.MC_EINVAL, "dense_blocks"), ("mask then mass", _lib.MC_EINVAL, "static tile mask"),
    ("mass then mask", _lib.MC_EINVAL, "tile mass"), ("qwen short prompt", _lib.MC_ESTATE, "txt_valid"),
    ("stale geometry", _lib.MC_ESTATE, "512")])
def test_refusals(what, status, names):
    if what == "sequence parallel":
        e = Flux.engine((256, 64), weights=False, sp_rank=0, sp_size=2)
        call = lambda: e.set_attention_tile_mask(make_mask(1))                       # noqa: E731
    elif what == "qwen short prompt":
        geo = (((1, 12, 24),), 64)
        e, inp = Qwen.engine(geo), Qwen.inputs(geo)
        e.set_attention_tile_mask(torch.ones(1, 4, 8, dtype=torch.bool))
        call = lambda: fwd(e, inp, FULL, b=0)                                        # noqa: E731  (37 of 64 text rows)
    else:
        e, inp = engine("flux")
        call = {"wrong sizes": lambda: e.set_attention_tile_mask(torch.ones(1, 2, 4, dtype=torch.bool)),
                "mass 1.5": lambda: e.set_attention_tile_mass(1.5), "dense -1": lambda: e.set_attention_tile_mass(MASS, -1),
                "mask then mass": lambda: (e.set_attention_tile_mask(make_mask(1)), e.set_attention_tile_mass(MASS)),
                "mass then mask": lambda: (e.set_attention_tile_mass(MASS), e.set_attention_tile_mask(make_mask(1))),
                "stale geometry": lambda: (e.set_attention_tile_mask(make_mask(1)), e.set_geometry(108, (0, 0, 0), 64),
                                           fwd(e, Flux.inputs((108, 64)), FULL))}[what]
    with pytest.raises(_lib.MagCacheHipError) as ex:
        call()
    assert ex.value.status == status and names in str(ex.value), str(ex.value)

"""CPU: the host side of the FLUX IP-Adapters (magcache_amd/ip_adapter.py) and the restatement the GPU tests compare with
(tests/flux_ip_adapter_ref.py): the helper's plain forward against the golden's first outputs (no reference checkout needed:
call 0 is never skipped), the scale forms, the state-dict spellings, the checks on the embeds and the two image slots against a
recording fake engine."""
import json
import math
import os

import numpy as np
import pytest
import torch

from magcache_amd import ip_adapter as IP
from oracle import flux_ref as FR

import flux_ip_adapter_ref as IR

# the golden stores fp16: half an ulp is 2^-11 of every element, so 2^-10 bounds the relative L2 with room for the fp32
# summation order of another CPU
FP16_BAR = 2.0 ** -10


def rel_l2(a, b):
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "flux_forward_golden.npz"))
    ip = np.load(os.path.join(golden_dir, "flux_ip_adapter_golden.npz"))
    cn = np.load(os.path.join(golden_dir, "flux_controlnet_golden.npz"))
    meta, imeta = json.loads(str(g["meta"])), json.loads(str(ip["meta"]))
    cfg = dict(meta["cfg"], axes_dims_rope=tuple(meta["cfg"]["axes_dims_rope"]))
    return dict(g=g, ip=ip, cn=cn, meta=meta, imeta=imeta, cfg=cfg)


def oracle(gold, adapters, cfg=None, seed=None):
    meta, ad = gold["meta"], gold["imeta"]["adapters"]
    o = FR.init_synthetic_(FR.FluxTransformer2DModel(**(cfg or gold["cfg"])), seed=meta["weight_seed"] if seed is None else seed,
                           std=meta["weight_std"])
    return IR.add_ip_adapters_(o, [tuple(ad[k]["spec"]) for k in adapters], [ad[k]["seed"] for k in adapters], gold["imeta"]["ip_std"])


def forward(gold, model, names, t, **extra):
    g, im = gold["g"], gold["imeta"]
    emb = [torch.from_numpy(gold["ip"]["embeds_%s_q" % k]).float()[None] * im["embed_scale"] for k in names]
    with torch.no_grad():
        return IR.plain_forward(model, torch.from_numpy(g["latent0"]), torch.from_numpy(g["ctx"]), torch.from_numpy(g["pooled"]),
                                torch.tensor([t]), torch.from_numpy(g["img_ids"]), torch.from_numpy(g["txt_ids"]),
                                torch.tensor([gold["meta"]["guidance"]]), dict(ip_adapter_image_embeds=emb) if names else None,
                                **extra)[0]


@pytest.mark.parametrize("case", ["one", "two"])
def test_helper_forward_reproduces_the_first_call_of_the_loops(gold, case):
    c = gold["imeta"]["cases"][case]
    m = oracle(gold, c["adapters"])
    IR.set_ip_adapter_scale(m, IP.normalise_scales(c["scale"], len(c["adapters"]), gold["cfg"]["num_layers"]))
    t0 = float(gold["g"]["sigmas"][0])
    out = forward(gold, m, c["adapters"], t0)
    assert rel_l2(out, gold["ip"][case + "_outs"][0].astype(np.float32)) < FP16_BAR
    # the same model without the key is the plain golden's, and the key moves it by what the generator recorded
    plain = forward(gold, m, (), t0)
    assert rel_l2(plain, gold["g"]["outs"][0]) < 1e-5
    assert abs(rel_l2(out, plain) - c["first_call_moved"]) < 1e-3 and c["first_call_moved"] > 3 * gold["imeta"]["loop_bar"]


def test_helper_forward_reproduces_the_single_forward_cases(gold):
    im = gold["imeta"]
    ld = oracle(gold, ("A",), dict(gold["cfg"], num_single_layers=0), im["last_double"]["weight_seed"])
    assert rel_l2(forward(gold, ld, ("A",), im["last_double"]["timestep"]), gold["ip"]["last_double_out"].astype(np.float32)) < FP16_BAR
    cscale = json.loads(str(gold["cn"]["meta"]))["sample_scale"]
    samples = dict(controlnet_block_samples=[torch.from_numpy(q).float()[None] * cscale for q in gold["cn"]["double_q"]],
                   controlnet_single_block_samples=[torch.from_numpy(q).float()[None] * cscale for q in gold["cn"]["single_q"]])
    out = forward(gold, oracle(gold, ("A",)), ("A",), im["with_controlnet"]["timestep"], **samples)
    assert rel_l2(out, gold["ip"]["with_controlnet_out"].astype(np.float32)) < FP16_BAR
    assert min(im["last_double"]["moved"], im["with_controlnet"]["moved"], im["two_vs_one"]) > 3 * im["loop_bar"]


def test_ip_attention_of_the_helper_is_the_stated_formula(gold):
    """sum_j scale_j softmax(q_n K_j^T / sqrt(128)) V_j on the q after norm_q and before RoPE, written out with matmuls"""
    m = oracle(gold, ("A", "B"))
    attn = m.transformer_blocks[1].attn
    attn.processor.scale = [0.7, -0.3]
    g = torch.Generator().manual_seed(2)
    hidden, enc = torch.randn(1, 20, 256, generator=g), torch.randn(1, 6, 256, generator=g)
    ip_h = [torch.randn(1, 1, 4, 256, generator=g), torch.randn(1, 2, 16, 256, generator=g)]
    with torch.no_grad():
        got = attn(hidden, enc, None, ip_hidden_states=ip_h)[2]
        q = attn.norm_q(attn._heads(attn.to_q(hidden)))                      # [1, heads, 20, 128]
        want = torch.zeros_like(hidden)
        for j, h in enumerate(ip_h):
            k = attn.processor.to_k_ip[j](h.reshape(1, -1, 256)).view(1, -1, 2, 128).transpose(1, 2)
            v = attn.processor.to_v_ip[j](h.reshape(1, -1, 256)).view(1, -1, 2, 128).transpose(1, 2)
            p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(128), dim=-1)
            want += attn.processor.scale[j] * (p @ v).transpose(1, 2).reshape(1, 20, 256)
    assert rel_l2(got, want) < 1e-5


# ----------------------------------------------------------------------------- scales
def test_scale_forms():
    assert IP.normalise_scales(0.5, 2, 3) == [[0.5] * 3, [0.5] * 3]
    assert IP.normalise_scales([1, 0.25], 2, 3) == [[1.0] * 3, [0.25] * 3]
    assert IP.normalise_scales([[1, 2, 3], 0.5], 2, 3) == [[1.0, 2.0, 3.0], [0.5] * 3]
    assert IP.normalise_scales([[0.0, 1.0]], 1, 2) == [[0.0, 1.0]]
    for bad, n in (([1.0], 2), ([1.0, 1.0, 1.0], 2), ([[1.0, 1.0]], 1), ([[1.0] * 4, 1.0], 2)):
        with pytest.raises(ValueError):
            IP.normalise_scales(bad, n, 3)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        IP.normalise_scales(1.0, 0, 3)


# ----------------------------------------------------------------------------- state dicts
def test_state_dict_spellings_names_and_shapes(gold):
    m = oracle(gold, ("A", "B"))
    n_double = gold["cfg"]["num_layers"]
    for j, (tokens, spell) in enumerate(((4, IR.checkpoint_state_dict), (16, IR.adapter_state_dict))):
        a = IP.parse_state_dict(spell(m, j), n_double)
        assert (a["embed_dim"], a["cross_dim"], a["tokens"], a["unknown"]) == (64, 256, tokens, [])
        assert list(a["weights"]) == IP.name_templates(n_double)
        sd = m.state_dict()
        for name, t in a["weights"].items():               # the names, index filled in, are the loaded model's own
            assert torch.equal(t, sd[name.format(j=j)])
        assert [n.format(j=j) for n in a["weights"]] == IP.weight_names(j, n_double)
    assert IP.weight_names(1, 1) == [
        "encoder_hid_proj.image_projection_layers.1.image_embeds.weight", "encoder_hid_proj.image_projection_layers.1.image_embeds.bias",
        "encoder_hid_proj.image_projection_layers.1.norm.weight", "encoder_hid_proj.image_projection_layers.1.norm.bias",
        "transformer_blocks.0.attn.processor.to_k_ip.1.weight", "transformer_blocks.0.attn.processor.to_k_ip.1.bias",
        "transformer_blocks.0.attn.processor.to_v_ip.1.weight", "transformer_blocks.0.attn.processor.to_v_ip.1.bias"]
    ck = IR.checkpoint_state_dict(m, 0)
    flat = {"image_proj." + k: v for k, v in ck["image_proj"].items()}
    flat.update({"ip_adapter." + k: v for k, v in ck["ip_adapter"].items()})
    assert list(IP.parse_state_dict(flat, n_double)["weights"]) == IP.name_templates(n_double)
    assert IP.parse_state_dict(dict(flat, extra=torch.zeros(1)), n_double)["unknown"] == ["extra"]
    assert IP.parse_state_dict(flat, n_double, tokens_per_image=4)["tokens"] == 4
    with pytest.raises(ValueError):
        IP.parse_state_dict(flat, n_double, tokens_per_image=16)
    with pytest.raises(ValueError):
        IP.parse_state_dict(flat, n_double + 1)             # a block without weights
    with pytest.raises(ValueError):
        IP.parse_state_dict(flat, n_double - 1)             # weights without a block
    with pytest.raises(ValueError):
        IP.parse_state_dict({k: v for k, v in flat.items() if k != "image_proj.norm.bias"}, n_double)
    both = dict(IR.adapter_state_dict(m, 0), **IR.adapter_state_dict(m, 1))
    with pytest.raises(ValueError, match="one adapter per call"):
        IP.parse_state_dict(both, n_double)


# ----------------------------------------------------------------------------- embeds and slots
def test_embeds_are_checked_before_anything_is_set():
    ad = [(64, 4), (64, 16)]
    a, b = torch.zeros(1, 1, 64), torch.zeros(2, 64, dtype=torch.bfloat16)
    out = IP.check_embeds([a, b], ad)
    assert [tuple(t.shape) for t in out] == [(1, 64), (2, 64)]
    with pytest.raises(ValueError, match="load_ip_adapter"):
        IP.check_embeds([a], [])
    for bad in ([a], [a, b, b], a, [a, torch.zeros(2, 32)], [a, torch.zeros(2, 64).long()], [a[0, 0], b], [a, torch.zeros(17, 64)],
                [torch.zeros(2, 3, 64), b], [a, None]):
        with pytest.raises(ValueError):
            IP.check_embeds(bad, ad)
    assert tuple(IP.check_embeds([torch.zeros(64, 64), torch.zeros(16, 64)], ad)[0].shape) == (64, 64)   # 256 keys each


class FakeEngine:
    def __init__(self, fail_on=None):
        self.log, self.fail_on = [], fail_on

    def set_ip_adapter_image(self, adapter, slot, embeds):
        if self.fail_on == adapter:
            raise RuntimeError("refused")
        self.log.append(("set", adapter, slot, embeds.data_ptr()))

    def select_ip_adapter(self, slot):
        self.log.append(("select", slot))


def test_two_slots_follow_the_tensors():
    e, s = FakeEngine(), IP.ImageSlots()
    pos, neg, third = [torch.zeros(1, 8), torch.zeros(2, 8)], [torch.ones(1, 8), torch.ones(2, 8)], [torch.ones(1, 8), torch.ones(2, 8)]
    sets = lambda: [x for x in e.log if x[0] == "set"]  # noqa: E731
    assert [s.use(e, t) for t in (pos, neg, pos, neg, pos, neg)] == [0, 1, 0, 1, 0, 1]
    assert len(sets()) == 4 and [x[2] for x in sets()] == [0, 0, 1, 1]       # both adapters, once per list
    assert e.log[-1] == ("select", 1) and sum(x[0] == "select" for x in e.log) == 6
    # a view of the same storage is the same tensor; a clone is not
    assert s.use(e, [t[:] for t in pos]) == 0 and len(sets()) == 4
    pos[1].add_(1.0)                                       # one tensor of the list written in place: that slot again
    assert s.use(e, pos) == 0 and len(sets()) == 6
    assert s.use(e, neg) == 1 and len(sets()) == 6
    # a third list replaces the slot used least recently (pos; neg was used last)
    assert s.use(e, third) == 0 and s.use(e, neg) == 1 and len(sets()) == 8
    assert s.use(e, pos) == 0 and len(sets()) == 10        # ... third was older than neg
    # another list length is another image prompt
    assert s.use(e, pos[:1]) == 1 and len(sets()) == 11
    s.forget()
    assert s.use(e, pos[:1]) == 0 and len(sets()) == 12


def test_a_failed_set_leaves_the_slot_unclaimed():
    s, t = IP.ImageSlots(), [torch.zeros(1, 8), torch.zeros(1, 8)]
    with pytest.raises(RuntimeError):
        s.use(FakeEngine(fail_on=1), t)
    e = FakeEngine()
    assert s.use(e, t) == 0 and [x[0] for x in e.log] == ["set", "set", "select"]


def test_shim_drops_nothing_silently():
    """the three FLUX forwards hand the key to the slots, select none without it, and refuse it without an adapter"""
    from types import SimpleNamespace
    from magcache_amd import mmdit as MM
    e = FakeEngine()
    e._ip = [(8, 4)]
    model = SimpleNamespace(engine=e, _ip_slots=lambda s=IP.ImageSlots(): s)
    t = torch.zeros(1, 1, 8)
    MM._flux_set_ip_adapter(model, dict(ip_adapter_image_embeds=[t], scale=0.5))
    MM._flux_set_ip_adapter(model, dict(ip_adapter_image_embeds=[t]))
    MM._flux_set_ip_adapter(model, None)
    MM._flux_set_ip_adapter(model, {"scale": 1.0})
    assert [x[0:1] + x[1:2] for x in e.log] == [("set", 0), ("select", 0), ("select", 0), ("select", None), ("select", None)]
    e._ip = []
    n = len(e.log)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        MM._flux_set_ip_adapter(model, dict(ip_adapter_image_embeds=[t]))
    MM._flux_set_ip_adapter(model, None)                   # no adapter, no key: not a single call
    assert len(e.log) == n
    import inspect
    for fn in (MM.flux_plain_forward, MM.flux_magcache_forward, MM.flux_magcache_calibration):
        assert "_flux_set_ip_adapter(self, joint_attention_kwargs)" in inspect.getsource(fn)

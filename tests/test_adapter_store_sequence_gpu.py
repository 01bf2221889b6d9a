"""GPU: one fixed, seeded sequence of adapter-store calls on the tiny Wan engine and on the tiny FLUX engine, which pins what
the store's bookkeeping decides: the order of the terms of a merge (set order within each kind, a replaced term keeps its
place), the limit of summed terms per weight, the one magnitude per weight, the base copies and their release.

The engines have no call that reads a weight back, so a live weight is observed through the forward it produces.  After every
apply the engine under test must equal, BIT FOR BIT,

  (a) a second engine that was given, through plain set_weight, the weights the single ops (mc_op_adapter_merge,
      mc_op_lora_merge, mc_op_lora_merge_f32, mc_op_param_delta) build from the pristine weights and this file's own list of
      surviving terms -- set order within kind, multiplier fp32(scale) * fp32(factor), the dispatch the store documents;
  (b) in lora_info, the counts this file derives from its own list;
  (c) after the last remove, the forward recorded before the first set, with no base copy left;

and its forwards must hash to the digests in tests/golden/adapter_store_sequence.json ({engine: [one SHA-256 per apply]}).
They were recorded by running this file's two cases, every check included, on an MI355X against the library built from commit
6ff4cfa -- the parent of the commit that joined the store's three per-kind lists into one -- and writing the lists the cases
return to that file; they are the statement that the change did not move a bit.

Pairs and Kronecker / Hadamard operands are random (bf16-representable where the store keeps bf16), deltas random fp32, and
the scales no powers of two: the fp32 sums then depend on the order of the terms, which the sequence asserts of its own
yardstick on the fp32 matrix and the bias, where no bf16 rounding hides it."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import adapter_kinds_ref as AR  # noqa: E402
import test_wan_lora_gpu as TW  # noqa: E402
from magcache_amd import _lib  # noqa: E402
from magcache_amd.lora import lora_factor  # noqa: E402
from test_adapter_merge_gpu import c_terms  # noqa: E402
from test_mmdit_lora_gpu import flux  # noqa: E402,F401  (a fixture)

DEV = "cuda:0"
OK, EINVAL = _lib.MC_OK, _lib.MC_EINVAL
RANK = 4
FIXTURE = "adapter_store_sequence.json"


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(shape, gen, amp):
    """bf16-representable fp32 values on the device: the store's bf16 copy of a pair holds exactly these"""
    return (torch.randn(*shape, generator=gen) * amp).bfloat16().float().to(DEV)


class Sequence:
    """The store as this test states it: `terms` in set order (a replaced term keeps its place), `scales` of the adapters known."""

    def __init__(self, engine, wd, part, group, f32_matrix=None, bias=None):
        self.e, self.wd = engine, wd
        self.part, self.group, self.f32_matrix, self.bias = part, group, f32_matrix, bias
        self.terms, self.scales = [], {}
        self.gen = torch.Generator().manual_seed(20240)

    # ---- operands
    def shape(self, target):
        w = self.wd[target]
        return w.shape[0], w.numel() // w.shape[0]

    def make(self, kind, target):
        """(entry for LoraHost._lora_set, (kind, operands..., factor) for the list)"""
        rows, k = self.shape(target)
        g = self.gen
        if kind == "pair":      # alpha 8 at rank 4: factor 2
            down, up = rnd((RANK, k), g, 0.05), rnd((rows, RANK), g, 0.05)
            return ("pair", down, up, 8.0), ("pair", down, up, lora_factor(down, 8.0))
        if kind == "kron":
            s1, s2 = AR.kron_shapes(rows, k)
            w1, w2 = rnd(s1, g, 0.1), rnd(s2, g, 0.1)
            return ("kron", w1, w2, 0.75), ("kron", w1, w2, 0.75)
        if kind == "hada":
            ops = tuple(rnd(s, g, 0.2) for s in ((rows, RANK), (RANK, k), (rows, RANK), (RANK, k)))
            return ("hada",) + ops + (-1.5,), ("hada",) + ops + (-1.5,)
        if kind == "delta":     # kept in fp32 as given: full mantissas, so that a sum of three rounds and its order shows
            d = (torch.randn(*self.wd[target].shape, generator=g) * 0.05).to(DEV)
            return ("delta", d), ("delta", d, 1.0)
        raise AssertionError(kind)

    # ---- store calls, mirrored in the list
    def set(self, adapter, kind, target):
        entry, rec = self.make(kind, target)
        st = self.e._lora_set(adapter, target, entry)
        if st == OK:
            self._put(adapter, target, rec)
        return st

    def set_magnitude(self, adapter, target):
        rows, k = self.shape(target)
        w = self.wd[target].detach().reshape(rows, k).bfloat16().float().cpu()
        g = (w.norm(dim=1) * (0.5 + torch.rand(rows, generator=self.gen))).to(DEV).contiguous()
        st = self.e._lora_fn("set_magnitude")(self.e.h, adapter.encode(), target.encode(), ptr(g), rows, _lib.MC_F32, stream())
        torch.cuda.synchronize()
        if st == OK:
            self._put(adapter, target, ("magnitude", g, 1.0))
        return st

    def _put(self, adapter, target, rec):
        new = dict(adapter=adapter, target=target, kind=rec[0], ops=rec[1:-1], factor=rec[-1])
        for i, t in enumerate(self.terms):
            if (t["adapter"], t["target"], t["kind"]) == (adapter, target, rec[0]):
                self.terms[i] = new
                break
        else:
            self.terms.append(new)
        self.scales.setdefault(adapter, 1.0)

    def scale(self, adapter, value):
        _lib.check(self.e._lora_fn("scale")(self.e.h, adapter.encode(), float(value)))
        self.scales[adapter] = float(value)

    def remove(self, adapter=None):
        _lib.check(self.e._lora_fn("remove")(self.e.h, adapter.encode() if adapter else None))
        self.terms = [t for t in self.terms if adapter and t["adapter"] != adapter]
        if adapter:
            del self.scales[adapter]
        else:
            self.scales = {}

    # ---- what the list says the engine holds
    def live(self, target, kind, terms=None):
        """the live terms of one kind in set order (or in the order of `terms`), as the single ops take them"""
        out = []
        for t in self.terms if terms is None else terms:
            m = AR.multiplier(self.scales[t["adapter"]], t["factor"])
            if t["target"] == target and t["kind"] == kind and m != 0.0:
                out.append((kind,) + t["ops"] + (m,))
        return out

    def expected(self, target, terms=None):
        """the weight the single ops build from the pristine one (terms: from the list in another order)"""
        lib = _lib.load()
        rows, k = self.shape(target)
        pairs, krons, hadas = (self.live(target, kind, terms) for kind in ("pair", "kron", "hada"))
        mags = [t["ops"][0] for t in self.terms if t["target"] == target and t["kind"] == "magnitude" and self.scales[t["adapter"]] != 0.0]
        assert len(mags) <= 1
        keep = []
        if target != self.part:         # an fp32 parameter: the pairs of a matrix first, then the deltas on the result
            new = self.wd[target].detach().to(DEV).float().clone().contiguous()
            if pairs:
                arr = (_lib.McLoraTerm * len(pairs))(*[self._lora_term(p, keep) for p in pairs])
                _lib.check(lib.mc_op_lora_merge_f32(ptr(new), k, ptr(new), k, rows, k, arr, len(pairs), None, 0, stream()))
            dl = self.live(target, "delta", terms)
            if dl:
                pa = (C.c_void_p * len(dl))(*[d[1].data_ptr() for d in dl])
                ds = (C.c_float * len(dl))(*[d[2] for d in dl])
                _lib.check(lib.mc_op_param_delta(ptr(new), ptr(new), new.numel(), pa, ds, len(dl), stream()))
        else:
            base = self.wd[target].detach().to(DEV).reshape(rows, k).bfloat16().contiguous()
            new = base.clone()
            if krons or hadas or mags:
                arr, n = c_terms(pairs + krons + hadas, keep)
                _lib.check(lib.mc_op_adapter_merge(ptr(base), k, ptr(new), k, rows, k, arr, n, ptr(mags[0]) if mags else None, None, 0,
                                                   stream()))
            elif pairs:
                arr = (_lib.McLoraTerm * len(pairs))(*[self._lora_term(p, keep) for p in pairs])
                _lib.check(lib.mc_op_lora_merge(ptr(base), k, ptr(new), k, rows, k, arr, len(pairs), None, 0, stream()))
        torch.cuda.synchronize()
        return new.reshape(self.wd[target].shape)

    @staticmethod
    def _lora_term(p, keep):
        d, u = p[1].bfloat16().contiguous(), p[2].bfloat16().contiguous()
        keep += [d, u]
        return _lib.McLoraTerm(d.data_ptr(), u.data_ptr(), d.shape[0], p[3])

    def targets(self):
        return [t for t in (self.part, self.f32_matrix, self.bias) if t]

    def info(self):
        """adapters known; parameters with a base copy (the part's whole fused Linear counts once); bytes of the copies"""
        touched = {t["target"] for t in self.terms}
        nbytes = sum(self.wd[n].numel() * 2 for n in self.group) if self.part in touched else 0
        nbytes += sum(self.wd[t].numel() * 4 for t in touched if t != self.part)
        return len(self.scales), len(touched), nbytes


def run_sequence(seq, run, ref_engine, run_ref):
    """the sequence, every check included; returns the SHA-256 of the forward after every apply"""
    e = seq.e
    P, F, B = seq.part, seq.f32_matrix, seq.bias
    digests = []

    def apply(what):
        e.apply_lora()
        got = run()
        h = hashlib.sha256()
        for t in got:
            h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        digests.append(h.hexdigest())
        for target in seq.targets():                                                   # (a)
            ref_engine.set_weight(target, seq.expected(target))
        want = run_ref()
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), f"{what}: not the single ops' weights"
        info = e.lora_info()                                                           # (b)
        assert (info["adapters"], info["linears"], info["base_bytes"]) == seq.info(), (what, info, seq.info())
        return got

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    pristine = apply("before the first set")
    assert e.lora_info()["base_bytes"] == 0
    # Three adapters interleaved on one part, set in the order c, a, b -- not the order of their names, and no swap of its first
    # two, which a sum would not show: c and a with a pair, a Kronecker and a Hadamard term each, b with a pair and a Kronecker
    # term (eight summed terms), a's magnitude on top.  The fp32 matrix takes a pair of each, the bias a delta of each.
    for kind in ("pair", "kron", "hada"):
        for adapter in ("c", "a", "b")[:2 if kind == "hada" else 3]:
            assert seq.set(adapter, kind, P) == OK
    assert seq.set_magnitude("a", P) == OK
    if F:
        for adapter in ("c", "a", "b"):
            assert seq.set(adapter, "pair", F) == OK and seq.set(adapter, "delta", B) == OK
    seq.scale("c", 0.9)         # multipliers that are no powers of two: every product rounds
    seq.scale("b", 1.3)
    first = apply("eight terms and a magnitude")
    assert not same(first, pristine) and len(seq.terms) == (15 if F else 9)
    # Replaced terms keep their places.  c's were set FIRST and two other adapters follow them on every target: the kernels sum
    # (t0 + t1) + t2 from the first term on, so c's term moved to the end -- which is also the order of the adapters' names --,
    # (ta + tb) + tc, is another fp32 value than (tc + ta) + tb.
    assert seq.set("c", "pair", P) == OK and seq.set("c", "kron", P) == OK
    if F:
        assert seq.set("c", "pair", F) == OK and seq.set("c", "delta", B) == OK
    assert [t["adapter"] for t in seq.terms[:3]] == ["c", "a", "b"] and len(seq.terms) == (15 if F else 9)
    replaced = apply("c's pair, Kronecker term and delta replaced")
    assert not same(replaced, first)
    if F:
        # the yardstick tells these orders apart where nothing is rounded to bf16 afterwards (on the bf16 part most of an fp32
        # rounding's effect is below a bf16 value, so nothing is asked there)
        moved = [t for t in seq.terms if t["adapter"] != "c"] + [t for t in seq.terms if t["adapter"] == "c"]
        by_name = sorted(seq.terms, key=lambda t: t["adapter"])
        for target in (F, B):
            for other in (moved, by_name, seq.terms[::-1]):
                assert not torch.equal(seq.expected(target), seq.expected(target, other)), target
    # scale 0 leaves a's terms and its magnitude out (the copies stay), and back
    seq.scale("a", 0.0)
    off = apply("a at scale 0")
    assert not same(off, replaced) and not same(off, pristine)
    seq.scale("a", 1.0)
    assert same(apply("a back at scale 1"), replaced)
    # pairs, Kronecker and Hadamard terms count together: a ninth is refused, b's own and a new adapter's
    assert seq.set("b", "hada", P) == EINVAL and b"more than 8" in e.lib.mc_last_error()
    assert seq.set("d", "pair", P) == EINVAL and b"more than 8" in e.lib.mc_last_error()
    # one magnitude per weight
    assert seq.set_magnitude("b", P) == EINVAL and b"already has one on this weight" in e.lib.mc_last_error()
    assert same(apply("after the refusals"), replaced)      # ... which left terms, adapters and copies as they were
    assert seq.set_magnitude("a", P) == OK                  # the owner's replaces
    assert not same(apply("a's magnitude replaced"), replaced)
    seq.remove("a")
    without_a = apply("a removed")
    assert not same(without_a, replaced) and set(seq.scales) == {"b", "c"}
    seq.remove(None)
    last = apply("every adapter removed")                                              # (c)
    assert same(last, pristine) and e.lora_info()["base_bytes"] == 0 and e.lora_info()["linears"] == 0
    return digests


def recorded(golden_dir, engine, digests):
    with open(os.path.join(golden_dir, FIXTURE)) as f:
        want = json.load(f)[engine]
    assert digests == want, [i for i, (a, b) in enumerate(zip(digests, want)) if a != b]


def wan_case():
    cfg = TW.CFG
    wd = TW.weights(cfg)
    A, ref = TW.make_engine(cfg, wd), TW.make_engine(cfg, wd)
    group = ["blocks.0.self_attn.%s.weight" % p for p in "qkv"]
    seq = Sequence(A, wd, group[0], group, f32_matrix="time_embedding.0.weight", bias="blocks.0.self_attn.q.bias")
    return run_sequence(seq, lambda: TW.trace(A), ref, lambda: TW.trace(ref))


def flux_case(fx):
    m, ref = fx.make(), fx.make()
    group = ["transformer_blocks.0.attn.to_%s.weight" % p for p in "qkv"]
    seq = Sequence(m.engine, fx.sd, group[0], group)
    return run_sequence(seq, lambda: [fx.run(m).clone()], ref.engine, lambda: [fx.run(ref).clone()])


def test_wan_store_sequence_matches_single_ops_counts_and_recorded_digests(golden_dir):
    recorded(golden_dir, "wan", wan_case())


def test_flux_store_sequence_matches_single_ops_counts_and_recorded_digests(golden_dir, flux):  # noqa: F811
    recorded(golden_dir, "flux", flux_case(flux))

"""CPU, fake engines: every MagCache shim a user patches in (model.py, wan22.py, mmdit.py) against the oracle rule and against
the C rule on random configurations; the state a geometry change starts over against what the family's init_* sets; the
weight calls both engine classes share against a stub library."""
import ctypes as C

import numpy as np
import pytest
import torch

from magcache_amd import _lib, adapters, rule
from magcache_amd import engine as E
from magcache_amd import mmdit as MM
from magcache_amd import model as M
from magcache_amd import wan22
from oracle import magcache_ref as MR
from test_host_logic import make_experts22, make_shim

SINGLE = ("flux", "hunyuan")
WAN22 = ("wan22_t2v", "wan22_i2v", "wan22_ti2v")
FAMILIES = SINGLE + ("qwen",) + WAN22


class FakeMMDiTEngine:
    def __init__(self):
        self.geometries = []

    def reset(self):
        pass

    def residual(self, branch=None):
        return ("residual", branch)

    def calib_stats(self):
        return 1.25, 0.5, 0.125

    def set_geometry(self, img_tokens, latent_grid, txt_len):
        self.geometries.append((img_tokens, latent_grid, txt_len))


MMDIT = {"flux": (MM.FluxTransformer2DModelHIP, MM.init_flux_magcache, lambda m: m(hidden_states=None, return_dict=False)),
         "hunyuan": (MM.HYVideoDiffusionTransformerHIP, MM.init_hunyuan_magcache, lambda m: m(None, None, return_dict=False)),
         "qwen": (MM.QwenImageTransformer2DModelHIP, MM.init_qwen_magcache, lambda m: m(hidden_states=None, return_dict=False))}


def make_mmdit(family):
    """a model of a fresh subclass on a fake engine; its trace holds (branch, mode) of every engine forward"""
    base = MMDIT[family][0]
    cls = type("Patched" + base.__name__, (base,), {})
    m = cls.__new__(cls)
    m.engine, m.trace = FakeMMDiTEngine(), []
    if family == "qwen":
        cls._run = lambda self, *a: (self.trace.append((a[-1], a[-2])) or "out")
    else:
        cls._run = lambda self, *a: (self.trace.append((0, a[-1])) or "out")
    return m


def configurations(family, count=60):
    """The issue's draws: the gate stays shut until every slot has cached a residual (the reference alone would add None)."""
    rng = np.random.default_rng(sorted(FAMILIES + ("wan21",)).index(family) + 100)
    out = []
    for _ in range(count):
        thresh, K = float(rng.uniform(0.02, 0.4)), int(rng.integers(1, 7))
        if family in SINGLE:
            n, steps, split = int(rng.integers(12, 61)), None, None
            lo = 1.6 / n
            table = 1.0 + rng.normal(0.0, 0.05, size=n)
        else:
            steps = int(rng.integers(8, 41))
            n = 2 * steps
            split = int(rng.integers(4, steps - 3)) if family in ("wan22_t2v", "wan22_i2v") else None
            lo = 2.01 / n if split is None else 2.01 / (2 * split)
            table = np.concatenate(([1.0, 1.0], 1.0 + rng.normal(0.0, 0.03, size=n - 2)))
        out.append(dict(n=n, steps=steps, split=split, thresh=thresh, K=K, R=float(rng.uniform(lo, max(lo, 0.45))), table=table))
    return out


def run_shim(family, c):
    """Drive the family's shim for 2.5 passes over the schedule; after every call yields (skip, branch, cnt, err, steps, ratio)
    as the user reads them off the model (scalars as one-element lists)."""
    if family == "wan21":
        m = make_shim()
        M.init_magcache(m, c["steps"], c["thresh"], c["K"], c["R"], mag_ratios=c["table"])
        pick, call, trace = (lambda pos: m), (lambda m: m(["x"], t=0, context=["c"], seq_len=4)), m.trace
    elif family in WAN22:
        _, cls, hi, lo = make_experts22()
        wan22.init_magcache(hi, c["table"][2:], c["steps"], c["thresh"], c["K"], c["R"], split_steps=c["split"],
                            mode="i2v" if family == "wan22_i2v" else "t2v")
        pick = lambda pos: hi if c["split"] is None or pos < 2 * c["split"] else lo       # noqa: E731
        call, trace = (lambda m: m(["x"], t=0, context=["c"], seq_len=4)), cls.trace
    else:
        m = make_mmdit(family)
        init = MMDIT[family][1]
        if family == "qwen":
            init(m, c["steps"], c["thresh"], c["K"], c["R"], mag_ratios=list(c["table"][2:]))
        else:
            init(m, c["n"], c["thresh"], c["K"], c["R"], mag_ratios=c["table"])
        pick, call, trace = (lambda pos: m), MMDIT[family][2], m.trace
    for i in range(int(2.5 * c["n"])):
        m = pick(i % c["n"])
        call(m)
        branch, mode = trace[-1][-2:]
        aslist = (lambda v: list(v)) if family not in SINGLE else (lambda v: [v])
        yield (mode == _lib.MC_MODE_SKIP, branch, int(m.cnt), aslist(m.accumulated_err), aslist(m.accumulated_steps),
               aslist(m.accumulated_ratio))


def bits(values):
    return [float(v).hex() for v in values]


def split_step(c):
    return None if c["split"] is None else 2 * c["split"]


@pytest.mark.parametrize("family", FAMILIES)
def test_shim_equals_the_oracle_state_machine_on_random_configurations(family):
    """After every call: skip, branch and cnt, accumulated_err and accumulated_ratio bit for bit, accumulated_steps."""
    done = 0
    for c in configurations(family):
        want = MR.RuleState(family, c["n"], c["thresh"], c["K"], c["R"], c["table"], split_step=split_step(c))
        for i, (skip, branch, cnt, err, steps, ratio) in enumerate(run_shim(family, c)):
            skip_w, p_w = want.step()
            slots = 2 if want.two else 1
            assert (skip, branch, cnt) == (bool(skip_w), p_w, want.cnt), (family, c, i)
            assert bits(err) == bits(want.acc_err[:slots]) and bits(ratio) == bits(want.acc_ratio[:slots]), (family, c, i)
            assert [int(s) for s in steps] == [int(s) for s in want.acc_steps[:slots]], (family, c, i)
        done += 1
    assert done == 60


@pytest.mark.parametrize("family", FAMILIES + ("wan21",))
def test_shim_equals_the_c_rule_on_random_configurations(family):
    """The product's two implementations of the rule tied to each other: decision, branch and mc_rule_cnt after every call,
    mc_rule_state at the end.  The C rule never touches the device."""
    lib = _lib.load()
    done = 0
    for c in configurations(family):
        arr = (C.c_double * c["n"])(*c["table"].tolist())
        r = lib.mc_rule_create(_lib.RULE_VARIANTS[family], c["n"], c["thresh"], c["K"], c["R"], arr, c["n"], split_step(c) or 0)
        assert r, (family, c)
        b = C.c_int()
        for i, (skip, branch, cnt, err, steps, ratio) in enumerate(run_shim(family, c)):
            skip_c = lib.mc_rule_step(r, C.byref(b))
            assert (skip, branch, cnt) == (bool(skip_c), b.value, lib.mc_rule_cnt(r)), (family, c, i)
        e, s, q = (C.c_double * 2)(), (C.c_int * 2)(), (C.c_double * 2)()
        lib.mc_rule_state(r, e, s, q)
        slots = len(err)
        assert bits(err) == bits(list(e)[:slots]) and bits(ratio) == bits(list(q)[:slots]), (family, c)
        assert [int(x) for x in steps] == list(s)[:slots], (family, c)
        lib.mc_rule_destroy(r)
        done += 1
    assert done == 60


def _new_geometry(family, m):
    """a call of other shapes on a dynamic_geometry model, as far as the shim's _geometry"""
    m.dynamic_geometry, m.img_tokens, m.txt_len, m.latent_grid = True, 16, 8, (1, 8, 8)
    if family == "hunyuan":
        m._geometry(torch.zeros(1, 4, 2, 8, 8), torch.zeros(1, 12, 4))
        return (32, (2, 8, 8), 12)
    args = (torch.zeros(1, 32, 4), torch.zeros(1, 12, 4))
    m._geometry(*args) if family == "flux" else m._geometry(*args, None)
    return (32, (0, 0, 0), 12)


@pytest.mark.parametrize("calibration", [False, True])
@pytest.mark.parametrize("family", sorted(MMDIT))
def test_a_geometry_change_starts_the_state_init_sets(family, calibration, capsys):
    init, call = MMDIT[family][1:]
    started = rule.fresh_state(family, calibration)
    every = rule.fresh_state(family, None)
    assert set(started) <= set(every) and all(every[k] == v for k, v in started.items())
    assert set(every) == set(rule.fresh_state(family, False)) | set(rule.fresh_state(family, True))
    fresh = make_mmdit(family)
    init(fresh, 4, retention_ratio=0.5, calibration=calibration)
    # what init_* sets of these attributes is the family's fresh state of that mode, and nothing else of them
    assert {k: v for k, v in vars(type(fresh)).items() if k in every} == started
    if family == "qwen" and calibration:
        assert not hasattr(fresh, "magcache_thresh") and not hasattr(fresh, "accumulated_err")
    m = make_mmdit(family)
    init(m, 4, retention_ratio=0.5, calibration=calibration)   # the gate opens once every slot has cached a residual
    n = m.num_steps
    for _ in range(n):                          # one sample: residuals cached, statistics recorded, cnt back at 0
        call(m)
    if family != "hunyuan" or not calibration:  # the HunyuanVideo calibration never wraps cnt (upstream): a new sample starts by hand
        assert m.cnt == 0
    m.cnt = 0
    for k in started:
        if k != "cnt":
            setattr(m, k, "stale")
    assert m.engine.geometries == []
    want = _new_geometry(family, m)
    assert m.engine.geometries == [want] and (m.img_tokens, m.txt_len) == (want[0], want[2])
    for k in every:
        assert hasattr(m, k) == hasattr(fresh, k), k
        if hasattr(fresh, k):
            assert getattr(m, k) == getattr(fresh, k), k
    capsys.readouterr()


# ----------------------------------------------------------------------------- the engine host base on a stub library
class StubLib:
    """Python objects standing in for the ctypes functions of one prefix"""

    def __init__(self, abi, statuses=(), error=b"", missing=()):
        self.calls, self.statuses, self.error, self.missing = [], list(statuses), error, missing
        setattr(self, abi + "set_weight", self.set_weight)
        setattr(self, abi + "weights_missing", self.weights_missing)

    def set_weight(self, h, name, ptr, dtype, shape, ndim, stream):
        self.calls.append((name, dtype, list(shape), ndim))
        return self.statuses.pop(0) if self.statuses else _lib.MC_OK

    def mc_last_error(self):
        return self.error

    def weights_missing(self, h, buf, size):
        buf.value = " ".join(self.missing).encode()
        return len(self.missing)


@pytest.fixture
def no_device(monkeypatch):
    """the stream calls of set_weight without a device: counts the stream synchronisations"""
    syncs = []
    monkeypatch.setattr(adapters, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: type("S", (), {"synchronize": lambda self: syncs.append(1)})())
    return syncs


def stub_engine(cls, **kw):
    e = cls.__new__(cls)
    e.lib, e.h, e.device = StubLib(cls._abi, **kw), None, torch.device("cpu")
    return e


@pytest.mark.parametrize("cls", [E.Engine, MM.MMDiTEngine])
def test_set_weight_retries_a_bf16_tensor_as_fp32_once_and_only_when_asked(cls, no_device):
    w = torch.ones(3, 2, dtype=torch.bfloat16)
    e = stub_engine(cls, statuses=[_lib.MC_EINVAL], error=b"weight 'b': must be given as fp32 (bias, norm weight, modulation)")
    e.set_weight("b", w)
    assert e.lib.calls == [(b"b", _lib.MC_BF16, [3, 2], 2), (b"b", _lib.MC_F32, [3, 2], 2)] and no_device == [1]
    e = stub_engine(cls, statuses=[_lib.MC_EINVAL, _lib.MC_EINVAL], error=b"weight 'b': must be given as fp32")
    with pytest.raises(_lib.MagCacheHipError):
        e.set_weight("b", w)                        # the fp32 retry is refused too: no third call
    assert len(e.lib.calls) == 2
    e = stub_engine(cls, statuses=[_lib.MC_EINVAL], error=b"unknown weight 'b'")
    with pytest.raises(_lib.MagCacheHipError):
        e.set_weight("b", w)
    assert e.lib.calls == [(b"b", _lib.MC_BF16, [3, 2], 2)]
    e = stub_engine(cls)
    e.set_weight("w", torch.ones(2, dtype=torch.float16))      # neither fp32 nor bf16: widened before the call
    assert e.lib.calls == [(b"w", _lib.MC_F32, [2], 1)]


@pytest.mark.parametrize("cls", [E.Engine, MM.MMDiTEngine])
def test_load_weights_names_the_first_missing_weights(cls, no_device):
    names = [f"blocks.{i}.weight" for i in range(7)]
    e = stub_engine(cls, missing=names)
    with pytest.raises(KeyError) as ex:
        e.load_weights({"a": torch.ones(2), "b": torch.ones(2)})
    assert [c[0] for c in e.lib.calls] == [b"a", b"b"]
    assert "7 weights missing" in str(ex.value) and all(n in str(ex.value) for n in names[:5]) and names[5] not in str(ex.value)
    e = stub_engine(cls)
    e.load_weights([("a", torch.ones(2))])                      # a list of pairs, nothing missing
    assert [c[0] for c in e.lib.calls] == [b"a"]

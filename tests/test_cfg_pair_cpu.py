"""Host side of the declared CFG pair: sample() brackets the two model calls of a step with pair_begin / pair_end exactly when
this rank evaluates both branches, WanModelHIP passes the declaration on to an engine that has the call and ignores it on one
that has not.  (The engine's side: tests/test_cfg_pair_gpu.py.)"""
import pytest
import torch

from magcache_amd import model as M
from magcache_amd.sampler import sample


class Recorder:
    def __init__(self, fail_at=None):
        self.log, self.fail_at = [], fail_at

    def pair_begin(self):
        self.log.append("begin")

    def pair_end(self):
        self.log.append("end")

    def __call__(self, x, t, context, seq_len):
        self.log.append(context[0])
        if self.fail_at == len(self.log):
            raise RuntimeError("forward failed")
        return [torch.zeros_like(x[0])]


def host_lincomb(coefs, tensors, out=None):
    return sum(float(c) * t for c, t in zip(coefs, tensors))


def run(model, **kw):
    return sample(model, torch.zeros(2, 1, 2, 2), "c", "u", sampling_steps=2, seq_len=1, lincomb=host_lincomb, **kw)


def test_sample_declares_the_pair_around_the_two_calls_of_a_step():
    m = Recorder()
    run(m)
    assert m.log == ["begin", "c", "u", "end"] * 2


def test_sample_without_declaration_and_with_a_model_that_has_none():
    m = Recorder()
    run(m, cfg_pair=False)
    assert m.log == ["c", "u"] * 2
    plain = lambda x, t, context, seq_len: [torch.zeros_like(x[0])]      # noqa: E731  (no pair_begin attribute)
    run(plain)


def test_pair_ends_when_a_forward_raises():
    m = Recorder(fail_at=3)              # begin, c, u <- raises
    with pytest.raises(RuntimeError):
        run(m)
    assert m.log == ["begin", "c", "u", "end"]


def test_model_passes_the_declaration_to_an_engine_that_has_it():
    class Eng:
        calls = []
        pair_begin = lambda self: self.calls.append("begin")     # noqa: E731
        pair_end = lambda self: self.calls.append("end")         # noqa: E731
    m = object.__new__(M.WanModelHIP)
    m.engine = Eng()
    m.pair_begin(), m.pair_end()
    assert Eng.calls == ["begin", "end"]
    m.engine = object()                  # an engine without the call (a stub, an older library): nothing happens
    m.pair_begin(), m.pair_end()

"""No GPU: the Python surface of token_timestep_sets -- frame_timesteps' token order and tag, the shim's capacity check and
trust rules on a fake engine, sample_frames against a plain torch loop with a fake model, the config struct's tail."""
import ctypes as C

import pytest
import torch

from magcache_amd import _lib, model as M, wan22
from magcache_amd._lib import MC_MODE_FULL


def test_mc_config_ends_with_token_timestep_sets():
    names = [n for n, _ in _lib.McConfig._fields_]
    assert names[-1] == "token_timestep_sets" and names[-2] == "sp_phases"
    assert _lib.McConfig._fields_[-1][1] is C.c_int
    assert "mc_engine_token_timestep_sets" in _lib.SIGNATURES and "mc_op_gemm_bf16_resid_sets" in _lib.SIGNATURES
    # mc_create_sized with a struct that ends before the field is the ABI's "as before": the field's offset is the old size
    assert getattr(_lib.McConfig, "token_timestep_sets").offset == C.sizeof(_lib.McConfig) - C.sizeof(C.c_int)


def test_frame_timesteps_token_order_and_tag():
    grid = (3, 4, 6)                                     # 3 frames of 2 x 3 patches
    tt = wan22.frame_timesteps([999.0, 0.0, 500.0], grid)
    assert tt.shape == (1, 18) and tt.dtype == torch.float32 and tt.is_contiguous()
    assert tt[0].tolist() == [999.0] * 6 + [0.0] * 6 + [500.0] * 6            # frame-major, as patchify orders the tokens
    assert tt._mc_distinct_at_most == 3
    assert wan22.frame_timesteps(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), grid).dtype == torch.float32
    with pytest.raises(ValueError, match="3 latent frames"):
        wan22.frame_timesteps([1.0, 2.0], grid)


class FakeEvent:
    def record(self): pass
    def synchronize(self): pass
    def query(self): return True


class FakeEngine:
    """what WanModelHIP._run touches, on the CPU: counts tokens outside its capacity like "tok_t2" does"""
    sp_size, sharded = 1, False

    def __init__(self, capacity, seq_len=12):
        self.device = torch.device("cpu")
        self.seq_len = seq_len
        self.token_timestep_capacity = capacity
        self.tok, self.record, self.calls = None, torch.zeros(4), 0

    def set_token_timesteps(self, t):
        self.tok = t

    def buffer(self, name, dtype):
        assert name == "tok_t2"
        return self.record

    def forward(self, lat, t, ctx, branch=0, mode=0):
        self.calls += 1
        if self.tok is not None:
            vals = torch.unique(self.tok).flip(0)
            kept = vals[:self.token_timestep_capacity]
            lost = int((self.tok[:, None] != kept[None, :]).all(dim=1).sum()) if self.token_timestep_capacity > 2 else \
                int(((self.tok != vals[0]) & (self.tok != vals[-1])).sum())
            self.record = torch.tensor([float(vals[0]), float(vals[-1]), float(lost), float(len(kept))])
        return torch.zeros_like(lat)


def fake_model(capacity):
    m = type("FakeShim", (M.WanModelHIP,), {})({k: 1 for k in ("dim", "ffn_dim", "freq_dim", "text_len", "text_dim", "in_dim",
                                                               "out_dim", "num_heads", "num_layers")}, (3, 4, 4),
                                              engine=FakeEngine(capacity))
    m._tok_ring = [[torch.zeros(3), FakeEvent(), False, 0] for _ in range(4)]
    m._tok_next = 0
    return m


def run(m, t):
    return m._run([torch.zeros(1, 3, 4, 4)], t, [torch.zeros(2, 1)], 0, MC_MODE_FULL)


def tokens(values):
    return torch.tensor(values, dtype=torch.float32).repeat_interleave(12 // len(values)).reshape(1, 12)


def test_default_engine_still_refuses_three_values_with_todays_message():
    m = fake_model(2)
    run(m, tokens([5.0, 0.0]))
    with pytest.raises(ValueError, match="3 distinct values: the engine supports at most two per forward") as ex:
        run(m, tokens([5.0, 3.0, 0.0]))
    assert "token_timestep_sets" not in str(ex.value) and m.engine.calls == 1
    lie = tokens([5.0, 3.0, 0.0])
    lie._mc_two_valued = True
    run(m, lie)
    with pytest.raises(ValueError, match="carried neither t = 5 nor t = 0"):
        m.check_token_timesteps()
    # a per-frame tag does not make a default engine trust more than two values
    three = tokens([5.0, 3.0, 0.0])
    three._mc_distinct_at_most = 3
    with pytest.raises(ValueError, match="distinct values"):
        run(m, three)


def test_capacity_check_and_trust_rules():
    m = fake_model(4)
    run(m, tokens([9.0, 5.0, 3.0, 0.0]))                                    # four values, untagged: checked, accepted
    with pytest.raises(ValueError, match=r"6 distinct values.*token_timestep_sets = 4") as ex:
        run(m, tokens([9.0, 7.0, 5.0, 3.0, 1.0, 0.0]))
    assert "distinct values" in str(ex.value) and m.engine.calls == 1       # refused before anything ran
    calls = []
    orig = torch.unique
    try:
        torch.unique = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        honest = tokens([9.0, 5.0, 3.0, 0.0])
        honest._mc_distinct_at_most = 4
        run(m, honest)                                                      # vouched for within the capacity: no value check
        n_shim = len(calls) - 1                                             # (the fake engine's own torch.unique)
        m.check_token_timesteps()
        too_many = tokens([9.0, 7.0, 5.0, 3.0, 1.0, 0.0])
        too_many._mc_distinct_at_most = 6                                   # vouches for more than the capacity: not trusted
        with pytest.raises(ValueError, match="distinct values"):
            run(m, too_many)
    finally:
        torch.unique = orig
    assert n_shim == 0
    lie = tokens([9.0, 7.0, 5.0, 3.0, 1.0, 0.0])
    lie._mc_distinct_at_most = 4
    run(m, lie)
    with pytest.raises(ValueError, match="4 tokens received no modulation set") as ex:
        m.check_token_timesteps()
    assert "neither" not in str(ex.value) and "token_timestep_sets = 4" in str(ex.value)
    m.check_token_timesteps()                                               # drained


class FakeFrameModel:
    """eps = a + b * latent + 1e-3 * t per frame, another pair for the null context: enough to tell the calls apart"""
    def __init__(self, grid):
        self.engine = type("E", (), {"seq_len": grid[0] * (grid[1] // 2) * (grid[2] // 2)})()
        self.grid, self.log, self.checked = grid, [], 0

    def __call__(self, x, t, context, seq_len):
        F_, H_, W_ = self.grid
        assert t.shape == (1, seq_len) and getattr(t, "_mc_distinct_at_most", None) == F_
        tf = t.reshape(F_, -1)
        assert bool((tf == tf[:, :1]).all())
        self.log.append((float(context[0][0, 0]), tf[:, 0].tolist()))
        a, b = (0.5, 0.25) if float(context[0][0, 0]) > 0 else (-0.125, 0.75)
        return [a + b * x[0] + 1e-3 * tf[:, 0].reshape(1, F_, 1, 1)]

    def check_token_timesteps(self):
        self.checked += 1


def test_sample_frames_is_the_per_frame_euler_loop():
    grid = (4, 4, 4)
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(2, *grid, generator=g)
    sig = torch.tensor([1.0, 0.8, 0.55, 0.3, 0.0], dtype=torch.float64)
    # frame 3 sits at the last sigma throughout (a clean frame): its index never moves, not behind the last row either
    steps = torch.tensor([[0, 0, 0, 4], [1, 0, 0, 4], [2, 1, 0, 4], [3, 2, 1, 4], [4, 3, 2, 4]])
    ctx, ctxn = torch.ones(1, 1), -torch.ones(1, 1)
    guide = 3.0
    model = FakeFrameModel(grid)
    out = wan22.sample_frames(model, noise, ctx, ctxn, steps, sig, guide)
    # the plain loop
    x = noise.clone().float()
    want_log = []
    for i in range(steps.shape[0]):
        cur = steps[i]
        nxt = steps[i + 1] if i + 1 < steps.shape[0] else torch.clamp(cur + 1, max=4)
        tf = (sig[cur] * 1000.0).float()
        want_log += [(1.0, tf.tolist()), (-1.0, tf.tolist())]
        ec = 0.5 + 0.25 * x + 1e-3 * tf.reshape(1, 4, 1, 1)
        eu = -0.125 + 0.75 * x + 1e-3 * tf.reshape(1, 4, 1, 1)
        v = eu + guide * (ec - eu)
        for f in range(4):
            if int(nxt[f]) != int(cur[f]):
                x[:, f] = x[:, f] + float((sig[nxt[f]] - sig[cur[f]]).float()) * v[:, f]
    assert model.log == want_log                                     # cond, then uncond, once per iteration
    assert model.checked == 1
    assert torch.equal(out[:, 3], noise[:, 3])                       # a frame whose index never moves keeps its bits
    assert torch.equal(out, x)
    # conditioning frames are re-imposed
    z = torch.full((2, 1, 4, 4), 7.0)
    out = wan22.sample_frames(FakeFrameModel(grid), noise, ctx, ctxn, steps, sig, guide, z_cond=z)
    assert torch.equal(out[:, :1], z) and not torch.equal(out[:, 1], noise[:, 1])
    with pytest.raises(ValueError, match="outside sigmas"):
        wan22.sample_frames(FakeFrameModel(grid), noise, ctx, ctxn, steps + 1, sig, guide)
    assert not torch.equal(out[:, 2], noise[:, 2])                   # (frame 2 moved: 0 -> 1 -> 2 -> 3)

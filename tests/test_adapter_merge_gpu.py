"""GPU: the adapter merge of every kind alone (magcache_amd/csrc/adapter_merge.hip) through mc_op_adapter_merge:

    delta = pairs (as mc_op_lora_merge_f32 forms them on a zero base) + m * kron(w1, w2) + m * (u1 d1) * (u2 d2), fp32
    V     = fp32(W) + delta,   out = bf16(V)   or   bf16(g[r] / |V[r, :]| * V[r, :]) with a DoRA magnitude g

A single LoKr term without a magnitude is three fp32 roundings in a stated order, so it is held to torch's fp32 result bit for
bit.  Every other case is held to the float64 oracle (tests/adapter_kinds_ref.py) rounded to bf16: an element may be off by one
bf16 value, and at most 1e-3 of the elements may differ (the cap of test_lora_merge_gpu.py).  Every run writes into the
middle of a poisoned buffer with ld_out > K, so a store outside [rows, K] shows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import adapter_kinds_ref as AR  # noqa: E402
from magcache_amd import _lib  # noqa: E402

DEV = "cuda:0"
POISON = 0x7FC1
# rows, K, kron factors, rank: off the 128 tile in both directions with K = 8 * 65; one case of several tiles
SHAPES = {"160x520": (160, 520, ((8, 5), (20, 104)), 5), "384x1536": (384, 1536, ((16, 48), (24, 32)), 16)}
EINVAL = _lib.MC_EINVAL


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16)


def c_terms(terms, keep):
    """oracle terms (tensors on the device) -> mc_adapter_term array; pairs go in as bf16, factors as fp32"""
    out = []
    for t in terms:
        if t[0] == "pair":
            d, u = t[1].bfloat16().contiguous(), t[2].bfloat16().contiguous()
            keep += [d, u]
            out.append(_lib.McAdapterTerm(_lib.MC_ADAPTER_PAIR, t[3], d.data_ptr(), u.data_ptr(), 0, 0, d.shape[0], 0, 0, 0, 0))
        elif t[0] == "kron":
            w1, w2 = t[1].float().contiguous(), t[2].float().contiguous()
            keep += [w1, w2]
            out.append(_lib.McAdapterTerm(_lib.MC_ADAPTER_KRON, t[3], w1.data_ptr(), w2.data_ptr(), 0, 0, 0, *w1.shape, *w2.shape))
        else:
            ops = [x.float().contiguous() for x in t[1:5]]
            keep += ops
            out.append(_lib.McAdapterTerm(_lib.MC_ADAPTER_HADA, t[5], *[x.data_ptr() for x in ops], ops[0].shape[1], 0, 0, 0, 0))
    return (_lib.McAdapterTerm * max(len(out), 1))(*out), len(out)


def run(W, terms, mag=None, alias=False, scratch=False):
    """merge into rows [rows, 2 rows) of a poisoned [3 rows, K + 8] buffer (alias: the base is copied there first and out
    aliases it); returns (the merged rows, whether everything else still holds the poison)"""
    rows, K = W.shape
    ld = K + 8
    buf = torch.full((3 * rows, ld), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    mid = buf[rows:2 * rows]
    keep = []
    arr, n = c_terms(terms, keep)
    base, ld_base = W, K
    if alias:
        mid[:, :K] = W
        base, ld_base = mid, ld
    g = None if mag is None else mag.float().contiguous()
    lib = _lib.load()
    sp, sb = None, 0
    if scratch:
        need = lib.mc_op_adapter_merge_scratch(rows, K, arr, n)
        raw = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        off = (-raw.data_ptr()) % 256
        keep.append(raw)
        sp, sb = C.c_void_p(raw.data_ptr() + off), need
    _lib.check(lib.mc_op_adapter_merge(ptr(base), ld_base, ptr(mid), ld, rows, K, arr, n, ptr(g), sp, sb, stream()))
    torch.cuda.synchronize()
    b = bits(buf)
    untouched = bool((b[:rows] == POISON).all()) and bool((b[2 * rows:] == POISON).all()) and bool((b[rows:2 * rows, K:] == POISON).all())
    return mid[:, :K].clone(), untouched


def rep(*shape, gen, amp):
    """bf16-representable fp32 values, uniform in (-amp, amp)"""
    return ((torch.rand(*shape, generator=gen, device=DEV) * 2 - 1) * amp).bfloat16().float()


@pytest.fixture(scope="module")
def cases():
    """per shape: the weight, one term of every kind, a magnitude -- made once, never written.

    One bf16 value is a meaningful unit of error only away from zero: where W and the delta cancel, the absolute error of ANY
    fp32 evaluation (2^-24 of the operands) spans many of the ever finer bf16 values near zero, and a restatement of the
    formula in torch fp32 then misses the rounded fp64 value on 1e-3 of Gaussian data and by thousands of bf16 values on a few
    elements.  So the data here keep V away from zero by construction: |W| in [0.04, 0.08) with random signs, and bounded
    factors whose terms cannot reach that together -- |m kron| <= 1.3 * 0.1^2 = 0.013, |m hada| <= 0.7 * (rank a^2)^2 = 0.009,
    |m pair| <= 0.9 * rank a^2 = 0.009, so |V| >= 0.009 in every mix below.  The terms still move most elements: their typical
    size, 1e-3 .. 4e-3, is several bf16 values of W (2^-12 .. 2^-11)."""
    gen = torch.Generator(device=DEV).manual_seed(4321)
    out = {}
    for name, (rows, K, ((r1, c1), (r2, c2)), rank) in SHAPES.items():
        sign = torch.randint(0, 2, (rows, K), generator=gen, device=DEV).float() * 2 - 1
        W = (sign * (0.04 + 0.04 * torch.rand(rows, K, generator=gen, device=DEV))).bfloat16()
        kron = ("kron", rep(r1, c1, gen=gen, amp=0.1), rep(r2, c2, gen=gen, amp=0.1), 1.3)
        ah, ap = (0.113 / rank) ** 0.5, (0.01 / rank) ** 0.5
        hada = ("hada", rep(rows, rank, gen=gen, amp=ah), rep(rank, K, gen=gen, amp=ah), rep(rows, rank, gen=gen, amp=ah),
                rep(rank, K, gen=gen, amp=ah), -0.7)
        pair = ("pair", rep(rank, K, gen=gen, amp=ap), rep(rows, rank, gen=gen, amp=ap), 0.9)
        # a magnitude that is not the row norm: the rows change length, each by its own factor
        mag = W.float().norm(dim=1) * (0.5 + torch.rand(rows, generator=gen, device=DEV))
        out[name] = dict(W=W, kron=kron, hada=hada, pair=pair, mag=mag)
    return out


def f32_scale(t):
    """the term with its scale as the fp32 value the kernel receives"""
    s = float(torch.tensor(t[-1], dtype=torch.float32))
    return t[:-1] + (s,)


def held_to_oracle(got, W, terms, mag, what):
    want = AR.to_bf16(AR.merged_weight(W, [f32_scale(t) for t in terms], mag))
    share, worst = AR.compare(got, want)
    print(f"adapter_merge {what}: share of elements off the rounded fp64 value {share:.3e}, largest distance {worst} bf16 values")
    assert worst <= 1, (what, worst)
    assert share <= 1e-3, (what, share)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_lokr_term_is_torch_fp32_bit_for_bit(cases, shape):
    c = cases[shape]
    W, (_, w1, w2, m) = c["W"], c["kron"]
    got, untouched = run(W, [c["kron"]])
    prod = torch.kron(w1, w2)                                   # one fp32 multiply per element (exact for bf16 factors)
    term = torch.tensor(m, dtype=torch.float32, device=DEV) * prod
    want = (W.float() + term).bfloat16()
    assert torch.equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert untouched
    assert float((bits(got) != bits(W)).double().mean()) > 0.5, "the term moves almost nothing: the case checks nothing"


MIXES = {"hada": ("hada",), "pair": ("pair",), "pair+kron+hada": ("pair", "kron", "hada"), "kron+kron": ("kron", "kron"),
         "hada+pair": ("hada", "pair")}


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mixes_without_a_magnitude_against_fp64(cases, shape, mix):
    c = cases[shape]
    terms = [c[k] for k in MIXES[mix]]
    if mix == "kron+kron":
        terms[1] = terms[1][:3] + (-0.4,)
    got, untouched = run(c["W"], terms)
    assert untouched
    held_to_oracle(got, c["W"], terms, None, f"{shape} {mix}")


@pytest.mark.parametrize("mix", ["pair", "kron", "hada", "pair+kron+hada", "none"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dora_against_fp64_and_the_magnitude_moves_the_weight(cases, shape, mix):
    c = cases[shape]
    terms = [] if mix == "none" else [c[k] for k in mix.split("+")]
    got, untouched = run(c["W"], terms, mag=c["mag"])
    assert untouched
    held_to_oracle(got, c["W"], terms, c["mag"], f"{shape} DoRA over {mix}")
    plain, _ = run(c["W"], terms)
    moved = float((bits(got) != bits(plain)).double().mean())
    print(f"adapter_merge {shape} DoRA over {mix}: the magnitude moves {moved:.3f} of the elements")
    assert moved >= 0.9, moved


def test_aliased_out_given_scratch_and_two_runs_give_the_same_bits(cases):
    c = cases["160x520"]
    terms = [c["pair"], c["kron"], c["hada"]]
    for mag in (None, c["mag"]):
        first, ok1 = run(c["W"], terms, mag=mag)
        again, ok2 = run(c["W"], terms, mag=mag)
        aliased, ok3 = run(c["W"], terms, mag=mag, alias=True)
        own, ok4 = run(c["W"], terms, mag=mag, scratch=True)
        assert ok1 and ok2 and ok3 and ok4
        assert torch.equal(bits(first), bits(again)), "two runs differ"
        assert torch.equal(bits(first), bits(aliased)), "out aliased to base differs"
        assert torch.equal(bits(first), bits(own)), "caller-owned scratch differs"


def test_no_term_and_no_magnitude_copies_the_base(cases):
    W = cases["160x520"]["W"].clone()
    W[0, 0] = -0.0                                             # V = W + delta is not formed where there is no delta
    got, untouched = run(W, [])
    assert untouched and torch.equal(bits(got), bits(W))


def test_refusals_leave_out_untouched(cases):
    c = cases["160x520"]
    W, rows, K = c["W"], 160, 520
    lib = _lib.load()
    out = torch.full((rows, K), POISON, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    keep = []
    good, _ = c_terms([c["kron"]], keep)
    g = good[0]

    def call(arr, n, base=None, ld_base=K, out_p=None, ld_out=K, scratch=None, nbytes=0):
        return lib.mc_op_adapter_merge(base or ptr(W), ld_base, out_p or ptr(out), ld_out, rows, K, arr, n, None, scratch, nbytes, stream())

    def one(**kw):
        t = _lib.McAdapterTerm(g.kind, g.scale, g.a, g.b, g.c, g.d, g.rank, g.r1, g.c1, g.r2, g.c2)
        for k, v in kw.items():
            setattr(t, k, v)
        return (_lib.McAdapterTerm * 1)(t)
    assert call(one(kind=9), 1) == EINVAL                                               # an unknown kind
    assert call(one(r2=21), 1) == EINVAL and call(one(c2=100), 1) == EINVAL             # shapes that do not factor
    pair, _ = c_terms([c["pair"]], keep)
    pair[0].rank = 0
    assert call(pair, 1) == EINVAL
    hada, _ = c_terms([c["hada"]], keep)
    hada[0].rank = 0
    assert call(hada, 1) == EINVAL
    many = (_lib.McAdapterTerm * (_lib.MC_LORA_MAX_TERMS + 1))(*[g] * (_lib.MC_LORA_MAX_TERMS + 1))
    assert call(many, _lib.MC_LORA_MAX_TERMS + 1) == EINVAL and b"at most" in lib.mc_last_error()
    # the alignment and pitch rules of mc_op_lora_merge
    assert call(good, 1, base=C.c_void_p(W.data_ptr() + 2)) == EINVAL
    assert call(good, 1, out_p=C.c_void_p(out.data_ptr() + 8)) == EINVAL
    assert call(good, 1, ld_out=K + 4) == EINVAL and call(good, 1, ld_out=K - 8) == EINVAL and call(good, 1, ld_base=K - 8) == EINVAL
    # a scratch one byte short, and a misaligned one
    need = lib.mc_op_adapter_merge_scratch(rows, K, good, 1)
    raw = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    assert call(good, 1, scratch=C.c_void_p(raw.data_ptr() + off), nbytes=need - 1) == EINVAL
    assert call(good, 1, scratch=C.c_void_p(raw.data_ptr() + off + 16), nbytes=need) == EINVAL
    torch.cuda.synchronize()
    assert bool((bits(out) == POISON).all()), "a refused call wrote"
    # the maximum itself is fine
    eight = (_lib.McAdapterTerm * _lib.MC_LORA_MAX_TERMS)(*[one(scale=0.15)[0]] * _lib.MC_LORA_MAX_TERMS)   # 8 * 0.15 * 0.1^2 = 0.012
    _lib.check(call(eight, _lib.MC_LORA_MAX_TERMS, scratch=C.c_void_p(raw.data_ptr() + off), nbytes=need))
    torch.cuda.synchronize()
    held_to_oracle(out, W, [c["kron"][:3] + (0.15,)] * _lib.MC_LORA_MAX_TERMS, None, "eight terms")

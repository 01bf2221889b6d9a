"""The float64 oracle of the adapter merge (low-rank pairs, LoKr, LoHa, DoRA) and builders of adapter state dicts in
every spelling the readers take.  Pure torch on the CPU: no library call, no engine.

    delta = sum_j m_j * term_j          pair: up @ down;  kron: kron(w1, w2);  hada: (u1 @ d1) * (u2 @ d2)
    V     = W + delta
    out   = V                            without a magnitude
    out   = g[r] / |V[r, :]| * V[r, :]   with a DoRA magnitude g [rows]
"""
import numpy as np
import torch


def f64(t):
    return t.detach().double().cpu()


def multiplier(scale, factor):
    """scale * factor as the store forms it: both fp32, one fp32 product"""
    return float(np.float32(np.float32(scale) * np.float32(factor)))


def merged_weight(W, terms, magnitude=None):
    """float64 merged weight of W [rows, K]; terms: ("pair", down [r, K], up [rows, r], m) | ("kron", w1, w2, m) |
    ("hada", u1 [rows, r], d1 [r, K], u2, d2, m); magnitude: [rows] or None"""
    V = f64(W).clone()
    for t in terms:
        if t[0] == "pair":
            V += float(t[3]) * (f64(t[2]) @ f64(t[1]))
        elif t[0] == "kron":
            V += float(t[3]) * torch.kron(f64(t[1]), f64(t[2]))
        elif t[0] == "hada":
            V += float(t[5]) * ((f64(t[1]) @ f64(t[2])) * (f64(t[3]) @ f64(t[4])))
        else:
            raise ValueError(t[0])
    if magnitude is None:
        return V
    return (f64(magnitude).reshape(-1) / V.norm(dim=1))[:, None] * V


def to_bf16(v64):
    """fp64 -> fp32 -> bf16: double rounding is possible only within 2^-29 relative of a tie"""
    return v64.float().bfloat16()


def ordered(b16):
    """bf16 bit patterns (int16 view) as integers that count representable values: neighbours differ by 1"""
    b = b16.contiguous().view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


def compare(got_bf16, want_bf16):
    """(share of elements whose bits differ, largest distance in representable bf16 values)"""
    d = (ordered(got_bf16.cpu()) - ordered(want_bf16.cpu())).abs()
    return float((d != 0).double().mean()), int(d.max())


def _half(t):
    """a LoKr half as float64: a tensor, or (a, b) multiplied out"""
    return f64(t[0]) @ f64(t[1]) if isinstance(t, tuple) else f64(t)


def entry_terms(entry, scale, lora_factor):
    """a reader's entry -> (oracle terms at adapter scale `scale`, magnitude or None); lora_factor: lora.lora_factor"""
    if entry[0] == "dora":
        terms, _ = entry_terms(entry[1], scale, lora_factor)
        return terms, entry[2]
    if entry[0] == "pair":
        return [("pair", entry[1], entry[2], multiplier(scale, lora_factor(entry[1], entry[3])))], None
    if entry[0] == "kron":
        return [("kron", _half(entry[1]), _half(entry[2]), multiplier(scale, entry[3]))], None
    if entry[0] == "hada":
        return [("hada",) + tuple(entry[1:5]) + (multiplier(scale, entry[5]),)], None
    raise ValueError(entry[0])


# ---------------------------------------------------------------------------------------------------- state dicts
MAGNITUDE_SPELLINGS = (".lora_magnitude_vector", ".lora_magnitude_vector.weight", ".lora_magnitude_vector.default.weight", ".dora_scale")


def pair_keys(module, down, up, alpha=None, infix=""):
    sd = {f"{module}.lora_A{infix}.weight": down, f"{module}.lora_B{infix}.weight": up}
    if alpha is not None:
        sd[module + ".alpha"] = torch.tensor(float(alpha))
    return sd


def magnitude_keys(module, g, spelling=".lora_magnitude_vector", column=False):
    """column: LyCORIS's [out, 1] shape instead of PEFT's [out]"""
    return {module + spelling: g.reshape(-1, 1) if column else g.reshape(-1)}


def lokr_keys(module, w1, w2, alpha=None, infix=""):
    """w1, w2: a tensor (lokr_w<n>) or a tuple (a, b) (lokr_w<n>_a, lokr_w<n>_b)"""
    sd = {}
    for n, w in ((1, w1), (2, w2)):
        if isinstance(w, tuple):
            sd[f"{module}.lokr_w{n}_a{infix}"], sd[f"{module}.lokr_w{n}_b{infix}"] = w
        else:
            sd[f"{module}.lokr_w{n}{infix}"] = w
    if alpha is not None:
        sd[module + ".alpha"] = torch.tensor(float(alpha))
    return sd


def loha_keys(module, w1a, w1b, w2a, w2b, alpha=None, infix=""):
    sd = {f"{module}.hada_w1_a{infix}": w1a, f"{module}.hada_w1_b{infix}": w1b, f"{module}.hada_w2_a{infix}": w2a,
          f"{module}.hada_w2_b{infix}": w2b}
    if alpha is not None:
        sd[module + ".alpha"] = torch.tensor(float(alpha))
    return sd


def dyadic(shape, gen, exp=-5):
    """entries in {-1, -1/2, 0, 1/2, 1} * 2^exp: products and short sums of them are exact in fp32"""
    return torch.randint(-2, 3, shape, generator=gen).float() / 2 * 2.0 ** exp


def kron_shapes(rows, k):
    """a factorisation [r1, c1] (x) [r2, c2] of [rows, k] with small first factors"""
    r1 = next(d for d in (4, 2, 1) if rows % d == 0)
    c1 = next(d for d in (8, 4, 2, 1) if k % d == 0)
    return (r1, c1), (rows // r1, k // c1)

"""CPU: the MXFP4 format as tests/mxfp4_ref.py states it (the reference the GPU tests compare the kernels with bit for bit):
the code book, the block exponent at and just above amax = 6 2^n, zero blocks, every tie to the even mantissa, the clamp of
the exponent at +-127, and the pack / unpack round trip."""
import math

import pytest
import torch

import mxfp4_ref as R


def block(values):
    """one 32-element block (zero-padded) as a [1, 32] fp32 row"""
    x = torch.zeros(1, 32)
    x[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    return x


def test_code_book():
    codes = torch.arange(16, dtype=torch.uint8)
    vals = R.code_values(codes).tolist()
    assert vals[:8] == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert vals[8:] == [-0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert math.copysign(1.0, vals[8]) == -1.0
    # every code-book value quantises to itself under the unit scale of a block whose amax is 6 (e = 0)
    codes, e = R.quantize(block([6.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]))
    assert int(e[0, 0]) == 0
    assert codes[0, :15].tolist() == [7, 0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15]


@pytest.mark.parametrize("n", [-126, -20, -1, 0, 1, 7, 100, 125])
def test_exponent_at_and_just_above_six_times_a_power_of_two(n):
    at = torch.tensor(6.0 * 2.0 ** n, dtype=torch.float32)
    above = torch.nextafter(at, torch.tensor(float("inf")))
    below = torch.nextafter(at, torch.tensor(0.0))
    assert int(R.exponent(at)) == n              # amax / 6 = 2^n exactly: ceil(log2) = n, the largest element is code 7
    assert int(R.exponent(above)) == n + 1       # one ulp more: nothing may saturate
    assert int(R.exponent(below)) == n
    for amax, e in ((at, n), (above, n + 1)):
        codes, ex = R.quantize(block([float(amax)]))
        assert int(ex[0, 0]) == e
        assert float(R.dequantize(codes, ex)[0, 0]) <= float(amax) * (1 + 1e-12) or e == n
    # no element of a block exceeds 6 after scaling, whatever amax is
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 32, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 1), generator=g).float())
    e = R.exponent(x.abs().amax(dim=-1))
    scaled = x.double().abs() * torch.exp2(-e.double())[:, None]
    assert float(scaled.max()) <= 6.0 and float(scaled.amax(dim=-1).min()) > 3.0


def test_zero_block():
    codes, e = R.quantize(torch.zeros(2, 64))
    assert e.tolist() == [[-127, -127], [-127, -127]]
    assert int(codes.max()) == 0
    assert bool((R.scale_image(e, 64)[:, [0, 4]] == 0).all())      # byte e + 127 = 0 (rows 0, 1 sit at 0, 4 of their group)
    codes, e = R.quantize(block([-0.0]))
    assert int(e[0, 0]) == -127 and int(codes[0, 0]) == 8          # the sign bit is x's own


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("shift", [0, -3, 5])
def test_every_tie_goes_to_the_even_mantissa(sign, shift):
    s = 2.0 ** shift
    for value, want in R.TIES:
        codes, e = R.quantize(block([6.0 * s, sign * value * s]))    # amax = 6 s: e = shift, the tie is met exactly
        assert int(e[0, 0]) == shift
        got = float(R.code_values(codes)[0, 1])
        assert abs(got) == want and (int(codes[0, 1]) & 1) == 0, (value, got)
        assert (int(codes[0, 1]) >> 3) == (1 if sign < 0 else 0)
        # one ulp to either side of the tie goes to the nearer value
        t = torch.tensor(value * s, dtype=torch.float32)
        up = float(torch.nextafter(t, torch.tensor(float("inf"))))
        dn = float(torch.nextafter(t, torch.tensor(0.0)))
        codes, _ = R.quantize(block([6.0 * s, up, dn]))
        vals = R.code_values(codes)[0]
        lo = max(v for v in R.CODEBOOK if v < value)
        hi = min(v for v in R.CODEBOOK if v > value)
        assert float(vals[1]) == hi and float(vals[2]) == lo


def test_exponent_clamps_at_plus_and_minus_127():
    tiny = torch.tensor(2.0 ** -140, dtype=torch.float32)            # a denormal: ceil(log2(amax / 6)) = -142
    assert int(R.exponent(tiny)) == -127
    codes, e = R.quantize(block([2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -129, 2.0 ** -126, 2.0 ** -140]))
    assert int(e[0, 0]) == -127
    assert R.code_values(codes)[0, :5].tolist() == [1.0, 1.5, 0.0, 2.0, 0.0]    # x 2^127; 0.25 is a tie to 0
    huge = torch.tensor(torch.finfo(torch.float32).max)
    assert int(R.exponent(huge)) == 126                               # the largest float: below the clamp
    # no finite fp32 reaches +127; the clamp itself, on a wider type
    assert int(R.exponent(torch.tensor(6.0 * 2.0 ** 127, dtype=torch.float64))) == 127
    assert int(R.exponent(torch.tensor(2.0 ** 200, dtype=torch.float64))) == 127
    assert R.scale_image(torch.tensor([[127, -127]]), 64)[:, 0].tolist() == [254, 0]


def test_pack_unpack_round_trip_and_nibble_order():
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 16, (5, 96), generator=g).to(torch.uint8)
    q = R.pack(codes)
    assert q.shape == (5, 48)
    assert torch.equal(R.unpack(q), codes)
    one = torch.zeros(1, 32, dtype=torch.uint8)
    one[0, 0], one[0, 1] = 0x3, 0xA
    assert int(R.pack(one)[0, 0]) == 0xA3                              # even k in the low nibble
    x = torch.randn(7, 64, generator=g)
    codes, e = R.quantize(x)
    back = R.dequantize(R.unpack(R.pack(codes)), e)
    assert float((back - x.double()).abs().max()) <= float(x.abs().max())   # a coarse format, but a round trip of the bytes
    assert torch.equal(R.dequantize(codes, e), back)


def test_scale_image_row_order():
    e = torch.arange(70 * 2).view(70, 2) % 50 - 25
    s = R.scale_image(e, 128, fill=0xEE)
    assert torch.equal(R.scale_rows(s, 70), e)
    assert int(s[0, 4 * 5 + 1]) == int(e[16 + 5, 0]) + 127             # row 21 = 16 + 5 sits at 4 * 5 + 1 of its group of 64
    assert int((s == 0xEE).sum()) == 2 * (128 - 70)

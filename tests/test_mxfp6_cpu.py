"""CPU: the MXFP6 format as tests/mxfp6_ref.py states it (the reference the GPU tests compare the kernels with bit for bit):
the 64-entry code book, the block exponent at and just above amax = 7.5 2^n, zero blocks, every one of the 31 ties to the even
mantissa, the clamp of the exponent at +-127, the pack / unpack round trip and the bit order of a group of 32, the row order
of the scale image -- and the premise of the mode: on a Gaussian GEMM W6A6 (e2m3) is as close to float64 as MX fp8 (e4m3)
and at least twice as close as MXFP4."""
import math

import pytest
import torch

import mxfp4_ref as R4
import mxfp6_ref as R


def block(values):
    """one 32-element block (zero-padded) as a [1, 32] fp32 row"""
    x = torch.zeros(1, 32)
    x[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    return x


def test_code_book_all_64_codes():
    vals = R.code_values(torch.arange(64, dtype=torch.uint8)).tolist()
    want = ([i * 0.125 for i in range(8)] + [1.0 + i * 0.125 for i in range(8)] + [2.0 + i * 0.25 for i in range(8)] +
            [4.0 + i * 0.5 for i in range(8)])
    assert vals[:32] == want and want[-1] == 7.5 == R.MAX
    assert vals[32:] == [-v for v in want]
    assert math.copysign(1.0, vals[32]) == -1.0                      # code 32 is -0
    assert all(b > a for a, b in zip(want, want[1:]))
    # every code-book value quantises to itself, both signs, under the unit scale of a block whose amax is 7.5 (e = 0)
    codes, e = R.quantize(block(want))
    assert int(e[0, 0]) == 0 and codes[0].tolist() == list(range(32))
    codes, e = R.quantize(block([-v for v in want]))
    assert int(e[0, 0]) == 0 and codes[0].tolist() == list(range(32, 64))


@pytest.mark.parametrize("n", [-126, -20, -1, 0, 1, 7, 100, 125])
def test_exponent_at_and_just_above_seven_and_a_half_times_a_power_of_two(n):
    at = torch.tensor(7.5 * 2.0 ** n, dtype=torch.float32)
    above = torch.nextafter(at, torch.tensor(float("inf")))
    below = torch.nextafter(at, torch.tensor(0.0))
    assert int(R.exponent(at)) == n              # amax / 7.5 = 2^n exactly: ceil(log2) = n, the largest element is code 31
    assert int(R.exponent(above)) == n + 1       # one ulp more: nothing may saturate
    assert int(R.exponent(below)) == n
    assert int(R.exponent(above)) == math.ceil(math.log2(float(above.double()) / 7.5)) and n == round(math.log2(float(at.double()) / 7.5))
    codes, ex = R.quantize(block([float(at)]))
    assert int(ex[0, 0]) == n and int(codes[0, 0]) == 31
    codes, ex = R.quantize(block([float(above)]))
    assert int(ex[0, 0]) == n + 1 and int(codes[0, 0]) == 23         # a hair above 3.75 under the doubled scale: code 23
    # no element of a block exceeds 7.5 after scaling, whatever amax is, and the maximum uses the top binade
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 32, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 1), generator=g).float())
    e = R.exponent(x.abs().amax(dim=-1))
    scaled = x.double().abs() * torch.exp2(-e.double())[:, None]
    assert float(scaled.max()) <= 7.5 and float(scaled.amax(dim=-1).min()) > 3.75


def test_zero_block():
    codes, e = R.quantize(torch.zeros(2, 64))
    assert e.tolist() == [[-127, -127], [-127, -127]]
    assert int(codes.max()) == 0
    assert bool((R.scale_image(e, 64)[:, [0, 4]] == 0).all())      # byte e + 127 = 0 (rows 0, 1 sit at 0, 4 of their group)
    codes, e = R.quantize(block([-0.0]))
    assert int(e[0, 0]) == -127 and int(codes[0, 0]) == 32         # the sign bit is x's own


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("shift", [0, -3, 5])
def test_every_one_of_the_31_ties_goes_to_the_even_mantissa(sign, shift):
    s = 2.0 ** shift
    assert len(R.TIES) == 31
    for value, want in R.TIES:
        codes, e = R.quantize(block([7.5 * s, sign * value * s]))    # amax = 7.5 s: e = shift, the tie is met exactly
        assert int(e[0, 0]) == shift
        got = float(R.code_values(codes)[0, 1])
        assert abs(got) == want and (int(codes[0, 1]) & 1) == 0, (value, got)
        assert (int(codes[0, 1]) >> 5) == (1 if sign < 0 else 0)
        assert abs(want - value) == min(abs(v - value) for v in R.CODEBOOK)
        # one ulp to either side of the tie goes to the nearer value
        t = torch.tensor(value * s, dtype=torch.float32)
        up = float(torch.nextafter(t, torch.tensor(float("inf"))))
        dn = float(torch.nextafter(t, torch.tensor(0.0)))
        codes, _ = R.quantize(block([7.5 * s, up, dn]))
        vals = R.code_values(codes)[0]
        lo = max(v for v in R.CODEBOOK if v < value)
        hi = min(v for v in R.CODEBOOK if v > value)
        assert float(vals[1]) == hi and float(vals[2]) == lo


def test_exponent_clamps_at_plus_and_minus_127():
    tiny = torch.tensor(2.0 ** -140, dtype=torch.float32)            # a denormal: ceil(log2(amax / 7.5)) = -142
    assert int(R.exponent(tiny)) == -127
    codes, e = R.quantize(block([2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -131, 2.0 ** -126, 2.0 ** -140, 3 * 2.0 ** -131]))
    assert int(e[0, 0]) == -127
    # x 2^127: 1, 1.5, 0.0625 (a tie between 0 and 0.125: to 0), 2, 0, 0.1875 (a tie between 0.125 and 0.25: to 0.25)
    assert R.code_values(codes)[0, :6].tolist() == [1.0, 1.5, 0.0, 2.0, 0.0, 0.25]
    huge = torch.tensor(torch.finfo(torch.float32).max)
    assert int(R.exponent(huge)) == 126                               # the largest float: below the clamp
    # no finite fp32 reaches +127; the clamp itself, on a wider type
    assert int(R.exponent(torch.tensor(7.5 * 2.0 ** 127, dtype=torch.float64))) == 127
    assert int(R.exponent(torch.tensor(2.0 ** 200, dtype=torch.float64))) == 127
    assert R.scale_image(torch.tensor([[127, -127]]), 64)[:, 0].tolist() == [254, 0]


def test_pack_unpack_round_trip_and_the_bit_order_of_a_group_of_32():
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 64, (5, 96), generator=g).to(torch.uint8)
    q = R.pack(codes)
    assert q.shape == (5, 72)
    assert torch.equal(R.unpack(q), codes)
    # the documented order, bit by bit: bit b of a block's 192 is bit b % 6 of the code of k = b / 6
    blk = codes[2, 32:64].tolist()
    stream = q[2, 24:48].tolist()
    for b in range(192):
        assert (stream[b // 8] >> (b % 8)) & 1 == (blk[b // 6] >> (b % 6)) & 1, b
    one = torch.zeros(1, 32, dtype=torch.uint8)
    one[0, 0], one[0, 1], one[0, 31] = 0x21, 0x3F, 0x2A
    p = R.pack(one)[0].tolist()
    assert p[0] == 0x21 | (0x3F << 6) & 0xFF and p[1] == (0x3F >> 2) and p[2] == 0    # code 1 straddles bytes 0 and 1
    assert p[23] == 0x2A << 2 and sum(p[3:23]) == 0                                   # code 31 is the top six bits of byte 23
    x = torch.randn(7, 64, generator=g)
    codes, e = R.quantize(x)
    back = R.dequantize(R.unpack(R.pack(codes)), e)
    assert torch.equal(R.dequantize(codes, e), back)
    assert float((back - x.double()).abs().max()) <= float(x.abs().max()) / 15.0      # half a top-binade step of 0.5 / 7.5


def test_scale_image_row_order():
    e = torch.arange(70 * 2).view(70, 2) % 50 - 25
    s = R.scale_image(e, 128, fill=0xEE)
    assert torch.equal(R.scale_rows(s, 70), e)
    assert int(s[0, 4 * 5 + 1]) == int(e[16 + 5, 0]) + 127             # row 21 = 16 + 5 sits at 4 * 5 + 1 of its group of 64
    assert int((s == 0xEE).sum()) == 2 * (128 - 70)
    assert torch.equal(R.mx_perm(torch.arange(300)), R4.mx_perm(torch.arange(300)))   # the image of the other MX formats


def _mx_fp8(x):
    """the values MX fp8 holds of x: e = ceil(log2(amax / 448)) (448 = 0.875 2^9), elements e4m3 of x 2^-e"""
    M, K = x.shape
    xb = x.double().view(M, K // 32, 32)
    f, ex = torch.frexp(xb.abs().amax(dim=-1))
    e = torch.where(f <= 0.875, ex - 9, ex - 8).clamp(-127, 127).double()[..., None]
    q = (xb * torch.exp2(-e)).float().to(torch.float8_e4m3fn).double()
    return (q * torch.exp2(e)).view(M, K)


def test_w6a6_is_as_close_as_mx_fp8_and_twice_as_close_as_mxfp4_on_a_gaussian_gemm():
    g = torch.Generator().manual_seed(14)
    M, N, K = 256, 512, 1536
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.02
    ref = a.double() @ w.double().t()

    def err(fq):
        return float((fq(a) @ fq(w).t() - ref).norm() / ref.norm())

    e8, e6 = err(_mx_fp8), err(R.fake_quant)
    e4 = err(lambda x: R4.dequantize(*R4.quantize(x)))
    print(f"relative L2 from float64: MX fp8 {e8:.4f}, MXFP6 e2m3 {e6:.4f} ({e6 / e8:.2f} x), MXFP4 {e4:.4f} ({e6 / e4:.2f} x)")
    assert e6 <= 1.25 * e8
    assert e6 <= 0.5 * e4

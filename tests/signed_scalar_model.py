"""A pure-Python model of how the engine recodes the signed and 128-bit narrow scalar formats (test infrastructure; no GPU, no oracle).

A format is (width in bytes, signed).  A signed format holds two's-complement little-endian integers; the engine recodes the MAGNITUDE |v| with
the windows of the width and applies the sign to every digit (include/msm_hip.h, MSM_HIP_SCALAR_SIGNED):
  - widths 1 and 2 (byte windows): window j is byte j of |v|, an unsigned digit weighing 2^(8 j);
  - widths 4, 8 and 16: nwin = (8 w + C) / C signed C-bit digits of |v| -- chunk + carry, minus 2^C with a carry into the next window when
    that reaches 2^(C-1) (recode.h, bias_scalar) -- weighing 2^(C k); the top window holds only what the carry leaves.
tests/test_signed_scalar_abi.py checks that the digits reassemble every value; tests/test_gpu_signed_scalars.py compares the engine's digit
planes with them."""

FORMATS = {"i8": (1, True), "i16": (2, True), "i32": (4, True), "i64": (8, True), "u128": (16, False), "i128": (16, True)}
WINDOW_BITS = (12, 14, 16)


def value_range(width, signed):
    """(min, max) of the format"""
    bits = 8 * width
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def edge_values(width, signed):
    """0, +1, -1, the maximum, the minimum (whose magnitude does not fit the signed type), and 2^127 for the 128-bit formats' magnitude"""
    lo, hi = value_range(width, signed)
    vals = [0, 1, hi, lo]
    if signed:
        vals += [-1, lo + 1]
    if width == 16:
        vals.append(-(1 << 127) if signed else 1 << 127)
    return vals


def encode(values, width, signed):
    """integers -> n x width bytes, little-endian (two's complement if signed): the wire form of the format"""
    lo, hi = value_range(width, signed)
    assert all(lo <= v <= hi for v in values)
    return b"".join(int(v).to_bytes(width, "little", signed=signed) for v in values)


def scalars32(values, r):
    """the 32-byte canonical scalars v mod r: what the oracle, and the 32-byte path of the engine, are fed"""
    return b"".join((int(v) % r).to_bytes(32, "little") for v in values)


def byte_windows(width):
    return width in (1, 2)


def windows(width, c):
    """windows of one value: the bytes (byte windows), or (8 w + C) / C"""
    return width if byte_windows(width) else (8 * width + c) // c


def weights(width, c):
    """what window k weighs in the host's combine"""
    return [1 << ((8 if byte_windows(width) else c) * k) for k in range(windows(width, c))]


def magnitude_digits(mag, width, c):
    """the digits of the magnitude: bytes, or the signed C-bit recode"""
    assert 0 <= mag < 1 << (8 * width)
    if byte_windows(width):
        return [(mag >> (8 * j)) & 0xFF for j in range(width)]
    half, out, carry = 1 << (c - 1), [], 0
    for k in range(windows(width, c)):
        d = ((mag >> (c * k)) & ((1 << c) - 1)) + carry
        carry = 0
        if d >= half:
            d -= 1 << c
            carry = 1
        out.append(d)
    assert carry == 0, "the recode of a narrow magnitude never overflows its windows"
    return out


def digits(v, width, signed, c):
    """the digits the engine accumulates for v: those of |v| with v's sign applied"""
    lo, hi = value_range(width, signed)
    assert lo <= v <= hi
    return [-d if v < 0 else d for d in magnitude_digits(abs(v), width, c)]


def decode_plane(code, c):
    """a debug digit plane's u16 code (msm_hip_read_digits) -> the digit: bit 15 the sign, the low bits the magnitude, magnitude 0 under a set sign
    bit = 2^(C-1)"""
    mag = code & 0x7FFF
    return -(mag or 1 << (c - 1)) if code >> 15 else mag


def plane_digit(d, c):
    """what the debug planes can show of digit d: themselves, except +2^(C-1) -- the negation of a magnitude's digit -2^(C-1) -- for which
    the u16 code has no room at 16 bits and which reads as 0 at every width (the sort entry, slot 0 with a clear sign bit, is right: the MSM's
    result shows that)"""
    return 0 if d == 1 << (c - 1) else d

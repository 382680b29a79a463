"""Pure-Python model of the scalar-field transform of libmsm_fr.so (include/msm_fr.h): out[i] = c * t^i * sum_j s^j * omega^(i j) * a[j] over
Python integers -- an iterative radix-2 NTT, and the O(n^2) definition it is checked against (tests/test_ntt_host.py)."""


def ntt_definition(a, omega, r, pre=1, post=1, c=1):
    n = len(a)
    return [c * pow(post, i, r) * sum(pow(pre, j, r) * pow(omega, i * j, r) * a[j] for j in range(n)) % r for i in range(n)]


def ntt(a, omega, r, pre=1, post=1, c=1):
    """a: n = 2^k integers below r; omega: a primitive n-th root of unity mod r.  Natural order in and out."""
    n = len(a)
    assert n and n & (n - 1) == 0
    bits = n.bit_length() - 1
    x, s = [0] * n, 1
    for j in range(n):  # the pre-shift, into bit-reversed order
        x[int(format(j, "0%db" % bits)[::-1], 2) if bits else 0] = a[j] * s % r
        s = s * pre % r
    half = 1
    while half < n:
        w_step = pow(omega, n // (2 * half), r)
        for start in range(0, n, 2 * half):
            w = 1
            for k in range(start, start + half):
                u, v = x[k], x[k + half] * w % r
                x[k], x[k + half] = (u + v) % r, (u - v) % r
                w = w * w_step % r
        half *= 2
    t = c % r
    for i in range(n):
        x[i] = x[i] * t % r
        t = t * post % r
    return x


def intt(a, omega, r, shift=1):
    """the inverse of ntt(a, omega, r, pre=shift)"""
    n = len(a)
    return ntt(a, pow(omega, r - 2, r), r, post=pow(shift, r - 2, r), c=pow(n, r - 2, r))


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]

"""Pure-Python model of libmsm_frvec.so (include/msm_frvec.h) over Python integers: the five maps, the inverse with 1 / 0 = 0, and the four scans.
Values are PLAIN integers below r; a vector in the mont256 form is taken out of it and put back with mont()."""

MAPS = ("add", "sub", "mul", "mul_add", "mul_sub")
OPS = {"add": 0, "sub": 1, "mul": 2, "mul_add": 3, "mul_sub": 4}  # MSM_FRVEC_ADD ..
SCANS = {"sum": 0, "product": 1}  # MSM_FRVEC_SUM, MSM_FRVEC_PRODUCT


def _broadcast(v, n):
    return [v] * n if isinstance(v, int) else list(v)


def map_op(op, a, b, c, r):
    """a: a list; b, c: a list of the same length, or an integer that is broadcast (c: None where the op has no third operand)"""
    n = len(a)
    b = _broadcast(b, n)
    c = _broadcast(c, n) if c is not None else [0] * n
    assert len(b) == n and len(c) == n
    f = {"add": lambda x, y, z: x + y, "sub": lambda x, y, z: x - y, "mul": lambda x, y, z: x * y, "mul_add": lambda x, y, z: x * y + z,
         "mul_sub": lambda x, y, z: x * y - z}[op]
    return [f(x, y, z) % r for x, y, z in zip(a, b, c)]


def inverse(a, r):
    return [pow(x, r - 2, r) if x % r else 0 for x in a]


def scan(a, op, exclusive, r, batch=1):
    """-> (out, totals): `batch` rows of len(a) / batch values, each scanned on its own"""
    n = len(a) // batch
    assert n * batch == len(a)
    out, totals = [], []
    for v in range(batch):
        acc = 1 if op == "product" else 0
        for x in a[v * n:(v + 1) * n]:
            if exclusive:
                out.append(acc)
            acc = acc * x % r if op == "product" else (acc + x) % r
            if not exclusive:
                out.append(acc)
        totals.append(acc)
    return out, totals


def mont(vals, r, back=False):
    """plain values -> a * 2^256 mod r (back=True: the other way)"""
    f = pow(2, 256, r)
    if back:
        f = pow(f, r - 2, r)
    return [v * f % r for v in vals]


def to_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def from_bytes(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]

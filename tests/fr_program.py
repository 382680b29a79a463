"""Programs over the nine scalar-field libraries (libmsm_fr, frvec, frpoly, frmle, frmat, frgate, frlook, frhash, frcol): a generator, and a model interpreter
that predicts every byte a program leaves on the device.  Needs no GPU, no HIP and no torch: tools/fuzz_fr.py runs the programs on the device and
compares, tests/test_fr_program.py checks the tester itself.

A program is a list of steps (kind, field index, arguments): tuples of ints, strings, lists and dicts, replayable from their repr alone.  Every
field of a program has an ARENA of 32-byte scalars on the device; an operand is a range [off16, n] of it: n scalars from byte 16 * off16 on.  The
arena has two halves: in the first a scalar starts at 0 mod 32, in the second at 16 mod 32 (the arena's base is aligned far more strictly), so every
byte is always read at the same alignment and stays part of one canonical scalar.  Each half is four banks; an output is exactly one of the inputs
or lies in a bank that no input of the call touches -- or, in an "overlap" step, overlaps an input in part, which the headers say is refused.

The model mirrors an arena as its STORED bytes: a step decodes its operands under the field's current form (canonical, or a * 2^256 mod r),
computes with the per-library models of this directory, and encodes again -- so set_scalar_format changes no byte, only how later steps read.

libmsm_frhash's steps: "poseidon" makes a handle in a slot from a seed (its constants: poseidon_constants) and touches no device -- the handle's
table goes there inside its first call, on whichever stream and under whichever form that call has; "permute", "sponge" and "tree" call it on
ranges of the arena or, with host set, on the bytes of those ranges, in which case the result is the step's host value and no range is
written.  An output that cuts the input is refused by the Python layer (REFUSED), not by the library.  A "plant" step with quiet set puts a value
that is not below r where the next step does NOT read (the padding between a sponge's rows): that step must not be refused, and heals it.
"poseidon2" makes a Poseidon2 handle (frhash2_model.Poseidon2; its constants: poseidon2_constants) in the same three slots; the three calls take
it unchanged.

libmsm_frcol's steps: "expand", "pair" and "gather" (msm_webgpu_amd.columns) move scalars AS STORED, whatever the field's form, by 32-bit WORD
VECTORS, of which every field keeps up to three in slots -- lists in the model, int32 or uint32 tensors on the device.  A slot is filled by a
"mult" step that names it (cslot: its counts, islot: its indices; the backend keeps the very tensor the call returned) or by a "words" step,
which uploads a vector the generator drew and calls no library.  Counts that do not add up to the outputs and an index that is neither inside
`a` nor MISSING are refused by the Python layer (REFUSED) after the library looked: the output range is then among the step's writes -- unchanged
for a wrong sum, with that element zero for a bad index.  An output that cuts an input or the other output is refused before the C call like a
hash step's cut (column_cut), and like it is not flagged "overlap".  NO VALUE >= r IS PLANTED before a column step: the library does not
compare with r, so the value would be copied into the arena and the NEXT step refused for the wrong reason.

libmsm_frmle's steps "mle_fold", "mle_eval", "eq" and "round" take an ORDER: order="low" is MSM_FRMLE_LOW_FIRST (the variable x_j at bit j of the
index; the device side calls msm_webgpu_amd.multilinear), no order argument is top first (the context's scalars_* methods), so a program printed
before there was an order replays as it is.  The model of a low-first step is tests/frmle_low_model.py.  A low-first bind IN PLACE -- an
mle_fold onto its input, a round with `fold` -- leaves the scalars [n / 2, n) of every row UNSPECIFIED (include/msm_frmle.h): the model keeps
them as they were and names exactly those ranges in "rewrite", so the driver writes the model's bytes there; [0, n / 2) is compared, and [n, stride)
and all the rest must not change, which the whole-arena compare at the end sees to.  "gemini" is multilinear.gemini_folds of one row of 2^k
scalars, k >= 1: the folds f_1 | .. | f_k, n - 1 scalars, copied from the tensor the call returns into a range of the arena; a planted value in
the row refuses it (ERR_NONCANONICAL) before that copy, so the range stays as it was.  Behind a top-first step the generator sometimes puts the
same entry point low first with no step between -- on either field, small behind large and large behind small --, and behind an mle_eval a
low-first fused round of fewer levels: the scratch rows of the round then lie where the eval's levels lay."""
import functools
import hashlib
import random

from tests import frcol_model, frgate_model, frhash2_model, frhash_model, frlook_model, frmat_model, frmle_low_model, frmle_model, frpoly_model, frvec_model, ntt_model

FIELD_R = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "grumpkin": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
    "pallas": 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001,
    "vesta": 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
    "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}
BANK, BANKS = 4608, 4  # scalars to a bank, banks to a half of the arena
HALF = BANK * BANKS
ARENA16 = 4 * HALF + 2  # the arena in units of 16 bytes: half A, 16 bytes that nobody writes, half B, 16 more
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2051, 4097)
# The work of a Poseidon step is permutations x rounds x t^2, and the generator keeps it at or below HASH_WORK so that the Python model of one step
# (frhash_model.Poseidon.permute) stays at about 0.1 s.  Measured on a CPU without a GPU, BN254 (BLS12-381 within 6 %), microseconds per unit of work:
# t = 2, rounds (2, 0): 3.6; t = 3, (2, 0): 2.5; t = 3, (2, 1): 2.3; t = 4, (4, 2): 1.7; t = 5, (2, 3): 1.3; t = 7, (2, 2): 1.1; t = 9, (4, 2): 0.96;
# t = 12, (2, 1): 0.83; t = 3, (8, 57): 1.8; t = 12, (8, 60): 0.69.  37000 units are 0.094 s at t = 3, the width of the widest step there is (a
# tree over 2048 leaves, rounds (2, 0): 36846 units), and at most 0.09 s above it; at t = 2 the largest step the lengths below allow is 1025 lanes
# of 8 rounds, 32800 units: 0.12 s.
HASH_WORK = 37000
# Poseidon2 (frhash2_model.Poseidon2.permute) has no matrix product: an external round costs t S-boxes and a few additions, an internal one an S-box
# and t products.  Its unit of work is permutations x (3 R_F t + R_P (t + 3)).  (Per permutations x (R_F t + R_P) x t the cost is no constant: 0.23 us
# at t = 12, (4, 2) and 1.64 at t = 2, (8, 56).)  Measured on the same kind of CPU, BN254 (BLS12-381 within 5 %), microseconds per unit: t = 2,
# rounds (2, 0): 0.86; t = 2, (2, 3): 0.74; t = 3, (2, 0): 0.79; t = 3, (2, 1): 0.75; t = 3, (4, 2): 0.75; t = 4, (4, 2): 0.73; t = 4, (2, 3): 0.74;
# t = 8, (2, 1): 0.89; t = 8, (4, 2): 0.86; t = 8, (8, 0): 0.88; t = 12, (2, 1): 0.85; t = 12, (2, 3): 0.79; t = 12, (4, 2): 0.79; t = 2, (8, 56): 0.72;
# t = 3, (8, 57): 0.70; t = 4, (8, 56): 0.68; t = 8, (8, 60): 0.68; t = 12, (8, 60): 0.67.  112000 units are 0.1 s at the dearest of these and 0.075 s
# at the cheapest.
HASH2_WORK = 112000
LARGE, SMALL = 1023, 65  # a "large" step has an operand of at least LARGE scalars to a row, a "small" one at most SMALL
ERR_INVALID_ARG, ERR_NONCANONICAL, REFUSED = -2, -4, "refused"  # MSM_HIP_ERR_*; REFUSED: the Python layer raises ValueError before the C call
HOOKS = {"fr_test_pass_bits": (0, 1, 2, 3, 5), "frvec_test_tile": (0, 2, 3, 8, 64), "frpoly_test_tile": (0, 2, 3, 8, 64), "frmle_test_tile": (0, 2, 8, 64),
         "frmat_test_tile": (0, 2, 8, 64), "frlook_test_hash_bits": (0, 1, 3, 8), "frhash_test_tile": (0, 1, 3, 4, 64), "frcol_test_tile": (0, 2, 3, 8, 64)}
LIBRARY = {"map": "frvec", "inverse": "frvec", "scan": "frvec", "fft": "fr", "eval": "frpoly", "divide": "frpoly", "dot": "frpoly", "combine": "frpoly",
           "powers": "frpoly", "mle_fold": "frmle", "mle_eval": "frmle", "eq": "frmle", "round": "frmle", "gemini": "frmle", "matrix": "frmat", "matvec": "frmat", "gate": "frgate",
           "vanishing_inverse": "frgate", "quotient": "frgate", "table": "frlook", "mult": "frlook", "poseidon": "frhash", "poseidon2": "frhash", "permute": "frhash", "sponge": "frhash", "tree": "frhash", "expand": "frcol", "pair": "frcol", "gather": "frcol"}
LIBRARIES = ("fr", "frvec", "frpoly", "frmle", "frmat", "frgate", "frlook", "frhash", "frcol")
GRUMPKIN_KINDS = ("mle_fold", "mle_eval", "eq", "round", "gemini", "matrix", "matvec", "gate", "table", "mult", "poseidon", "poseidon2", "permute", "sponge", "tree", "expand", "pair",
                  "gather")  # the libraries that serve its scalar field
FRMLE_ORDERED = ("mle_fold", "mle_eval", "eq", "round")  # the steps that take an order: "low" (MSM_FRMLE_LOW_FIRST), or none, which is top first
HASH_CALLS = ("permute", "sponge", "tree")  # the steps that call libmsm_frhash ("poseidon" and "poseidon2" touch no device)
HASH_MAKERS = ("poseidon", "poseidon2")  # the steps that make a handle: its kind
COLUMN_CALLS = ("expand", "pair", "gather")  # the steps that call libmsm_frcol
HASH_WIDTHS = (2, 3, 4, 5, 7, 8, 9, 10, 12)
HASH2_WIDTHS = frhash2_model.WIDTHS
MISSING = frcol_model.MISSING
WORD_SLOTS = 3
# the widest state whose S-box input the kernel leaves untidied, and the first it tidies: (t + 4)^2 against the field's FQ_HEADROOM (csrc/frhash_kernels.h)
HASH_BOUNDARY = {"bls12_381": (4, 5), "pallas": (7, 8), "vesta": (7, 8), "bn254": (9, 10), "grumpkin": (9, 10)}
KINDS = tuple(LIBRARY) + ("words", "format", "hook", "close", "stream", "plant", "overlap")


def label(step):
    """what a step counts as: its kind, "overlap" where its output overlaps an input in part"""
    return "overlap" if step[2].get("overlap") else step[0]


@functools.lru_cache(maxsize=None)
def root_of_unity(r, log_n):
    """the smallest quadratic non-residue raised to (r - 1) / 2^log_n: what api.root_of_unity gives (the driver compares the two)"""
    g = 2
    while pow(g, (r - 1) // 2, r) != r - 1:
        g += 1
    return pow(g, (r - 1) >> log_n, r)


def expand(seed, count, r):
    """`count` integers below r from an integer seed, by SHAKE-256: no random generator is needed to replay a step"""
    raw = hashlib.shake_256(b"fr_program/%d" % seed).digest(40 * count)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % r for i in range(count)]


def initial_arena(seed):
    """16 * ARENA16 bytes whose every aligned 16-byte half ends in a byte below 16: a scalar read at either alignment is below 2^252 < r"""
    b = bytearray(hashlib.shake_256(b"fr_program/arena/%d" % seed).digest(16 * ARENA16))
    b[15::16] = bytes(x & 15 for x in b[15::16])
    return b


def _cuts(a, b):
    """do the ranges [off16, n] a and b share a byte"""
    return a[0] < b[0] + 2 * b[1] and b[0] < a[0] + 2 * a[1]


class Model:
    """the interpreter: step() applies a step to the mirrored arenas and returns what the device must have done --
    {"error": None / ERR_* / REFUSED, "writes": [(off16, n), ..] ranges the step wrote (compared), "rewrite": ranges that are unspecified after a
    predicted ERR_NONCANONICAL (the driver rewrites them from the model), "host": the host values the call returns (None where there are none)}"""

    def __init__(self, fields):
        self.fields = list(fields)
        self.r = [FIELD_R[f] for f in self.fields]
        self.arena = [bytearray(16 * ARENA16) for _ in self.fields]
        self.mont = [False] * len(self.fields)
        self.mats = [{} for _ in self.fields]
        self.tabs = [{} for _ in self.fields]
        self.hashes = [{} for _ in self.fields]  # slot -> frhash_model.Poseidon or frhash2_model.Poseidon2
        self.words = [{} for _ in self.fields]  # slot -> a list of 32-bit words
        self.planted = [{} for _ in self.fields]  # off16 -> the 32 bytes a planted value replaced
        self.quiet = [{} for _ in self.fields]  # the same for a value planted where the next step does NOT read: it must not be refused
        self.hooks = {h: 0 for h in HOOKS}
        self.side_stream = False

    # ---- the arena -------------------------------------------------------------------------------------------------------------------------
    def raw(self, f, rng):
        return bytes(self.arena[f][16 * rng[0]:16 * rng[0] + 32 * rng[1]])

    def stored(self, f, rng):
        return frvec_model.from_bytes(self.raw(f, rng))

    def plain(self, f, rng):
        v = self.stored(f, rng)
        return frvec_model.mont(v, self.r[f], back=True) if self.mont[f] else v

    def enc(self, f, vals):
        """plain values -> bytes in the field's current form"""
        vals = [v % self.r[f] for v in vals]
        return frvec_model.to_bytes(frvec_model.mont(vals, self.r[f]) if self.mont[f] else vals)

    def put(self, f, off16, data):
        self.arena[f][16 * off16:16 * off16 + len(data)] = data

    def _heal(self, f, planted):
        spots = []
        for off16, old in planted.items():
            self.put(f, off16, old)
            spots.append((off16, 1))
        planted.clear()
        return spots

    def _run(self, f, reads, writes, compute, loose=(), kept=False):
        """reads: the ranges whose every scalar the call compares with r; writes: what it writes; compute() -> ([(off16, bytes), ..], host);
        loose: ranges that the call leaves unspecified even where it succeeds (the model keeps them as they were, the driver rewrites them);
        kept: a refused call leaves `writes` as they were (the whole-arena compare at the end sees to it) instead of unspecified"""
        if self.planted[f]:
            hit = any(_cuts((p, 1), rd) and (p - rd[0]) % 2 == 0 for p in self.planted[f] for rd in reads)
            assert hit, "a planted value must be read by the step that follows it"
            lost = [] if kept else [tuple(w) for w in writes] + [tuple(w) for w in loose]
            return {"error": ERR_NONCANONICAL, "writes": [], "rewrite": lost + self._heal(f, self.planted[f]), "host": None}
        assert not any(_cuts((p, 1), rd) for p in self.quiet[f] for rd in reads), "a quietly planted value lies where the step that follows it does not read"
        puts, host = compute()
        for off16, data in puts:
            self.put(f, off16, data)
        return {"error": None, "writes": [(off16, len(data) // 32) for off16, data in puts], "rewrite": [tuple(w) for w in loose] + self._heal(f, self.quiet[f]), "host": host}

    @staticmethod
    def _fail(code):
        return {"error": code, "writes": [], "rewrite": [], "host": None}

    @staticmethod
    def _partial(out, ins):
        """an output that shares bytes with an input without starting where it starts"""
        return any(_cuts(out, i) and out[0] != i[0] for i in ins)

    def step(self, step):
        kind, f, a = step
        out = getattr(self, "op_" + kind)(f, **{k: v for k, v in a.items() if k != "overlap"})
        assert bool(a.get("overlap")) == (out["error"] == ERR_INVALID_ARG), "an overlap step, and only that, is refused with ERR_INVALID_ARG"
        return out

    # ---- steps that call no library ------------------------------------------------------------------------------------------------------------
    def op_init(self, f, seed):
        self.arena[f] = initial_arena(seed)
        self.planted[f].clear()
        self.quiet[f].clear()
        return {"error": None, "writes": [], "rewrite": [(0, ARENA16 // 2)], "host": None}

    def op_format(self, f, mont):
        self.mont[f] = bool(mont)
        return self._fail(None)

    def op_hook(self, f, name, value):
        assert value in HOOKS[name]
        self.hooks[name] = value
        return self._fail(None)

    def op_stream(self, f, side):
        self.side_stream = bool(side)
        return self._fail(None)

    def op_close(self, f, what, slot):
        del {"mat": self.mats, "tab": self.tabs, "hash": self.hashes}[what][f][slot]
        return self._fail(None)

    def op_plant(self, f, at, value, quiet=False):
        assert self.r[f] <= value < 1 << 256 and at not in self.planted[f] and at not in self.quiet[f]
        (self.quiet if quiet else self.planted)[f][at] = self.raw(f, (at, 1))
        self.put(f, at, value.to_bytes(32, "little"))
        return {"error": None, "writes": [(at, 1)], "rewrite": [], "host": None}

    # ---- libmsm_frvec --------------------------------------------------------------------------------------------------------------------------
    def op_map(self, f, op, a, b, c, out):
        dst = a if out is None else out
        vecs = [v for v in (a, b, c) if isinstance(v, (list, tuple))]
        if self._partial(dst, vecs):
            return self._fail(ERR_INVALID_ARG)

        def compute():
            val = lambda v: v if v is None or isinstance(v, int) else self.plain(f, v)
            return [(dst[0], self.enc(f, frvec_model.map_op(op, self.plain(f, a), val(b), val(c), self.r[f])))], None
        return self._run(f, vecs, [dst], compute)

    def op_inverse(self, f, a, out):
        dst = a if out is None else out
        if self._partial(dst, [a]):
            return self._fail(ERR_INVALID_ARG)
        return self._run(f, [a], [dst], lambda: ([(dst[0], self.enc(f, frvec_model.inverse(self.plain(f, a), self.r[f])))], None))

    def op_scan(self, f, a, op, exclusive, batch, out, totals):
        dst = a if out is None else out
        if self._partial(dst, [a]):
            return self._fail(ERR_INVALID_ARG)

        def compute():
            res, tot = frvec_model.scan(self.plain(f, a), op, exclusive, self.r[f], batch)
            return [(dst[0], self.enc(f, res))], (self.enc(f, tot) if totals else None)
        return self._run(f, [a], [dst], compute)

    # ---- libmsm_fr -----------------------------------------------------------------------------------------------------------------------------
    def op_fft(self, f, a, log_n, batch, inverse, shift, omega):
        r, n = self.r[f], 1 << log_n
        assert a[1] == batch * n

        def compute():
            w = root_of_unity(r, log_n) if omega is None else omega
            v, res = self.plain(f, a), []
            for k in range(batch):
                row = v[k * n:(k + 1) * n]
                res += ntt_model.intt(row, w, r, shift or 1) if inverse else ntt_model.ntt(row, w, r, pre=shift or 1)
            return [(a[0], self.enc(f, res))], None
        return self._run(f, [a], [a], compute)

    # ---- libmsm_frpoly -------------------------------------------------------------------------------------------------------------------------
    def op_eval(self, f, a, z, batch):
        return self._run(f, [a], [], lambda: ([], self.enc(f, [frpoly_model.evaluate(row, z, self.r[f]) for row in frpoly_model.rows_of(self.plain(f, a), batch)])))

    def op_divide(self, f, a, z, batch, out, values):
        dst = a if out is None else out
        if self._partial(dst, [a]):
            return self._fail(ERR_INVALID_ARG)

        def compute():
            q, vals = [], []
            for row in frpoly_model.rows_of(self.plain(f, a), batch):
                qq, y = frpoly_model.divide(row, z, self.r[f])
                q += qq
                vals.append(y)
            return [(dst[0], self.enc(f, q))], (self.enc(f, vals) if values else None)
        return self._run(f, [a], [dst], compute)

    def op_dot(self, f, a, b, batch):
        def compute():
            rows, other = frpoly_model.rows_of(self.plain(f, a), batch), self.plain(f, b)
            n = len(rows[0])
            return [], self.enc(f, [frpoly_model.dot(row, other[:n] if b[1] == n else other[k * n:(k + 1) * n], self.r[f]) for k, row in enumerate(rows)])
        return self._run(f, [a, b], [], compute)

    def op_combine(self, f, a, coeffs, out):
        if self._partial(out, [a]):
            return self._fail(ERR_INVALID_ARG)
        return self._run(f, [a], [out], lambda: ([(out[0], self.enc(f, frpoly_model.combine(frpoly_model.rows_of(self.plain(f, a), len(coeffs)), coeffs, self.r[f])))], None))

    def op_powers(self, f, g, n, scale, out):
        assert out[1] == n
        return self._run(f, [], [out], lambda: ([(out[0], self.enc(f, frpoly_model.powers(g, n, self.r[f], scale)))], None))

    # ---- libmsm_frmle --------------------------------------------------------------------------------------------------------------------------
    def _rows(self, f, a, batch, n):
        """-> (stride, the first n plain values of every row, the ranges of those)"""
        stride = a[1] // batch
        assert stride * batch == a[1] and n <= stride
        v = self.plain(f, a)
        return stride, [v[k * stride:k * stride + n] for k in range(batch)], [(a[0] + 2 * k * stride, n) for k in range(batch)]

    @staticmethod
    def _mle(order):
        """the model of an order: "top" (the steps leave it out) or "low" (MSM_FRMLE_LOW_FIRST) -- the latter never with code from the package"""
        assert order in ("top", "low")
        return frmle_low_model if order == "low" else frmle_model

    @staticmethod
    def _upper_halves(first, batch, stride, n):
        """the scalars [n / 2, n) of every row: what a low-first bind in place leaves unspecified (include/msm_frmle.h)"""
        return [(first + 2 * (k * stride + n // 2), n // 2) for k in range(batch)]

    def op_mle_fold(self, f, a, c, batch, n, out, order="top"):
        dst = a if out is None else out
        stride = a[1] // batch
        span = (dst[0], (batch - 1) * stride + n)
        if self._partial(span, [(a[0], span[1])]):
            return self._fail(ERR_INVALID_ARG)
        _, rows, reads = self._rows(f, a, batch, n)
        model = self._mle(order)
        loose = self._upper_halves(dst[0], batch, stride, n) if order == "low" and dst[0] == a[0] else []
        return self._run(f, reads, [(dst[0] + 2 * k * stride, n // 2) for k in range(batch)],
                         lambda: ([(dst[0] + 2 * k * stride, self.enc(f, model.fold(row, c, self.r[f]))) for k, row in enumerate(rows)], None), loose)

    def op_mle_eval(self, f, a, point, batch, n, order="top"):
        _, rows, reads = self._rows(f, a, batch, n)
        model = self._mle(order)
        return self._run(f, reads, [], lambda: ([], self.enc(f, [model.evaluate(row, point, self.r[f]) for row in rows])))

    def op_eq(self, f, point, scale, out, order="top"):
        assert out[1] == 1 << len(point)
        model = self._mle(order)
        return self._run(f, [], [out], lambda: ([(out[0], self.enc(f, model.eq(point, self.r[f], scale)))], None))

    def op_round(self, f, a, terms, batch, n, fold, order="top"):
        stride, rows, ranges = self._rows(f, a, batch, n)
        named = sorted({row for _, which in terms for row in which})
        reads = ranges if fold is not None else [ranges[k] for k in named]
        model = self._mle(order)

        def compute():
            puts, cur = [], rows
            if fold is not None:
                cur = [model.fold(row, fold, self.r[f]) for row in rows]
                puts = [(a[0] + 2 * k * stride, self.enc(f, row)) for k, row in enumerate(cur)]
            return puts, self.enc(f, model.round_values(cur, [(c, tuple(w)) for c, w in terms], self.r[f]))
        loose = self._upper_halves(a[0], batch, stride, n) if order == "low" and fold is not None else []
        return self._run(f, reads, [(rg[0], n // 2) for rg in ranges] if fold is not None else [], compute, loose)

    def op_gemini(self, f, a, point, out):
        """multilinear.gemini_folds of one row, copied into `out`: f_1 | .. | f_k; a refused call never gets as far as the copy"""
        n = a[1]
        assert n == 1 << len(point) and n >= 2 and out[1] == n - 1 and not _cuts(out, a)
        return self._run(f, [a], [out], lambda: ([(out[0], self.enc(f, [x for fj in frmle_low_model.gemini_folds(self.plain(f, a), point, self.r[f]) for x in fj]))], None),
                         kept=True)

    # ---- libmsm_frmat --------------------------------------------------------------------------------------------------------------------------
    def op_matrix(self, f, slot, rows, cols, row_ptr, col_idx, vseed, transpose):
        assert slot not in self.mats[f] and len(self.mats[f]) < 3
        self.mats[f][slot] = (rows, cols, list(row_ptr), list(col_idx), expand(vseed, len(col_idx), self.r[f]), bool(transpose))
        return self._fail(None)

    def op_matvec(self, f, slot, x, out, transpose, pad_to):
        rows, cols, row_ptr, col_idx, values, has_t = self.mats[f][slot]
        assert has_t or not transpose
        in_len, out_len = (rows, cols) if transpose else (cols, rows)
        y_len = out_len if pad_to is None else pad_to
        assert x[1] == in_len and out[1] == y_len
        if _cuts(out, x):
            return self._fail(ERR_INVALID_ARG)
        used = sorted({i for i in range(rows) if row_ptr[i + 1] > row_ptr[i]} if transpose else set(col_idx))  # the elements of x that are read

        def compute():
            y = frmat_model.matvec(rows, cols, row_ptr, col_idx, values, self.plain(f, x), self.r[f], transpose)
            return [(out[0], self.enc(f, y + [0] * (y_len - out_len)))], None
        return self._run(f, [(x[0] + 2 * j, 1) for j in used], [out], compute)

    # ---- libmsm_frgate -------------------------------------------------------------------------------------------------------------------------
    def op_gate(self, f, a, terms, batch, n, step, scale, out, accumulate):
        stride, rows, ranges = self._rows(f, a, batch, n)
        assert out[1] == n
        if _cuts(out, a) or (scale is not None and _cuts(out, scale)):
            return self._fail(REFUSED)  # (never in place: the Python layer raises before the C call)
        named = sorted({fr[0] for _, factors in terms for fr in factors})
        reads = [ranges[k] for k in named] + ([scale] if scale is not None else []) + ([out] if accumulate else [])

        def compute():
            res = frgate_model.apply(rows, terms, n, step, self.plain(f, scale) if scale is not None else None, self.plain(f, out) if accumulate else None, self.r[f])
            return [(out[0], self.enc(f, res))], None
        return self._run(f, reads, [out], compute)

    def op_vanishing_inverse(self, f, log_n, log_ext, shift, out):
        r = self.r[f]
        assert out[1] == 1 << log_ext
        return self._run(f, [], [out], lambda: ([(out[0], self.enc(f, frgate_model.vanishing_inverse(log_n, log_ext, shift, root_of_unity(r, log_n + log_ext), r)))], None))

    def op_quotient(self, f, a, terms, batch, log_n, log_ext, shift, out):
        r, n = self.r[f], 1 << log_n
        assert a[1] == batch * n and out[1] == n << log_ext

        def compute():
            cols = frpoly_model.rows_of(self.plain(f, a), batch)
            return [(out[0], self.enc(f, frgate_model.quotient(cols, terms, log_n, log_ext, shift, root_of_unity(r, log_n + log_ext), r)))], None
        return self._run(f, [a], [out], compute)

    # ---- libmsm_frlook -------------------------------------------------------------------------------------------------------------------------
    def op_table(self, f, slot, t, n):
        assert slot not in self.tabs[f] and len(self.tabs[f]) < 3 and n <= t[1]

        def compute():
            self.tabs[f][slot] = (self.stored(f, (t[0], n)), self.mont[f])  # keys are compared AS STORED; the form belongs to the handle
            return [], len(set(self.tabs[f][slot][0]))
        return self._run(f, [(t[0], n)], [], compute)  # (ERR_NONCANONICAL: no handle is made)

    def op_mult(self, f, slot, v, batch, n, out, indices, counts, cslot=None, islot=None):
        assert (cslot is None or counts) and (islot is None or indices) and (cslot is None or cslot != islot)
        keys, form = self.tabs[f][slot]
        stride = v[1] // batch
        assert out[1] == len(keys) and stride * batch == v[1] and 1 <= n <= stride and not _cuts(out, v)
        if form != self.mont[f]:
            return self._fail(REFUSED)  # (a count whose form differs from the handle's is refused)
        stored = self.stored(f, v)

        def compute():
            cnt, idx, missing, first, _ = frlook_model.lookup(keys, [stored[k * stride:(k + 1) * stride] for k in range(batch)], n)
            for wslot, words in ((cslot, cnt), (islot, idx)):  # the word vectors the call returned stay in the slots it names
                if wslot is not None:
                    self.words[f][wslot] = list(words)
            host = ((idx,) if indices else ()) + ((cnt,) if counts else ()) + ((missing, first if missing else None),)
            return [(out[0], self.enc(f, cnt))], host
        return self._run(f, [(v[0] + 2 * k * stride, n) for k in range(batch)], [out], compute)

    # ---- libmsm_frhash -------------------------------------------------------------------------------------------------------------------------
    def op_poseidon(self, f, slot, t, full_rounds, partial_rounds, seed, capacity, capacity_at, out_at):
        assert slot not in self.hashes[f] and len(self.hashes[f]) < 3 and t in HASH_WIDTHS
        rc, mds = poseidon_constants(seed, t, full_rounds, partial_rounds, self.r[f])
        self.hashes[f][slot] = frhash_model.Poseidon(self.r[f], t, full_rounds, partial_rounds, rc, mds, capacity, capacity_at, out_at)
        return self._fail(None)  # (no device is touched: the table goes there with the handle's first call)

    def op_poseidon2(self, f, slot, t, full_rounds, partial_rounds, seed, capacity, capacity_at, out_at):
        assert slot not in self.hashes[f] and len(self.hashes[f]) < 3 and t in HASH2_WIDTHS
        rc, mu = poseidon2_constants(seed, t, full_rounds, partial_rounds, self.r[f])
        self.hashes[f][slot] = frhash2_model.Poseidon2(self.r[f], t, full_rounds, partial_rounds, rc, mu, capacity, capacity_at, out_at)
        return self._fail(None)

    def _hashed(self, f, reads, out, host, values):
        """a call of libmsm_frhash: values() -> the plain results, which go to `out`, or come back as host bytes in the data's form where `host` is set"""
        def compute():
            data = self.enc(f, values())
            return ([], data) if host else ([(out[0], data)], None)
        return self._run(f, reads, [] if host else [out], compute)

    def op_permute(self, f, slot, a, out, host):
        p = self.hashes[f][slot]
        dst = a if out is None else out
        assert a[1] % p.t == 0 and dst[1] == a[1] and not (host and out is not None)
        if hash_cut(("permute", f, {"a": a, "out": out, "host": host})):
            return self._fail(REFUSED)

        def values():
            v = self.plain(f, a)
            return [x for i in range(0, len(v), p.t) for x in p.permute(v[i:i + p.t])]
        return self._hashed(f, [a], dst, host, values)

    def op_sponge(self, f, slot, a, batch, length, out, host):
        p = self.hashes[f][slot]
        stride = a[1] // batch
        assert stride * batch == a[1] and 1 <= length <= stride and (host or out[1] == batch)
        if hash_cut(("sponge", f, {"a": a, "out": out, "host": host})):
            return self._fail(REFUSED)

        def values():
            v = self.plain(f, a)  # (the padding behind `length` decodes to whatever it does: it is not used)
            return [p.hash(v[k * stride:k * stride + length]) for k in range(batch)]
        return self._hashed(f, [(a[0] + 2 * k * stride, length) for k in range(batch)], out, host, values)

    def op_tree(self, f, slot, leaves, levels, out, host):
        p = self.hashes[f][slot]
        assert (levels is not None and leaves[1] == 1) if p.t == 2 else levels is None
        if hash_cut(("tree", f, {"leaves": leaves, "out": out, "host": host})):
            return self._fail(REFUSED)

        def values():
            v = self.plain(f, leaves)
            nodes = p.merkle_chain(v[0], levels) if p.t == 2 else [x for level in p.merkle(v) for x in level]
            assert host or len(nodes) == out[1]
            return nodes
        return self._hashed(f, [leaves], out, host, values)


    # ---- libmsm_frcol: scalars AS STORED, whatever the field's form ---------------------------------------------------------------------------------
    def op_words(self, f, slot, values):
        assert 0 <= slot < WORD_SLOTS and values and all(0 <= w < 1 << 32 for w in values)
        self.words[f][slot] = list(values)
        return self._fail(None)

    def _moved(self, f, puts, refused=False):
        """a column call that copies: puts [(range, stored values)] -- nothing is compared with r; refused: the Python layer raises all the same"""
        out = self._run(f, [], [rng for rng, _ in puts], lambda: ([(rng[0], frvec_model.to_bytes(vals)) for rng, vals in puts], None))
        return dict(out, error=REFUSED) if refused else out

    def op_expand(self, f, t, counts, bias, out):
        cnt = self.words[f][counts]
        assert len(cnt) == t[1] and bias in (0, 1) and 1 <= out[1] <= BANK
        if column_cut(("expand", f, {"t": t, "out": out})):
            return self._fail(REFUSED)
        if frcol_model.total(cnt, bias) != out[1]:  # (the sum in 64 bits: one that is n_out only in 32 bits is refused too)
            return self._moved(f, [(out, self.stored(f, out))], True)
        return self._moved(f, [(out, frcol_model.expand(self.stored(f, t), cnt, bias))])

    def op_pair(self, f, t, counts, out, s_out):
        cnt = self.words[f][counts]
        assert len(cnt) == t[1] == out[1] == s_out[1]
        if column_cut(("pair", f, {"t": t, "out": out, "s_out": s_out})):
            return self._fail(REFUSED)
        if frcol_model.total(cnt) != t[1]:
            return self._moved(f, [(out, self.stored(f, out)), (s_out, self.stored(f, s_out))], True)
        a_perm, s_perm, _ = frcol_model.pair(self.stored(f, t), cnt)
        return self._moved(f, [(out, a_perm), (s_out, s_perm)])

    def op_gather(self, f, a, idx, out):
        words = self.words[f][idx]
        assert len(words) == out[1]
        if column_cut(("gather", f, {"a": a, "out": out})):
            return self._fail(REFUSED)
        vals, ok = frcol_model.gather(self.stored(f, a), words)
        return self._moved(f, [(out, vals)], not ok)  # (a bad index: that element zero, the others as usual, and ValueError)


FRMLE_TILE = 1024  # csrc/frmle_kernels.h; frmle_test_tile replaces it


def plan_levels(n, tile):
    """csrc/frmle_plan.h's plan_levels: the values per row, level by level, until one tile holds a level"""
    lens = [n]
    while -(-lens[-1] // tile) > 1:
        lens.append(-(-lens[-1] // tile))
    return lens


def eval_levels(n, hook=0):
    """the levels (launches) of an mle_eval of n scalars under frmle_test_tile `hook`: levels 1 .. live in the shared scratch"""
    return len(plan_levels(n, hook or FRMLE_TILE))


def low_fused_partials(n, hook=0):
    """the levels of partial sums of a low-first fused round of n >= 4 scalars under frmle_test_tile `hook`: they lie in the shared scratch between
    `partial` and the scratch rows (csrc/frmle_plan.h: plan_low_fused, plan_levels_low_fused; csrc/frmle_host.h: rows = scratch + lv.words).  0: one
    pair, one launch, the values go straight to the result"""
    tile = hook or FRMLE_TILE
    pairs, launch_tile = n // 4, tile // 2
    lower = pairs // 2
    partials = sum(-(-count // launch_tile) for count in (lower, pairs - lower) if count)
    return len(plan_levels(partials, tile)) if partials > 1 else 0


def column_cut(step):
    """is this a call of libmsm_frcol whose output shares bytes with an input or with the other output -- a same start included: the Python
    layer refuses it (REFUSED) before the C call, with nothing written"""
    kind, _, a = step
    if kind == "expand":
        return _cuts(a["out"], a["t"])
    if kind == "pair":
        return _cuts(a["out"], a["t"]) or _cuts(a["s_out"], a["t"]) or _cuts(a["out"], a["s_out"])
    return kind == "gather" and _cuts(a["out"], a["a"])


def poseidon2_constants(seed, t, full_rounds, partial_rounds, r):
    """-> (round constants, mu) of a Poseidon2 handle from its integer seed; 0, 1 and r - 1 are among the round constants (there are at least
    four) and among mu (at t = 2, which has room for two, 1 and r - 1)"""
    n = full_rounds * t + partial_rounds
    vals = expand(seed, n + t, r)
    for k, special in enumerate((0, 1, r - 1)):
        vals[(seed + k) % n] = special
        vals[n + ((seed >> 8) + k) % t] = special
    return vals[:n], vals[n:]


def poseidon_constants(seed, t, full_rounds, partial_rounds, r):
    """-> (round constants, matrix rows) of a handle from its integer seed, as expand gives matrix values; 0, 1 and r - 1 are among them"""
    n = (full_rounds + partial_rounds) * t
    vals = expand(seed, n + t * t, r)
    for k, special in enumerate((0, 1, r - 1)):
        vals[(seed + k) % n] = special  # among the round constants (there are at least four)
        vals[n + ((seed >> 8) + k) % (t * t)] = special  # and in the matrix
    return vals[:n], [vals[n + i * t:n + (i + 1) * t] for i in range(t)]


def hash_cut(step):
    """is this a device-form call of libmsm_frhash whose output shares bytes with its input where it must not: the Python layer refuses it
    (REFUSED) before the C call.  A permutation may be in place; a sponge's and a tree's output lies apart from the whole input."""
    kind, _, a = step
    if kind not in HASH_CALLS or a["host"]:
        return False
    if kind == "permute":
        return a["out"] is not None and Model._partial(a["out"], [a["a"]])
    return _cuts(a["out"], a["a"] if kind == "sponge" else a["leaves"])


class Refused(Exception):
    """what a backend raises where a call fails: code is ERR_* or REFUSED"""

    def __init__(self, code):
        super().__init__("refused: %r" % (code,))
        self.code = code


class ModelBackend:
    """a backend that IS the model: tools/fuzz_fr.py run against it must report success (tests/test_fr_program.py plants its faults in
    subclasses of this).  One method per step kind, plus the arena's read and write."""

    def __init__(self, fields):
        self.m = Model(fields)

    def read16(self, f, lo, hi):
        """the bytes of the 16-byte units lo .. hi of the arena"""
        return bytes(self.m.arena[f][16 * lo:16 * hi])

    def write(self, f, off16, data):
        self.m.put(f, off16, data)

    def reset(self):
        """between programs: no hook, no handle, the canonical form; the arenas stay as they are"""
        arenas = self.m.arena
        self.m = Model(self.m.fields)
        self.m.arena = arenas

    def close(self):
        pass

    def __getattr__(self, name):
        if not name.startswith("op_"):
            raise AttributeError(name)
        return lambda f, **a: self.call(name[3:], f, a)

    def call(self, kind, f, a):
        """one step: the model's own; a call the model refuses raises Refused like the device side"""
        out = getattr(self.m, "op_" + kind)(f, **a)
        if out["error"] is not None:
            raise Refused(out["error"])
        return out["host"]


def sizes(steps):
    """-> [(index, kind, field, scalars per row)] of the steps that call a library and have a size: the length of a row of the largest operand; for
    a sparse product the entries of its matrix (its work); for a Poseidon step its lanes: the states of a permute, the rows of a sponge, the nodes
    of a tree's first level; for a column step its outputs (of a pair: to a column), and none where its output cuts an operand: the library is
    not called.  What "large" (>= LARGE) and "small" (<= SMALL) are measured on."""
    out, nnz, width = [], {}, {}
    for i, (kind, f, a) in enumerate(steps):
        if kind == "matrix":
            nnz[f, a["slot"]] = len(a["col_idx"])
        if kind in HASH_MAKERS:
            width[f, a["slot"]] = a["t"]
        if a.get("overlap") or kind not in LIBRARY or column_cut((kind, f, a)):
            continue
        if kind in ("map", "inverse", "gemini"):
            n = a["a"][1]
        elif kind in ("scan", "eval", "divide", "dot"):
            n = a["a"][1] // a["batch"]
        elif kind == "fft":
            n = 1 << a["log_n"]
        elif kind in ("combine", "eq", "expand", "pair", "gather"):
            n = a["out"][1]
        elif kind in ("powers", "mle_fold", "mle_eval", "round", "gate", "mult"):
            n = a["n"]
        elif kind == "matvec":
            n = nnz[f, a["slot"]]
        elif kind == "table":
            n = a["t"][1]
        elif kind == "permute":
            n = a["a"][1] // width[f, a["slot"]]
        elif kind == "sponge":
            n = a["batch"]
        elif kind == "tree":
            n = a["leaves"][1] // max(width[f, a["slot"]] - 1, 1)  # (arity 1: a chain over one leaf)
        else:
            continue
        out.append((i, kind, f, n))
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------------
_WEIGHT = {"map": 10, "inverse": 5, "scan": 8, "fft": 8, "eval": 4, "divide": 5, "dot": 4, "combine": 4, "powers": 4, "mle_fold": 5, "mle_eval": 4, "eq": 5,
           "round": 6, "gemini": 6, "matrix": 4, "matvec": 8, "gate": 7, "vanishing_inverse": 2, "quotient": 2, "table": 4, "mult": 8, "poseidon": 4, "poseidon2": 4, "permute": 10, "sponge": 9, "tree": 7,
           "expand": 7, "pair": 6, "gather": 6, "words": 4, "format": 5, "hook": 8, "close": 3, "stream": 3, "overlap": 4}
_LEN_WEIGHT = {1: 6, 2: 6, 63: 6, 64: 6, 65: 6, 255: 3, 256: 3, 257: 3, 1023: 1.6, 1024: 1.6, 1025: 1.6, 2051: 0.9, 4097: 0.6}
_PLANTABLE = ("map", "inverse", "scan", "fft", "eval", "divide", "dot", "combine", "mle_fold", "mle_eval", "round", "gemini", "matvec", "gate", "table", "mult", "permute", "sponge", "tree")
_OVERLAPS = ("map", "inverse", "scan", "divide", "combine", "mle_fold", "matvec", "expand", "pair", "gather")  # (the last three: cuts, refused by the Python layer)
_BAD_WORDS = 0.07  # how often a word vector drawn for a column call is one that must be refused


class _Gen:
    def __init__(self, rnd, fields, kinds):
        self.rnd, self.fields, self.r = rnd, list(fields), [FIELD_R[f] for f in fields]
        self.kinds = [k for k in _WEIGHT if kinds is None or k in kinds]
        self.mont = [False] * len(fields)
        self.mats = [{} for _ in fields]  # slot -> (rows, cols, transpose, row_ptr, col_idx)
        self.tabs = [{} for _ in fields]  # slot -> (n, form, the range it was made of)
        self.hashes = [{} for _ in fields]  # slot -> (t, the work of one permutation, the handle's kind)
        self.words = [{} for _ in fields]  # slot -> {"what": "counts" / "idx", "n": its length, "total": the sum of the counts, "bound": the least n_a of an idx}
        self.host_before = False  # was the last call of libmsm_frhash a host-form one
        self.last_hash, self.force_slot, self.no_plant = None, None, False  # the handle of the last hash call; the handle the next one is to take
        self.side = False
        self.steps = []
        self.prev_f, self.follow = None, None  # follow: (field, kind) of a large step that a small one of the same entry point is to follow
        self.plant_ok = kinds is None or "plant" in kinds
        self.last_fft = {}  # field -> (log_n, omega) of its last transform
        self.hooks_set = []  # the names the last hook draw set
        self.hooks = {h: 0 for h in HOOKS}  # as the steps so far leave them
        # what run() asks of the next frmle step: its order, a table of 2^10 or more, a fused round, a table of exactly force_n scalars
        self.force_order, self.force_big, self.force_fold, self.force_n = None, False, False, None

    # ---- draws ---------------------------------------------------------------------------------------------------------------------------
    def scalar(self, f):
        c = self.rnd.random()
        return self.rnd.choice((0, 1, 2, self.r[f] - 1)) if c < 0.15 else self.rnd.randrange(self.r[f])

    def length(self, small, cap=BANK):
        if small:
            return self.rnd.choice((1, 2, 63, 64, 65))
        pool = [n for n in LENGTHS if n <= cap]
        return self.rnd.choices(pool, [_LEN_WEIGHT[n] for n in pool])[0]

    def log_n(self, small, least=0, most=12):
        if self.force_n is not None:
            return self.force_n.bit_length() - 1
        if self.force_big:
            return self.rnd.choice((10, 10, 11, 12))
        if small:
            return self.rnd.randrange(least, 7)
        pool = list(range(least, most + 1))
        return self.rnd.choices(pool, [6 if k <= 6 else 3 if k <= 8 else 1.5 if k <= 10 else 0.8 for k in pool])[0]

    def batch(self, n, most=5):
        return self.rnd.choice([b for b in (1, 1, 2, 3, 5) if b * n <= BANK and b <= most])

    def place(self, n, avoid=()):
        """a range of n scalars in a bank that none of the ranges `avoid` touches: (off16, n)"""
        taken = {self.bank_of(a) for a in avoid}
        while True:
            half, bank = (1 if self.rnd.random() < 0.4 else 0), self.rnd.randrange(BANKS)
            if (half, bank) not in taken:
                break
        at = 0 if self.rnd.random() < 0.3 else self.rnd.randrange(BANK - n + 1)
        return [half * (2 * HALF + 1) + 2 * (bank * BANK + at), n]

    @staticmethod
    def bank_of(rng):
        half = 1 if rng[0] > 2 * HALF else 0
        return half, (rng[0] - half * (2 * HALF + 1)) // 2 // BANK

    def out_for(self, ins, n, same):
        """an output of n scalars: exactly one of the ranges `same` (in place), or in a bank of its own"""
        same = [s for s in same if s[1] == n and not Model._partial(s, ins)]  # (two inputs may overlap one another, but then neither is the output)
        if same and self.rnd.random() < 0.5:
            return list(self.rnd.choice(same))
        return self.place(n, ins)

    def emit(self, kind, f, **a):
        self.steps.append((kind, f, a))

    def order(self):
        """the order of a frmle step, drawn per step: -> the step's order argument, which a top-first step leaves out (an old printed program replays)"""
        low = self.force_order == "low" if self.force_order else self.rnd.random() < 0.5
        return {"order": "low"} if low else {}

    def maybe_plant(self, f, kind, spots, chance=0.09):
        """before a step that reads the scalars `spots` (off16 each): sometimes plant a value >= r in one of them"""
        if self.plant_ok and not self.no_plant and kind in _PLANTABLE and spots and self.rnd.random() < chance:
            r = self.r[f]
            self.emit("plant", f, at=self.rnd.choice(spots), value=self.rnd.choice((r, r + 1, (1 << 256) - 1, r + self.rnd.randrange(1 << 200))))

    @staticmethod
    def spots(rng, rnd, rows=None, stride=None, n=None):
        """some scalars of a range (of the first n of its rows): first, last, one between"""
        if rows is None:
            picks = {0, rng[1] - 1, rnd.randrange(rng[1])}
        else:
            picks = {k * stride + i for k in rows for i in (0, n - 1, rnd.randrange(n))}
        return [rng[0] + 2 * i for i in sorted(picks)]

    # ---- one step kind each; `small` asks for operands of at most SMALL scalars; -> the scalars per row, or None ---------------------------------
    def g_map(self, f, small, overlap=False):
        n = self.length(small, 2051 if overlap else BANK)
        n = max(n, 2) if overlap else n
        op = self.rnd.choice(frvec_model.MAPS)
        a = self.place(n)
        operand = lambda: self.scalar(f) if self.rnd.random() < 0.35 else (list(a) if self.rnd.random() < 0.15 else self.place(n))
        b = operand()
        c = operand() if op in ("mul_add", "mul_sub") else None
        vecs = [v for v in (a, b, c) if isinstance(v, list)]
        if overlap:
            out = self.shifted(self.rnd.choice(vecs))
        else:
            out = self.out_for(vecs, n, vecs)
            if out == a and self.rnd.random() < 0.5:
                out = None
            self.maybe_plant(f, "map", self.spots(self.rnd.choice(vecs), self.rnd))
        self.emit("map", f, op=op, a=a, b=b, c=c, out=out, **({"overlap": True} if overlap else {}))
        return n

    def shifted(self, rng, n=None, least=1):
        """a range of n scalars (default: as many) that starts `least` or more scalars into rng and stays inside its bank; rng is moved to the
        start of the bank where there is no room behind it"""
        n = rng[1] if n is None else n
        half, bank = self.bank_of(rng)
        base = half * (2 * HALF + 1) + 2 * bank * BANK
        room = BANK - (rng[0] - base) // 2 - n  # the largest shift that keeps the n scalars inside the bank
        if room < least:
            rng[0], room = base, BANK - n
        return [rng[0] + 2 * self.rnd.randrange(least, min(rng[1] - 1, room) + 1), n]

    def g_inverse(self, f, small, overlap=False):
        n = max(self.length(small, 2051 if overlap else BANK), 2 if overlap else 1)
        a = self.place(n)
        if overlap:
            out = self.shifted(a)
        else:
            out = self.out_for([a], n, [a]) if self.rnd.random() < 0.6 else None
            self.maybe_plant(f, "inverse", self.spots(a, self.rnd))
        self.emit("inverse", f, a=a, out=out, **({"overlap": True} if overlap else {}))
        return n

    def g_scan(self, f, small, overlap=False):
        n = self.length(small, 2051 if overlap else BANK)
        batch = self.batch(n)
        if overlap and n * batch < 2:
            n = 2
        a = self.place(n * batch)
        if overlap:
            out = self.shifted(a)
        else:
            out = self.out_for([a], n * batch, [a]) if self.rnd.random() < 0.6 else None
            self.maybe_plant(f, "scan", self.spots(a, self.rnd))
        self.emit("scan", f, a=a, op=self.rnd.choice(("sum", "product")), exclusive=self.rnd.random() < 0.5, batch=batch, out=out, totals=self.rnd.random() < 0.5,
                  **({"overlap": True} if overlap else {}))
        return n

    def g_fft(self, f, small):
        log_n = self.log_n(small)
        again = self.last_fft.get(f)
        if again and again[0] >= 2 and not small and self.rnd.random() < 0.4:  # the length of this field's last transform, with another root
            log_n = again[0]
        n = 1 << log_n
        batch = self.batch(n, 3)
        a = self.place(n * batch)
        omega = None
        if (again[1] is None) if again and again[0] == log_n else self.rnd.random() < 0.4:  # a caller's root: an odd power of the default one is primitive too
            omega = pow(root_of_unity(self.r[f], log_n), self.rnd.choice((3, 5, 7)) if log_n else 1, self.r[f])
        self.last_fft[f] = (log_n, omega)
        self.maybe_plant(f, "fft", self.spots(a, self.rnd))
        self.emit("fft", f, a=a, log_n=log_n, batch=batch, inverse=self.rnd.random() < 0.4, shift=self.rnd.randrange(1, self.r[f]) if self.rnd.random() < 0.4 else None,
                  omega=omega)
        return n

    def g_eval(self, f, small):
        n = self.length(small)
        batch = self.batch(n)
        a = self.place(n * batch)
        self.maybe_plant(f, "eval", self.spots(a, self.rnd))
        self.emit("eval", f, a=a, z=self.scalar(f), batch=batch)
        return n

    def g_divide(self, f, small, overlap=False):
        n = self.length(small, 2051 if overlap else BANK)
        batch = self.batch(n)
        if overlap and n * batch < 2:
            n = 2
        a = self.place(n * batch)
        if overlap:
            out = self.shifted(a)
        else:
            out = self.out_for([a], n * batch, [a]) if self.rnd.random() < 0.6 else None
            self.maybe_plant(f, "divide", self.spots(a, self.rnd))
        self.emit("divide", f, a=a, z=self.scalar(f), batch=batch, out=out, values=self.rnd.random() < 0.5, **({"overlap": True} if overlap else {}))
        return n

    def g_dot(self, f, small):
        n = self.length(small)
        batch = self.batch(n)
        a = self.place(n * batch)
        b = list(a) if self.rnd.random() < 0.15 else self.place(n if batch > 1 and self.rnd.random() < 0.5 else n * batch)
        self.maybe_plant(f, "dot", self.spots(self.rnd.choice((a, b)), self.rnd))
        self.emit("dot", f, a=a, b=b, batch=batch)
        return n

    def g_combine(self, f, small, overlap=False):
        n = max(self.length(small, 1025), 2 if overlap else 1)
        k = self.rnd.choice([k for k in (1, 2, 3, 4) if k * n <= BANK])
        a = self.place(n * k)
        if overlap:
            out = self.shifted(a, n)
        else:
            out = [a[0], n] if self.rnd.random() < 0.4 else self.place(n, [a])
            self.maybe_plant(f, "combine", self.spots(a, self.rnd))
        self.emit("combine", f, a=a, coeffs=[self.scalar(f) for _ in range(k)], out=out, **({"overlap": True} if overlap else {}))
        return n

    def g_powers(self, f, small):
        n = self.length(small)
        g = self.rnd.choice((1, self.r[f] - 1, 2)) if self.rnd.random() < 0.4 else self.scalar(f)  # (a base of small order: a table with repeated values)
        self.emit("powers", f, g=g, n=n, scale=self.scalar(f) if self.rnd.random() < 0.5 else 1, out=self.place(n))
        return n

    def table_rows(self, small, least, most_batch):
        """-> (n, batch, stride) of a call over rows `stride` apart whose first n = 2^k scalars are the table"""
        n = 1 << self.log_n(small, least)
        batch = self.batch(n + 1, most_batch)
        return n, batch, n + self.rnd.choice((0, 0, 1, 3) if (n + 3) * batch <= BANK else (0,))

    def g_mle_fold(self, f, small, overlap=False):
        n, batch, stride = self.table_rows(small, 1, 5)
        order = self.order()
        wide = bool(order) and not small and not overlap and self.force_n is None and self.rnd.random() < 0.12
        if wide:  # low first over several workgroups to a launch, rows further apart than the scratch rows: mostly in place
            n = self.rnd.choice((1024, 1024, 2048))
            batch, stride = (2 if n == 2048 else self.rnd.choice((2, 3))), n + self.rnd.choice((1, 3))
        a = self.place(batch * stride)
        if overlap:  # (what counts is the span from the first row's first scalar to the last row's n-th)
            span = [a[0], (batch - 1) * stride + n]
            out = self.shifted(span, batch * stride)
            a[0] = span[0]
        elif order and 2 * batch * n <= BANK and self.rnd.random() < 0.2:  # low first, apart: out begins on the byte behind a's last, as a Gemini fold's does
            stride = n
            a = self.place(2 * batch * n)
            a[1] = batch * n
            out = [a[0] + 2 * batch * n, batch * n]
            self.maybe_plant(f, "mle_fold", self.spots(a, self.rnd, range(batch), stride, n))
        else:
            out = self.out_for([a], batch * stride, [a]) if self.rnd.random() < (0.2 if wide else 0.5) else None
            in_place = out is None or out[0] == a[0]  # (low first in place: two launches read the row, a value is planted more often)
            self.maybe_plant(f, "mle_fold", self.spots(a, self.rnd, range(batch), stride, n), 0.2 if order and in_place and not wide else 0.09)
        self.emit("mle_fold", f, a=a, c=self.scalar(f), batch=batch, n=n, out=out, **order, **({"overlap": True} if overlap else {}))
        return n

    def g_mle_eval(self, f, small):
        n, batch, stride = self.table_rows(small, 0, 5)
        if not small and self.force_n is None and not self.force_big and self.rnd.random() < 0.2:
            # several levels in the shared scratch more often than log_n has them: two tiles of the design's 1024, or 2^6 and more under a small hook
            n = self.rnd.choice((64, 256, 512) if self.hooks["frmle_test_tile"] in (2, 8) else (2048, 2048, 4096))
            batch = self.rnd.choice((1, 2)) if 2 * n + 2 <= BANK else 1
            stride = n + self.rnd.choice((0, 1))
        a = self.place(batch * stride)
        self.maybe_plant(f, "mle_eval", self.spots(a, self.rnd, range(batch), stride, n))
        self.emit("mle_eval", f, a=a, point=[self.scalar(f) for _ in range(n.bit_length() - 1)], batch=batch, n=n, **self.order())
        return n

    def g_eq(self, f, small):
        k = self.log_n(small)
        if not small and self.force_n is None and self.rnd.random() < 0.12:  # (a long table more often than log_n has it: a short one is to follow it)
            k = self.rnd.choice((10, 11, 12))
        self.emit("eq", f, point=[self.scalar(f) for _ in range(k)], scale=self.scalar(f) if self.rnd.random() < 0.5 else 1, out=self.place(1 << k), **self.order())
        return 1 << k

    def g_round(self, f, small):
        fold = self.scalar(f) if self.rnd.random() < 0.5 or self.force_fold else None
        order = self.order()
        # a low-first fused round under a hook of 2 or 8 is long enough for several levels of partial sums between `partial` and the scratch rows
        if order and fold is not None and not small and self.force_n is None and not self.force_big and self.hooks["frmle_test_tile"] not in (2, 8) and not self.no_plant and "hook" in self.kinds and self.rnd.random() < 0.3:
            self.hooks["frmle_test_tile"] = self.rnd.choice((2, 8))  # (the hook steps alone set it too rarely for the schedules below)
            self.emit("hook", 0, name="frmle_test_tile", value=self.hooks["frmle_test_tile"])
        tiled = bool(order) and fold is not None and self.hooks["frmle_test_tile"] in (2, 8) and not small
        n, batch, stride = self.table_rows(small, 6 if tiled else 1 if fold is None else 2, 4)
        if tiled and self.force_n is None and self.hooks["frmle_test_tile"] == 8 and self.rnd.random() < 0.4:
            n, batch = 2048, min(batch, 2)  # tiles of four pairs: 128 partial sums, three levels of them
            stride = n + self.rnd.choice((0, 1))
        if order and fold is not None and self.force_n is None and not tiled and not self.force_big and self.rnd.random() < 0.3:
            pad = stride - n
            n = self.rnd.choice((4, 8))  # one pair in one launch; two launches of one pair
            stride = n + pad
        terms = [[self.scalar(f), [self.rnd.randrange(batch) for _ in range(self.rnd.randrange(1, 4 if n > 256 else 5))]] for _ in range(self.rnd.randrange(1, 4))]
        a = self.place(batch * stride)
        named = sorted({row for _, which in terms for row in which})
        self.maybe_plant(f, "round", self.spots(a, self.rnd, named, stride, n))
        self.emit("round", f, a=a, terms=terms, batch=batch, n=n, fold=fold, **order)
        return n

    def g_gemini(self, f, small):
        """the folds of one table of 2^k scalars, k >= 1, into n - 1 scalars of another bank; the lengths stop at 2^10: the model folds in Python"""
        n = 1 << self.log_n(small, 1, 10)
        a = self.place(n)
        self.maybe_plant(f, "gemini", self.spots(a, self.rnd))
        self.emit("gemini", f, a=a, point=[self.scalar(f) for _ in range(n.bit_length() - 1)], out=self.place(n - 1, [a]))
        return n

    def g_matrix(self, f, small):
        if len(self.mats[f]) == 3:
            self.g_close(f, small, "mat")
        slot = self.rnd.choice([s for s in range(3) if s not in self.mats[f]])
        rows, cols = self.rnd.choice((1, 2) if small else (1, 2, 63, 64, 65, 255, 257)), self.rnd.choice((1, 2, 63, 64, 65, 256, 257))
        row_ptr, col_idx = [0], []
        long_row = self.rnd.randrange(rows) if self.rnd.random() < 0.4 and not small else -1  # one row that crosses tiles, even without the hook's small ones
        for i in range(rows):
            k = self.rnd.choice((70, 300, 1100)) if i == long_row else (0 if self.rnd.random() < 0.3 else self.rnd.randrange(1, 5))
            col_idx += [self.rnd.randrange(cols) for _ in range(k)]
            row_ptr.append(len(col_idx))
        transpose = self.rnd.random() < 0.5
        self.mats[f][slot] = (rows, cols, transpose, row_ptr, col_idx)
        self.emit("matrix", f, slot=slot, rows=rows, cols=cols, row_ptr=row_ptr, col_idx=col_idx, vseed=self.rnd.randrange(1 << 30), transpose=transpose)
        return None

    def g_matvec(self, f, small, overlap=False):
        if not self.mats[f] or (small and min(len(m[4]) for m in self.mats[f].values()) > SMALL):
            self.g_matrix(f, small)
        slot = min(self.mats[f], key=lambda s: len(self.mats[f][s][4])) if small else self.rnd.choice(sorted(self.mats[f]))
        rows, cols, has_t, row_ptr, col_idx = self.mats[f][slot]
        transpose = has_t and self.rnd.random() < 0.5
        in_len, out_len = (rows, cols) if transpose else (cols, rows)
        pad_to = self.rnd.choice((None, None, out_len + 3, 1 << (out_len - 1).bit_length()))
        y_len = pad_to or out_len
        if not small and len(col_idx) >= LARGE and len(self.mats[f]) < 3 and min(len(m[4]) for m in self.mats[f].values()) > SMALL:
            self.g_matrix(f, True)  # a small matrix, alive for the small product that is to follow this large one with no step between
        x = self.place(in_len)
        if overlap:  # (x and y lie apart: the same start is refused too)
            out = self.shifted(x, y_len, 0)
        else:
            out = self.place(y_len, [x])
            used = sorted({i for i in range(rows) if row_ptr[i + 1] > row_ptr[i]} if transpose else set(col_idx))
            self.maybe_plant(f, "matvec", [x[0] + 2 * j for j in used[:1] + used[-1:]])
        self.emit("matvec", f, slot=slot, x=x, out=out, transpose=transpose, pad_to=pad_to, **({"overlap": True} if overlap else {}))
        return len(col_idx)  # (the work of a product is its entries)

    def g_gate(self, f, small):
        n, batch, stride = self.table_rows(small, 0, 5)
        big = n > 256
        terms = []
        for _ in range(self.rnd.randrange(1, 3 if big else 6)):
            rot = lambda: self.rnd.choice((0, 0, 1, -1, 2, -3, 5, 2 ** 31 - 1, -2 ** 31))
            terms.append([self.scalar(f), [[self.rnd.randrange(batch), rot()] for _ in range(self.rnd.randrange(1, 4 if big else 9))]])
        a = self.place(batch * stride)
        scale = self.place(1 << self.rnd.randrange(n.bit_length())) if self.rnd.random() < 0.5 else None
        out = self.place(n, [a] + ([scale] if scale else []))
        named = sorted({fr[0] for _, factors in terms for fr in factors})
        self.maybe_plant(f, "gate", self.spots(a, self.rnd, named, stride, n) + (self.spots(scale, self.rnd) if scale else []))
        self.emit("gate", f, a=a, terms=terms, batch=batch, n=n, step=self.rnd.choice((1, 1, n, 1 << self.rnd.randrange(n.bit_length()))), scale=scale, out=out,
                  accumulate=self.rnd.random() < 0.4)
        return n

    def coset_shift(self, f, log_n):
        while True:
            shift = self.rnd.randrange(2, self.r[f])
            if pow(shift, 1 << log_n, self.r[f]) not in (0, 1):
                return shift

    def g_vanishing_inverse(self, f, small):
        log_n, log_ext = self.rnd.randrange(0, 7), self.rnd.randrange(0, 4)
        self.emit("vanishing_inverse", f, log_n=log_n, log_ext=log_ext, shift=self.coset_shift(f, log_n + log_ext), out=self.place(1 << log_ext))
        return None

    def g_quotient(self, f, small):
        log_n, log_ext, batch = self.rnd.randrange(0, 5), self.rnd.randrange(0, 3), self.rnd.randrange(1, 4)
        top = (1 << log_ext) + 1  # 2^log_ext >= D - 1
        terms = [[self.scalar(f), [[self.rnd.randrange(batch), self.rnd.choice((0, 1, -1))] for _ in range(self.rnd.randrange(1, top + 1))]]
                 for _ in range(self.rnd.randrange(1, 4))]
        a = self.place(batch << log_n)
        self.emit("quotient", f, a=a, terms=terms, batch=batch, log_n=log_n, log_ext=log_ext, shift=self.coset_shift(f, log_n + log_ext),
                  out=self.place(1 << (log_n + log_ext), [a]))
        return None

    def g_table(self, f, small):
        if len(self.tabs[f]) == 3:
            self.g_close(f, small, "tab")
        slot = self.rnd.choice([s for s in range(3) if s not in self.tabs[f]])
        total = self.length(small, 1025)
        t = self.place(total)
        if self.fields[f] != "grumpkin" and self.rnd.random() < 0.3:  # repeated values: the powers of 1 or -1
            self.emit("powers", f, g=self.rnd.choice((1, self.r[f] - 1)), n=total, scale=self.scalar(f), out=list(t))
        n = total if self.rnd.random() < 0.7 else self.rnd.randrange(1, total + 1)
        before = len(self.steps)
        self.maybe_plant(f, "table", [t[0], t[0] + 2 * (n - 1)])
        if len(self.steps) == before:  # (a planted value: no handle is made)
            self.tabs[f][slot] = (n, self.mont[f], list(t))
        self.emit("table", f, slot=slot, t=t, n=n)
        return total

    def g_mult(self, f, small):
        if not self.tabs[f]:
            self.g_table(f, small)
            if not self.tabs[f]:
                return None
        slot = self.rnd.choice(sorted(self.tabs[f]))
        t_n, form, src = self.tabs[f][slot]
        n = self.length(small, 2051)
        batch = self.batch(n + 1, 3)
        stride = n + self.rnd.choice((0, 0, 2))
        c = self.rnd.random()
        if c < 0.45 and batch * stride <= src[1]:  # the table's own source: found, while nobody has written there since
            v = [src[0], batch * stride]
        elif c < 0.75:  # a window that lies partly on the source
            v = [src[0] + 2 * (src[1] // 2), batch * stride]
            half, _ = self.bank_of(src)
            if (v[0] - half * (2 * HALF + 1)) // 2 + v[1] > HALF:
                v = self.place(batch * stride)
        else:
            v = self.place(batch * stride)
        out = self.place(t_n, [v, [v[0] + 2 * v[1] - 2, 1]])
        before = len(self.steps)
        if form == self.mont[f]:
            self.maybe_plant(f, "mult", self.spots(v, self.rnd, range(batch), stride, n))
        indices, islot = self.rnd.random() < 0.6, None
        if indices and form == self.mont[f] and len(self.steps) == before and self.rnd.random() < 0.5:  # the call computes: its indices stay, -1 where a value is missing
            islot = self.rnd.randrange(WORD_SLOTS)
            self.words[f][islot] = {"what": "idx", "n": batch * n, "bound": t_n}
        self.emit("mult", f, slot=slot, v=v, batch=batch, n=n, out=out, indices=indices, counts=self.rnd.random() < 0.5, cslot=None, islot=islot)
        return n

    def chain(self, f, n_t, batch, n, want):
        """a table over n_t scalars and at once, under the same form and with nothing written between, the count of its source's first batch
        rows of n scalars -- every value is found, so the counts add up to batch * n -- which keeps its counts or indices (`want`) in a word
        slot: what libmsm_frcol is there to be chained behind.  -> (the table's source, the slot)"""
        assert batch * n <= n_t
        if len(self.tabs[f]) == 3:
            self.g_close(f, False, "tab")
        slot = self.rnd.choice([s for s in range(3) if s not in self.tabs[f]])
        t = self.place(n_t)
        if self.fields[f] != "grumpkin" and self.rnd.random() < 0.3:  # repeated values: every match goes to the lowest index, the other counts are 0
            self.emit("powers", f, g=self.rnd.choice((1, self.r[f] - 1)), n=n_t, scale=self.scalar(f), out=list(t))
        self.tabs[f][slot] = (n_t, self.mont[f], list(t))
        self.emit("table", f, slot=slot, t=list(t), n=n_t)
        wslot = self.rnd.randrange(WORD_SLOTS)
        other = (wslot + 1 + self.rnd.randrange(WORD_SLOTS - 1)) % WORD_SLOTS if self.rnd.random() < 0.3 else None  # the other vector too
        cslot, islot = (wslot, other) if want == "counts" else (other, wslot)
        for s, rec in ((cslot, {"what": "counts", "n": n_t, "total": batch * n}), (islot, {"what": "idx", "n": batch * n, "bound": n_t})):
            if s is not None:
                self.words[f][s] = rec
        self.emit("mult", f, slot=slot, v=[t[0], batch * n], batch=batch, n=n, out=self.place(n_t, [t]), indices=islot is not None, counts=cslot is not None, cslot=cslot,
                  islot=islot)
        return t, wslot

    # ---- libmsm_frcol: word vectors (words, or a count's that a chain left) and the three calls that take them.  `overlap`: an output that cuts an operand.
    def g_words(self, f, small):
        """a vector for a later column call to find: counts or indices"""
        if self.rnd.random() < 0.55:
            n_t = self.length(small, 2051)
            self.draw_counts(f, n_t, self.length(small, BANK - n_t))
        else:
            self.draw_indices(f, self.length(small), self.length(small))

    def draw_counts(self, f, n_t, total, zeros=None):
        """a `words` step of n_t counts that add up to `total` -- or, rarely, do not: off by one -> the slot.  zeros: must some counts be 0?"""
        names = [c for c in frcol_model.COUNT_SETS if zeros is None or (c != "all ones") == zeros]
        values = frcol_model.counts(self.rnd.choice(names), n_t, total, self.rnd)
        if self.rnd.random() < _BAD_WORDS:
            at = self.rnd.choice([j for j, c in enumerate(values) if c] or [0])
            values[at] += 1 if self.rnd.random() < 0.5 or not values[at] else -1
        return self.put_words(f, values, {"what": "counts", "n": n_t, "total": total})

    def draw_indices(self, f, n_a, n):
        """a `words` step of n indices into n_a scalars, MISSING among them -- or, rarely, one that is n_a or more -> the slot"""
        values = [MISSING if self.rnd.random() < 0.2 else self.rnd.randrange(n_a) for _ in range(n)]
        if self.rnd.random() < _BAD_WORDS:
            values[self.rnd.randrange(n)] = self.rnd.choice((n_a, n_a, n_a + 1, MISSING - 1))
        return self.put_words(f, values, {"what": "idx", "n": n, "bound": n_a})

    def put_words(self, f, values, rec):
        slot = self.rnd.randrange(WORD_SLOTS)
        self.words[f][slot] = rec
        self.emit("words", f, slot=slot, values=values)
        return slot

    def live_words(self, f, what, small, fits=lambda w: True):
        return [s for s, w in sorted(self.words[f].items()) if w["what"] == what and fits(w) and (not small or w["n"] <= SMALL)]

    def column_out(self, n, avoid, cut):
        """an output of n scalars apart from the ranges `avoid` -- or, where `cut` names one of them, across it: from its start or from inside it"""
        if cut is None:
            return self.place(n, avoid)
        if cut[1] > 1 and self.rnd.random() < 0.7:
            return self.shifted(cut, n, 0)
        half, bank = self.bank_of(cut)
        base = half * (2 * HALF + 1) + 2 * bank * BANK
        if (cut[0] - base) // 2 + n > BANK:  # (no room behind it in its bank: it moves to the bank's start, as in shifted)
            cut[0] = base
        return [cut[0], n]

    def g_expand(self, f, small, overlap=False):
        c, bias = self.rnd.random(), self.rnd.randrange(2)
        live = self.live_words(f, "counts", small, lambda w: 1 <= w["total"] + bias * w["n"] <= (SMALL if small else BANK))
        t = None
        if c < 0.04 and not small:  # four counts of 2^31: with the bias their sum is n_out in 32 bits, and 2^33 + 4 in fact
            n_t, bias, total = 4, 1, 0
            slot = self.put_words(f, [0x80000000] * 4, {"what": "counts", "n": 4, "total": 0})
        elif live and c < 0.35:  # a vector that is there: a count's that an earlier chain left, as the call left it, or an earlier step's
            slot = self.rnd.choice(live)
            n_t, total = self.words[f][slot]["n"], self.words[f][slot]["total"]
        elif c < 0.65 and not overlap:
            n_t = self.rnd.choice((1, 2, 21, 32)) if small else self.length(False, 1025)  # (a lookup table: as long as g_table's)
            n = self.rnd.choice([k for k in (1, 2, 21, 32) + LENGTHS if k <= n_t])
            batch = self.rnd.choice([b for b in (1, 1, 2, 3, 5) if b * n <= n_t])
            total = batch * n
            t, slot = self.chain(f, n_t, batch, n, "counts")
            t = list(t) if self.rnd.random() < 0.5 else None  # the table's own source, or any other range
        else:
            n_out = self.length(small)
            bias = bias if n_out > 1 else 0
            n_t = self.rnd.choice([k for k in LENGTHS if k < n_out]) if bias else self.length(small or self.rnd.random() < 0.3, 2051)
            total = n_out - bias * n_t
            slot = self.draw_counts(f, n_t, total)
        t = self.place(n_t) if t is None else t
        out = self.column_out(total + bias * n_t, [t], t if overlap else None)
        self.emit("expand", f, t=t, counts=slot, bias=bias, out=out)
        return None if overlap else out[1]

    def g_pair(self, f, small, overlap=False):
        c = self.rnd.random()
        live = self.live_words(f, "counts", small, lambda w: w["total"] == w["n"])
        t = None
        if c < 0.03 and not small:
            n = 4
            slot = self.put_words(f, [0x80000000] * 4, {"what": "counts", "n": 4, "total": 0})
        elif live and c < 0.25:
            slot = self.rnd.choice(live)
            n = self.words[f][slot]["n"]
        elif c < 0.65 and not overlap:  # a count of the table's own source, whole: batch rows of n / batch
            n = self.length(small, 1025)
            batch = self.rnd.choice([b for b in (1, 1, 2, 3, 5) if n % b == 0])
            t, slot = self.chain(f, n, batch, n // batch, "counts")
        else:
            n = self.length(small)
            slot = self.draw_counts(f, n, n, zeros=self.rnd.random() < 0.7)
        t = self.place(n) if t is None else list(t)
        cut = self.rnd.randrange(3) if overlap else None  # A' across t, S' across t, S' across A'
        out = self.column_out(n, [t], t if cut == 0 else None)
        s_out = self.column_out(n, [t, out], None if cut in (None, 0) else t if cut == 1 else out)
        self.emit("pair", f, t=t, counts=slot, out=out, s_out=s_out)
        return None if overlap else n

    def g_gather(self, f, small, overlap=False):
        c = self.rnd.random()
        live = self.live_words(f, "idx", small)
        if live and c < 0.4:  # indices that are there: a count's, with -1 for a value it did not find, or an earlier step's
            slot = self.rnd.choice(live)
        elif c < 0.6 and not overlap:
            n_t = self.rnd.choice((1, 2, 21, 32)) if small else self.length(False, 1025)  # (a lookup table: as long as g_table's)
            n = self.rnd.choice([k for k in (1, 2, 21, 32) + LENGTHS if k <= n_t])
            _, slot = self.chain(f, n_t, self.rnd.choice([b for b in (1, 1, 2, 3, 5) if b * n <= n_t]), n, "idx")
        else:
            slot = self.draw_indices(f, self.length(small and self.rnd.random() < 0.5), self.length(small))
        w = self.words[f][slot]
        a = self.place(min(w["bound"] + self.rnd.choice((0, 0, 3)), BANK))
        out = self.column_out(w["n"], [a], a if overlap else None)
        self.emit("gather", f, a=a, idx=slot, out=out)
        return None if overlap else w["n"]

    # ---- libmsm_frhash: a handle of either kind (poseidon, poseidon2) and the three calls on it.  The work of a call stays within HASH_WORK or HASH2_WORK.
    def g_poseidon(self, f, small):
        if len(self.hashes[f]) == 3:
            self.g_close(f, small, "hash")
        slot = self.rnd.choice([s for s in range(3) if s not in self.hashes[f]])
        edge = HASH_BOUNDARY[self.fields[f]]
        t = self.rnd.choices(HASH_WIDTHS, [4 if w in edge else 2 if w <= 4 else 1 for w in HASH_WIDTHS])[0]  # (t <= 4: the widths that a large call can have)
        t = self.width_of_the_other_kind(f, "poseidon2", t)
        rf, rp = self.rounds()
        self.hashes[f][slot] = (t, (rf + rp) * t * t, "poseidon")
        self.emit("poseidon", f, slot=slot, t=t, full_rounds=rf, partial_rounds=rp, seed=self.rnd.randrange(1 << 30), **self.convention(f, t))
        return None

    def g_poseidon2(self, f, small):
        if len(self.hashes[f]) == 3:
            self.g_close(f, small, "hash")
        slot = self.rnd.choice([s for s in range(3) if s not in self.hashes[f]])
        t = self.rnd.choice(HASH2_WIDTHS)
        t = self.width_of_the_other_kind(f, "poseidon", t, HASH2_WIDTHS)
        rf, rp = self.rounds()
        self.hashes[f][slot] = (t, 3 * rf * t + rp * (t + 3), "poseidon2")
        self.emit("poseidon2", f, slot=slot, t=t, full_rounds=rf, partial_rounds=rp, seed=self.rnd.randrange(1 << 30), **self.convention(f, t))
        return None

    def rounds(self):
        rf, rp = self.rnd.choice(((2, 0), (2, 0), (2, 1), (2, 1), (2, 3), (4, 2), (8, 0)))
        if self.rnd.random() < 0.06:  # as long as the standard shapes: its calls have few lanes, by their work
            rf, rp = 8, self.rnd.randrange(56, 67)
        return rf, rp

    def convention(self, f, t):
        """a sponge's capacity convention: circomlib's (0, 0, 0), halo2's (L 2^64, t - 1, 0), neptune's (2^arity - 1, 0, 1), and others"""
        r = self.r[f]
        return {"capacity": self.rnd.choice((0, (3 << 64) % r, (1 << (t - 1)) - 1, r - 1, self.rnd.randrange(r))), "capacity_at": self.rnd.choice((0, t - 1, self.rnd.randrange(t))),
                "out_at": self.rnd.choice((0, 1 % t, self.rnd.randrange(t)))}

    def width_of_the_other_kind(self, f, kind, t, widths=HASH_WIDTHS):
        """t, or sometimes the width of a live handle of the other kind: both kinds alive at one width"""
        there = sorted({h[0] for h in self.hashes[f].values() if h[2] == kind and h[0] in widths})
        return self.rnd.choice(there) if there and self.rnd.random() < 0.5 else t

    def hash_handle(self, f, small):
        """-> (slot, t, the permutations one call may run): a live handle, made first where there is none"""
        if self.force_slot is not None:
            slot = self.force_slot
        else:
            if not self.hashes[f] or (len(self.hashes[f]) < 3 and self.rnd.random() < 0.15):
                (self.g_poseidon if self.rnd.random() < 0.5 else self.g_poseidon2)(f, small)
            slot = self.rnd.choice(sorted(self.hashes[f]))
        t, unit, kind = self.hashes[f][slot]
        self.last_hash = (f, slot)
        return slot, t, max((HASH_WORK if kind == "poseidon" else HASH2_WORK) // unit, 1)

    def twin(self, f, slot):
        """the live handles of the other kind at the width of handle `slot`"""
        t, _, kind = self.hashes[f][slot]
        return [s for s, h in sorted(self.hashes[f].items()) if h[0] == t and h[2] != kind]

    def lanes(self, small, cap):
        pool = [n for n in LENGTHS if n <= cap and (n <= SMALL or not small)]
        return self.rnd.choices(pool, [_LEN_WEIGHT[n] for n in pool])[0]

    def hash_host(self, small):
        """is the call a host-form one: a small call behind a large host-form one mostly is too"""
        host = self.rnd.random() < (0.8 if small and self.host_before else 0.3)
        self.host_before = host
        return host

    def g_permute(self, f, small):
        slot, t, most = self.hash_handle(f, small)
        n = self.lanes(small, min(most, BANK // t))
        a, host, out = self.place(n * t), self.hash_host(small), None
        c = self.rnd.random()
        if not host and c < 0.5:
            out = self.place(n * t, [a])
        elif not host and c < 0.56 and n * t >= 2:  # cuts the input: refused by the Python layer
            out = self.shifted(a)
        if out is None or not _cuts(out, a):
            self.maybe_plant(f, "permute", self.spots(a, self.rnd))
        self.emit("permute", f, slot=slot, a=a, out=out, host=host)
        return n

    def g_sponge(self, f, small):
        slot, t, most = self.hash_handle(f, small)
        length = max(self.rnd.choice((1, t - 2, t - 1, t, 2 * (t - 1), 2 * (t - 1) + 1)), 1)  # the last block: empty, short or full
        stride = length + self.rnd.choice((0, 0, 1, 3))
        batch = self.lanes(small, min(max(most // -(-length // (t - 1)), 1), BANK // stride))
        a, host, out = self.place(batch * stride), self.hash_host(small), None
        if not host:
            out = self.place(batch, [a])
            if self.rnd.random() < 0.06:  # cuts the input, be it the padding behind the last row: refused by the Python layer
                out = [a[0] + 2 * self.rnd.randrange(a[1] - batch + 1), batch]
        if host or not _cuts(out, a):
            rows = sorted({0, batch - 1, self.rnd.randrange(batch)})
            before = len(self.steps)
            self.maybe_plant(f, "sponge", self.spots(a, self.rnd, rows, stride, length))
            if len(self.steps) == before and self.plant_ok and not self.no_plant and batch > 1 and stride > length and self.rnd.random() < 0.3:
                # a value that is not below r in the padding behind the first row (far from every output's neighbourhood): not read, so not refused
                self.emit("plant", f, at=a[0] + 2 * self.rnd.randrange(length, stride), value=self.rnd.choice((self.r[f], (1 << 256) - 1)), quiet=True)
        self.emit("sponge", f, slot=slot, a=a, batch=batch, length=length, out=out, host=host)
        return batch

    def g_tree(self, f, small):
        slot, t, most = self.hash_handle(f, small)
        arity = t - 1
        if arity == 1:  # a chain over one leaf
            n, levels, first = 1, self.rnd.choice((1, 2, 3, 64, self.rnd.randrange(1, 65))), 1
            count = levels
        else:
            depths = [k for k in range(1, 13) if arity ** k <= BANK and (arity ** k - 1) // (arity - 1) <= most and (arity ** (k - 1) <= SMALL or not small)] or [1]
            k = self.rnd.choice(depths + depths[-1:])  # (the deepest there is twice: a large first level is rare enough)
            n, levels, first = arity ** k, None, arity ** (k - 1)
            count = (n - 1) // (arity - 1)
        leaves, host, out = self.place(n), self.hash_host(small), None
        if not host:
            out = self.place(count, [leaves])
            if arity > 1 and self.rnd.random() < 0.06:  # cuts the leaves: refused by the Python layer
                out = [leaves[0] + 2 * self.rnd.randrange(n - count + 1), count]
        if host or not _cuts(out, leaves):
            self.maybe_plant(f, "tree", self.spots(leaves, self.rnd))
        self.emit("tree", f, slot=slot, leaves=leaves, levels=levels, out=out, host=host)
        return first

    def g_format(self, f, small):
        self.mont[f] = not self.mont[f] if self.rnd.random() < 0.8 else self.mont[f]
        self.emit("format", f, mont=self.mont[f])

    def g_hook(self, f, small):
        names = sorted(HOOKS)
        self.hooks_set = self.rnd.sample(names, self.rnd.choice((1, 2, 2, 3)))
        for name in self.hooks_set:  # (more than one at a time: no suite sets two hooks at once)
            value = self.rnd.choice(HOOKS[name])
            self.hooks[name] = value
            self.emit("hook", 0, name=name, value=value)

    def g_close(self, f, small, what=None):
        kept = {"mat": self.mats, "tab": self.tabs, "hash": self.hashes}
        live = [(w, s) for w, d in kept.items() for s in sorted(d[f]) if what in (None, w)]
        if live:
            w, s = self.rnd.choice(live)
            del kept[w][f][s]
            self.emit("close", f, what=w, slot=s)

    def g_stream(self, f, small):
        self.side = not self.side
        self.emit("stream", 0, side=self.side)

    def g_overlap(self, f, small):
        ok = [k for k in _OVERLAPS if self.serves(f, k)]
        getattr(self, "g_" + self.rnd.choice(ok))(f, small, overlap=True)

    def serves(self, f, kind):
        return self.fields[f] != "grumpkin" or kind in GRUMPKIN_KINDS or kind not in LIBRARY

    def low_behind_top(self, f, kind, n):
        """behind a top-first frmle step of n scalars to a row, sometimes and with no step between: the same entry point low first -- on the same
        field or the other one, small behind large or large behind small; or, behind an mle_eval, a low-first fused round of fewer levels, whose
        scratch rows then lie where the eval's levels lay (csrc/frmle_host.h: one scratch buffer to a device).  No value is planted: the call is
        to compute on the state the top-first call left.  -> the field of the last step"""
        hook = self.hooks["frmle_test_tile"]
        shorter = [m for m in (4, 8, 16, 32, 64, 128, 256) if m <= n and 1 + low_fused_partials(m, hook) < eval_levels(n, hook)] if kind == "mle_eval" and "round" in self.kinds else []
        c = self.rnd.random()
        if c >= (0.9 if shorter else 0.75 if n >= LARGE else 0.4):
            return f
        self.no_plant, self.force_order = True, "low"
        if shorter and c >= 0.2:
            self.force_fold, self.force_n = True, self.rnd.choice(shorter)
            self.g_round(f, False)
        else:
            if len(self.fields) > 1 and self.rnd.random() < 0.5:
                f = 1 - f
            d = self.rnd.random()
            self.force_big = n <= SMALL and d < 0.5
            getattr(self, "g_" + kind)(f, n >= LARGE and d < 0.7)
        self.no_plant, self.force_order, self.force_big, self.force_fold, self.force_n = False, None, False, False, None
        return f

    # ---- the program ---------------------------------------------------------------------------------------------------------------------
    def run(self, count):
        for f in range(len(self.fields)):
            self.emit("init", f, seed=self.rnd.randrange(1 << 30))
        while len(self.steps) < count:
            if self.follow and self.rnd.random() < 0.6:  # a small step on the entry point that has just run a large one
                f, kind = self.follow
                small = True
            else:
                f = self.rnd.randrange(len(self.fields))
                if self.prev_f is not None and len(self.fields) > 1 and self.rnd.random() < 0.8:  # the other field's turn (a draw may be several steps on one field)
                    f = 1 - self.prev_f
                pool = [k for k in self.kinds if self.serves(f, k)]
                kind = self.rnd.choices(pool, [_WEIGHT[k] for k in pool])[0]
                small = False
            self.follow, self.last_hash = None, None
            per_row = getattr(self, "g_" + kind)(f, small)
            if kind in HASH_CALLS and self.last_hash and self.twin(*self.last_hash) and self.rnd.random() < 0.5:
                # the same call at once on a live handle of the OTHER kind at the same width (the two kinds share a table's head and the lane
                # functions' template): nothing in between, so no planted value
                self.force_slot, self.no_plant = self.rnd.choice(self.twin(*self.last_hash)), True
                getattr(self, "g_" + kind)(f, small)
                self.force_slot, self.no_plant = None, False
            elif kind in COLUMN_CALLS and not small and per_row is not None and per_row > SMALL and self.rnd.random() < 0.4:
                # libmsm_frcol's nodes, rel, used and z only grow and are per device, not per field: a small call of the same entry point right
                # behind one that is larger, not only behind a "large" one
                getattr(self, "g_" + kind)(f, True)
            elif kind == "inverse" and per_row > SMALL and not small and self.rnd.random() < 0.3:
                self.g_inverse(f, True)  # a shorter inverse behind a longer one, not only behind a "large" one: its scratch keeps the longer one's tail
            elif kind in FRMLE_ORDERED and "order" not in self.steps[-1][2]:
                f = self.low_behind_top(f, kind, per_row)
            elif kind == "hook" and "frmle_test_tile" in self.hooks_set and self.hooks["frmle_test_tile"] in (2, 8) and "round" in self.kinds and self.rnd.random() < 0.7:
                # launch tiles of one or four pairs: a low-first fused round long enough for three levels of partial sums under its scratch rows
                self.force_order, self.force_fold = "low", True
                self.force_n = self.rnd.choice((64, 256, 2048) if self.hooks["frmle_test_tile"] == 8 else (64, 128, 256))
                self.g_round(f, False)
                self.force_order, self.force_fold, self.force_n = None, False, None
            self.prev_f = f
            if per_row is not None and per_row >= LARGE and not small:
                self.follow = (f, kind)
        return self.steps


def program(seed, case, fields, kinds=None, steps=28):
    """the steps of case `case` of seed `seed` over `fields` (one or two names): the same on every run and on every machine.  kinds: None, or the
    step kinds to draw from (FUZZ_FR_KINDS)."""
    fields = [fields] if isinstance(fields, str) else list(fields)
    assert 1 <= len(fields) <= 2 and all(f in FIELD_R for f in fields)
    rnd = random.Random("fr_program/%d/%d/%s" % (seed, case, ",".join(fields)))
    return _Gen(rnd, fields, kinds).run(steps + len(fields))

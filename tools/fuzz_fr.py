"""Randomised differential test of the nine scalar-field libraries as CHAINED programs on shared state (tests/fr_program.py): random steps over
one or two fields in one arena per field -- every entry point of the scalars_* methods of scalars.py, in place or into another range, at starts of 0 and
16 mod 32, after a larger call, after another field's call, after a refused call, under both scalar forms, with several test hooks set at once,
with matrices, lookup tables, Poseidon and Poseidon2 handles kept alive across all of it (a handle's constants go to the device inside its first
call, on whichever stream and under whichever form that call has; a hashing call is a device-form one on ranges of the arena or a host-form
one on their bytes), and with the counts and indices that a lookup call returned kept on the device for the column calls of
msm_webgpu_amd.columns behind it.  After EVERY step each range the step wrote and each host value it returned is compared byte for byte with the model; at the end
of a program the whole arena is.
The four steps of libmsm_frmle carry an order: a low-first one (order="low": MSM_FRMLE_LOW_FIRST) runs through msm_webgpu_amd.multilinear, a
top-first one, which has no order argument, through the context's scalars_* methods, so both call paths run.  A low-first bind in place leaves the
scalars [n / 2, n) of every row unspecified: the model names them, they are rewritten from the model before the step's outputs [0, n / 2) and their
guards are compared.  A "gemini" step is multilinear.gemini_folds of one row, its n - 1 scalars copied into the arena.
Usage: python tools/fuzz_fr.py [cases] [seed] [field[,field]] [--case K]   (fields: bn254 pallas vesta bls12_381 grumpkin; --case K replays one case)
FUZZ_FR_KINDS=a,b,... restricts the step kinds that are drawn (tests/fr_program.py: KINDS)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import fr_program as P  # noqa: E402

GUARD = 2  # 16-byte units compared on either side of a range a step wrote: a store just past an output fails at the step that made it


class Mismatch(Exception):
    def __init__(self, index, what):
        super().__init__("step %d: %s" % (index, what))
        self.index, self.what = index, what


def _first_difference(got, want):
    return next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))


def run_program(steps, fields, backend):
    """Run the steps on the backend beside the model; raises Mismatch(index of the failing step, what differed).  The only calls that may fail
    are the ones the model predicted would fail, with the code it predicted."""
    model = P.Model(fields)
    try:
        for i, step in enumerate(steps):
            kind, f, args = step
            want = model.step(step)
            if kind == "init":
                backend.write(f, 0, bytes(model.arena[f]))
                continue
            try:
                host, err = getattr(backend, "op_" + kind)(f, **{k: v for k, v in args.items() if k != "overlap"}), None
            except P.Refused as e:
                host, err = None, e.code
            if err != want["error"]:
                raise Mismatch(i, "the call returned %r, the model predicts %r" % (err, want["error"]))
            if err is None and host != want["host"]:
                raise Mismatch(i, "host values differ: got %r, the model predicts %r" % (host, want["host"]))
            for off16, n in want["rewrite"]:  # (unspecified: after a predicted ERR_NONCANONICAL, behind a low-first bind in place; or the planted scalar itself)
                backend.write(f, off16, model.raw(f, (off16, n)))
            for off16, n in want["writes"]:  # (behind the rewrites: a guard may lie on an unspecified scalar, the first behind a low-first bind's outputs)
                lo, hi = max(off16 - GUARD, 0), min(off16 + 2 * n + GUARD, P.ARENA16)
                got, ref = backend.read16(f, lo, hi), bytes(model.arena[f][16 * lo:16 * hi])
                if got != ref:
                    at = 16 * lo + _first_difference(got, ref)
                    raise Mismatch(i, "field %d (%s): byte %d of the arena differs (the step wrote [%d, %d): byte %d of it)" % (
                        f, fields[f], at, 16 * off16, 16 * off16 + 32 * n, at - 16 * off16))
        for f in range(len(fields)):
            got, ref = backend.read16(f, 0, P.ARENA16), bytes(model.arena[f])
            if got != ref:
                raise Mismatch(len(steps) - 1, "field %d (%s): after the program byte %d of the arena differs" % (f, fields[f], _first_difference(got, ref)))
    finally:
        backend.reset()


def run_cases(cases, seed, fields, backend, kinds=None, say=print):
    """-> 0, or 1 after the first mismatch, which is printed with its seed, case, failing step and the program up to that step"""
    t0 = time.time()
    for n, case in enumerate(cases):
        steps = P.program(seed, case, fields, kinds)
        try:
            run_program(steps, fields, backend)
        except Mismatch as e:
            say("MISMATCH seed %d case %d fields %s step %d (%s): %s" % (seed, case, ",".join(fields), e.index, P.label(steps[e.index]), e.what))
            say("program = %r" % (steps[:e.index + 1],))
            return 1
        if (n + 1) % 10 == 0:
            say("  %d cases ok, %.0f s" % (n + 1, time.time() - t0))
    say("fuzz ok: %d cases in %.1f s (seed %d, %s)" % (len(cases), time.time() - t0, seed, ",".join(fields)))
    return 0


def _translated(fn):
    def call(self, f, **args):
        from msm_webgpu_amd import api
        try:
            with self.torch.cuda.stream(self.cur):
                return fn(self, f, **args)
        except api.MsmHipError as e:
            raise P.Refused(e.code)
        except ValueError:
            raise P.Refused(P.REFUSED)
    return call


class DeviceBackend:
    """the device side: one method per step kind, each a call of MsmContext on ranges of the field's arena (one CUDA uint8 tensor per field)"""

    def __init__(self, fields):
        import torch

        import msm_webgpu_amd as m
        from msm_webgpu_amd import api, columns, multilinear
        self.torch, self.api, self.columns, self.multilinear, self.fields = torch, api, columns, multilinear, list(fields)
        for name in fields:
            r = P.FIELD_R[name]
            assert api.SCALAR_FIELDS[name] == r and (name == "grumpkin" or all(api.root_of_unity(name, k) == P.root_of_unity(r, k) for k in range(13)))
        self.ctx = [m.MsmContext(0, curve=name) for name in fields]
        self.arena = [torch.zeros(16 * P.ARENA16, dtype=torch.uint8, device="cuda:0") for _ in fields]
        assert all(t.data_ptr() % 32 == 0 for t in self.arena)  # (so that an odd off16 IS a start at 16 mod 32)
        self.default = torch.cuda.current_stream(0)
        self.own = torch.cuda.ExternalStream(api.lib().msm_hip_stream(self.ctx[0]._h), device="cuda:0")  # the first context's own stream
        self.side = torch.cuda.Stream(0)
        self.cur = self.default
        self.mats, self.tabs, self.hashes = [{} for _ in fields], [{} for _ in fields], [{} for _ in fields]
        self.words = [{} for _ in fields]  # slot -> a CUDA tensor of 32-bit words: the one a lookup call returned, or an uploaded one

    def t(self, f, rng):
        return None if rng is None else self.arena[f][16 * rng[0]:16 * rng[0] + 32 * rng[1]]

    def read16(self, f, lo, hi):
        with self.torch.cuda.stream(self.cur):
            return self.arena[f][16 * lo:16 * hi].cpu().numpy().tobytes()

    def write(self, f, off16, data):
        with self.torch.cuda.stream(self.cur):
            self.arena[f][16 * off16:16 * off16 + len(data)].copy_(self.torch.frombuffer(bytearray(data), dtype=self.torch.uint8))
            self.cur.synchronize()

    def _switch(self, to):
        to.wait_stream(self.cur)  # what the caller enqueued so far comes first
        self.cur = to

    def reset(self):
        """between programs: no hook, no handle, the canonical form, the default stream"""
        for name in P.HOOKS:
            self._hook(name)(0)
        for d in self.words:
            d.clear()
        for d in self.mats + self.tabs + self.hashes:
            for h in d.values():
                h.close()
            d.clear()
        for c in self.ctx:
            c.set_scalar_format(mont256=False)
        self._switch(self.default)

    def _hook(self, name):
        """a test hook by its name: the scalar-field libraries' are the API's, the columns' its own module's"""
        return getattr(self.api, name, None) or getattr(self.columns, name)

    def close(self):
        self.reset()
        self.torch.cuda.synchronize()
        for c in self.ctx:
            c.close()
        self.api.frhash_release()
        self.columns.frcol_release()

    def host_bytes(self, f, rng):
        """the bytes of a range, for a host-form call"""
        return self.t(f, rng).cpu().numpy().tobytes()

    def _operand(self, f, v):
        return v if v is None or isinstance(v, int) else self.t(f, v)

    @_translated
    def op_map(self, f, op, a, b, c, out):
        rest = [self._operand(f, b)] + ([self._operand(f, c)] if op in ("mul_add", "mul_sub") else [])
        getattr(self.ctx[f], "scalars_" + op)(self.t(f, a), *rest, out=self.t(f, out))

    @_translated
    def op_inverse(self, f, a, out):
        self.ctx[f].scalars_inverse(self.t(f, a), out=self.t(f, out))

    @_translated
    def op_scan(self, f, a, op, exclusive, batch, out, totals):
        res = self.ctx[f].scalars_scan(self.t(f, a), op=op, exclusive=exclusive, batch=batch, out=self.t(f, out), totals=totals)
        return res[1] if totals else None

    @_translated
    def op_fft(self, f, a, log_n, batch, inverse, shift, omega):
        self.ctx[f].scalars_fft(self.t(f, a), log_n, omega=omega, inverse=inverse, shift=shift, batch=batch)

    @_translated
    def op_eval(self, f, a, z, batch):
        return self.ctx[f].scalars_eval(self.t(f, a), z, batch)

    @_translated
    def op_divide(self, f, a, z, batch, out, values):
        res = self.ctx[f].scalars_divide(self.t(f, a), z, batch, out=self.t(f, out), values=values)
        return res[1] if values else None

    @_translated
    def op_dot(self, f, a, b, batch):
        return self.ctx[f].scalars_dot(self.t(f, a), self.t(f, b), batch)

    @_translated
    def op_combine(self, f, a, coeffs, out):
        self.ctx[f].scalars_combine(self.t(f, a), coeffs, out=self.t(f, out))

    @_translated
    def op_powers(self, f, g, n, scale, out):
        self.ctx[f].scalars_powers(g, n, scale, out=self.t(f, out))

    # a top-first frmle step goes through the context's scalars_* method, a low-first one through msm_webgpu_amd.multilinear: both call paths run
    @_translated
    def op_mle_fold(self, f, a, c, batch, n, out, order="top"):
        if order == "low":
            self.multilinear.fold(self.ctx[f], self.t(f, a), c, batch, n, out=self.t(f, out), order="low")
        else:
            self.ctx[f].scalars_mle_fold(self.t(f, a), c, batch, n, out=self.t(f, out))

    @_translated
    def op_mle_eval(self, f, a, point, batch, n, order="top"):
        if order == "low":
            return self.multilinear.evaluate(self.ctx[f], self.t(f, a), point, batch, n, order="low")
        return self.ctx[f].scalars_mle_eval(self.t(f, a), point, batch, n)

    @_translated
    def op_eq(self, f, point, scale, out, order="top"):
        if order == "low":
            self.multilinear.eq(self.ctx[f], point, scale, out=self.t(f, out), order="low")
        else:
            self.ctx[f].scalars_eq(point, scale, out=self.t(f, out))

    @_translated
    def op_round(self, f, a, terms, batch, n, fold, order="top"):
        if order == "low":
            return self.multilinear.sumcheck_round(self.ctx[f], self.t(f, a), terms, batch, n, fold, order="low")
        return self.ctx[f].scalars_sumcheck_round(self.t(f, a), terms, batch, n, fold)

    @_translated
    def op_gemini(self, f, a, point, out):
        self.t(f, out).copy_(self.multilinear.gemini_folds(self.ctx[f], self.t(f, a), point).view(-1))

    @_translated
    def op_matrix(self, f, slot, rows, cols, row_ptr, col_idx, vseed, transpose):
        self.mats[f][slot] = self.ctx[f].scalars_matrix(rows, cols, row_ptr, col_idx, P.expand(vseed, len(col_idx), P.FIELD_R[self.fields[f]]), transpose)

    @_translated
    def op_matvec(self, f, slot, x, out, transpose, pad_to):
        self.ctx[f].scalars_matvec(self.mats[f][slot], self.t(f, x), out=self.t(f, out), transpose=transpose, pad_to=pad_to)

    @_translated
    def op_gate(self, f, a, terms, batch, n, step, scale, out, accumulate):
        self.ctx[f].scalars_gate(self.t(f, a), terms, batch, n, step, scale=self.t(f, scale), out=self.t(f, out), accumulate=accumulate)

    @_translated
    def op_vanishing_inverse(self, f, log_n, log_ext, shift, out):
        self.t(f, out).copy_(self.ctx[f].vanishing_inverse(log_n, log_ext, shift).view(-1))

    @_translated
    def op_quotient(self, f, a, terms, batch, log_n, log_ext, shift, out):
        self.t(f, out).copy_(self.ctx[f].quotient(self.t(f, a), terms, batch, log_n, log_ext, shift).view(-1))

    @_translated
    def op_table(self, f, slot, t, n):
        self.tabs[f][slot] = self.ctx[f].lookup_table(self.t(f, t), n)
        return self.tabs[f][slot].distinct

    @_translated
    def op_mult(self, f, slot, v, batch, n, out, indices, counts, cslot=None, islot=None):
        res = self.ctx[f].scalars_multiplicities(self.tabs[f][slot], self.t(f, v), batch, n, out=self.t(f, out), indices=indices, counts=counts, strict=False)
        for wslot, at in ((islot, 1), (cslot, 2 if indices else 1)):  # the very tensors the call returned, not copies
            if wslot is not None:
                self.words[f][wslot] = res[at]
        words = [[int(x) & 0xFFFFFFFF for x in w.cpu().reshape(-1).tolist()] for w in res[1:-1]]  # (idx: -1 where the value is missing)
        return tuple(words) + (tuple(res[-1]),)

    @_translated
    def op_poseidon(self, f, slot, t, full_rounds, partial_rounds, seed, capacity, capacity_at, out_at):
        rc, mds = P.poseidon_constants(seed, t, full_rounds, partial_rounds, P.FIELD_R[self.fields[f]])
        self.hashes[f][slot] = self.ctx[f].poseidon(t, full_rounds, partial_rounds, round_constants=rc, mds=mds, capacity=capacity, capacity_at=capacity_at, out_at=out_at)

    @_translated
    def op_poseidon2(self, f, slot, t, full_rounds, partial_rounds, seed, capacity, capacity_at, out_at):
        rc, mu = P.poseidon2_constants(seed, t, full_rounds, partial_rounds, P.FIELD_R[self.fields[f]])
        self.hashes[f][slot] = self.ctx[f].poseidon2(t, full_rounds, partial_rounds, round_constants=rc, diagonal=mu, capacity=capacity, capacity_at=capacity_at, out_at=out_at)

    @_translated
    def op_words(self, f, slot, values):
        self.words[f][slot] = self.torch.tensor([w - (1 << 32) if w >> 31 else w for w in values], dtype=self.torch.int32, device="cuda:0")

    @_translated
    def op_expand(self, f, t, counts, bias, out):
        self.columns.expand(self.ctx[f], self.t(f, t), self.words[f][counts], out[1], bias=bias, out=self.t(f, out))

    @_translated
    def op_pair(self, f, t, counts, out, s_out):
        self.columns.permuted_pair(self.ctx[f], self.t(f, t), self.words[f][counts], out=(self.t(f, out), self.t(f, s_out)))

    @_translated
    def op_gather(self, f, a, idx, out):
        self.columns.gather(self.ctx[f], self.t(f, a), self.words[f][idx], out=self.t(f, out))

    @_translated
    def op_permute(self, f, slot, a, out, host):
        if host:
            return self.ctx[f].scalars_permute(self.hashes[f][slot], self.host_bytes(f, a))
        self.ctx[f].scalars_permute(self.hashes[f][slot], self.t(f, a), out=self.t(f, a if out is None else out))

    @_translated
    def op_sponge(self, f, slot, a, batch, length, out, host):
        if host:
            return self.ctx[f].scalars_hash(self.hashes[f][slot], self.host_bytes(f, a), length, batch=batch)
        self.ctx[f].scalars_hash(self.hashes[f][slot], self.t(f, a), length, batch=batch, out=self.t(f, out))

    @_translated
    def op_tree(self, f, slot, leaves, levels, out, host):
        if host:
            return self.ctx[f].merkle_tree(self.hashes[f][slot], self.host_bytes(f, leaves), levels=levels)
        self.ctx[f].merkle_tree(self.hashes[f][slot], self.t(f, leaves), out=self.t(f, out), levels=levels)

    @_translated
    def op_format(self, f, mont):
        self.ctx[f].set_scalar_format(mont256=mont)

    @_translated
    def op_hook(self, f, name, value):
        self._hook(name)(value)

    @_translated
    def op_close(self, f, what, slot):
        {"mat": self.mats, "tab": self.tabs, "hash": self.hashes}[what][f].pop(slot).close()

    def op_stream(self, f, side):
        self._switch(self.side if side else self.own)

    def op_plant(self, f, at, value, quiet=False):
        self.write(f, at, value.to_bytes(32, "little"))


def main(argv):
    argv, one = list(argv), None
    if "--case" in argv:
        at = argv.index("--case")
        one = int(argv[at + 1])
        del argv[at:at + 2]
    cases = int(argv[0]) if len(argv) > 0 else 50
    seed = int(argv[1]) if len(argv) > 1 else 1
    fields = (argv[2] if len(argv) > 2 else "bn254").split(",")
    kinds = os.environ["FUZZ_FR_KINDS"].split(",") if os.environ.get("FUZZ_FR_KINDS") else None
    backend = DeviceBackend(fields)
    try:
        return run_cases([one] if one is not None else range(cases), seed, fields, backend, kinds)
    finally:
        backend.close()


if __name__ == "__main__":
    if main(sys.argv[1:]):
        sys.exit(1)

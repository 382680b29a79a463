"""The tester tested, on the CPU: the generator of tests/fr_program.py is deterministic and covers what it is there to cover on the committed
seeds of tests/test_gpu_fr_fuzz.py; the comparison loop of tools/fuzz_fr.py passes a backend that IS the model, and fails -- at the step that
carries the fault, with a printed program that replays to the same failure -- a backend with one planted fault.  The faults live here, not in
the product."""
import copy
import importlib
import importlib.util
import os

import pytest

from tests import fr_program as P
from tests import frlook_model
from tests.test_gpu_fr_fuzz import COMMITTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_fr", os.path.join(ROOT, "tools", "fuzz_fr.py"))
fuzz_fr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fuzz_fr)

VECTOR_KEYS = ("a", "b", "c", "out", "x", "v", "t", "scale")


@pytest.fixture(scope="module")
def programs():
    """every committed program: [(fields, seed, case, steps)], generated once"""
    return [(fields.split(","), seed, case, P.program(seed, case, fields.split(","))) for fields, (seed, cases) in COMMITTED.items() for case in range(cases)]


def test_field_constants_agree_with_the_oracles():
    for name, r in P.FIELD_R.items():
        assert importlib.import_module("oracle.%s_ref" % name).R == r


def test_same_seed_same_program_and_repr_round_trip(programs):
    for fields, seed, case, steps in programs[::7]:
        assert P.program(seed, case, fields) == steps
        assert eval(repr(steps)) == steps
    assert P.program(1, 0, ["bn254"]) != P.program(1, 1, ["bn254"]) != P.program(2, 1, ["bn254"])
    only = P.program(3, 0, ["pallas"], kinds=["map", "scan"])
    assert {s[0] for s in only} == {"init", "map", "scan"}


def test_every_step_kind_is_drawn(programs):
    count = {k: 0 for k in P.KINDS}
    for _, _, _, steps in programs:
        for s in steps:
            if s[0] != "init":
                count[P.label(s)] += 1
    assert min(count.values()) >= 5, count
    per_field = {}
    for fields, _, _, steps in programs:
        for s in steps:
            if s[0] in P.LIBRARY:
                per_field.setdefault(fields[s[1]], set()).add(s[0])
    assert per_field["grumpkin"] == set(P.GRUMPKIN_KINDS)  # only the libraries that serve it
    assert all(per_field[f] == set(P.LIBRARY) for f in ("bn254", "pallas", "vesta", "bls12_381")), per_field


def test_every_hook_is_set_together_with_another(programs):
    together = set()
    for _, _, _, steps in programs:
        state = {}
        for kind, _, a in steps:
            if kind == "hook":
                state[a["name"]] = a["value"]
                live = [h for h, v in state.items() if v]
                if a["value"] and len(live) > 1:
                    together.update(live)
    assert together == set(P.HOOKS)


def test_a_fifth_of_the_vector_operands_start_at_16_mod_32(programs):
    odd = total = 0
    for _, _, _, steps in programs:
        for kind, _, a in steps:
            for key in VECTOR_KEYS:
                if isinstance(a.get(key), list) and kind in P.LIBRARY:
                    total += 1
                    odd += a[key][0] % 2
    assert total > 1000 and 5 * odd >= total, (odd, total)


def test_every_library_sees_large_then_small_and_a_planted_value(programs):
    pairs, planted = set(), set()
    for _, _, _, steps in programs:
        sized = P.sizes(steps)
        for (i, kind, f, n), (j, kind2, f2, m) in zip(sized, sized[1:]):
            between = steps[i + 1:j]
            if kind == kind2 and f == f2 and n >= P.LARGE and m <= P.SMALL and all(s[0] == "plant" for s in between):
                pairs.add(P.LIBRARY[kind])
        for s, nxt in zip(steps, steps[1:]):
            if s[0] == "plant":
                assert nxt[0] in P.LIBRARY and nxt[1] == s[1]  # (the very next step reads it)
                planted.add(P.LIBRARY[nxt[0]])
    assert pairs == set(P.LIBRARIES), pairs
    assert planted == set(P.LIBRARIES), planted


def test_transforms_change_the_root_at_one_length(programs):
    """the twiddle cache is keyed by (field, log_n, omega): a caller's root right after the default one at the same length, and the other way round"""
    to_custom = to_default = 0
    for _, _, _, steps in programs:
        last = {}
        for kind, f, a in steps:
            if kind == "fft":
                if last.get(f, (None,))[0] == a["log_n"] >= 2 and (last[f][1] is None) != (a["omega"] is None):
                    to_custom += a["omega"] is not None
                    to_default += a["omega"] is None
                last[f] = (a["log_n"], a["omega"])
    assert to_custom >= 5 and to_default >= 5, (to_custom, to_default)


def test_two_fields_take_turns(programs):
    """over two fields a library call follows one on the OTHER field more often than a coin would have it"""
    switches = pairs = 0
    for fields, _, _, steps in programs:
        if len(fields) == 2:
            turns = [s[1] for s in steps if s[0] in P.LIBRARY]
            switches += sum(x != y for x, y in zip(turns, turns[1:]))
            pairs += len(turns) - 1
    assert pairs > 500 and 2 * switches > pairs, (switches, pairs)


def test_the_loop_passes_a_backend_that_is_the_model(capsys):
    for fields, (seed, cases) in COMMITTED.items():
        backend = P.ModelBackend(fields.split(","))
        assert fuzz_fr.run_cases(range(min(cases, 4)), seed, fields.split(","), backend) == 0
    assert capsys.readouterr().out.count("fuzz ok: ") == len(COMMITTED)


# ---- the planted faults: each a ModelBackend that goes wrong in ONE situation, and notes the step at which it did ------------------------------
class Faulty(P.ModelBackend):
    fields_to_run = "bn254"

    def __init__(self, fields):
        super().__init__(fields)
        self.calls, self.fired_at = 0, None
        self.fresh()

    def fresh(self):
        """the state a fault keeps across calls; it does not outlive a program, so that a printed program replays on its own"""

    def reset(self):
        super().reset()
        self.calls = 0
        self.fresh()

    def fired(self):
        if self.fired_at is None:
            self.fired_at = len(self.m.fields) + self.calls - 1  # (the steps before the first call are the arenas' init)

    def flip(self, f, off16, byte=0):
        self.m.arena[f][16 * off16 + byte] ^= 1

    def call(self, kind, f, a):
        self.calls += 1
        return self.faulty(kind, f, a)

    def faulty(self, kind, f, a):
        return super().call(kind, f, a)

    def plain_call(self, kind, f, a):
        return P.ModelBackend.call(self, kind, f, a)


class ScanTileBoundary(Faulty):
    """one element wrong at a tile boundary of a scan: the first of the second tile"""

    def faulty(self, kind, f, a):
        host = self.plain_call(kind, f, a)
        tile = self.m.hooks["frvec_test_tile"] or 1024
        if kind == "scan" and a["a"][1] // a["batch"] > tile:
            self.flip(f, (a["out"] or a["a"])[0] + 2 * tile)
            self.fired()
        return host


class ScratchKeepsTheTail(Faulty):
    """a scratch that keeps the previous call's tail: an inverse shorter than the one before it gets its last element from there"""

    def fresh(self):
        self.longest = 0

    def faulty(self, kind, f, a):
        host = self.plain_call(kind, f, a)
        if kind == "inverse":
            if a["a"][1] < self.longest:
                self.flip(f, (a["out"] or a["a"])[0] + 2 * (a["a"][1] - 1), 5)
                self.fired()
            self.longest = max(self.longest, a["a"][1])
        return host


class NttReusesTheTable(Faulty):
    """an NTT that reuses the table of the previous omega at the same log_n"""

    def fresh(self):
        self.table = {}

    def faulty(self, kind, f, a):
        if kind != "fft" or a["log_n"] < 2:
            return self.plain_call(kind, f, a)
        omega = a["omega"] or P.root_of_unity(self.m.r[f], a["log_n"])
        cached = self.table.setdefault((f, a["log_n"]), omega)
        if cached != omega and not self.m.planted[f]:
            self.fired()
        return self.plain_call(kind, f, dict(a, omega=cached))


class TableAnswersForAnother(Faulty):
    """a table handle that answers with the other handle's indices"""
    fields_to_run = "grumpkin"

    def faulty(self, kind, f, a):
        if kind != "mult" or not a["indices"]:
            return self.plain_call(kind, f, a)
        others = [keys for slot, (keys, form) in sorted(self.m.tabs[f].items()) if slot != a["slot"] and form == self.m.mont[f]]
        stored, stride = self.m.stored(f, a["v"]), a["v"][1] // a["batch"]
        host = self.plain_call(kind, f, a)
        if others:
            idx = frlook_model.lookup(others[0], [stored[k * stride:(k + 1) * stride] for k in range(a["batch"])], a["n"])[1]
            if idx != host[0]:
                self.fired()
                host = (idx,) + host[1:]
        return host


class ErrorWordNotCleared(Faulty):
    """an error word that is not cleared after a refusal: the library's next call reports it again"""
    fields_to_run = "pallas"

    def fresh(self):
        self.stale = set()

    def faulty(self, kind, f, a):
        lib = P.LIBRARY.get(kind)
        try:
            host = self.plain_call(kind, f, a)
        except P.Refused as e:
            if e.code == P.ERR_NONCANONICAL:
                self.stale.add(lib)
            raise
        if lib in self.stale and kind not in ("matrix", "vanishing_inverse"):  # (those two touch no device)
            self.stale.discard(lib)
            self.fired()
            raise P.Refused(P.ERR_NONCANONICAL)
        return host


class SecondHalfFromFurtherOn(Faulty):
    """the second half of an operand at 16 mod 32 read from 16 bytes further on"""
    fields_to_run = "vesta"

    def faulty(self, kind, f, a):
        if kind != "map" or a["a"][0] % 2 == 0 or a["a"][1] < 2 or self.m.planted[f]:
            return self.plain_call(kind, f, a)
        dst, src = a["out"] or a["a"], self.m.raw(f, (a["a"][0], a["a"][1] + 1))
        there = copy.deepcopy(self.m)
        there.put(f, a["a"][0], b"".join(src[32 * i:32 * i + 16] + src[32 * i + 32:32 * i + 48] for i in range(a["a"][1])))
        there.op_map(f, **a)
        host = self.plain_call(kind, f, a)
        if there.raw(f, dst) != self.m.raw(f, dst):
            self.m.put(f, dst[0], there.raw(f, dst))
            self.fired()
        return host


class MontComputedAsCanonical(Faulty):
    """a step under mont256 computed as canonical"""
    fields_to_run = "bls12_381"

    def faulty(self, kind, f, a):
        if not (kind == "inverse" or kind == "map" and a["op"] == "mul") or not self.m.mont[f] or self.m.planted[f] or a.get("out") and P.Model._partial(a["out"], [a["a"]]):
            return self.plain_call(kind, f, a)
        self.m.mont[f] = False
        try:
            host = self.plain_call(kind, f, a)
        finally:
            self.m.mont[f] = True
        self.fired()
        return host


class OneByteTooMany(Faulty):
    """one byte written just past an output"""
    fields_to_run = "pallas,vesta"

    def faulty(self, kind, f, a):
        host = self.plain_call(kind, f, a)
        if kind in ("powers", "eq", "gate"):
            self.flip(f, a["out"][0] + 2 * a["out"][1])
            self.fired()
        return host


@pytest.mark.parametrize("fault", [ScanTileBoundary, ScratchKeepsTheTail, NttReusesTheTable, TableAnswersForAnother, ErrorWordNotCleared, SecondHalfFromFurtherOn,
                                   MontComputedAsCanonical, OneByteTooMany], ids=lambda c: c.__name__)
def test_a_planted_fault_is_caught_at_its_step_and_replays(fault):
    fields = fault.fields_to_run.split(",")
    seed, cases = COMMITTED[fault.fields_to_run]
    backend, said = fault(fields), []
    assert fuzz_fr.run_cases(range(cases), seed, fields, backend, say=said.append) == 1, "the fault went unnoticed on the committed cases"
    head, listing = [line for line in said if not line.startswith("  ")]
    assert head.startswith("MISMATCH seed %d case " % seed) and listing.startswith("program = ")
    step = int(head.split(" step ")[1].split()[0])
    assert step == backend.fired_at, (head, backend.fired_at)  # caught where it happened, not later
    replay = eval(listing[len("program = "):])
    assert len(replay) == step + 1
    again = fault(fields)
    with pytest.raises(fuzz_fr.Mismatch) as e:
        fuzz_fr.run_program(replay, fields, again)
    assert e.value.index == step == again.fired_at and e.value.what in head

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
from tests import frhash2_model, frhash_model, frlook_model, frmle_low_model, frvec_model
from tests.test_gpu_fr_fuzz import COMMITTED, SECOND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_fr", os.path.join(ROOT, "tools", "fuzz_fr.py"))
fuzz_fr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fuzz_fr)

VECTOR_KEYS = ("a", "b", "c", "out", "s_out", "x", "v", "t", "scale", "leaves")


@pytest.fixture(scope="module")
def programs():
    """every committed program: [(fields, seed, case, steps)], generated once"""
    return [(fields.split(","), seed, case, P.program(seed, case, fields.split(","))) for fields, (seed, cases) in list(COMMITTED.items()) + list(SECOND.items())
            for case in range(cases)]


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
    assert planted == set(P.LIBRARIES) - {"frcol"}, planted  # (libmsm_frcol does not compare with r: a planted value would be copied into the arena)


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


def hash_calls(steps):
    """the calls of libmsm_frhash of a program, in order: dicts of the step's index and kind, its field index, the handle (its `poseidon` or
    `poseidon2` step's index), its width and its kind (`made`: that step's kind), the field's form and the stream at the call, and whether it
    is a host-form call, cuts its input (refused by the Python layer: the library is not called) or follows a planted value (refused by the
    library)"""
    mont, side, made, out = {}, False, {}, []
    for i, (kind, f, a) in enumerate(steps):
        if kind == "format":
            mont[f] = a["mont"]
        elif kind == "stream":
            side = a["side"]
        elif kind in P.HASH_MAKERS:
            made[f, a["slot"]] = (i, a["t"], kind)
        elif kind in P.HASH_CALLS:
            handle, t, maker = made[f, a["slot"]]
            out.append({"index": i, "kind": kind, "f": f, "handle": handle, "t": t, "made": maker, "mont": bool(mont.get(f)), "side": side, "host": a["host"],
                        "cut": P.hash_cut(steps[i]), "planted": steps[i - 1][0] == "plant" and not steps[i - 1][2].get("quiet")})
    return out


def test_hashing_reaches_each_fields_tidy_boundary(programs):
    """the widest state that goes into the S-box untidied and the narrowest that is tidied first, per field, in calls that compute"""
    used = {}
    for fields, _, _, steps in programs:
        for c in hash_calls(steps):
            if c["made"] == "poseidon" and c["kind"] in ("permute", "sponge") and not c["cut"] and not c["planted"]:  # (Poseidon2 tidies by rules of its own)
                used[fields[c["f"]], c["t"]] = used.get((fields[c["f"]], c["t"]), 0) + 1
    for field, widths in P.HASH_BOUNDARY.items():
        assert all(used.get((field, t), 0) >= 3 for t in widths), (field, used)
    assert {t for _, t in used} == set(P.HASH_WIDTHS)


def test_poseidon2_runs_at_every_width_of_every_field(programs):
    """calls that compute, on every field at every Poseidon2 width: on BLS12-381 t = 3 tidies the S-box input and t = 12 the sums, and no other
    field does either"""
    used = {}
    for fields, _, _, steps in programs:
        for c in hash_calls(steps):
            if c["made"] == "poseidon2" and not c["cut"] and not c["planted"]:
                used[fields[c["f"]], c["t"]] = used.get((fields[c["f"]], c["t"]), 0) + 1
    assert all(used.get((field, t), 0) >= 3 for field in P.FIELD_R for t in P.HASH2_WIDTHS), used


def test_the_two_kinds_of_handle_alternate_at_one_width(programs):
    """a call that computes on a handle of one kind, and in the very next step one on a handle of the other kind at the same width on the same
    field: both ways round"""
    to = {"poseidon": 0, "poseidon2": 0}
    for _, _, _, steps in programs:
        calls = [c for c in hash_calls(steps) if not c["cut"] and not c["planted"]]
        for before, c in zip(calls, calls[1:]):
            if c["index"] == before["index"] + 1 and c["f"] == before["f"] and c["t"] == before["t"] and c["made"] != before["made"]:
                to[c["made"]] += 1
    assert min(to.values()) >= 5, to


def test_a_poseidon2_handle_first_goes_to_the_device_under_either_form_on_either_stream(programs):
    first_form, first_side, seen = {False: 0, True: 0}, {False: 0, True: 0}, set()
    for n, (_, _, _, steps) in enumerate(programs):
        for c in hash_calls(steps):
            if c["made"] == "poseidon2" and not c["cut"] and (n, c["handle"]) not in seen:  # (a cut never reaches the library)
                seen.add((n, c["handle"]))
                first_form[c["mont"]] += 1
                first_side[c["side"]] += 1
    assert min(first_form.values()) >= 5 and min(first_side.values()) >= 5, (first_form, first_side)


def test_hash_handles_meet_both_forms_both_streams_and_one_another(programs):
    """a handle's constants go to the device inside its FIRST call, whichever form and stream that has; the form is a flag of every later call;
    the handles of one device share the library's state"""
    first_form, first_side, forms, after_another, unused_closed = {False: 0, True: 0}, {False: 0, True: 0}, {}, 0, 0
    for n, (_, _, _, steps) in enumerate(programs):
        calls = [c for c in hash_calls(steps) if not c["cut"]]  # (a cut never reaches the library)
        for c in calls:
            key = (n, c["handle"])
            if key not in forms:
                first_form[c["mont"]] += 1
                first_side[c["side"]] += 1
            forms.setdefault(key, set()).add(c["mont"])
        for before, c in zip(calls, calls[1:]):
            after_another += c["index"] == before["index"] + 1 and (before["f"], before["handle"]) != (c["f"], c["handle"]) and before["t"] != c["t"]
        made = {}
        for i, (kind, f, a) in enumerate(steps):
            if kind in P.HASH_MAKERS:
                made[f, a["slot"]] = i
            elif kind == "close" and a["what"] == "hash":
                unused_closed += (n, made[f, a["slot"]]) not in forms
    assert min(first_form.values()) >= 5 and min(first_side.values()) >= 5, (first_form, first_side)
    assert sum(len(v) == 2 for v in forms.values()) >= 5
    assert after_another >= 5, after_another  # the very next step, on another handle of another width
    assert unused_closed >= 1  # a handle that never went to the device is closed too


def test_host_form_hashing_sees_large_then_small_and_refusals_stay_rare(programs):
    """the staging buffer of the host forms only grows: a small host-form call right behind a large one.  And no more than a fifth of the calls
    are refused -- by a planted value or a cut --, so that the refusals do not hide the paths that compute."""
    pairs = refused = total = 0
    for _, _, _, steps in programs:
        sized = [s for s in P.sizes(steps) if s[1] in P.HASH_CALLS and steps[s[0]][2]["host"]]
        pairs += sum(n >= P.LARGE and m <= P.SMALL and kind == kind2 for (_, kind, _, n), (_, kind2, _, m) in zip(sized, sized[1:]))  # (no host-form call between)
        calls = hash_calls(steps)
        total += len(calls)
        refused += sum(c["cut"] or c["planted"] for c in calls)
    quiet = [nxt for _, _, _, steps in programs for s, nxt in zip(steps, steps[1:]) if s[0] == "plant" and s[2].get("quiet")]
    assert all(s[0] == "sponge" for s in quiet) and sum(s[2]["host"] for s in quiet) >= 5 and sum(not s[2]["host"] for s in quiet) >= 5  # the padding is not read
    assert pairs >= 1, pairs
    assert total > 500 and 5 * refused <= total, (refused, total)
    assert 20 * refused >= total  # (but they are there)


def column_calls(steps):
    """the calls of libmsm_frcol of a program, in order: dicts of the step's index and kind, its field index, the field's form and the hooks
    that are set at the call, what filled its word slot ("mult": the very tensor a lookup call returned; "words": an uploaded vector), the
    length of its table, its operands, and how it ends -- None: it computes; "cut": an output shares bytes with an operand; "sum": the counts
    do not add up to the outputs; "index": an index is neither inside `a` nor MISSING.  Worked out from the steps alone: a `mult` step names
    a slot only where it computes, its indices lie below its table's length, and where it keeps its counts every value it looks up is in
    the table (fr_program._Gen.chain), so that they add up to batch * n."""
    mont, hooks, slots, out = {}, {}, {}, []
    for i, (kind, f, a) in enumerate(steps):
        if kind == "format":
            mont[f] = a["mont"]
        elif kind == "hook":
            hooks[a["name"]] = a["value"]
        elif kind == "words":
            slots[f, a["slot"]] = {"from": "words", "total": sum(a["values"]), "n": len(a["values"]), "least": max([w + 1 for w in a["values"] if w != P.MISSING] or [0])}
        elif kind == "mult":
            if a["cslot"] is not None:
                slots[f, a["cslot"]] = {"from": "mult", "total": a["batch"] * a["n"], "n": a["out"][1]}
            if a["islot"] is not None:
                slots[f, a["islot"]] = {"from": "mult", "n": a["batch"] * a["n"], "least": a["out"][1]}  # (the least n_a that holds every index)
        elif kind in P.COLUMN_CALLS:
            w = slots[f, a["idx" if kind == "gather" else "counts"]]
            if P.column_cut(steps[i]):
                end = "cut"
            elif kind == "gather":
                end = "index" if w["least"] > a["a"][1] else None
            else:
                end = "sum" if w["total"] + a.get("bias", 0) * w["n"] != a["out"][1] else None
            out.append({"index": i, "kind": kind, "f": f, "mont": bool(mont.get(f)), "hooks": {h for h, v in hooks.items() if v}, "from": w["from"], "n_t": a["a" if kind == "gather" else "t"][1],
                        "operands": [a[k] for k in ("t", "a", "out", "s_out") if k in a], "end": end})
    return out


def test_column_calls_take_what_a_lookup_left_at_either_alignment_under_either_form(programs):
    calls = [(fields[c["f"]], c) for fields, _, _, steps in programs for c in column_calls(steps)]
    computing = [(field, c) for field, c in calls if c["end"] is None]
    assert min(sum(c["from"] == "mult" and c["kind"] == kind for _, c in computing) for kind in P.COLUMN_CALLS) >= 5  # the chain the library exists for
    assert sum(rng[0] % 2 for _, c in computing for rng in c["operands"]) >= 5  # 32 bytes as two 16-byte accesses: 16 mod 32 is legal
    assert {(c["kind"], c["mont"]) for _, c in computing} == {(kind, form) for kind in P.COLUMN_CALLS for form in (False, True)}
    assert {c["kind"] for field, c in computing if field == "grumpkin"} == set(P.COLUMN_CALLS)
    assert sum("frcol_test_tile" in c["hooks"] and len(c["hooks"]) > 1 for _, c in computing) >= 5
    assert sum("frcol_test_tile" in c["hooks"] and "frlook_test_hash_bits" in c["hooks"] and c["from"] == "mult" for _, c in computing) >= 1
    assert any(c["kind"] == "expand" and c["n_t"] >= 1025 and "frcol_test_tile" not in c["hooks"] for _, c in computing)  # two tiles of the design's 1024


def test_column_refusals_stay_rare_but_present(programs):
    """a wrong sum, a bad index and a cut: together no more than a fifth of the column calls, so that they do not hide the paths that compute,
    and no fewer than a twentieth; and every vector that must be refused is among them"""
    calls = [c for _, _, _, steps in programs for c in column_calls(steps)]
    ends = [c["end"] for c in calls]
    refused = sum(e is not None for e in ends)
    assert len(calls) > 300 and 5 * refused <= len(calls) and 20 * refused >= len(calls), (refused, len(calls))
    assert min(ends.count(e) for e in ("cut", "sum", "index")) >= 3, {e: ends.count(e) for e in set(ends)}
    assert {(c["kind"], c["end"]) for c in calls if c["end"]} >= {("expand", "cut"), ("pair", "cut"), ("gather", "cut"), ("expand", "sum"), ("pair", "sum"), ("gather", "index")}
    wrapped = off_by_one = at_n_a = 0
    for _, _, _, steps in programs:
        words = {}
        for kind, f, a in steps:
            if kind == "words":
                words[f, a["slot"]] = a["values"]
            elif kind == "mult":
                words.pop((f, a["cslot"]), None), words.pop((f, a["islot"]), None)
            elif kind in ("expand", "pair") and (f, a["counts"]) in words and not P.column_cut((kind, f, a)):
                off = sum(words[f, a["counts"]]) + a.get("bias", 0) * a["t"][1] - a["out"][1]
                wrapped += off != 0 and off % (1 << 32) == 0  # a sum that is right in 32 bits
                off_by_one += off in (1, -1)
            elif kind == "gather" and (f, a["idx"]) in words and not P.column_cut((kind, f, a)):
                at_n_a += a["a"][1] in words[f, a["idx"]]
    assert wrapped >= 1 and off_by_one >= 3 and at_n_a >= 1, (wrapped, off_by_one, at_n_a)


def frmle_calls(steps):
    """the calls of libmsm_frmle of a program, in order: dicts of the step's index and kind, its field index, its order ("top" / "low"), the
    scalars n of a row's table, batch and stride (eq, gemini: one row of n), whether it binds in place (a fold onto its input, a fused round),
    the field's form, the stream and frmle_test_tile at the call, the step's arguments, and how it ends -- None: it computes; "planted": it
    reads a planted value and is refused by the library (`at`: that scalar's index in its row); "overlap": refused for its output"""
    mont, side, tile, out = {}, False, 0, []
    for i, (kind, f, a) in enumerate(steps):
        if kind == "format":
            mont[f] = a["mont"]
        elif kind == "stream":
            side = a["side"]
        elif kind == "hook" and a["name"] == "frmle_test_tile":
            tile = a["value"]
        elif P.LIBRARY.get(kind) == "frmle":
            rows = a["a"] if "a" in a else a["out"]
            batch = a.get("batch", 1)
            stride = rows[1] // batch
            n = a.get("n", rows[1])
            c = {"index": i, "kind": kind, "f": f, "order": "low" if kind == "gemini" else a.get("order", "top"), "n": n, "batch": batch, "stride": stride, "mont": bool(mont.get(f)),
                 "side": side, "tile": tile, "args": a, "end": "overlap" if a.get("overlap") else None, "at": None,
                 "in_place": (kind == "mle_fold" and (a["out"] is None or a["out"][0] == a["a"][0])) or (kind == "round" and a["fold"] is not None)}
            before = steps[i - 1]
            if before[0] == "plant" and not before[2].get("quiet"):
                c["end"], c["at"] = "planted", (before[2]["at"] - rows[0]) // 2 % stride
            out.append(c)
    return out


def low_calls(programs, kind, **where):
    """(fields, call) of the low-first calls of one entry point that compute, over all programs; where: in_place=.."""
    return [(fields, c) for fields, _, _, steps in programs for c in frmle_calls(steps)
            if c["kind"] == kind and c["order"] == "low" and c["end"] is None and all(c[k] == v for k, v in where.items())]


def test_every_single_field_entry_draws_the_frmle_steps_in_both_orders_and_gemini(programs):
    drawn = {}
    for fields, _, _, steps in programs:
        if len(fields) == 1:
            for c in frmle_calls(steps):
                drawn.setdefault(fields[0], set()).add((c["kind"], c["order"]))
    want = {(kind, order) for kind in P.FRMLE_ORDERED for order in ("top", "low")} | {("gemini", "low")}
    assert set(drawn) == {"bn254", "pallas", "vesta", "bls12_381", "grumpkin"} and all(got == want for got in drawn.values()), drawn


def test_the_low_first_fold_in_place_runs_at_every_size_form_stream_and_alignment(programs):
    """csrc/frmle_plan.h: n = 2 is one launch and no copy, n = 4 has a lower half of one output, n >= 1024 has several workgroups to a launch; the
    scratch rows are n / 4 apart, the rows themselves `stride`"""
    calls = [c for _, c in low_calls(programs, "mle_fold", in_place=True)]
    assert sum(c["n"] == 2 for c in calls) >= 3 and sum(c["n"] == 4 for c in calls) >= 3
    assert sum(c["n"] >= 1024 and c["batch"] >= 2 and c["stride"] > c["n"] for c in calls) >= 3
    assert min(sum(c["mont"] == form for c in calls) for form in (False, True)) >= 5
    assert sum(c["side"] for c in calls) >= 5
    assert sum(c["args"]["a"][0] % 2 for c in calls) >= 5  # a start at 16 mod 32


def test_a_low_first_fold_writes_directly_behind_its_input(programs):
    """apart, with `out` on the byte behind the last byte of a's span: every fold of a Gemini step behind its first (multilinear.gemini_folds),
    and mle_fold steps placed so"""
    folds = [c for _, c in low_calls(programs, "mle_fold", in_place=False)]
    behind = [c for c in folds if c["args"]["out"][0] == c["args"]["a"][0] + 2 * ((c["batch"] - 1) * c["stride"] + c["n"])]
    gemini = [c for _, c in low_calls(programs, "gemini") if c["n"] >= 4]
    assert len(behind) >= 5 and len(gemini) >= 20, (len(behind), len(gemini))
    assert any(c["batch"] >= 2 for c in behind)


def test_the_low_first_fused_round_runs_at_every_schedule(programs):
    """csrc/frmle_plan.h: n = 4 is one pair, one launch and no scratch rows; n = 8 two launches of one pair; frmle_test_tile 2 gives launches tiles
    of one pair; under a hook of 2 or 8 several levels of partial sums lie between `partial` and the scratch rows"""
    calls = [c for _, c in low_calls(programs, "round", in_place=True)]
    assert sum(c["n"] == 4 for c in calls) >= 3 and sum(c["n"] == 8 for c in calls) >= 3 and sum(c["n"] >= 1024 for c in calls) >= 3
    for tile in (2, 8):
        hooked = [c for c in calls if c["tile"] == tile and c["n"] >= 64]
        assert len(hooked) >= 3, (tile, len(hooked))
        assert any(P.low_fused_partials(c["n"], tile) >= 3 for c in hooked), tile  # three or more levels of partials
    assert sum(c["batch"] >= 3 and any(c["batch"] - 1 in which for _, which in c["args"]["terms"]) for c in calls) >= 3  # a term names the last row


def test_a_low_first_call_directly_follows_a_top_first_one_of_its_entry_point(programs):
    """the very next step, both of them computing: on the same field; on the other field of a two-field entry; small behind large and large behind
    small; and a low-first fused round behind an mle_eval of more levels, whose scratch rows lie where the eval's levels lay"""
    same, other, to_small, to_large, behind_eval = set(), set(), set(), set(), 0
    for fields, _, _, steps in programs:
        calls = frmle_calls(steps)
        for before, c in zip(calls, calls[1:]):
            if c["index"] != before["index"] + 1 or c["order"] != "low" or before["order"] != "top" or c["end"] or before["end"]:
                continue
            if c["kind"] == before["kind"]:
                (same if c["f"] == before["f"] else other).add(c["kind"])
                if before["n"] >= P.LARGE and c["n"] <= P.SMALL:
                    to_small.add(c["kind"])
                if before["n"] <= P.SMALL and c["n"] >= P.LARGE:
                    to_large.add(c["kind"])
        for before, c in zip(calls, calls[1:]):  # (the eval in either order)
            behind_eval += (c["index"] == before["index"] + 1 and before["kind"] == "mle_eval" and c["kind"] == "round" and c["order"] == "low" and c["in_place"]
                            and not c["end"] and not before["end"] and c["f"] == before["f"] and P.eval_levels(before["n"], before["tile"]) > 1 + P.low_fused_partials(c["n"], c["tile"]))
    every = set(P.FRMLE_ORDERED)
    assert same == every and other == every and to_small == every and to_large == every, (same, other, to_small, to_large)
    assert behind_eval >= 3, behind_eval


def test_a_planted_value_reaches_both_launches_of_a_low_first_fold_in_place_and_an_overlap_is_refused(programs):
    """[0, n / 2) of a row is read by the launch that stores to the scratch rows, [n / 2, n) by the one that stores in place (n >= 4); the call
    is refused and the field's next step computes"""
    lower = upper = overlaps = 0
    for fields, _, _, steps in programs:
        for c in frmle_calls(steps):
            overlaps += c["kind"] == "mle_fold" and c["order"] == "low" and c["end"] == "overlap"
            if c["kind"] == "mle_fold" and c["order"] == "low" and c["in_place"] and c["end"] == "planted" and c["n"] >= 4:
                after = next((j for j in range(c["index"] + 1, len(steps)) if steps[j][1] == c["f"] and steps[j][0] in P.LIBRARY), None)
                if after is not None:
                    model = P.Model(fields)
                    errors = [model.step(s)["error"] for s in steps[:after + 1]]
                    assert errors[c["index"]] == P.ERR_NONCANONICAL
                    if errors[after] is None:
                        lower += c["at"] < c["n"] // 2
                        upper += c["at"] >= c["n"] // 2
    assert lower >= 1 and upper >= 1 and overlaps >= 1, (lower, upper, overlaps)


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
        there = copy.deepcopy(self.m)
        there.mont[f] = False
        getattr(there, "op_" + kind)(f, **a)
        host, dst = self.plain_call(kind, f, a), a["out"] or a["a"]
        if there.raw(f, dst) != self.m.raw(f, dst):  # (a product with 0 is 0 in either form: the fault shows where the bytes differ)
            self.m.put(f, dst[0], there.raw(f, dst))
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


class HashFault(Faulty):
    """a fault in libmsm_frhash: answer(kind, f, a, p, right) -> the wrong plain values of a call that computes, or None where the fault does
    not show; they go where the right ones went (the output range, or the host bytes)"""

    def answer(self, kind, f, a, p, right):
        return None

    def decode(self, f, data):
        """bytes in the field's current form -> plain values"""
        stored = frvec_model.from_bytes(data)
        return frvec_model.mont(stored, self.m.r[f], back=True) if self.m.mont[f] else stored

    def faulty(self, kind, f, a):
        host = self.plain_call(kind, f, a)  # (a refused call raises here: nothing was computed)
        if kind not in P.HASH_CALLS:
            return host
        dst = a["leaves" if kind == "tree" else "a"] if a["out"] is None else a["out"]
        right = host if a["host"] else self.m.raw(f, dst)
        wrong = self.answer(kind, f, a, self.m.hashes[f][a["slot"]], right)
        if wrong is None or self.m.enc(f, wrong) == right:
            return host
        self.fired()
        if a["host"]:
            return self.m.enc(f, wrong)
        self.m.put(f, dst[0], self.m.enc(f, wrong))
        return host


class HandleAnswersForTheOneBefore(HashFault):
    """a handle that answers with the constants of the handle created before it (here: with constants of its own shape from that one's seed)"""
    fields_to_run = "bn254,grumpkin"

    def fresh(self):
        self.seed_before, self.stale = {}, {}

    def faulty(self, kind, f, a):
        if kind == "poseidon":
            if f in self.seed_before:
                self.stale[f, a["slot"]] = self.seed_before[f]
            else:
                self.stale.pop((f, a["slot"]), None)
            self.seed_before[f] = a["seed"]
        elif kind == "poseidon2":  # (a handle of the other kind in that slot: it answers for itself)
            self.stale.pop((f, a["slot"]), None)
        return super().faulty(kind, f, a)

    def answer(self, kind, f, a, p, right):
        if (f, a["slot"]) not in self.stale or (kind == "permute" and a["out"] is None and not a["host"]):  # (in place the input is gone: it shows in every other call)
            return None
        rc, mds = P.poseidon_constants(self.stale[f, a["slot"]], p.t, p.full_rounds, p.partial_rounds, p.r)
        other = frhash_model.Poseidon(p.r, p.t, p.full_rounds, p.partial_rounds, rc, mds, p.capacity, p.capacity_at, p.out_at)
        v = self.m.plain(f, a["leaves" if kind == "tree" else "a"])
        if kind == "permute":
            return [x for i in range(0, len(v), p.t) for x in other.permute(v[i:i + p.t])]
        if kind == "sponge":
            stride = len(v) // a["batch"]
            return [other.hash(v[k * stride:k * stride + a["length"]]) for k in range(a["batch"])]
        return other.merkle_chain(v[0], a["levels"]) if p.t == 2 else [x for level in other.merkle(v) for x in level]


class SpongeReadsThePadding(HashFault):
    """a sponge that reads one scalar of the padding behind `length` as data when the last block is short"""
    fields_to_run = "pallas"

    def answer(self, kind, f, a, p, right):
        stride = a["a"][1] // a["batch"] if kind == "sponge" else 0
        if kind != "sponge" or a["length"] % (p.t - 1) == 0 or stride == a["length"]:
            return None
        v = self.m.plain(f, a["a"])
        return [p.hash(v[k * stride:k * stride + a["length"] + 1]) for k in range(a["batch"])]


class SpongeTakesTheOtherFormsConstants(HashFault):
    """a sponge that converts with the constants of the a * 2^256 form whatever the call's flag says: canonical data hashed as if they were not"""
    fields_to_run = "bn254,bls12_381"

    def answer(self, kind, f, a, p, right):
        if kind != "sponge" or self.m.mont[f]:
            return None
        v, stride = frvec_model.mont(self.m.stored(f, a["a"]), p.r, back=True), a["a"][1] // a["batch"]
        return frvec_model.mont([p.hash(v[k * stride:k * stride + a["length"]]) for k in range(a["batch"])], p.r)


class SecondLevelFromTheLeaves(HashFault):
    """a tree whose second level is hashed from the leaves instead of from the first level"""
    fields_to_run = "grumpkin"

    def answer(self, kind, f, a, p, right):
        arity = p.t - 1
        if kind != "tree" or arity == 1 or a["leaves"][1] < arity * arity:
            return None
        v = self.m.plain(f, a["leaves"])
        levels = [[p.hash(v[arity * j:arity * j + arity]) for j in range(len(v) // arity)]]
        levels.append(levels[0][:len(levels[0]) // arity])  # (the hashes of the first leaves once more)
        while len(levels[-1]) > 1:
            levels.append([p.hash(levels[-1][arity * j:arity * j + arity]) for j in range(len(levels[-1]) // arity)])
        return [x for level in levels for x in level]


class HostOutputFromTheStaleSpot(HashFault):
    """a host-form call whose output comes from where the previous, larger call's output lay in the staging area (the input at its start, the
    output behind it; a permutation in place)"""
    fields_to_run = "vesta"

    def fresh(self):
        self.staging, self.out_at = bytearray(), 0

    def faulty(self, kind, f, a):
        self.operand = self.m.raw(f, a["leaves" if kind == "tree" else "a"]) if kind in P.HASH_CALLS and a["host"] else None  # (before an in-place call changes it)
        return super().faulty(kind, f, a)

    def answer(self, kind, f, a, p, right):
        if not a["host"]:
            return None
        if kind == "sponge":  # (of the last row only what is read)
            self.operand = self.operand[:len(self.operand) - 32 * (a["a"][1] // a["batch"] - a["length"])]
        at = 0 if kind == "permute" else len(self.operand)
        need = at + len(right)
        self.staging.extend(bytes(max(need - len(self.staging), 0)))
        self.staging[:len(self.operand)] = self.operand
        self.staging[at:need] = right
        before, self.out_at = self.out_at, at
        if before <= at:
            return None
        return self.decode(f, bytes(self.staging[before:before + len(right)]).ljust(len(right), b"\0"))  # (canonical scalars: enc() gives these bytes again)


class FirstTidiedWidthGoesWrong(HashFault):
    """a permutation at the field's first tidied width computed with one S-box input unreduced: some wrong but canonical value at exactly that
    width (here: the state's first element gives way to its second)"""
    fields_to_run = "bls12_381"

    def answer(self, kind, f, a, p, right):
        if kind != "permute" or p.t != P.HASH_BOUNDARY[self.m.fields[f]][1]:
            return None
        plain = self.decode(f, right)
        return [plain[1]] + plain[1:]


def hashed_with(other, m, kind, f, a):
    """the plain values of a call of libmsm_frhash as the permutation `other` gives them"""
    v = m.plain(f, a["leaves" if kind == "tree" else "a"])
    if kind == "permute":
        return [x for i in range(0, len(v), other.t) for x in other.permute(v[i:i + other.t])]
    if kind == "sponge":
        stride = len(v) // a["batch"]
        return [other.hash(v[k * stride:k * stride + a["length"]]) for k in range(a["batch"])]
    return other.merkle_chain(v[0], a["levels"]) if other.t == 2 else [x for level in other.merkle(v) for x in level]


class SumTakenLate(frhash2_model.Poseidon2):
    def internal(self, s):
        out = list(s)
        for i in range(self.t):  # (the sum of the state as it stands: behind element 0 it holds what has already changed)
            out[i] = (self.mu[i] * out[i] + sum(out)) % self.r
        return out


class InternalSumTakenLate(HashFault):
    """a Poseidon2 internal round whose sum is taken after s[0]'s neighbours changed: every element but the first takes a sum that holds the
    new values of those before it"""
    fields_to_run = "bls12_381"

    def answer(self, kind, f, a, p, right):
        if not isinstance(p, frhash2_model.Poseidon2) or not p.partial_rounds or (kind == "permute" and a["out"] is None and not a["host"]):  # (in place the input is gone)
            return None
        return hashed_with(SumTakenLate(p.r, p.t, p.full_rounds, p.partial_rounds, p.rc, p.mu, p.capacity, p.capacity_at, p.out_at), self.m, kind, f, a)


class AnsweredWithTheOtherKindsCode(HashFault):
    """a Poseidon2 handle answered with the code of the other kind: its table read as Poseidon's -- the round constants as far as they go and
    round again, the internal layer's matrix J + diag(mu) as the MDS matrix"""
    fields_to_run = "pallas,vesta"

    def answer(self, kind, f, a, p, right):
        if not isinstance(p, frhash2_model.Poseidon2) or (kind == "permute" and a["out"] is None and not a["host"]):
            return None
        need = (p.full_rounds + p.partial_rounds) * p.t
        rc = (p.rc * (need // len(p.rc) + 1))[:need]
        mds = [[1 + (p.mu[i] if i == j else 0) for j in range(p.t)] for i in range(p.t)]
        return hashed_with(frhash_model.Poseidon(p.r, p.t, p.full_rounds, p.partial_rounds, rc, mds, p.capacity, p.capacity_at, p.out_at), self.m, kind, f, a)


class ColumnFault(Faulty):
    """a fault in libmsm_frcol: spoil(kind, f, a, before) changes what a call that computed left in the arena and calls fired() where that
    shows; before: the bytes of its outputs as they were"""

    def spoil(self, kind, f, a, before):
        pass

    def faulty(self, kind, f, a):
        if kind not in P.COLUMN_CALLS:
            return self.plain_call(kind, f, a)
        before = {k: self.m.raw(f, a[k]) for k in ("out", "s_out") if k in a}
        host = self.plain_call(kind, f, a)  # (a refused call raises here)
        self.spoil(kind, f, a, before)
        return host

    def replace(self, f, rng, at, count, stored):
        """`count` scalars from element `at` of the range on become the stored value; -> did a byte change"""
        data = frvec_model.to_bytes([stored] * count)
        changed = self.m.raw(f, (rng[0] + 2 * at, count)) != data
        self.m.put(f, rng[0] + 2 * at, data)
        return changed


class RunOnATileBoundaryCopiesThePreviousEntry(ColumnFault):
    """an expand whose run that starts on a tile boundary copies the previous entry: the last of the tile before"""
    fields_to_run = "grumpkin"

    def spoil(self, kind, f, a, before):
        if kind != "expand":
            return
        tile, t, off = self.m.hooks["frcol_test_tile"] or 1024, self.m.stored(f, a["t"]), 0
        for j, c in enumerate(self.m.words[f][a["counts"]]):
            if j and j % tile == 0 and c + a["bias"] and self.replace(f, a["out"], off, c + a["bias"], t[j - 1]):
                self.fired()
            off += c + a["bias"]


class FillersFromThePreviousCallsZ(ColumnFault):
    """a pair whose fillers come from the z of the previous, larger call: the entries that call never looked up, as far as they lie inside
    this table"""
    fields_to_run = "vesta"

    def fresh(self):
        self.z, self.n = [], 0

    def spoil(self, kind, f, a, before):
        if kind != "pair":
            return
        t, counts = self.m.stored(f, a["t"]), self.m.words[f][a["counts"]]
        if self.n > len(t):
            k = used = 0
            for c in counts:
                for d in range(c):
                    rank = k - used - 1
                    if d and rank < len(self.z) and self.z[rank] < len(t) and self.replace(f, a["s_out"], k, 1, t[self.z[rank]]):
                        self.fired()
                    k += 1
                used += c > 0
        self.z, self.n = [j for j, c in enumerate(counts) if c == 0], len(t)


class MissingElementLeftAsItWas(ColumnFault):
    """a gather that leaves a MISSING element as it was and does not zero it"""
    fields_to_run = "vesta"

    def spoil(self, kind, f, a, before):
        if kind != "gather":
            return
        for i, at in enumerate(self.m.words[f][a["idx"]]):
            if at == P.MISSING and any(before["out"][32 * i:32 * i + 32]):
                self.m.put(f, a["out"][0] + 2 * i, before["out"][32 * i:32 * i + 32])
                self.fired()


class OneScalarPastTheOutput(ColumnFault):
    """a column call that writes one scalar past its output: the output's last once more"""
    fields_to_run = "pallas"

    def spoil(self, kind, f, a, before):
        out = a["s_out" if kind == "pair" else "out"]
        if 16 * (out[0] + 2 * out[1]) + 32 <= len(self.m.arena[f]) and self.replace(f, out, out[1], 1, self.m.stored(f, (out[0] + 2 * out[1] - 2, 1))[0]):
            self.fired()


class LowFault(Faulty):
    """a fault in a low-first call of libmsm_frmle that computes: spoil(kind, f, a, before) changes what the call left in the arena and calls
    fired() where a byte changed; before: a copy of the model as it was"""

    def spoil(self, kind, f, a, before):
        pass

    def faulty(self, kind, f, a):
        if P.LIBRARY.get(kind) != "frmle" or (kind != "gemini" and a.get("order") != "low"):
            return self.plain_call(kind, f, a)
        before = copy.deepcopy(self.m)
        host = self.plain_call(kind, f, a)  # (a refused call raises here)
        self.spoil(kind, f, a, before)
        return host

    def replace(self, f, off16, plain):
        """the plain values go to off16 in the field's form; fired() where that changes a byte"""
        data = self.m.enc(f, plain)
        if self.m.raw(f, (off16, len(plain))) != data:
            self.m.put(f, off16, data)
            self.fired()

    @staticmethod
    def folds_in_place(kind, a):
        return kind == "mle_fold" and (a["out"] is None or a["out"][0] == a["a"][0])


class OrderFlagDropped(Faulty):
    """an eq that answers top first when asked low first; at k <= 1 the orders agree"""
    fields_to_run = "bn254"

    def faulty(self, kind, f, a):
        if kind != "eq" or a.get("order") != "low" or len(a["point"]) < 2:
            return self.plain_call(kind, f, a)
        host = self.plain_call(kind, f, {k: v for k, v in a.items() if k != "order"})
        if self.m.raw(f, a["out"]) != self.m.enc(f, frmle_low_model.eq(a["point"], self.m.r[f], a["scale"])):
            self.fired()
        return host


class ScratchRowsComeHomeForTheFirstRowOnly(LowFault):
    """a low-first fold in place whose copy brings home the first scratch row only: the rows behind it keep their old [0, n / 4)"""
    fields_to_run = "grumpkin"

    def spoil(self, kind, f, a, before):
        if self.folds_in_place(kind, a) and a["batch"] >= 2 and a["n"] >= 4:
            stride = a["a"][1] // a["batch"]
            for k in range(1, a["batch"]):
                self.replace(f, a["a"][0] + 2 * k * stride, before.plain(f, (a["a"][0] + 2 * k * stride, a["n"] // 4)))


class LowerLaunchRunsSecond(LowFault):
    """a low-first fold in place whose launches run the wrong way round: the outputs [n / 8, n / 4) are computed from [n / 4, n / 2) of a row that
    already holds the upper launch's outputs"""
    fields_to_run = "bls12_381"

    def spoil(self, kind, f, a, before):
        if self.folds_in_place(kind, a) and a["n"] >= 8:
            n, stride = a["n"], a["a"][1] // a["batch"]
            for k in range(a["batch"]):
                row = a["a"][0] + 2 * k * stride
                late = self.m.plain(f, (row + 2 * (n // 4), n // 4))  # the outputs [n / 4, n / 2)
                self.replace(f, row + 2 * (n // 8), frmle_low_model.fold(late, a["c"], self.m.r[f]))


class ScratchRowsOverThePartials(LowFault):
    """a low-first fused round under a tile hook whose scratch rows begin on the first level of partial sums where there are more levels than
    one: the first folded scalar of row 0 gives way to the first partial sum (here: the first launch tile's share of g(0))"""
    fields_to_run = "grumpkin"

    def spoil(self, kind, f, a, before):
        hook = self.m.hooks["frmle_test_tile"]
        if kind == "round" and a["fold"] is not None and hook and P.low_fused_partials(a["n"], hook) > 1:
            stride, rows, _ = self.m._rows(f, a["a"], a["batch"], a["n"] // 2)
            share = frmle_low_model.round_values([row[:hook] for row in rows], [(c, tuple(w)) for c, w in a["terms"]], self.m.r[f])[0]
            self.replace(f, a["a"][0], [share])


class GeminiSliceFromTheTable(LowFault):
    """a Gemini step whose second fold reads the head of `a` in place of f_1"""
    fields_to_run = "vesta"

    def spoil(self, kind, f, a, before):
        if kind == "gemini" and len(a["point"]) >= 2:
            r, table = self.m.r[f], self.m.plain(f, a["a"])
            f_1 = frmle_low_model.fold(table, a["point"][0], r)
            rest = frmle_low_model.gemini_folds(table[:len(f_1)], a["point"][1:], r)
            self.replace(f, a["out"][0], f_1 + [x for f_j in rest for x in f_j])


@pytest.mark.parametrize("fault", [ScanTileBoundary, ScratchKeepsTheTail, NttReusesTheTable, TableAnswersForAnother, ErrorWordNotCleared, SecondHalfFromFurtherOn,
                                   MontComputedAsCanonical, OneByteTooMany, HandleAnswersForTheOneBefore, SpongeReadsThePadding, SpongeTakesTheOtherFormsConstants, SecondLevelFromTheLeaves,
                                   HostOutputFromTheStaleSpot, FirstTidiedWidthGoesWrong, InternalSumTakenLate, AnsweredWithTheOtherKindsCode, RunOnATileBoundaryCopiesThePreviousEntry,
                                   FillersFromThePreviousCallsZ, MissingElementLeftAsItWas, OneScalarPastTheOutput, OrderFlagDropped,
                                   ScratchRowsComeHomeForTheFirstRowOnly, LowerLaunchRunsSecond, ScratchRowsOverThePartials, GeminiSliceFromTheTable], ids=lambda c: c.__name__)
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

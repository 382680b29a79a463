"""Randomised differential test of the nine scalar-field libraries as chained programs on shared state: tools/fuzz_fr.py runs the programs of
tests/fr_program.py on the device and compares every range a step wrote, every host value it returned and at last the whole arena with the model.

Case counts.  The time of a test is the Python model's, not the device's.  The model side alone (tools/fuzz_fr.py's loop against
fr_program.ModelBackend, i.e. the model run twice) was measured on a machine without a GPU for every committed seed, and the count of each
test chosen so that it stays at or below about 3 s there.  Measured again with libmsm_frhash's steps among the programs, three runs each, the
median first (the machine's own noise is a fifth of a figure):
    bn254 (seed 20261101) 30 cases 2.7 s (2.4 .. 2.8); pallas (20261102) 30: 2.7 s (2.6 .. 3.1); vesta (20261103) 28: 2.4 s (2.1 .. 3.0);
    bls12_381 (20261104) 15: 1.2 s; grumpkin (20261105) 40: 2.8 s (2.4 .. 2.9).
The three entries over two fields went past the limit at their old counts -- bn254,bls12_381 (20261106) 30: 3.1 .. 4.0 s; pallas,vesta
(20261107) 25: 3.2 .. 3.5 s; bn254,grumpkin (20261108) 40: 3.1 .. 3.5 s -- and not for the Poseidon steps, whose model is 0.3 to 0.7 s of each and
is bounded by fr_program.HASH_WORK: the slowest steps are the model's inverses and folds at 4097 scalars.  A tighter bound does not bring them
back, so each runs as two tests with two seeds and no fewer cases in all:
    bn254,bls12_381 (20261106) 20: 2.5 s (2.1 .. 3.1) and (20261110) 12: 1.8 s (1.7 .. 2.0); pallas,vesta (20261107) 20: 2.3 s (2.0 .. 2.6) and
    (20261109) 12: 0.9 s; bn254,grumpkin (20261108) 28: 2.2 s (1.9 .. 3.0) and (20261111) 14: 1.6 s (1.4 .. 1.6).
The slowest single case took 0.7 s.
With Poseidon2 handles and libmsm_frcol's steps among the programs every draw shifted, so the programs of the same seeds are new ones.  Measured
again the same way on another machine without a GPU, three runs each, the parent commit first, then these programs (median, least .. most):
    bn254 30: parent 2.3 s (2.3 .. 2.5), now 1.8 s; pallas 30: 2.5 s (2.4 .. 2.7), now 2.2 s (2.1 .. 2.3); vesta 28: 2.3 s (2.2 .. 2.4), now
    1.5 s (1.4 .. 1.5); bls12_381 15: 1.1 s (1.1 .. 1.2), now 30 cases: 1.6 s (1.6 .. 1.7); grumpkin 40: 2.6 s (2.3 .. 2.8), now 2.3 s
    (2.2 .. 2.3); bn254,bls12_381 20: 1.9 s (1.8 .. 1.9), now 1.2 s, and 12: 1.3 s, now 1.7 s; pallas,vesta 20: 1.9 s, now 1.5 s, and 12: 0.7 s,
    now 0.5 s; bn254,grumpkin 28: 1.7 s (1.7 .. 1.8), now 2.1 s, and 14: 1.0 s, now 0.9 s (0.9 .. 1.0).
The slowest single case took 0.4 s (parent: 0.55 s).  No entry is past 3 s, so none is split further; bls12_381 has twice its cases, because its 15 did not reach every Poseidon2 width three times (t = 2: once),
and only on that field do t = 3 and t = 12 take paths of their own.  The column steps' model copies lists and is cheap; the Poseidon2 steps are
bounded by fr_program.HASH2_WORK as the Poseidon steps are by HASH_WORK.
With an order on libmsm_frmle's four steps (low first through msm_webgpu_amd.multilinear) and the `gemini` step among the programs every draw
shifted once more.  Measured the same way on a machine without a GPU, three runs each, the parent commit first, then these programs (entry, cases:
median, least .. most):
    bn254 30: parent 1.8 s (1.8 .. 2.0), now 2.2 s (2.0 .. 2.2); pallas 30: 2.2 s (2.2 .. 2.6), now 1.9 s; vesta 28: 1.4 s (1.4 .. 1.5), now 2.7 s
    (2.6 .. 2.7); bls12_381 30: 1.6 s (1.6 .. 1.7), now 2.2 s (2.0 .. 2.2); grumpkin 40: 2.3 s (2.3 .. 2.4), now 2.3 s (2.3 .. 2.6);
    bn254,bls12_381 20: 1.4 s (1.2 .. 1.5), now 1.2 s, and 12: 1.7 s, now 1.4 s (1.4 .. 1.5); pallas,vesta 20: 1.7 s (1.6 .. 2.2), now 1.9 s, and
    12: 0.5 s, now 1.3 s (1.3 .. 1.4); bn254,grumpkin 28: 2.3 s (2.2 .. 2.5), now 1.7 s (1.7 .. 1.9), and 14: 1.0 s, now 2.2 s.
No entry is past 3 s, so no count changes and none is split.  The low-first steps are not what moves the figures: one pass of the model over the
30 bn254 programs (1.2 s) spends 0.07 s in them (tests/frmle_low_model.py's evaluate builds the eq table, n log n products to a row, at no more
than 4096 scalars; a `gemini` step has at most 1024) against 0.24 s in the inverses and 0.47 s in the hashing steps, and which of those a seed
draws is what changed.
Nobody has measured the device side of these counts on its own: the device work is milliseconds, and a test's time is the model's on whatever
CPU the GPU machine has."""
import os
import runpy
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# fields -> (seed, cases): what tests/test_fr_program.py checks the generator's coverage on
COMMITTED = {
    "bn254": (20261101, 30),
    "pallas": (20261102, 30),
    "vesta": (20261103, 28),
    "bls12_381": (20261104, 30),
    "grumpkin": (20261105, 40),
    "bn254,bls12_381": (20261106, 20),
    "pallas,vesta": (20261107, 20),
    "bn254,grumpkin": (20261108, 28),
}
# an entry whose model time went past the limit with one seed runs as two tests, the second with a seed of its own; together no fewer cases than before
SECOND = {"pallas,vesta": (20261109, 12), "bn254,bls12_381": (20261110, 12), "bn254,grumpkin": (20261111, 14)}


def _fuzz(capsys, fields, committed=COMMITTED):
    seed, cases = committed[fields]
    argv = sys.argv
    sys.argv = ["fuzz_fr.py", str(cases), str(seed), fields]
    try:
        runpy.run_path(os.path.join(ROOT, "tools", "fuzz_fr.py"), run_name="__main__")
    finally:
        sys.argv = argv
    assert "fuzz ok: %d cases" % cases in capsys.readouterr().out


@pytest.mark.parametrize("field", ["bn254", "pallas", "vesta", "bls12_381", "grumpkin"])
def test_fuzz_programs_over_one_field(built, capsys, field):
    _fuzz(capsys, field)


@pytest.mark.parametrize("fields", ["bn254,bls12_381", "pallas,vesta", "bn254,grumpkin"])
def test_fuzz_programs_over_two_fields(built, capsys, fields):
    """the two fields share every library's per-device state: a step on one follows a step on the other more often than not"""
    _fuzz(capsys, fields)


@pytest.mark.parametrize("fields", sorted(SECOND))
def test_fuzz_programs_of_a_second_seed(built, capsys, fields):
    _fuzz(capsys, fields, SECOND)

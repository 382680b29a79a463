"""Randomised differential test of the seven scalar-field libraries as chained programs on shared state: tools/fuzz_fr.py runs the programs of
tests/fr_program.py on the device and compares every range a step wrote, every host value it returned and at last the whole arena with the model.

Case counts.  The time of a test is the Python model's, not the device's.  The model side alone (tools/fuzz_fr.py's loop against
fr_program.ModelBackend, i.e. the model run twice) was measured on a machine without a GPU for every committed seed, and the count of each
test chosen so that it stays at or below about 3 s there:
    bn254 (seed 20261101) 30 cases 2.3 s; pallas (20261102) 30: 2.9 s; vesta (20261103) 28: 2.9 s (29: 3.4 s); bls12_381 (20261104) 15: 2.7 s
    (16: 3.0 s); grumpkin (20261105) 40: 1.7 s; bn254,bls12_381 (20261106) 30: 2.7 s; pallas,vesta (20261107) 25: 2.8 s (30: 4.2 s);
    bn254,grumpkin (20261108) 40: 2.9 s.  The slowest single case took 1.6 s (its model steps at 4097 scalars).
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
    "bls12_381": (20261104, 15),
    "grumpkin": (20261105, 40),
    "bn254,bls12_381": (20261106, 30),
    "pallas,vesta": (20261107, 25),
    "bn254,grumpkin": (20261108, 40),
}


def _fuzz(capsys, fields):
    seed, cases = COMMITTED[fields]
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

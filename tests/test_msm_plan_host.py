"""The launch planner of libmsm_hip.so on the CPU: csrc/msm_plan.h includes nothing from HIP, so a stand-alone program
(tests/host_harness/msm_plan_harness.cpp, g++ -O2 -std=c++17) runs plan_launch, whole_msm_request and batch_group on cases read from stdin and
prints every LaunchPlan field.  Checked here: the documented width and group-size rules (tests/launch_model.py) over the whole matrix of formats,
base modes, window settings and sizes; the invariants every accepted plan must satisfy, at the sizes where a ceiling can go wrong; every
rejection plan_launch has, with its code; n = 0; the chunk length under two environment settings; and the bound on the wide tables' top digit
against exact integers.  The same program built with AddressSanitizer and UBSan runs the rejections and the invariant cases once more.
Host logic only, seconds."""
import importlib
import os
import subprocess

import pytest

from tests import launch_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_harness", "msm_plan_harness.cpp")
OK, ERR_INVALID_ARG, ERR_NO_BASES = 0, -2, -6
MODE_PLAIN, MODE_TABLES, MODE_HALVES, MODE_WIDE, MODE_NARROW = range(5)
# include/msm_hip.h: MSM_HIP_SCALARS_*, MSM_HIP_SCALAR_U128, MSM_HIP_SCALAR_SIGNED
FORMAT_ID = {"canonical": 0, "mont256": 1, "u8": 2, "u16": 3, "u32": 4, "u64": 5, "u128": 8, "i8": 18, "i16": 19, "i32": 20, "i64": 21, "i128": 24}
FORMATS = list(FORMAT_ID)
BASE_MODES = ["plain", "endomorphism", "tables", "wide16", "wide17", "wide19", "wide20"]
WINDOWS = [0, 12, 14, 16]
# csrc/msm_layout.h, csrc/msm_plan.h (test_the_limits_the_planner_works_within holds the program to them)
MAXLW, BYTE_MAXLW, NWIN, MAX_TILES, MAX_POINTS, NSLOT = 64, 32, 16, 1024, 1 << 28, 4
SMVP_CHUNK_MIN, SMVP_CHUNK_MAX, SMVP_TARGET_LANES, LIST_SUB = 8, 1024, 9 << 16, 2048
CUS = 256  # an MI355X


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "msm-webgpu_amd", "csrc"), SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msm_plan"), "msm_plan_harness", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msm_plan_san"), "msm_plan_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def line(verb, **kw):
    return verb + "".join(" %s=%d" % (k, int(v)) for k, v in kw.items())


def run(exe, lines, env=None, inherit=False):
    """one answer per line: a dict of integers.  The program sees no MSM_HIP_* setting but those of `env` (inherit: this process's as well)"""
    full = {k: v for k, v in os.environ.items() if inherit or not k.startswith("MSM_HIP_")}
    full.update(env or {})
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=full)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = [dict((k, int(v)) for k, v in (tok.split("=") for tok in ans.split())) for ans in p.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def wide_bits_of(mode):
    return int(mode[4:]) if mode.startswith("wide") else 0


def context(fmt, mode, fixed=0, n_bases=1 << 20, **more):
    """the PlanInputs of a context that holds n_bases bases in `mode` and takes scalars in `fmt`"""
    return dict(dict(n_bases=n_bases, scalar_format=FORMAT_ID[fmt], window_bits=fixed, endo=mode == "endomorphism", precomputed=mode == "tables",
                     wide_bits=wide_bits_of(mode), cus=CUS), **more)


def model_mode(mode):
    return "wide" if mode.startswith("wide") else mode


def per_msm_and_room(fmt, mode, bits):
    """local windows one MSM of the launch takes at `bits`-bit windows, and how many a launch has room for (include/msm_hip.h)"""
    nb = model.NB[fmt]
    if nb:
        return (nb, BYTE_MAXLW) if nb <= 2 else (model.narrow_nwin_of(bits, nb), MAXLW)
    if mode.startswith("wide"):
        return 1 << (wide_bits_of(mode) - 16), 24
    if mode == "tables":
        return 1, MAXLW
    return model.nwin_of(bits, mode == "endomorphism"), MAXLW


def test_the_limits_the_planner_works_within(harness):
    (c,) = run(harness, ["consts"])
    assert c == dict(MAXLW=MAXLW, BYTE_MAXLW=BYTE_MAXLW, NWIN=NWIN, MAX_TILES=MAX_TILES, MAX_POINTS=MAX_POINTS, NSLOT=NSLOT, SMVP_CHUNK_MIN=SMVP_CHUNK_MIN,
                     SMVP_CHUNK_MAX=SMVP_CHUNK_MAX, SMVP_TARGET_LANES=SMVP_TARGET_LANES, LIST_SUB=LIST_SUB, target_lanes=SMVP_TARGET_LANES, chunk_search=1)
    assert (model.MAXLW, model.BYTE_MAXLW) == (MAXLW, BYTE_MAXLW)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------
MODEL_N = [1, 4096, 4097, 65536, 65537, 1 << 20]
MODEL_NVEC = [1, 2, 5]
MODEL_BATCH = [1, 3, 64, 100]


def test_planned_widths_and_group_sizes_follow_the_documented_rules(harness):
    cells = [(f, b, w, n, v) for f in FORMATS for b in BASE_MODES for w in WINDOWS for n in MODEL_N for v in MODEL_NVEC]
    plans = run(harness, [line("plan", whole=1, n=n, nvec=v, **context(f, b, w)) for f, b, w, n, v in cells])
    accepted = 0
    for (f, b, w, n, v), p in zip(cells, plans):
        bits = model.run_bits(f, model_mode(b), w, n, v)
        per_msm, room = per_msm_and_room(f, b, bits)
        if v * per_msm > room:
            assert p == dict(rc=ERR_INVALID_ARG), (f, b, w, n, v, p)  # no room: rejected, never planned at another shape
            continue
        accepted += 1
        assert p["rc"] == OK and p["wbits"] == bits, (f, b, w, n, v, p)
        assert p["w_count"] == v * per_msm and p["whole"] == 1 and p["nvec"] == v and p["n"] == n, (f, b, w, n, v, p)
        assert (p["nb"], p["nb_signed"]) == (model.NB[f], int(f.startswith("i"))), (f, p)
    assert accepted > len(cells) * 3 // 4  # (what does not fit: 5 plain MSMs, and the wide tables' 19 / 20-bit widths with several)
    groups = [(f, b, w, n, k) for f in FORMATS for b in BASE_MODES for w in WINDOWS for n in MODEL_N for k in MODEL_BATCH]
    got = run(harness, [line("group", n=n, batch=k, **context(f, b, w)) for f, b, w, n, k in groups])
    for (f, b, w, n, k), g in zip(groups, got):
        want = model.batch_groups(f, model_mode(b), w, n, k, 1 << max(wide_bits_of(b) - 16, 0))
        assert g["group"] == want[0], (f, b, w, n, k, g, want)


# ---- invariants --------------------------------------------------------------------------------------------------------------------------------------
EDGE_N = [1, 2047, 2048, 2049, 2048 * 1024, 2048 * 1024 + 1, 1 << 24, 1 << 28]
MOST_POINTS = {"endomorphism": 1 << 27, "tables": 1 << 24}  # what a base set of the mode can hold (include/msm_hip.h); the wide tables: 2^24 as well


def invariant_cases():
    """(what, the case's line): whole MSMs of every base mode and a few formats at the edge sizes, one and two vectors, and the shares"""
    out = []
    for n in EDGE_N:
        for b in BASE_MODES:
            if n > MOST_POINTS.get(b, (1 << 24) if b.startswith("wide") else MAX_POINTS):
                continue
            for f in ("canonical", "u8", "i16", "u32", "i64", "u128"):
                for v in (1, 2):
                    if (f, b, v) != ("canonical", "wide20", 2):  # (two MSMs of 16 virtual windows: no room, a rejection)
                        out.append((("whole", f, b, n, v), line("plan", whole=1, n=n, nvec=v, **context(f, b, 0, n_bases=n))))
            if b == "plain":  # 2 of the 16 windows, to device memory
                out.append((("share", "canonical", b, n, 3), line("plan", n=n, nvec=3, w_begin=6, w_end=8, sums_dev=1, **context("canonical", b, 0, n_bases=n))))
            if b == "endomorphism":  # 1 of the 8 half-length windows
                out.append((("share", "canonical", b, n, 2), line("plan", n=n, nvec=2, mode=MODE_HALVES, w_begin=7, w_end=8, sums_dev=1,
                                                                  **context("canonical", b, 0, n_bases=n))))
            if b in ("wide19", "wide20"):  # 2 (the list path) and 6 of the virtual windows
                c = wide_bits_of(b)
                for vc in (2, 6):
                    out.append((("vshare", "canonical", b, n, vc), line("plan", n=n, nvec=2, mode=MODE_WIDE, w_end=(254 + c) // c, wbits=c, v_begin=1, v_count=vc,
                                                                        sums_dev=1, **context("canonical", b, 0, n_bases=n))))
    return out


def check_invariants(what, p):
    kind, f, b, n, v = what
    assert p["rc"] == OK, (what, p)
    halves, wide, tables, nb = p["mode"] == MODE_HALVES, p["mode"] == MODE_WIDE, p["mode"] == MODE_TABLES, p["nb"]
    assert p["chunks"] * p["chunk_len"] >= p["n_entries"] >= 1, (what, p)
    assert p["tiles"] * p["tile_len"] >= p["n_sc"] and p["tiles"] <= MAX_TILES and (p["tiles"] - 1) * p["tile_len"] < p["n_sc"], (what, p)
    assert p["subtiles"] * LIST_SUB >= p["n_sc"] > (p["subtiles"] - 1) * LIST_SUB, (what, p)
    assert p["stride"] % 4 == 0 and p["n_entries"] <= p["stride"] < p["n_entries"] + 4, (what, p)
    assert 1 <= p["w_count"] <= MAXLW and p["half"] == 1 << (p["wbits"] - 1) and p["ncoarse"] * 256 == p["half"], (what, p)
    assert p["n_sc"] == (2 * n if halves else n), (what, p)
    if not wide:  # (the wide tables plan the longest chunk the device may pick: beyond the kernel's own limits for skewed scalars)
        assert SMVP_CHUNK_MIN <= p["chunk_len"] <= SMVP_CHUNK_MAX, (what, p)
        assert (p["chunks"] - 1) * p["chunk_len"] < p["n_entries"], (what, p)
    # LaunchPlan's comments: wbits settled (16 behind the wide tables' recode), v_count the virtual windows run, nwin the window sums per MSM,
    # combine_bits the bits between consecutive windows (byte windows: 8), whole = every vector's windows make a whole MSM
    whole_windows = (nb if nb <= 2 else model.narrow_nwin_of(p["wbits"], nb)) if nb else NWIN if tables else model.nwin_of(wide_bits_of(b) or p["wbits"], halves)
    assert p["w_count_vec"] == p["w_end"] - p["w_begin"], (what, p)
    assert p["whole"] == int(not p["pairs"] and p["w_count_vec"] == whole_windows) == int(kind == "whole"), (what, p)
    assert p["combine_bits"] == (8 if nb in (1, 2) else p["wbits"]), (what, p)
    if wide:
        vwin = 1 << (wide_bits_of(b) - 16)
        assert p["wbits"] == 16 and p["wide_bits"] == wide_bits_of(b) and p["pairs"] == int(kind == "vshare"), (what, p)
        assert p["v_count"] == (v if kind == "vshare" else vwin) and p["nwin"] == p["v_count"] and p["full_windows"] == vwin, (what, p)
        assert p["w_count"] == p["nvec"] * p["v_count"] and p["n_entries"] == n * p["w_count_vec"], (what, p)
        assert p["share_shape"] == int(kind == "vshare" and v <= 4) == p["list_path"], (what, p)
        if p["list_path"]:
            assert p["tile_len"] % LIST_SUB == 0, (what, p)
    elif tables:
        assert p["nwin"] == 1 and p["w_count"] == p["nvec"] and p["n_entries"] == n * NWIN and p["full_windows"] == 1, (what, p)
    else:
        assert p["nwin"] == whole_windows == p["full_windows"] and p["w_count"] == p["nvec"] * p["w_count_vec"] and p["n_entries"] == p["n_sc"], (what, p)
    # digit planes: window shares of 32-byte scalars (at most 8 of a vector's windows), never whole MSMs, tables or narrow scalars
    assert p["planes"] == int(kind == "share"), (what, p)


def test_every_accepted_plan_keeps_the_invariants(harness):
    cases = invariant_cases()
    plans = run(harness, [c for _, c in cases])
    for (what, _), p in zip(cases, plans):
        check_invariants(what, p)
    masked = run(harness, [line("plan", whole=1, n=100, **context("canonical", "plain", n_bases=100, n_identity=k)) for k in (0, 1, 7)])
    assert [p["mask"] for p in masked] == [0, 1, 1]
    assert len({what[0] for what, _ in cases}) == 3 and len(cases) > 400


# ---- rejections --------------------------------------------------------------------------------------------------------------------------------------
def rejection_cases():
    """(what, code, line); the accepted neighbours of the rejections come first, code 0"""
    plain = context("canonical", "plain", n_bases=1000)
    u32 = dict(context("u32", "plain", n_bases=1000), mode=MODE_NARROW, w_end=3)  # 3 windows of 16 bits hold 4 bytes
    u8 = dict(context("u8", "plain", n_bases=1000), mode=MODE_NARROW, w_end=1)
    sparse = dict(plain, sparse=1, indices=1)
    w17 = dict(context("canonical", "wide17", n_bases=1000), mode=MODE_WIDE, w_end=15, wbits=17)
    w19 = dict(context("canonical", "wide19", n_bases=1000), mode=MODE_WIDE, w_end=14, wbits=19)
    w20 = dict(context("canonical", "wide20", n_bases=1000), mode=MODE_WIDE, w_end=13, wbits=20)
    I, ok = ERR_INVALID_ARG, OK
    return [
        ("plain", ok, line("plan", n=100, **plain)),
        ("the last slot, the last bases", ok, line("plan", n=100, slot=NSLOT - 1, base_off=900, **plain)),
        ("4 plain MSMs", ok, line("plan", n=100, nvec=4, **plain)),
        ("narrow u32", ok, line("plan", n=100, wbits=16, **u32)),
        ("narrow u32 at 4 bytes past the boundary", ok, line("plan", n=100, wbits=16, align=4, **u32)),
        ("narrow u8 at 12 bits", ok, line("plan", n=100, wbits=12, align=1, **u8)),
        ("sparse, more entries than bases", ok, line("plan", n=5000, **sparse)),
        ("wide 17", ok, line("plan", n=100, nvec=12, **w17)),
        ("wide 19, a share", ok, line("plan", n=100, v_begin=6, v_count=2, sums_dev=1, **w19)),
        ("null context", I, line("plan", n=100, null_ctx=1)),
        ("null scalars", I, line("plan", n=100, scalars=0, **plain)),
        ("no bases", ERR_NO_BASES, line("plan", n=100, **dict(plain, n_bases=0))),
        ("n > 2^28", I, line("plan", n=MAX_POINTS + 1, **dict(plain, n_bases=1 << 29))),
        ("dense n > n_bases", I, line("plan", n=1001, **plain)),
        ("base_off + n > n_bases", I, line("plan", n=100, base_off=901, **plain)),
        ("slot past the last", I, line("plan", n=100, slot=NSLOT, **plain)),
        ("negative slot", I, line("plan", n=100, slot=-1, **plain)),
        ("empty window range", I, line("plan", n=100, w_begin=3, w_end=3, **plain)),
        ("reversed window range", I, line("plan", n=100, w_begin=5, w_end=2, **plain)),
        ("negative first window", I, line("plan", n=100, w_begin=-1, w_end=2, **plain)),
        ("window range past the last", I, line("plan", n=100, w_begin=0, w_end=17, **plain)),
        ("w_count > MAXLW", I, line("plan", n=100, nvec=5, **plain)),
        ("no vectors", I, line("plan", n=100, nvec=0, **plain)),
        ("narrow mode on 32-byte scalars", I, line("plan", n=100, mode=MODE_NARROW, w_end=3, **plain)),
        ("narrow with a window share", I, line("plan", n=100, wbits=16, **dict(u32, w_end=2))),
        ("narrow with a later first window", I, line("plan", n=100, wbits=16, w_begin=1, **u32)),
        ("narrow with sums_dev", I, line("plan", n=100, wbits=16, sums_dev=1, **u32)),
        ("narrow with base_off", I, line("plan", n=100, wbits=16, base_off=4, **u32)),
        ("narrow from a misaligned pointer", I, line("plan", n=100, wbits=16, align=2, **u32)),
        ("narrow beyond its windows", I, line("plan", n=100, wbits=16, nvec=22, **u32)),
        ("byte windows at 16 bits", I, line("plan", n=100, wbits=16, **u8)),
        ("sparse with wide tables", I, line("plan", n=100, sparse=1, indices=1, **w17)),
        ("sparse with nvec = 2", I, line("plan", n=100, nvec=2, **sparse)),
        ("sparse with sums_dev", I, line("plan", n=100, sums_dev=1, **sparse)),
        ("sparse with base_off", I, line("plan", n=100, base_off=1, **sparse)),
        ("sparse with null indices", I, line("plan", n=100, **dict(sparse, indices=0))),
        ("sparse with a window share", I, line("plan", n=100, w_end=8, **sparse)),
        ("wide at another width than the context's", I, line("plan", n=100, **dict(w17, w_end=14, wbits=19))),
        ("wide on a context without wide tables", I, line("plan", n=100, mode=MODE_WIDE, w_end=15, wbits=17, **plain)),
        ("whole wide MSMs, nvec * vwin > 24", I, line("plan", n=100, nvec=2, **w20)),
        ("whole wide MSMs, 13 x 2", I, line("plan", n=100, nvec=13, **w17)),
        ("whole wide MSMs with sums_dev", I, line("plan", n=100, sums_dev=1, **w17)),
        ("virtual windows past the tables'", I, line("plan", n=100, v_begin=7, v_count=2, sums_dev=1, **w19)),
        ("virtual windows from a negative one", I, line("plan", n=100, v_begin=-1, v_count=2, sums_dev=1, **w19)),
        ("a negative number of virtual windows", I, line("plan", n=100, v_begin=2, v_count=-1, sums_dev=1, **w19)),
        ("v_count without wide tables", I, line("plan", n=100, v_count=1, **plain)),
    ]


def test_every_rejection_with_its_code(harness):
    cases = rejection_cases()
    for (what, code, _), p in zip(cases, run(harness, [c for _, _, c in cases])):
        assert p["rc"] == code and (code == OK or p == dict(rc=code)), (what, p)
    assert sum(code != OK for _, code, _ in cases) >= 30


def test_nothing_to_compute_is_the_plain_16_bit_request(harness):
    cells = [(f, b, w, nb) for f in FORMATS for b in BASE_MODES for w in WINDOWS for nb in (0, 1000)]
    for cell, p in zip(cells, run(harness, [line("plan", whole=1, n=0, scalars=0, **context(f, b, w, n_bases=nb)) for f, b, w, nb in cells])):
        assert (p["rc"], p["mode"], p["w_begin"], p["w_end"], p["wbits"], p["nb"], p["w_count"], p["nwin"], p["whole"]) == (OK, MODE_PLAIN, 0, NWIN, 16, 0, NWIN, NWIN, 1), (cell, p)


# ---- the environment ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [65536, 200000])
def test_the_plain_quotient_under_the_environment(harness, lanes):
    """MSM_HIP_CHUNK_SEARCH=0 and MSM_HIP_TARGET_LANES in a child process: the chunk length is ceil(n * w_count / target lanes), within the kernel's limits"""
    env = {"MSM_HIP_CHUNK_SEARCH": "0", "MSM_HIP_TARGET_LANES": str(lanes)}
    (c,) = run(harness, ["consts"], env)
    assert (c["target_lanes"], c["chunk_search"]) == (lanes, 0)
    cells = [(b, n, v) for b in ("plain", "endomorphism", "tables") for n in (1, 4097, 70000, 1 << 20, (1 << 22) + 3, 1 << 23) for v in (1, 2, 3)]
    plans = run(harness, [line("plan", whole=1, n=n, nvec=v, **context("canonical", b, 0, n_bases=n)) for b, n, v in cells], env)
    lengths = set()
    for (b, n, v), p in zip(cells, plans):
        want = min(max(-(-p["n_entries"] * p["w_count"] // lanes), SMVP_CHUNK_MIN), SMVP_CHUNK_MAX)
        assert p["rc"] == OK and p["chunk_len"] == want and p["chunks"] == -(-p["n_entries"] // want), (b, n, v, p)
        lengths.add(want)
    assert len(lengths) >= 6 and {SMVP_CHUNK_MIN, SMVP_CHUNK_MAX} <= lengths  # both limits, and lengths between them


# ---- the wide tables' top digit ------------------------------------------------------------------------------------------------------------------------
def test_the_bound_on_the_wide_tables_top_digit(harness):
    """As tests/test_abi.py::test_wide_table_shapes_follow_the_scalar_field computes it: the top digit of a C-bit signed recode is at most
    ((r - 1 + bias) >> P) - 2^(C-1); wide_top_max (a 64-bit fraction) must never be below that, and a width fits exactly when the digit does"""
    moduli = {cid: importlib.import_module("oracle." + name).R for cid, name in
              ((0, "bn254_ref"), (1, "grumpkin_ref"), (2, "pallas_ref"), (3, "vesta_ref"), (4, "bls12_381_ref"), (5, "bn254_g2_ref"), (6, "bls12_381_g2_ref"))}
    cells = [(cid, bits) for cid in moduli for bits in (16, 17, 18, 19, 20)]
    for (cid, bits), g in zip(cells, run(harness, [line("wide", curve=cid, bits=bits, wide_bits_choice=bits, n=1 << 20) for cid, bits in cells])):
        r, t = moduli[cid], (254 + bits) // bits
        pos, half = bits * (t - 1), 1 << (bits - 1)
        dmax = ((r - 1 + sum(1 << (bits * w + bits - 1) for w in range(t))) >> pos) - half
        assert g["top_pos"] == pos and g["top_max"] >= dmax and g["fit"] == int(dmax <= half), (cid, bits, g, dmax)
        assert g["pick"] == (bits if dmax <= half else -1), (cid, bits, g)
    sizes = [1000, 1 << 16, (1 << 16) + 1, 1 << 20, (1 << 20) + 1, 1 << 24]
    for cid, r in moduli.items():
        fits17 = r < (1 << 254) + (1 << 200)  # BN254, Grumpkin, Pallas, Vesta; not BLS12-381
        got = run(harness, [line("wide", curve=cid, n=n) for n in sizes])
        assert [g["pick"] for g in got] == [16, 16, 17 if fits17 else 19, 17 if fits17 else 19, 20, 20], cid


# ---- once more under the sanitizers --------------------------------------------------------------------------------------------------------------------
def test_the_same_answers_under_asan_and_ubsan(harness, sanitized):
    lines = [c for _, _, c in rejection_cases()] + [c for _, c in invariant_cases()] + [line("group", n=4097, batch=64, **context("u64", "plain"))]
    lines += [line("wide", curve=cid, bits=bits) for cid in range(7) for bits in (16, 17, 18, 19, 20)]
    assert run(sanitized, lines) == run(harness, lines)

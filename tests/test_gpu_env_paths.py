"""The code paths the MSM_HIP_* environment settings select, oracle-checked ("Environment variables").

The library reads each setting once per process, so every row starts tests/env_child.py as a fresh child with os.environ plus the row's
variables: the child runs a seeded workload aimed at the path the setting switches, checks every result bit-exactly against the CPU oracle,
and reports through the read-only test hook msm_hip_test_env_report what the library resolved and what shape its launches took.  A row
passes only if every result matched AND its evidence shows the setting took effect (no row passes vacuously).

Children run one at a time, each under its own time limit.  After a child that ends abnormally (a signal, a timeout, an abort) every
later row of this module fails at once without starting another process on the GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "env_child.py")
SMVP_CHUNK_MIN, SMVP_CHUNK_MAX = 8, 1024

# return codes after which no further child may use the GPU: killed by a signal (negative), timeout(1)'s 124 / 137, SIGABRT / SIGSEGV
# reported by a shell (134 / 139); None = the time limit of subprocess.run expired
ABNORMAL_CODES = (124, 134, 137, 139)


def is_abnormal(returncode):
    """True if a child's end means the GPU may be in a bad state (then nothing more is started on it)"""
    return returncode is None or returncode < 0 or returncode in ABNORMAL_CODES


_guard = {"tripped": None}


def _all(ev, key, pred):
    rows = ev.get(key, [])
    return bool(rows) and all(pred(r) for r in rows)


def _logr_ok(want):
    def check(ev):
        exp = {16: want, 14: 4 if want == 4 else 2, 12: 2}
        return _all(ev, "logr", lambda r: r[4] == exp[r[2]]) and {r[2] for r in ev["logr"]} == {12, 14, 16}
    return check


def _planes_max_w(max_w):
    def check(ev):
        nwin = {"share": 16, "half_share": 8, "whole": 16, "batch": 16, "whole_endo": 8}
        return _all(ev, "planes", lambda r: r[2] == (r[1] <= max_w and r[1] < nwin[r[0]]))
    return check


def _wide_bits(bits):
    return lambda ev: (ev["settings"]["wide_bits"] == bits and _all(ev, "wide_bits", lambda r: r[2] == bits)
                       and _all(ev, "precedence", lambda r: r[1] == r[2]))


def _upload(ev, name, n):
    return [r for r in ev.get("upload", []) + ev.get("parts", []) if r[1] == n and r[0] == name]


# (id, variables, workload, time limit in s, the evidence the row must show)
ROWS = [
    ("window_bits_12", {"MSM_HIP_WINDOW_BITS": "12"}, "window_bits", 180, lambda ev: _all(ev, "single_wbits", lambda r: r[2] == 12)),
    ("window_bits_14", {"MSM_HIP_WINDOW_BITS": "14"}, "window_bits", 180, lambda ev: _all(ev, "single_wbits", lambda r: r[2] == 14)),
    ("window_bits_16", {"MSM_HIP_WINDOW_BITS": "16"}, "window_bits", 180, lambda ev: _all(ev, "single_wbits", lambda r: r[2] == 16)),
    # 2^16 points x 16 windows over 1024 lanes: the plain quotient is SMVP_CHUNK_MAX; the workgroups-per-CU search may settle 25 % below it
    ("target_lanes_1024", {"MSM_HIP_TARGET_LANES": "1024"}, "chunk", 240,
     lambda ev: ev["settings"]["target_lanes"] == 1024 and _all(ev, "chunk_len", lambda r: r[3] != 16 or SMVP_CHUNK_MAX * 3 // 4 <= r[2] <= SMVP_CHUNK_MAX)),
    ("target_lanes_1024_no_search", {"MSM_HIP_TARGET_LANES": "1024", "MSM_HIP_CHUNK_SEARCH": "0"}, "chunk", 240,
     lambda ev: _all(ev, "chunk_len", lambda r: r[3] != 16 or r[2] == SMVP_CHUNK_MAX)),
    ("target_lanes_huge_no_search", {"MSM_HIP_TARGET_LANES": "67108864", "MSM_HIP_CHUNK_SEARCH": "0"}, "chunk", 240,
     lambda ev: ev["settings"]["chunk_search"] == 0 and _all(ev, "chunk_len", lambda r: r[2] == SMVP_CHUNK_MIN)
     and _all(ev, "chunk_len_batch", lambda r: r[1] == SMVP_CHUNK_MIN)),
    ("bpr_logr_2", {"MSM_HIP_BPR_LOGR": "2"}, "bpr", 180, _logr_ok(2)),
    ("bpr_logr_3", {"MSM_HIP_BPR_LOGR": "3"}, "bpr", 180, _logr_ok(3)),
    ("bpr_logr_4", {"MSM_HIP_BPR_LOGR": "4"}, "bpr", 180, _logr_ok(4)),
    ("planes_max_w_0", {"MSM_HIP_PLANES_MAX_W": "0"}, "planes", 120, _planes_max_w(0)),
    ("planes_max_w_15", {"MSM_HIP_PLANES_MAX_W": "15"}, "planes", 120, _planes_max_w(15)),
    ("planes_whole", {"MSM_HIP_PLANES_WHOLE": "1"}, "planes", 120, lambda ev: _all(ev, "planes", lambda r: r[2] == 1)),
    ("inline_reduce_0", {"MSM_HIP_INLINE_REDUCE": "0"}, "pipeline", 120,
     lambda ev: ev["settings"]["inline_reduce"] == 0 and _all(ev, "inline", lambda r: r[2] == 0)),
    ("reduce_priority_0", {"MSM_HIP_REDUCE_PRIORITY": "0"}, "pipeline", 120,
     lambda ev: ev["settings"]["reduce_priority"] == 0 and _all(ev, "inline", lambda r: r[2] == (r[0] == "sync"))),
    ("fine_hist_min_logn_0", {"MSM_HIP_FINE_HIST_MIN_LOGN": "0"}, "fine_hist", 120, lambda ev: _all(ev, "fine_hist", lambda r: r[1] == 1)),
    ("fine_hist_min_logn_39", {"MSM_HIP_FINE_HIST_MIN_LOGN": "39"}, "fine_hist", 120, lambda ev: _all(ev, "fine_hist", lambda r: r[1] == 0)),
    ("bases_auto_0", {"MSM_HIP_BASES_AUTO": "0"}, "bases_auto", 120,
     lambda ev: ev["settings"]["bases_auto"] == 0 and _all(ev, "uses_endomorphism", lambda r: r[1] is False)),
    # 2^10-point upload chunks: 69 at n = 70001, and more than 8 per part (the ring of 8 landing events is reused) from 2^13 points on
    ("oneshot_chunk_log_10", {"MSM_HIP_ONESHOT_CHUNK_LOG": "10"}, "oneshot_chunks", 240,
     lambda ev: ev["settings"]["oneshot_chunk"] == 1024 and all(r[3] == 69 for r in _upload(ev, "bn254", 70001))
     and all(r[2] == 2 and r[3] > 8 for r in _upload(ev, "bn254", (1 << 19) + 3) + _upload(ev, "bls12_381", (1 << 19) + 3))),
    ("oneshot_chunk_log_10_parts_3", {"MSM_HIP_ONESHOT_CHUNK_LOG": "10", "MSM_HIP_ONESHOT_PARTS": "3"}, "oneshot_chunks", 240,
     lambda ev: all(r[2] == 3 and r[3] > 8 for r in _upload(ev, "bn254", (1 << 19) + 3) + _upload(ev, "bls12_381", (1 << 19) + 3))
     and _upload(ev, "bls12_381", (1 << 19) + 3) != []),
    # (no overlapped upload: the one-shot call is set_bases + msm_hip_run, whose own parts start at 2^20 points)
    ("oneshot_overlap_0", {"MSM_HIP_ONESHOT_OVERLAP": "0"}, "parts", 240,
     lambda ev: _all(ev, "parts", lambda r: r[0] != "oneshot" or (r[2] == (2 if r[1] >= 1 << 20 else 1) and r[3] == 0))),
    ("oneshot_keep_0", {"MSM_HIP_ONESHOT_KEEP": "0"}, "parts", 240,
     lambda ev: ev["settings"]["oneshot_keep"] == 0 and _all(ev, "parts", lambda r: r[0] != "oneshot" or r[2] == 2)),
    ("oneshot_parts_1", {"MSM_HIP_ONESHOT_PARTS": "1"}, "parts", 240, lambda ev: _all(ev, "parts", lambda r: r[2] == 1)),
    ("oneshot_parts_4", {"MSM_HIP_ONESHOT_PARTS": "4"}, "parts", 240,
     lambda ev: _all(ev, "parts", lambda r: r[2] == (4 if r[0] == "oneshot" or r[1] >= 1 << 20 else 1))),
] + [
    ("wide_bits_%d" % b, {"MSM_HIP_WIDE_BITS": str(b)}, "wide", 180, _wide_bits(b)) for b in (16, 17, 18, 19, 20)
] + [
    # a forced shift of the top digit (round 4's shape): non-zero at 19 and 20 bits on BN254
    ("wide_top_shift_4", {"MSM_HIP_WIDE_TOP_SHIFT": "4"}, "wide", 240,
     lambda ev: all(any(r[0] == "bn254" and r[1] == b and r[2] > 0 for r in ev["top_shift"]) for b in (19, 20))),
    ("wide_slack_pct_0", {"MSM_HIP_WIDE_SLACK_PCT": "0"}, "wide", 240, lambda ev: ev["settings"]["wide_slack_ppm"] == 0),
    ("wide_slack_pct_100", {"MSM_HIP_WIDE_SLACK_PCT": "100"}, "wide", 240, lambda ev: ev["settings"]["wide_slack_ppm"] == 1000000),
    ("wide_share_lists_0", {"MSM_HIP_WIDE_SHARE_LISTS": "0"}, "wide", 240,
     lambda ev: ev["settings"]["wide_share_lists"] == 0 and _all(ev, "share_lists", lambda r: r[3] == 0)),
    ("combine_threads_1", {"MSM_HIP_COMBINE_THREADS": "1"}, "combine", 120,
     lambda ev: ev["settings"]["combine_helpers"] == 0 and _all(ev, "combine", lambda r: r[1] == 0)),
    ("combine_threads_8", {"MSM_HIP_COMBINE_THREADS": "8"}, "combine", 120,
     lambda ev: ev["settings"]["combine_helpers"] == 7 and _all(ev, "combine", lambda r: r[1] == 7)),
    ("debug_sync_1", {"MSM_HIP_DEBUG_SYNC": "1"}, "debug_sync", 240, lambda ev: ev["settings"]["debug_sync"] == 1),
]

# every MSM_HIP_* name the library reads is either set by a row above or listed here (tests/test_env_paths_listed.py checks it)
EXCLUDED = {
    "MSM_HIP_SMVP_LDS_PAD": "dynamic LDS padding for A/B; large values can exceed the workgroup's LDS",
}


def row_variables():
    return {k for _, env, _, _, _ in ROWS for k in env}


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_env_setting_path(built, row):
    rid, variables, workload, limit, took_effect = row
    if _guard["tripped"]:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _guard["tripped"])
    env = dict(os.environ)
    env.update(variables)
    try:
        p = subprocess.run([sys.executable, CHILD, workload, str(20261016 + len(rid))], env=env, cwd=os.path.dirname(HERE),
                           capture_output=True, text=True, timeout=limit)
        rc, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        rc, out, err = None, e.stdout or "", e.stderr or ""
    if is_abnormal(rc):
        _guard["tripped"] = "%s: return code %s" % (rid, rc)
    lines = [ln for ln in (out if isinstance(out, str) else out.decode()).splitlines() if ln.startswith("{")]
    tail = (err if isinstance(err, str) else err.decode())[-3000:]
    assert rc == 0 and lines, "child %s ended with %s\n%s" % (rid, rc, tail)
    res = json.loads(lines[-1])
    print(rid, json.dumps(res))
    assert res["cases"] > 0 and not res["failures"], res["failures"]
    assert took_effect(res["evidence"]), "%s: the setting did not show in the launches: %s" % (rid, json.dumps(res["evidence"])[:3000])

"""The documented rules for a whole-MSM launch's shape (include/msm_hip.h; the library's side is csrc/msm_plan.h): the window width a launch runs at
and the vectors per launch of the batch runners.  Pure Python, no device: tests/test_msm_plan_host.py holds the planner to it on the CPU, and
tests/test_gpu_launch_matrix.py every launch on the device."""
NB = {"canonical": 0, "mont256": 0, "u8": 1, "u16": 2, "u32": 4, "u64": 8, "u128": 16, "i8": 1, "i16": 2, "i32": 4, "i64": 8, "i128": 16}  # bytes of a narrow scalar
MAXLW, BYTE_MAXLW, BYTE_WBITS = 64, 32, 12


def nwin_of(bits, halves=False):
    return ((127 if halves else 254) + bits) // bits


def narrow_nwin_of(bits, nb):
    return (8 * nb + bits) // bits


def pick_window_bits(fixed, n, nvec, halves=False, nb=0):
    """msm_plan.h: the fixed width, or 12 bits up to 2^12 points and 16 beyond for one MSM per launch, 14 up to 2^16 for several; widened
    until the launch's windows fit MAXLW"""
    bits = fixed or ((14 if n <= 1 << 16 else 16) if nvec > 1 else (12 if n <= 1 << 12 else 16))
    while bits < 16 and nvec * (narrow_nwin_of(bits, nb) if nb else nwin_of(bits, halves)) > MAXLW:
        bits += 2
    return bits


def run_bits(fmt, mode, fixed, n, nvec=1):
    """the window width a whole-MSM launch of nvec vectors of n points (or a sparse launch of n entries) runs at"""
    nb = NB[fmt]
    if nb in (1, 2):
        return BYTE_WBITS  # byte windows
    if nb:
        return pick_window_bits(fixed, n, nvec, nb=nb)  # truncated signed windows, on the plain records whatever the base mode
    if mode in ("tables", "wide"):
        return 16  # (wide tables: everything behind the recode sees 16-bit local windows)
    return pick_window_bits(fixed, n, nvec, halves=mode == "endomorphism")


def batch_groups(fmt, mode, fixed, n, batch, wide_vwin=1):
    """vectors per launch of the batch runners (msm_plan.h: batch_group), in launch order"""
    nb = NB[fmt]
    if nb:
        fit = (BYTE_MAXLW // nb) if nb <= 2 else MAXLW // narrow_nwin_of(pick_window_bits(fixed, n, 2, nb=nb), nb)
    elif mode == "wide":
        fit = 24 // wide_vwin
    elif mode == "tables":
        fit = MAXLW
    else:
        halves = mode == "endomorphism"
        fit = MAXLW // nwin_of(pick_window_bits(fixed, n, 2, halves), halves)
    g = max(1, min((1 << 20) // n, fit, batch))
    return [min(g, batch - first) for first in range(0, batch, g)]

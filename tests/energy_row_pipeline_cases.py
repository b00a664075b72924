"""Inputs of tests/test_gpu_energy_row_pipeline.py and of tools/record_energy_row_pipeline_fixture.py, which records the device's outputs
for them (tests/golden/energy_row_pipeline.npz).  Nothing here needs a GPU; everything is seeded.

Two things of the register-resident energy kernel are aimed at:

  * where a lane reads a lagged stream.  Lane j's window of the stream that lags by `lag` samples is samples j C - lag .. j C - lag + C - 1
    (C = len/64 + 2).  A window wholly below sample 0 reads zeros from the guard, at an address of its own; one that holds a sample >= 0
    reads its true address.  ``guard_lanes`` counts the former.  The geometries below give every stream in turn no such lane, some, and
    all but one of the lanes that hold samples; windows that end exactly at sample -1 (a lag that is a multiple of C) and exactly at
    sample 0 (one less); odd and even lags.
  * the row loop: the next row's prefetch and the pending store of the last row's result, in both places the kernel has them (behind the
    staging: 1024-sample rows; behind pass 2: 4096-sample float32 rows).  Launches of one row, of fewer rows than the launch has
    wavefronts, of exactly two and exactly three rows a wavefront, of two for some and three for others; a NaN row as a wavefront's
    first, middle and last row; a row whose pick-off time is out of range between two that are in range."""
import functools

import numpy as np

import energy_carry_cases as K

F = np.float32


def guard_lanes(C, lag):
    """lanes whose window of the stream lagging by `lag` lies wholly below sample 0: j C - lag + C <= 0"""
    return min(64, lag // C)


def sample_lanes(wf_len):
    """lanes that hold samples of the row"""
    return (wf_len - 1) // K.chunk(wf_len) + 1


def guard_geometries(wf_len):
    """(trap, targs, what the three streams do: guard lanes per stream)"""
    C = K.chunk(wf_len)
    top = (sample_lanes(wf_len) - 1) * C  # the smallest lag that leaves one lane with samples a window that is not wholly below sample 0
    geo = [("trap_filter", (5, 3)),                   # lags 5, 8, 13: no lane reads the guard (odd, even, odd)
           ("trap_filter", (C - 2, 3)),               # C - 2, C + 1, 2 C - 1: none, some, some; the third ends exactly at sample 0
           ("trap_filter", (C, C)),                   # C, 2 C, 3 C: windows that end exactly at sample -1, all even
           ("trap_filter", (C + 1, C - 2)),           # C + 1, 2 C - 1, 3 C: odd, odd, even
           ("trap_filter", (top // 2 - 4, 8)),        # third stream: all but one lane (a multiple of C), the others about half
           ("trap_filter", (wf_len // 2 - 1, 2)),     # the widest trapezoid there is: 2 rise + flat = len (odd, odd, even)
           ("asym_trap_filter", (top, 1, 1)),         # all three streams: all but one lane (even, odd, even)
           ("asym_trap_filter", (C + 1, C - 1, 7))]   # C + 1, 2 C, 2 C + 7: some lanes in each (odd, even, odd)
    if top + 3 <= wf_len:
        geo.append(("asym_trap_filter", (top + 1, 1, 1)))  # (odd, even, odd), one sample past the multiple of C
    return [(trap, targs, tuple(guard_lanes(C, lag) for lag in K.lags_of(trap, targs))) for trap, targs in geo]


def guard_cases():
    """(id, wf_len, dtype, trap, targs, modes): 1024 and 2048 samples (their guard is longer than the windows that straddle sample 0 need),
    4096 (the benchmark's code), one case of 8192"""
    out = []
    for wf_len in (1024, 2048, 4096):
        for k, (trap, targs, _lanes) in enumerate(guard_geometries(wf_len)):
            dtype = np.int16 if k in (3, 5, 7) else F
            modes = "l" if k in (2, 5, 8) else "lh"
            out.append((wf_len, dtype, trap, targs, modes))
    trap, targs, _lanes = guard_geometries(8192)[4]
    out.append((8192, F, trap, targs, "lh"))
    return [(f"{wf_len}-{np.dtype(dtype).name}-{trap}-{'-'.join(map(str, targs))}-{modes}", wf_len, dtype, trap, targs, modes)
            for wf_len, dtype, trap, targs, modes in out]


# ---- the row loop: launches of n rows on `stride` wavefronts.  1024-sample rows (the kernel's build with the prefetch behind the
# staging) and 4096-sample float32 rows (the build whose prefetch and pending store sit behind pass 2, with the fall-back at the end of
# a row that never reaches pass 2): trap_filter with odd lags among the three
LOOP_GEOMETRY = {1024: (100, 31), 4096: (625, 188)}
LOOP_TRAP = "trap_filter"
LOOP_EXTRA = 104
# wavefronts (= first-round rows) that meet the special rows; all below LOOP_EXTRA, so that they filter three rows where some do
W_NAN_MID, W_NAN_FIRST, W_RANGE, W_NAN_LAST = 90, 91, 92, 93


def loop_launches(stride):
    """(id, wf_len, rows, mode)"""
    return [("one-row", 1024, 1, "l"), ("fewer-rows-than-wavefronts", 1024, 37, "l"), ("one-row-each", 1024, stride, "h"),
            ("two-rows-each", 1024, 2 * stride, "l"), ("three-rows-each", 1024, 3 * stride, "l"), ("three-rows-each-h", 1024, 3 * stride, "h"),
            ("two-or-three-rows", 1024, 2 * stride + LOOP_EXTRA, "l"),
            ("4096-one-row", 4096, 1, "l"), ("4096-fewer-rows-than-wavefronts", 4096, 37, "l"), 
            ("4096-three-rows-each", 4096, 3 * stride, "l"), ("4096-two-or-three-rows", 4096, 2 * stride + LOOP_EXTRA, "l"),
            ("4096-two-or-three-rows-h", 4096, 2 * stride + LOOP_EXTRA, "h")]


@functools.lru_cache(maxsize=None)
def loop_rows(wf_len, n, stride):
    """K.rows with the special rows placed by wavefront: row r + stride follows row r on its wavefront"""
    wf, bl, tp, _tau = (a.copy() for a in K.rows(wf_len, F, max(n, K.N_ROWS)))
    wf, bl, tp = wf[:n], bl[:n], tp[:n]
    wf[np.isnan(wf).any(axis=1)] = 0.0  # (K.rows' own NaN row: here the NaN rows are the ones placed below)
    C = K.chunk(wf_len)

    def put(r, what):
        if r < n:
            what(r)

    def nan_row(r):
        wf[r, 7 * C + 3] = np.nan

    def in_range(r):
        tp[r] = 400.25 + (r % 5) * C

    def out_of_range(r):
        tp[r] = wf_len + 6.0

    # a NaN row between two finite rows of one wavefront (its last row where wavefronts filter two); a NaN row as a wavefront's first, a
    # finite one behind it; a time out of range between two in range; a NaN row as the third and last row behind two finite ones
    for r, what in ((W_NAN_MID, in_range), (W_NAN_MID + stride, nan_row), (W_NAN_MID + stride, in_range), (W_NAN_MID + 2 * stride, in_range),
                    (W_NAN_FIRST, nan_row), (W_NAN_FIRST, in_range), (W_NAN_FIRST + stride, in_range), (W_NAN_FIRST + 2 * stride, in_range),
                    (W_RANGE, in_range), (W_RANGE + stride, out_of_range), (W_RANGE + 2 * stride, in_range),
                    (W_NAN_LAST, in_range), (W_NAN_LAST + stride, in_range), (W_NAN_LAST + 2 * stride, nan_row), (W_NAN_LAST + 2 * stride, in_range)):
        put(r, what)
    for a in (wf, bl, tp):
        a.setflags(write=False)
    return wf, bl, tp

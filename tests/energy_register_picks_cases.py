"""Inputs of tests/test_gpu_energy_register_picks.py and of tools/record_energy_register_picks_fixture.py, which records the device's
outputs for them (tests/golden/energy_register_picks.npz).  Nothing here needs a GPU; everything is seeded.

The register-resident energy kernel picks three kinds of value at a wave-uniform run-time position out of a lane's registers: the replay's
output at the pick-off samples i0 and i0 + 1 (offset 0 .. 15 of a 16-sample capture block, or the chunk's two-sample tail), the eight
samples of a carry's capture group (element 8 * group of the lane's pass-2 output) and the prefix sum in front of that group.  The cases put
each of those positions on every value it can take at 1024-sample rows (C = 18 samples a lane: two groups and the tail, one capture block)
and on every group boundary at 4096-sample rows (C = 66: eight groups and the tail, four capture blocks)."""
import functools

import numpy as np

from energy_carry_cases import TAU, capture_point, chunk, lags_of

F = np.float32
LENGTHS = (1024, 4096)
NAN_ROW = 40  # a row with a NaN sample, good rows on both sides of it


def last_lane(wf_len):
    """the highest lane that holds a sample of the row (lane 63 holds none at the even pitch: 63 C > len; its chunk is virtual samples)"""
    return (wf_len - 1) // chunk(wf_len)


def pick_lanes(wf_len):
    return (0, 1, last_lane(wf_len) // 2, last_lane(wf_len))


@functools.lru_cache(maxsize=None)
def pick_times(wf_len):
    """t + 0.5 with i0 on every chunk offset of four lanes (lane 0, the last lane that holds samples): every offset of every capture block,
    both samples of the tail, i0 and i0 + 1 in different blocks (offset 15, 31, 47) and in different lanes (offset C - 1); then whole-number
    times on the block edges and the tail, len - 1 (no second sample) and its neighbours"""
    C = chunk(wf_len)
    t = []
    for lane in pick_lanes(wf_len):
        t += [lane * C + off + 0.5 for off in range(C) if lane * C + off + 1 <= wf_len - 1]
    for lane in pick_lanes(wf_len):
        t += [float(lane * C + off) for off in (0, 1, 15, 16, C - 3, C - 2, C - 1) if lane * C + off <= wf_len - 1]
    t += [wf_len - 1.0, wf_len - 1.5, wf_len - 1.25, wf_len - 2.0, 0.0, 0.25, 0.75]
    out = np.array(t, F)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rows(wf_len, dtype):
    """pulses on a pedestal with noise, a row per pick-off time; float32 rows: one with a NaN sample.  Shared and left unchanged."""
    dtype = np.dtype(dtype)
    tp = pick_times(wf_len)
    n = len(tp)
    rng = np.random.default_rng(91 * wf_len + ord(dtype.char))
    i = np.arange(wf_len, dtype=np.float64)[None, :]
    ped = rng.uniform(-3000, 3000, (n, 1))
    amp = rng.uniform(500, 15000, (n, 1))
    t0 = np.floor(rng.uniform(0.05, 0.9, (n, 1)) * wf_len)
    x = ped + amp * np.exp(-(i - t0) / TAU) * (i >= t0) + 5.0 * rng.standard_normal((n, wf_len))
    wf = (np.rint(x) if dtype.kind in "iu" else x).astype(dtype)
    if dtype == F:
        wf[NAN_ROW, 5 * chunk(wf_len) + 3] = np.nan
    bl = ped[:, 0].astype(F)
    tau = rng.uniform(800, 2500, n).astype(F)
    for a in (wf, bl, tau):
        a.setflags(write=False)
    return wf, bl, tp, tau


def wanted_capture_points(wf_len):
    """samples r of the source lane's chunk in front of a carry's capture point.  1024: all of 0 .. C - 1 (group 0 with nothing in front and
    every count pn 0 .. 8, group 1 with every count 1 .. 8, the tail group with its count 1, whose eight-sample capture reaches 6 past the chunk).  4096:
    group 0 in full, the first and last sample of every later group, the tail"""
    C = chunk(wf_len)
    if wf_len == 1024:
        return tuple(range(C))
    return tuple(range(10)) + tuple(r for g in range(1, (C - 2) // 8) for r in (8 * g + 1, 8 * g + 8)) + (C - 1,)


@functools.lru_cache(maxsize=None)
def carry_geometries(wf_len):
    """(rise, flat) pairs that between them put a lag's capture point on every wanted value and have every parity of (rise, flat): a greedy
    cover, the pair that reaches most of what is left, the smallest of those"""
    C = chunk(wf_len)
    want = {("r", v) for v in wanted_capture_points(wf_len)} | {("p", a, b) for a in (0, 1) for b in (0, 1)}
    have = {(rise, flat): {("r", capture_point(C, 1, 0, lag)[0]) for lag in lags_of("trap_filter", (rise, flat))} | {("p", rise & 1, flat & 1)}
            for rise in range(5, 3 * C) for flat in range(3, 2 * C)}
    out = []
    while want:
        best = max(have, key=lambda g: (len(have[g] & want), -g[0], -g[1]))
        assert have[best] & want, want
        want -= have[best]
        out.append(best)
    return tuple(out)


def cases():
    """(id, wf_len, dtype, trap, targs, modes, per-event tau)"""
    out = []
    for wf_len in LENGTHS:
        for k, g in enumerate(carry_geometries(wf_len)):
            out.append((wf_len, F, "trap_filter", g, "nfclh" if k == 0 else "l", False))
    g = carry_geometries(1024)
    rise, flat = g[0]
    out.append((1024, F, "asym_trap_filter", (rise, flat, rise + 1), "l", False))  # third lag's parity not the sum of the other two's
    out.append((1024, F, "trap_norm", g[1], "l", False))
    out.append((4096, F, "trap_norm", carry_geometries(4096)[1], "h", False))
    out.append((1024, np.int16, "trap_filter", g[2], "l", False))
    out.append((1024, F, "trap_filter", g[3], "l", True))
    out.append((4096, F, "trap_filter", (625, 188), "lh", False))  # the benchmark's geometry
    named = []
    for wf_len, dtype, trap, targs, modes, per_event in out:
        cid = f"{wf_len}-{np.dtype(dtype).name}-{trap}-{'-'.join(map(str, targs))}-{modes}" + ("-tau" if per_event else "")
        named.append((cid, wf_len, dtype, trap, tuple(targs), modes, per_event))
    assert len({c[0] for c in named}) == len(named)
    return named

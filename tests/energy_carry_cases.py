"""Inputs of tests/test_gpu_energy_carry_plan.py and its CPU companion, and of tools/record_energy_carry_fixture.py, which records the
device's outputs for them (tests/golden/energy_carry_plan.npz).  Nothing here needs a GPU; everything is seeded.

The register-resident energy kernel takes from the host, per lag and replay sub-chain, where the speculative carry's prefix sum ends:
r samples into the chunk of a lane below (``capture_point``), split into the side-array element in front of an 8-sample group, the
group's address and the count pn of its samples (``split``).  The cases put r on every value at which that split changes form."""
import functools

import numpy as np

F = np.float32
TAU = 1716.28
LENGTHS = (1024, 2048, 4096, 8192)
N_ROWS = 200  # (a wavefront per row: the rows of a case differ in their pick-off position and their samples, not in the code they run)


def chunk(wf_len):
    return wf_len // 64 + 2


def lags_of(trap, targs):
    rise, flat = targs[0], targs[1]
    return (rise, rise + flat, rise + flat + (targs[2] if trap == "asym_trap_filter" else rise))


def capture_point(C, S, s, lag):
    """samples of the source lane's chunk in front of the capture point of sub-chain s, and that lane's distance: the lagged window of
    sub-chain s of lane j starts at sample j C + s CS - lag of the row = sample r of lane j - shift"""
    CS = (C - 2) // S
    pos = s * CS - lag
    return pos % C, (pos % C - pos) // C


def split(r):
    """(group offset in the chunk, side-array element or -1, pn): by brute force over the chunk's samples"""
    if r == 0:
        return 0, -1, 0
    g = (r - 1) // 8  # the group that holds sample r - 1 (the last one: the two-sample tail)
    return 8 * g, g - 1, r - 8 * g


def edge_points(C):
    return (0, 1, 8, 9, C - 2, C - 1)


@functools.lru_cache(maxsize=None)
def carry_geometries(wf_len):
    """(rise, flat) pairs with a first lag below C that between them put a capture point on every edge value and have every parity of
    (rise, flat); then one whose lags leave most lanes' windows wholly below sample 0"""
    C = chunk(wf_len)
    want = {("r", v) for v in edge_points(C)} | {("p", a, b) for a in (0, 1) for b in (0, 1)}
    have = {(rise, flat): {("r", capture_point(C, 1, 0, lag)[0]) for lag in lags_of("trap_filter", (rise, flat))} | {("p", rise & 1, flat & 1)}
            for rise in range(5, C) for flat in range(3, 2 * C)}
    out = []
    while want:  # greedy cover: the pair that reaches most of what is left, the first of those
        best = max(have, key=lambda g: (len(have[g] & want), -g[0], -g[1]))
        assert have[best] & want, want
        want -= have[best]
        out.append(best)
    return tuple(out) + ((int(0.45 * wf_len) | 1, 6),)


def pick_times(n, wf_len, rng):
    """every position the pick-off set-up and the tail treat differently, each as a whole number and between two samples; NaN; random ones"""
    C = chunk(wf_len)
    last = ((wf_len - 1) // C) * C
    fixed = [0.0, 0.25, 0.5, 1.0, wf_len - 1.0, wf_len - 1.5, wf_len - 2.0, wf_len - 1.25, -0.001, -1.0, wf_len - 1 + 0.001, wf_len + 2.0, np.nan]
    for base in (0, C, 5 * C, last - C):  # i0 at chunk offsets C - 3, C - 2, C - 1 and 0 of the next lane
        for off in (C - 3, C - 2, C - 1, C):
            fixed += [base + off, base + off + 0.5, base + off + 0.75]
    fixed += [15.0, 15.5, 16.0, 16.5, 31.5, 32.25]  # capture blocks of 16 samples
    tp = np.empty(n, F)
    assert len(fixed) < n
    tp[:len(fixed)] = fixed
    r = rng.uniform(0, wf_len - 1, n - len(fixed))
    r[::3] = np.floor(r[::3])
    tp[len(fixed):] = r
    return tp


NAN_ROW, ZERO_ROW, FLAT_ROW = 80, 81, 82


@functools.lru_cache(maxsize=None)
def rows(wf_len, dtype, n=N_ROWS):
    """pulses on a pedestal with noise.  float32 rows: one with a NaN sample, one of zeros with a -0.0 among them (baseline 0: the
    sign of a zero prefix sum is then visible in nothing but the bits), one constant.  Shared and left unchanged."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(77 * wf_len + ord(dtype.char))
    i = np.arange(wf_len, dtype=np.float64)[None, :]
    ped = rng.uniform(-3000, 3000, (n, 1)) + (20000 if dtype == np.uint16 else 0)
    amp = rng.uniform(500, 15000, (n, 1))
    t0 = np.floor(rng.uniform(0.05, 0.9, (n, 1)) * wf_len)
    x = ped + amp * np.exp(-(i - t0) / TAU) * (i >= t0) + 5.0 * rng.standard_normal((n, wf_len))
    x[FLAT_ROW] = ped[FLAT_ROW]
    wf = (np.rint(x) if dtype.kind in "iu" else x).astype(dtype)
    bl = ped[:, 0].astype(F)
    if dtype == F:
        wf[NAN_ROW, 3 * chunk(wf_len) + 9] = np.nan
        wf[ZERO_ROW] = 0.0
        wf[ZERO_ROW, ::7] = -0.0
        bl[ZERO_ROW] = 0.0
    tp = pick_times(n, wf_len, rng)
    tau = rng.uniform(800, 2500, n).astype(F)
    for a in (wf, bl, tp, tau):
        a.setflags(write=False)
    return wf, bl, tp, tau


def cases():
    """(id, wf_len, dtype, trap, targs, modes, per-event tau, replay sub-chains)"""
    out = []
    for wf_len in LENGTHS:
        for k, (rise, flat) in enumerate(carry_geometries(wf_len)):
            out.append((wf_len, F, "trap_filter", (rise, flat), "lh" if k == 0 else "l", False, 1))
    C = chunk(1024)
    g = carry_geometries(1024)
    out.append((1024, F, "trap_filter", g[0], "nfci", False, 1))  # every two-point mode ('i': whole-number times only, see the test)
    out.append((4096, F, "trap_filter", (625, 188), "nfclhi", False, 1))  # the benchmark's geometry, every mode
    for trap, targs in (("trap_norm", g[0]), ("trap_norm", g[1]), ("asym_trap_filter", g[0] + (C + 1,)), ("asym_trap_filter", g[1] + (2 * C,))):
        out.append((1024, F, trap, targs, "lh", False, 1))
    for dtype in (np.int16, np.uint16):
        out.append((1024, dtype, "trap_filter", g[1], "lh", False, 1))
        out.append((2048, dtype, "trap_norm", carry_geometries(2048)[0], "l", False, 1))
    out.append((1024, F, "trap_filter", g[1], "ln", True, 1))
    out.append((2048, np.int16, "asym_trap_filter", carry_geometries(2048)[1] + (40,), "l", True, 1))
    for wf_len in (1024, 4096):  # two replay sub-chains: twice the captures, the second sub-chain's from the middle of the chunk
        for rise, flat in carry_geometries(wf_len)[:2]:
            out.append((wf_len, F, "trap_filter", (rise, flat), "lh", False, 2))
    named = []
    for wf_len, dtype, trap, targs, modes, per_event, S in out:
        cid = f"{wf_len}-{np.dtype(dtype).name}-{trap}-{'-'.join(map(str, targs))}-{modes}" + ("-tau" if per_event else "") + (f"-S{S}" if S != 1 else "")
        named.append((cid, wf_len, dtype, trap, tuple(targs), modes, per_event, S))
    assert len({c[0] for c in named}) == len(named)
    return named


def times_for(mode, tp):
    """mode 'i' raises for a time between two samples: its launches get the whole-number times only (the test of the error has its own)"""
    if mode != "i":
        return tp
    t = np.where(np.isnan(tp), tp, np.floor(tp)).astype(F)
    t.setflags(write=False)
    return t

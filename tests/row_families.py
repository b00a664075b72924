"""Seeded waveform families for the parity tests: the shapes of data a digitiser or a simulation hands over beside the one pulse the
suite's `_synth` helpers draw.  Pure NumPy, no device code.

A family is a function of (length, dtype, rows, rng) that returns the samples before rounding, the true pedestal and the true onset of
every row (NaN where a row has no pulse).  `family()` rounds and clips them into the dtype; `interleaved()` and `sorted_runs()` lay
several families out as one batch.

Common settings: decay constant TAU = 1716.25 samples (the recipes' pole-zero constant), Gaussian noise of sigma 5, a step pulse
A exp(-(i - t0) / TAU) for i >= t0 with its onset at 45-55 % of the row (what the suite's pulses are).  Integer rows are rounded and
clipped to the dtype's range; float32 rows hold the same values unrounded, clipped to the range of an unsigned 16-bit digitiser."""
from dataclasses import dataclass

import numpy as np

TAU = 1716.25
SIGMA = 5.0
FAMILIES = ("control", "noise_only", "noise_free", "constant", "saturated", "full_scale", "negative", "pileup", "tail", "early", "late",
            "tau_short", "tau_long", "slow_rise", "tiny")
# families whose rows hold a pulse the filters see whole: an onset mid-row and an amplitude far above the noise
PULSE_FAMILIES = ("control", "noise_free", "saturated", "full_scale", "negative", "pileup", "tail", "tau_short", "tau_long", "slow_rise")


@dataclass
class Batch:
    rows: np.ndarray       # (n_rows, n) of the dtype asked for
    family: np.ndarray     # (n_rows,) family label of each row
    pedestal: np.ndarray   # (n_rows,) float32: the true pedestal (what a baseline column holds)
    onset: np.ndarray      # (n_rows,) float64: the first sample of the (first) pulse, NaN where there is none

    def __len__(self):
        return len(self.rows)

    def of(self, name):
        return self.family == name

    def take(self, index):
        return Batch(self.rows[index], self.family[index], self.pedestal[index], self.onset[index])


def sample_range(dtype):
    """(lowest, highest) sample value of a row of this dtype; float32 rows stand for an unsigned 16-bit digitiser"""
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return float(info.min), float(info.max)
    return 0.0, 65535.0


def _pedestal(rng, rows, dtype):
    # (as the suite's helpers place it: around zero on signed rows, 9000 .. 11000 otherwise)
    return rng.uniform(-3000, 3000, (rows, 1)) if np.dtype(dtype).kind == "i" else rng.uniform(9000, 11000, (rows, 1))


def _mid_onset(rng, rows, n):
    return np.floor(rng.uniform(0.45, 0.55, (rows, 1)) * n)


def _pulse(n, t0, amp, tau=TAU, rise=0.0, c=0.0):
    """amp * edge * exp(-(i - t0 - rise) / tau), then the decay; t0 may lie before the row.  The edge is a step at t0 (the suite's pulse), a
    linear ramp over `rise` samples, or -- c > 0, the charge collection of a real detector as the whole-recipe tests draw it -- a logistic
    step of width c samples around t0."""
    i = np.arange(n, dtype=np.float64)[None, :]
    d = i - t0
    if rise > 0:
        edge = np.clip(d / rise, 0.0, 1.0)
    elif c > 0:
        edge = 1.0 / (1.0 + np.exp(np.clip(-d / c, -60, 60)))
    else:
        edge = (d >= 0).astype(np.float64)
    return amp * edge * np.exp(-np.clip(d - rise, 0.0, None) / tau)


def _noise(rng, rows, n):
    return SIGMA * rng.standard_normal((rows, n))


def _control(n, dtype, rows, rng, c=0.0, amp=(500, 15000), tau=TAU, rise=0.0, noise=True, sign=1.0):
    B = _pedestal(rng, rows, dtype)
    t0 = _mid_onset(rng, rows, n)
    A = rng.uniform(*amp, (rows, 1))
    x = B + sign * _pulse(n, t0, A, tau, rise, c)
    eps = _noise(rng, rows, n)  # (drawn either way: a noise-free row is the same pulse as the noisy one of its seed)
    return x + (eps if noise else 0.0), B, t0


def _noise_only(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    return B + _noise(rng, rows, n), B, np.full((rows, 1), np.nan)


def _constant(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    if np.dtype(dtype).kind in "iu":
        B = np.rint(B)
    B = B.astype(np.float32).astype(np.float64)  # (the pedestal a float32 baseline column can hold: row - baseline == 0 exactly)
    return np.repeat(B, n, axis=1), B, np.full((rows, 1), np.nan)


def _saturated(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = _mid_onset(rng, rows, n)
    A = rng.uniform(2.0, 3.0, (rows, 1)) * (sample_range(dtype)[1] - B)
    return B + _pulse(n, t0, A, c=c) + _noise(rng, rows, n), B, t0


def _full_scale(n, dtype, rows, rng, c=0.0):
    lo, hi = sample_range(dtype)
    # an integer pedestal 9000 .. 11000 above the bottom of the range, whatever the dtype: the headroom of a 16-bit digitiser
    B = np.rint(lo + rng.uniform(9000, 11000, (rows, 1)))
    t0 = _mid_onset(rng, rows, n)
    A = rng.uniform(0.80, 0.98, (rows, 1)) * (hi - B)
    return np.rint(B + _pulse(n, t0, A, c=c) + _noise(rng, rows, n)), B, t0


def _negative(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = _mid_onset(rng, rows, n)
    A = np.minimum(rng.uniform(500, 15000, (rows, 1)), 0.8 * (B - sample_range(dtype)[0]))  # (no clipping at the bottom)
    return B - _pulse(n, t0, A, c=c) + _noise(rng, rows, n), B, t0


def _pileup(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = _mid_onset(rng, rows, n)
    t1 = t0 + np.floor(rng.uniform(40, min(1500, 0.4 * n), (rows, 1)))  # (inside the row whatever its length)
    x = B + _pulse(n, t0, rng.uniform(500, 12000, (rows, 1)), c=c) + _pulse(n, t1, rng.uniform(500, 12000, (rows, 1)), c=c)
    return x + _noise(rng, rows, n), B, t0


def _tail(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = _mid_onset(rng, rows, n)
    before = -np.floor(rng.uniform(200, 3000, (rows, 1)))
    x = B + _pulse(n, before, rng.uniform(500, 12000, (rows, 1)), c=c) + _pulse(n, t0, rng.uniform(500, 12000, (rows, 1)), c=c)
    return x + _noise(rng, rows, n), B, t0


def _early(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = np.floor(rng.uniform(0, 8, (rows, 1)))
    return B + _pulse(n, t0, rng.uniform(500, 15000, (rows, 1)), c=c) + _noise(rng, rows, n), B, t0


def _late(n, dtype, rows, rng, c=0.0):
    B = _pedestal(rng, rows, dtype)
    t0 = n - np.floor(rng.uniform(2, 151, (rows, 1)))
    return B + _pulse(n, t0, rng.uniform(500, 15000, (rows, 1)), c=c) + _noise(rng, rows, n), B, t0


_MAKERS = {
    "control": _control,
    "noise_only": _noise_only,
    "noise_free": lambda n, dt, r, rng, c=0.0: _control(n, dt, r, rng, c, noise=False),
    "constant": _constant,
    "saturated": _saturated,
    "full_scale": _full_scale,
    "negative": _negative,
    "pileup": _pileup,
    "tail": _tail,
    "early": _early,
    "late": _late,
    "tau_short": lambda n, dt, r, rng, c=0.0: _control(n, dt, r, rng, c, tau=0.5 * TAU),
    "tau_long": lambda n, dt, r, rng, c=0.0: _control(n, dt, r, rng, c, tau=2.0 * TAU),
    "slow_rise": lambda n, dt, r, rng, c=0.0: _control(n, dt, r, rng, c, rise=60.0),
    "tiny": lambda n, dt, r, rng, c=0.0: _control(n, dt, r, rng, c, amp=(5, 30)),
}
assert tuple(_MAKERS) == FAMILIES


def family(name, n, dtype, rows, seed=0, collect=0.0):
    """`rows` rows of one family: Batch.  collect: width in samples of every pulse's edge (0: the suite's step)"""
    rng = np.random.default_rng([int(seed), FAMILIES.index(name), int(n)])
    x, B, t0 = _MAKERS[name](int(n), dtype, int(rows), rng, float(collect))
    lo, hi = sample_range(dtype)
    if np.dtype(dtype).kind in "iu":
        x = np.rint(x)
    x = np.clip(x, lo, hi).astype(dtype)
    return Batch(x, np.full(rows, name), B[:, 0].astype(np.float32), t0[:, 0].astype(np.float64))


def _concat(parts):
    return Batch(np.concatenate([p.rows for p in parts]), np.concatenate([p.family for p in parts]),
                 np.concatenate([p.pedestal for p in parts]), np.concatenate([p.onset for p in parts]))


def interleaved(n, dtype, per_family=8, extra=11, seed=0, families=FAMILIES, collect=0.0):
    """`per_family` rows of every family and `extra` more of the first ones, in a seeded permutation: with the defaults 15 x 8 + 11 = 131
    rows, off any multiple of 64, so that every wavefront of a lane-per-row kernel holds mixed families"""
    counts = [per_family + (1 if k < extra else 0) for k in range(len(families))]
    b = _concat([family(f, n, dtype, k, seed, collect) for f, k in zip(families, counts)])
    return b.take(np.random.default_rng([int(seed), 99]).permutation(len(b)))


def sorted_runs(n, dtype, run=64, seed=0, families=FAMILIES, collect=0.0):
    """every family as a contiguous run of `run` rows: whole wavefronts of one family"""
    return _concat([family(f, n, dtype, run, seed, collect) for f in families])

"""The matrix-core FIR kernels (dsp_fir_f16.hip, dsp_fir_mfma.hip) at every tile and alignment edge: the kernels' geometry restated as
small pure functions, the cases made from them by rule, and two families of rows and taps for every case -- for
tests/test_gpu_fir_tiles.py (the device) and tests/test_fir_tile_cases_cpu.py (is the list what it claims? -- the planner and NumPy alone).
Nothing here needs a GPU; every row and tap comes from a seed.

The kept-output ("store") form of ``dsp_fir_f16_kernel`` computes a 320-column tile of ``convolve_wf`` from the window of the rows that
starts at sample ``c0 - dshift``, rounded down to a multiple of 8; the remainder ``e`` moves into the tap index and decides the tap-copy
shift, ``t_off``, the ``tap_slot[e]`` row, the masked first and last stages and the column-tile skip test.  ``launch_f16`` picks the
instantiation with resident taps (RES) where the longest window's 16 tap copies fit the two window buffers.  The amax form ('v' followed
by numpy.amax) has one window from sample 0 whose length comes from the longest kernel of the launch, and a pipelined prefix of its stages.
The float32 forms (DSPEED_HIP_FIR_F32=1) round the window start to 4 samples and stage 32 samples at a time.

The exact family makes an off-by-one anywhere an inequality of integers: taps are distinct integers of alternating sign with the largest at
both ends, rows are small integers, every operand fits float16's significand after its power-of-two scale (so both ``lo`` planes are zero)
and every partial sum is an integer below 2^24 -- the expectation is the int64 convolution, compared with ``np.array_equal``.  The fraction
family fills the ``lo`` planes (a wrong ``lo`` index passes the exact family): uniform taps in +-[0.5, 1] and rows with more than 11
significant bits, against the float64 convolution at 1e-6 of the row's filtered peak."""
import functools

import numpy as np

import oracle

M = "dspeed.processors"
TOL = 1e-6  # of the row's filtered peak (test_gpu_fir_mfma.py: north_star)
TAPS_FILE = "mem:fir_tile_taps"  # (a recipe reads its taps with loadlh5(TAPS_FILE, '<family>/<m>'))
ROW_TYPES = {"f32": np.float32, "i16": np.int16, "u16": np.uint16}
PEDESTAL = 1000
U16_MID = 30550
MODES = {"v": "valid", "s": "same", "f": "full"}

# ------------------------------------------------------------------------------------------------------------------------------------
# geometry of the float16 forms (dsp_fir_f16.hip, dsp_kernels.h)
# ------------------------------------------------------------------------------------------------------------------------------------
BM, BK, BN = 64, 64, 320  # dsp_kernels.h:46-52 (F16_BM, F16_BK), dsp_fir_f16.hip:39
TB = 336                  # dsp_kernels.h:56
TWIN = TB + BK            # dsp_kernels.h:57
TPITCH = ((TWIN + 8 + 15 * 8 + 127) // 128) * 128  # dsp_kernels.h:62
RES_HALFS = 2 * 16 * TPITCH                        # dsp_fir_f16.hip:185
KFLUSH, KFLUSH_STORE = 256, 128                    # dsp_fir_f16.hip:55-58


def _up(x, to):
    return ((x + to - 1) // to) * to


def res_pitch(kt):
    """dsp_fir_f16.hip:186"""
    return ((kt + TB + 8 + 15 * 8 + 127) // 128) * 128


def out_len(mode, m, n):
    """dsp_plan.cpp:781"""
    return {"v": n - m + 1, "s": n, "f": n + m - 1}[mode]


def dshift(mode, m):
    """dsp_plan.cpp:784"""
    return {"v": 0, "s": m // 2, "f": m - 1}[mode]


def parts(P):
    """column tiles of a kept output (dsp_fir_f16.hip:634)"""
    return (P + BN - 1) // BN


def tile_cols(P, part):
    """dsp_fir_f16.hip:218"""
    return min(P - part * BN, BN)


def align_e(mode, m, part=0):
    """dsp_fir_f16.hip:215-217: the same in every tile, 320 being a multiple of 8"""
    return (part * BN - dshift(mode, m)) & 7


def store_kt(mode, m, P, part, e=None):
    """dsp_fir_f16.hip:219 (STORE)"""
    e = align_e(mode, m, part) if e is None else e
    return _up(tile_cols(P, part) + m - 1 + e, BK)


def store_n_stage(mode, m, P, part):
    """dsp_fir_f16.hip:388"""
    return store_kt(mode, m, P, part) // BK


def kt_max(m, P):
    """dsp_fir_f16.hip:637"""
    return _up(min(P, BN) + m - 1 + 7, BK)


def resident(m, P):
    """dsp_fir_f16.hip:639 (DSPEED_HIP_FIR_NO_RESIDENT_TAPS unset)"""
    return 16 * res_pitch(kt_max(m, P)) <= RES_HALFS


def grid_decode(block, n_parts):
    """dsp_fir_f16.hip:206-208 -> (part, row block)"""
    xcd, slot = block & 7, block >> 3
    return slot % n_parts, (slot // n_parts) * 8 + xcd


def grid_blocks(n_rows, n_parts):
    """dsp_fir_f16.hip:632-635"""
    rblocks = (n_rows + BM - 1) // BM
    return 8 * ((rblocks + 7) // 8) * n_parts


def tile_skipped(m, e, wn, tn, kb):
    """dsp_fir_f16.hip:437-438: column tile (wn, tn) meets no tap in window samples kb .. kb + 31"""
    c_lo = 16 * (wn + 4 * tn) + e
    return not (kb + 31 >= c_lo and kb <= c_lo + 14 + m)


def amax_kend(n, ms):
    """dsp_plan.cpp:724-725"""
    return _up(min(n, 319 + max(ms)), 32)


def amax_n_stage(n, ms):
    """dsp_fir_f16.hip:219 (!STORE), 388"""
    return _up(amax_kend(n, ms), BK) // BK


def amax_n_pipe(n, ms):
    """dsp_fir_f16.hip:476, 492-499 (ks = 0)"""
    run = KFLUSH // BK
    last = min(amax_n_stage(n, ms) - 3, n // BK - 2)
    return ((last + 1) // run) * run if last >= 0 else 0


# ---- the float32 forms (dsp_fir_mfma.hip)
F32_BK, KCHUNK, SCHUNK = 32, 128, 64  # dsp_fir_mfma.hip:37, 271


def align_e32(mode, m, part=0):
    """dsp_fir_mfma.hip:284-285"""
    return (part * BN - dshift(mode, m)) & 3


def store_kt32(mode, m, P, part):
    """dsp_fir_mfma.hip:287"""
    return _up(tile_cols(P, part) + m - 1 + align_e32(mode, m, part), F32_BK)


# ---- the planner's admission (dsp_plan.cpp)
def takes_f16(tag, n, lo, row_len):
    """choose_fir_f16, dsp_plan.cpp:1917-1928 (DSPEED_HIP_FIR_F32 unset)"""
    es = 4 if tag == "f32" else 2
    return (row_len * es) % 16 == 0 and (lo * es) % 16 == 0 and (n % 8 == 0 or lo + _up(n, 8) <= row_len)


def takes_matrix_core(tag, lo, row_len):
    """match_fir_shape / match_fir_store_shape, dsp_plan.cpp:677-678, 752-753: 4 samples per staging load"""
    es, align = (4, 16) if tag == "f32" else (2, 8)
    return (row_len * es) % align == 0 and (lo * es) % align == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
#: (row type, baseline) in turn over the cases.  The first five can hold a NaN and an infinity (float32 rows themselves, integer rows
#: through a baseline column): the sweeps, where a class has one case, turn over these; the other three go to cases whose classes have
#: several.  No uint16 rows without a baseline: the rows of the exact family are signed
COMBOS = (("f32", "none"), ("i16", "col"), ("f32", "col"), ("u16", "col"), ("f32", "const"), ("i16", "none"), ("u16", "const"), ("i16", "const"))
NF = 5
ROWS = 70  # (more than one block of 64 rows)


class Case:
    """``form``: 'store' (convolve_wf kept) or 'amax' ('v' + numpy.amax); ``ms``: the kernels' lengths (one for 'store'); ``n``: samples of
    the slice ``waveform[lo : lo + n]`` of rows of ``row_len`` samples; ``why``: the class the case is in the list for (it is in
    ``classes(case)``)"""

    def __init__(self, form, why, mode, ms, n, rows, tag, bl, lo=0, row_len=None):
        self.form, self.why, self.mode, self.ms, self.n, self.rows, self.tag, self.bl, self.lo = form, why, mode, tuple(ms), n, rows, tag, bl, lo
        self.row_len = lo + n if row_len is None else row_len
        self.m = self.ms[0]
        self.whole = lo == 0 and self.row_len == n
        self.P = out_len(mode, self.m, n) if form == "store" else None
        self.ps = tuple(n - m + 1 for m in self.ms)
        self.id = f"{form}-{mode}-{'+'.join(map(str, self.ms))}taps-{n}of{self.row_len}at{lo}-{rows}rows-{tag}-bl_{bl}"
        assert all(64 <= m <= n for m in self.ms) and self.row_len >= lo + n and not (tag == "u16" and bl == "none")

    # geometry of the kept output
    @property
    def e(self):
        return align_e(self.mode, self.m)

    @property
    def res(self):
        return resident(self.m, self.P)

    @property
    def n_stages(self):
        """of every tile (store) or of the launch (amax)"""
        if self.form == "amax":
            return (amax_n_stage(self.n, self.ms),)
        return tuple(store_n_stage(self.mode, self.m, self.P, t) for t in range(parts(self.P)))

    @property
    def nonfinite(self):
        """rows 4 and 5 hold a NaN / an infinity: float32 rows carry them themselves, integer rows through a baseline column"""
        return self.rows >= 8 and (self.tag == "f32" or self.bl == "col")

    def kernel(self, f32_form):
        """the kernel the planner is expected to choose"""
        if self.form == "amax":
            return "dsp_fir_mfma_kernel" if f32_form else "dsp_fir_f16_kernel"
        return "dsp_fir_f16_kernel" if not f32_form and takes_f16(self.tag, self.n, self.lo, self.row_len) else "dsp_fir_store_kernel"


def classes(c):
    """the names of the classes the case belongs to, from its geometry"""
    out = [f"type {c.tag}", f"baseline {c.bl}"]
    if c.n % 8:
        out.append(f"{c.form} slice n%8={c.n % 8}")
    if c.form == "amax":
        out += [f"amax p={p}" for p in c.ps]
        out += [f"amax {len(c.ms)} kernel{'s' if len(c.ms) > 1 else ''}", f"amax n_stage={c.n_stages[0]} n_pipe={amax_n_pipe(c.n, c.ms)}"]
        out += ["amax m=64"] if 64 in c.ms else []
        out += ["amax longest m"] if c.n in c.ms else []
        out += ["amax kend = n rounded up to 32"] if amax_kend(c.n, c.ms) == _up(c.n, 32) and c.n % 32 and c.n == 319 + min(c.ms) else []
        return tuple(out)
    if not takes_f16(c.tag, c.n, c.lo, c.row_len):
        return tuple(out + ["unaligned offset"])  # (the float16 form never sees it)
    e, res = c.e, "resident" if c.res else "non-resident"
    out += [f"e={e} {res}", f"mode {c.mode} e={e}", f"mode {c.mode} {res}", f"type {c.tag} {res}", f"rows {c.rows}", f"e32={align_e32(c.mode, c.m)}"]
    out += [f"type {c.tag} odd e"] if e & 1 else []
    last = tile_cols(c.P, parts(c.P) - 1)
    out.append(f"single tile P={'320' if c.P == BN else '<320'}" if parts(c.P) == 1 else f"last tile {last} columns")
    out += [f"n_stage {s if s <= 3 else ('odd' if s & 1 else 'even') + ' above 3'}" for s in sorted(set(c.n_stages))]
    if any(store_kt(c.mode, c.m, c.P, t) > store_kt(c.mode, c.m, c.P, t, e=0) for t in range(parts(c.P))):
        out.append("last stage from the alignment alone")
    if c.m == 64 and c.P >= BN and skip_is_mixed(c):
        out.append("m=64 full tile: skip test mixed")
    if c.rows > 8 * BM and parts(c.P) >= 2:
        out.append("second group of row blocks with parts >= 2")
    return tuple(out)


def skip_is_mixed(c):
    """some (wavefront, column tile) pairs of the first tile skip a 32-sample group that others take, in one and the same stage"""
    for st in range(c.n_stages[0]):
        seen = {tile_skipped(c.m, c.e, wn, tn, st * BK + 32 * g) for g in range(BK // 32) for wn in range(4) for tn in range(5)}
        if seen == {True, False}:
            return True
    return False


def _store(why, mode, m, n, i, rows=ROWS, lo=0, row_len=None, combo=None):
    tag, bl = COMBOS[i] if combo is None else combo
    return Case("store", why, mode, (m,), n, rows, tag, bl, lo, row_len)


def _slice_len(lo, n):
    """the shortest row the float16 form takes the slice from: its last 8-sample vector ends inside the row (choose_fir_f16's second clause)"""
    return lo + _up(n, 8)


@functools.lru_cache(maxsize=None)
def store_cases():
    out = []
    # every e with resident taps: two tiles, a partial last one
    for i, m in enumerate(range(64, 72)):
        out.append(_store(f"e={align_e('f', m)} resident", "f", m, 328, i % NF))
    # ... and with the taps fetched stage by stage (m >= 443 for a full tile).  A FIR needs a slice as long as its taps: 464 samples for 457
    for i, m in enumerate(range(450, 458)):
        out.append(_store(f"e={align_e('f', m)} non-resident", "f", m, max(456, _up(m, 8)), (i + 3) % NF))
    # e = 3 and 7 through 'same'; 'valid' (e = 0) at both RES settings
    out.append(_store("mode s e=3", "s", 138, 328, 4))
    out.append(_store("mode s e=7", "s", 130, 328, 3))
    out.append(_store("mode v resident", "v", 64, 328, 7))
    out.append(_store("mode v non-resident", "v", 450, 776, 3))
    # widths of the last tile
    for i, (m, n) in enumerate(((66, 256), (64, 272), (65, 272), (66, 272), (64, 576), (65, 576))):
        out.append(_store(f"last tile {tile_cols(out_len('f', m, n), parts(out_len('f', m, n)) - 1)} columns", "f", m, n, (i + 1) % NF))
    # 64 taps under a full tile: the band covers a part of the tile's columns in every stage (integer rows without a pedestal)
    out.append(_store("m=64 full tile: skip test mixed", "f", 64, 336, 5))
    out.append(_store("single tile P=<320", "s", 70, 312, 6))
    # stage counts: the prefetch test st + 2 < n_stage and the parity of a run of two
    for i, (n, s) in enumerate(((64, "1"), (80, "2"), (136, "3"), (304, "odd above 3"))):
        out.append(_store(f"n_stage {s}", "v", 64, n, (4, 0, 1, 3)[i]))
    # A tile whose last stage exists because of e alone: cols + m - 1 <= 64 k < cols + m - 1 + e.  No FULL tile can be one: 320 is a multiple
    # of 64, 'valid' has e = 0, 'full' makes m - 1 + e a multiple of 8 (the next one: no multiple of 64 between), and 'same' has
    # e = -((r + 1) // 2) mod 8 for m - 1 = 64 j + r, which stays below 64 - r for every r.  The issue's m = 126 in mode 'f' (e = 3) with a
    # last tile of 3 columns: 3 + 125 = 128, with e 131
    out.append(_store("last stage from the alignment alone", "f", 126, 198, 0, lo=8, row_len=_slice_len(8, 198)))
    # slices of a longer row whose length is no multiple of 8: the `live < 8` select and the tail loop of the rows kernel
    out.append(_store("store slice n%8=1", "s", 64, 329, 2, lo=8, row_len=_slice_len(8, 329)))
    out.append(_store("store slice n%8=4", "f", 70, 332, 3, lo=8, row_len=_slice_len(8, 332)))
    out.append(_store("store slice n%8=7", "s", 451, 463, 1, lo=8, row_len=_slice_len(8, 463)))
    # an offset of 8 bytes: the float32 form's kernel, whatever DSPEED_HIP_FIR_F32 says
    out.append(_store("unaligned offset", "s", 64, 328, 0, lo=4, row_len=336, combo=("i16", "none")))
    out.append(_store("unaligned offset", "f", 66, 328, 0, lo=4, row_len=336, combo=("u16", "col")))
    # row counts; 577 rows are ten row blocks, the last of one row: the second group of eight has two live XCD slots, with two column tiles each
    for i, (rows, m, n) in enumerate(((1, 64, 64), (63, 67, 328), (64, 69, 328), (65, 70, 328))):
        out.append(_store(f"rows {rows}", "s" if rows == 1 else "f", m, n, (0, 1, 3, 2)[i], rows=rows))
    out.append(_store("second group of row blocks with parts >= 2", "f", 66, 328, 2, rows=577))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def amax_cases():
    def case(why, ms, n, i, lo=0):
        tag, bl = COMBOS[i]
        return Case("amax", why, "v", ms, n, ROWS, tag, bl, lo, lo + _up(n, 32))  # (the float32 form stages whole groups of 32 samples)

    return (case("amax n_stage=1 n_pipe=0", (64,), 64, 0),
            case("amax n_stage=2 n_pipe=0", (64,), 79, 1, lo=8),
            case("amax 3 kernels", (64, 66, 80), 80, 3),
            case("amax n_stage=3 n_pipe=0", (168, 64), 182, 2, lo=8),
            case("amax n_stage=5 n_pipe=0", (64, 320), 320, 4),
            case("amax n_stage=6 n_pipe=4", (64,), 382, 6),
            case("amax kend = n rounded up to 32", (64, 383), 383, 0, lo=8),
            case("amax n_stage=7 n_pipe=4", (129, 130), 448, 1))


def cases():
    return store_cases() + amax_cases()


#: every class the list must hit (test_fir_tile_cases_cpu.py holds the list against it)
STORE_CLASSES = tuple([f"e={e} {r}" for r in ("resident", "non-resident") for e in range(8)] + ["mode s e=3", "mode s e=7", "mode v resident", "mode v non-resident"] +
                      [f"last tile {w} columns" for w in (1, 15, 16, 17, 319, 320)] + ["single tile P=<320", "n_stage 1", "n_stage 2", "n_stage 3",
                       "n_stage odd above 3", "last stage from the alignment alone", "m=64 full tile: skip test mixed", "store slice n%8=1",
                       "store slice n%8=4", "store slice n%8=7", "unaligned offset", "rows 1", "rows 63", "rows 64", "rows 65",
                       "second group of row blocks with parts >= 2"] + [f"type {t} {r}" for t in ROW_TYPES for r in ("resident", "non-resident", "odd e")] +
                      [f"baseline {b}" for b in ("none", "col", "const")] + [f"e32={e}" for e in range(4)])
AMAX_CLASSES = tuple([f"amax p={p}" for p in (1, 15, 16, 17, 319, 320)] + ["amax m=64", "amax longest m", "amax 1 kernel", "amax 2 kernels", "amax 3 kernels"] +
                     [f"amax n_stage={s} n_pipe={p}" for s, p in ((1, 0), (2, 0), (3, 0), (5, 0), (6, 4), (7, 4))] +
                     ["amax kend = n rounded up to 32", "amax slice n%8=7", "amax slice n%8=6"] + [f"type {t}" for t in ROW_TYPES])

#: (taps, slice length, mode) of every launch of the float16 store form in tests/test_gpu_fir_mfma.py (its slices are multiples of 8 samples
#: but 644, which the float32 form takes): test_stored_output_all_modes, ..._integer_rows_slices_and_no_baseline, the 133-tap 'same'
#: filters of the magnitude and NaN tests and ``kb`` of the staged recipe (``ka`` is piecewise constant: dsp_fir_runs_kernel)
EXISTING_ALL_MODES = ((133, 8192, 70), (64, 1000, 64), (200, 2048, 131), (700, 1024, 3), (321, 644, 65))
EXISTING_STORE_SHAPES = tuple((m, n, mode) for m, n, _ in EXISTING_ALL_MODES if n % 8 == 0 for mode in "svf") + (
    (133, 4096, "s"), (133, 2872, "s"), (133, 2048, "s"), (100, 4096, "f"))


def e_res_pairs(shapes):
    return {(align_e(mode, m), resident(m, out_len(mode, m, n))) for m, n, mode in shapes}


# ------------------------------------------------------------------------------------------------------------------------------------
# taps and rows
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def taps(family, m):
    """float32, read-only.  exact: distinct integers of alternating sign, 1 + 37 t mod 1021 in magnitude (37 t mod 1021 is distinct for
    t < 1021), the two ends the largest: 1023 and -1022.  fraction: uniform in +-[0.5, 1], seeded by m"""
    t = np.arange(m)
    if family == "exact":
        k = (-1.0) ** t * (1 + (37 * t) % 1021)
        k[0], k[m - 1] = 1023, -1022
    else:
        rng = np.random.default_rng([m, 311])
        k = rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m)
    k = k.astype(np.float32)
    k.setflags(write=False)
    return k


def baseline_const(c, family):
    """the constant a recipe's bl_subtract takes off: the pedestal, but the middle of the range under the fraction family's uint16 rows"""
    return U16_MID if family == "fraction" and c.tag == "u16" else PEDESTAL


def _taps_loader(file, path):
    if file != TAPS_FILE:
        return None
    family, m = path.split("/")
    return taps(family, int(m))


def register_taps_loader():
    from dspeed_amd import lgdo_io

    if _taps_loader not in lgdo_io.CONSTANT_LOADERS:
        lgdo_io.CONSTANT_LOADERS.append(_taps_loader)


@functools.lru_cache(maxsize=None)
def table(case_id, family):
    """{'waveform': (rows, row_len) in the case's row type[, 'baseline': float32 column]}, read-only.  Where the case can hold them
    (``nonfinite``) row 4 has a NaN in the slice's last sample and row 5 +inf in its first; samples outside the slice are seeded too.
    exact: integers in [-4, 4] above the baseline (1000 + r % 7 as a column, 1000 as a constant: the pedestal); with 8 rows or more, row 0
    is an impulse in the slice's first sample, row 1 in its last, row 2 zeros, row 3 a constant.  fraction: every row seeded (a constant
    row under taps of random sign has a filtered peak far below its products: no 1e-6 quantity in any float32 arithmetic) -- float32 rows
    uniform in [-1, 1] above the baseline, integer rows the same spread over most of their type's range, the baseline column not integer"""
    c = by_id(case_id)
    rng = np.random.default_rng([len(case_id), sum(map(ord, case_id)), int(family == "exact")])
    R, L, lo, n = c.rows, c.row_len, c.lo, c.n
    r = np.arange(R)
    if family == "exact":
        body = rng.integers(-4, 5, (R, L)).astype(np.float64)
        bl = {"none": np.zeros(R), "col": PEDESTAL + r % 7.0, "const": np.full(R, float(PEDESTAL))}[c.bl]
        special = (4.0, -3.0, 3.0)
    else:
        v = rng.uniform(-1, 1, (R, L))
        if min(c.ps) < 8:  # a handful of outputs could all cancel: half of the samples take the sign of the tap of the longest kernel they meet first
            kr = taps("fraction", max(c.ms))[::-1]
            take = rng.random((R, max(c.ms))) < 0.5
            seg = v[:, lo:lo + max(c.ms)]
            seg[take] = (np.abs(seg) * np.sign(kr))[take]
        if c.tag == "f32":
            body = v
            bl = {"none": np.zeros(R), "col": rng.uniform(0.5, 1.5, R), "const": np.full(R, float(PEDESTAL))}[c.bl]
        else:
            # (uint16 rows swing about the middle of their range, and so does their baseline: a filter with taps of random sign takes a
            # pedestal off itself, and the filtered peak would lie far below the products that make it)
            mid, amp = (0, 30000) if c.tag == "i16" else (U16_MID, 29450)
            body = np.rint(mid + amp * v)
            bl = {"none": np.zeros(R), "col": mid + rng.uniform(-100, 100, R), "const": np.full(R, float(baseline_const(c, family)))}[c.bl]
    if R >= 8 and family == "exact":
        body[0, lo:lo + n] = 0
        body[0, lo] = special[0]
        body[1, lo:lo + n] = 0
        body[1, lo + n - 1] = special[1]
        body[2, lo:lo + n] = 0
        body[3, lo:lo + n] = special[2]
    bl32 = bl.astype(np.float32)
    if c.tag == "f32":
        wf = (body + bl32[:, None].astype(np.float64)).astype(np.float32)
    else:  # the integer part of the baseline is the rows' pedestal
        wf = (body + (np.floor(bl)[:, None] if family == "exact" or (c.bl == "const" and c.tag == "i16") else 0)).astype(ROW_TYPES[c.tag])
    if c.nonfinite:
        if c.tag == "f32":
            wf[4, lo + n - 1] = np.nan
            wf[5, lo] = np.inf
        else:
            bl32[4], bl32[5] = np.nan, np.inf
    out = {"waveform": wf}
    if c.bl == "col":
        out["baseline"] = bl32
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def by_id(case_id):
    return next(c for c in cases() if c.id == case_id)


@functools.lru_cache(maxsize=None)
def filtered_input(case_id, family):
    """what the convolution reads, in float32: the slice of the rows after bl_subtract (the oracle's: a NaN anywhere in the waveform, or in
    the baseline, makes the whole row NaN)"""
    c, t = by_id(case_id), table(case_id, family)
    x = t["waveform"].astype(np.float32)
    if c.bl != "none":
        bl = t["baseline"] if c.bl == "col" else np.full(c.rows, baseline_const(c, family), dtype=np.float32)
        with np.errstate(all="ignore"):
            x, rc = oracle.bl_subtract(x, bl)
        assert rc == 0
    x = np.ascontiguousarray(x[:, c.lo:c.lo + c.n])
    x.setflags(write=False)
    return x


def finite_rows(case_id, family):
    return np.isfinite(filtered_input(case_id, family)).all(axis=1)


def convolve_rows(x, k, mode, dtype):
    """np.convolve row by row in ``dtype`` (int64: exact; float64: the reference of the fraction family)"""
    k = np.asarray(k).astype(dtype)
    return np.stack([np.convolve(row.astype(dtype), k, mode=MODES[mode]) for row in x])


@functools.lru_cache(maxsize=None)
def expect(case_id, family):
    """Per kernel of the case, (want, peak, oracle's): the convolution of the finite rows in int64 (exact) or float64 (fraction) -- zeros
    in the other rows --, the filtered peak of every row, and oracle.convolve_wf on all rows in float32 (what decides NaN and
    infinities).  The amax form's expectation is the row maximum of these (``amax_of``)"""
    c = by_id(case_id)
    x = filtered_input(case_id, family)
    fin = finite_rows(case_id, family)
    out = []
    for m in c.ms:
        k = taps(family, m)
        dtype = np.int64 if family == "exact" else np.float64
        want = np.zeros((c.rows, out_len(c.mode, m, c.n)), dtype=dtype)
        want[fin] = convolve_rows(x[fin], k, c.mode, dtype)
        with np.errstate(all="ignore"):
            conv, rc = oracle.convolve_wf(x, k, c.mode, want.shape[1])
        assert rc == 0
        peak = np.abs(want).max(axis=1).astype(np.float64)
        for a in (want, conv, peak):
            a.setflags(write=False)
        out.append((want, peak, conv))
    return tuple(out)


def amax_of(a):
    """numpy.amax along the rows: a NaN wins"""
    with np.errstate(invalid="ignore"):
        return np.max(a, axis=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# recipes and the processor call
# ------------------------------------------------------------------------------------------------------------------------------------
def recipe(c, family):
    """LOAD [bl_subtract] convolve STORE, or LOAD [bl_subtract] convolve 'v' + numpy.amax per kernel -> (recipe, outputs' names)"""
    register_taps_loader()
    procs, src = {}, "waveform"
    if c.bl != "none":
        procs["wf_bl"] = f"{M}.bl_subtract(waveform, {'baseline' if c.bl == 'col' else baseline_const(c, family)}, wf_bl)"
        src = "wf_bl"
    sl = src if c.whole else f"{src}[{c.lo}:{c.lo + c.n}]"
    names = []
    for q, m in enumerate(c.ms):
        p = out_len(c.mode, m, c.n)
        procs[f"wf_{q}"] = {"function": "convolve_wf", "module": M, "args": [sl, f"loadlh5('{TAPS_FILE}', '{family}/{m}')", f"'{c.mode}'", f"wf_{q}({p}, 'f')"]}
        if c.form == "amax":
            procs[f"max_{q}"] = {"function": "amax", "module": "numpy", "args": [f"wf_{q}", 1, f"max_{q}"]}
        names.append(f"max_{q}" if c.form == "amax" else f"wf_{q}")
    return {"outputs": names, "processors": procs}, names


def has_call(c):
    """the processor call hands over contiguous rows: the case's launch where the slice is the whole row"""
    return c.form == "store" and c.whole


def call_rows(c, family):
    """the rows of ``P.convolve_wf``: the case's own where no baseline is subtracted, else the float32 rows after the subtraction"""
    return table(c.id, family)["waveform"] if c.bl == "none" else filtered_input(c.id, family)


def call(P, c, family):
    return P.convolve_wf(call_rows(c, family), taps(family, c.m), ord(c.mode), np.empty((c.rows, c.P), dtype=np.float32))


def call_program(c, family):
    """the program behind ``call`` (dsp_gufuncs.cpp, restated as in op_length_cases.processor_program): LOAD, CONVOLVE, STORE"""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program

    p = Program()
    p.slots = [c.n, c.P]
    io_in = p.add_io("wf", L.IO_WF_IN, call_rows(c, family).dtype, c.n)
    io_k = p.add_io("taps", L.IO_TAPS, np.float32, c.m)
    p.add_op(L.OP_LOAD, dst=0, io=io_in)
    p.add_op(L.OP_CONVOLVE, dst=1, src=0, io=io_k, ip=(ord(c.mode), 0))
    p.add_op(L.OP_STORE, src=1, io=p.add_io("out", L.IO_WF_OUT, np.float32, c.P))
    return p


# ------------------------------------------------------------------------------------------------------------------------------------
# the float16 form in NumPy (test_fir_tile_cases_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
def pow2_scale(a):
    """2^(14 - floor(log2(max |a|))) per row (dsp_fir_f16.hip:83-85, 173-177): the largest magnitude lands in [2^14, 2^15)"""
    mx = np.abs(a).max(axis=-1, keepdims=True).astype(np.float32)
    e = np.where(mx > 0, np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 14.0)
    return np.exp2(14.0 - e).astype(np.float32)


def split16(a, scale):
    """hi = half(y), lo = half(y - hi) of y = a * scale (dsp_fir_f16.hip:91-95, 293-298), both as float32"""
    y = (a.astype(np.float32) * scale).astype(np.float32)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def windows(x, m, mode):
    """(rows, P, m): the samples output column c multiplies, zeros outside the slice, against the REVERSED kernel"""
    d = dshift(mode, m)
    n = x.shape[1]
    P = out_len(mode, m, n)
    pad = np.zeros((x.shape[0], d + n + max(0, P + m - 1 - d - n)), dtype=x.dtype)
    pad[:, d:d + n] = x
    return np.lib.stride_tricks.sliding_window_view(pad, m, axis=1)[:, :P]


def emulate_f16(x, k, mode, chunk, order=None):
    """The float16 form's arithmetic on float32 rows ``x``, one float32 addition per product: scale, split, three products per sample
    (lo.hi, hi.lo, hi.hi as the kernel issues them) summed in float32 over ``chunk`` taps at a time -- in the order ``order`` (a
    permutation of the taps) --, the chunks added in float64, the scales undone.  For the exact family, where no order may matter"""
    m = len(k)
    xs, ks = pow2_scale(x), pow2_scale(np.asarray(k)[None, :])[0, 0]
    xh, xl = split16(x, xs)
    kh, kl = split16(np.asarray(k)[::-1], ks)
    order = np.arange(m) if order is None else order
    wh, wl = windows(xh, m, mode)[:, :, order], windows(xl, m, mode)[:, :, order]
    kh, kl = kh[order], kl[order]
    tot = np.zeros(wh.shape[:2], dtype=np.float64)
    for a in range(0, m, chunk):
        s = slice(a, min(a + chunk, m))
        terms = np.stack([wl[:, :, s] * kh[s], wh[:, :, s] * kl[s], wh[:, :, s] * kh[s]], axis=-1).reshape(wh.shape[0], wh.shape[1], -1)
        tot += np.cumsum(terms.astype(np.float32), axis=2, dtype=np.float32)[:, :, -1].astype(np.float64)
    return tot / (xs.astype(np.float64) * float(ks))


def emulate_f16_mfma(x, k, mode, chunk, batch=32):
    """The same with the matrix instruction's granularity: v_mfma_f32_16x16x32_f16 adds 32 products (each exact) to its float32
    accumulator and rounds once, so a partial sum of ``chunk`` taps sees 3 * chunk / 32 roundings; lo.lo is dropped; float64 totals"""
    m, g = len(k), 32
    ks = pow2_scale(np.asarray(k)[None, :])[0, 0]
    kh, kl = (np.concatenate([a, np.zeros(-m % g, dtype=np.float32)]).astype(np.float64) for a in split16(np.asarray(k)[::-1], ks))
    out = []
    for r0 in range(0, len(x), batch):
        xb = x[r0:r0 + batch]
        xs = pow2_scale(xb)
        d, n, P = dshift(mode, m), xb.shape[1], out_len(mode, m, xb.shape[1])
        planes = []
        for a in split16(xb, xs):
            pad = np.zeros((len(xb), d + n + m + g), dtype=np.float64)
            pad[:, d:d + n] = a
            planes.append(np.lib.stride_tricks.sliding_window_view(pad, g, axis=1))
        wh, wl = planes
        tot = np.zeros((len(xb), P), dtype=np.float64)
        acc = np.zeros((len(xb), P), dtype=np.float32)
        for t0 in range(0, m, g):
            for w, kk in ((wl, kh), (wh, kl), (wh, kh)):
                acc = (acc.astype(np.float64) + w[:, t0:t0 + P] @ kk[t0:t0 + g]).astype(np.float32)
            if (t0 + g) % chunk == 0 or t0 + g >= m:
                tot += acc
                acc[:] = 0
        out.append(tot / (xs.astype(np.float64) * float(ks)))
    return np.concatenate(out)


def emulate_f32_chain(x, k, mode, chunk, batch=32):
    """The float32 forms' arithmetic (dsp_fir_mfma.hip): a fused multiply-add per sample into a float32 partial sum of ``chunk`` samples
    (SCHUNK for a kept output, KCHUNK for the amax form), the partial sums added in float64"""
    m = len(k)
    kr = np.asarray(k)[::-1].astype(np.float64)
    out = []
    for r0 in range(0, len(x), batch):
        w = windows(x[r0:r0 + batch].astype(np.float64), m, mode)
        tot = np.zeros(w.shape[:2], dtype=np.float64)
        acc = np.zeros(w.shape[:2], dtype=np.float32)
        for t in range(m):
            acc = (acc.astype(np.float64) + w[:, :, t] * kr[t]).astype(np.float32)  # (a 48-bit product: exact in float64)
            if (t + 1) % chunk == 0 or t + 1 == m:
                tot += acc
                acc[:] = 0
        out.append(tot)
    return np.concatenate(out)

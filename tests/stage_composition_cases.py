"""The case book of recipes that chain the row kernels (test_stage_composition_cpu.py, test_gpu_stage_composition.py): one processor with a
kernel of its own reading what another one made.  Each family's own suite feeds its kernel chain inputs, slices of them and waveforms the
interpreter computes; here the source of a row kernel is another row kernel's result -- directly, through a slice of it, and with
``bl_subtract`` ahead of the producer --, with interpreter ops between two of them, three deep, and with one producer read by two consumers.

One small table: 13 rows (a partial workgroup of four) of 1000 samples, a baseline with noise and a step as in test_gpu_sort.py::_table;
row 11 is constant.  ``waveform`` holds them as uint16.  uint16 holds neither a NaN nor an infinity, so ``waveform_f`` holds the same rows as
float32 with a NaN in row 4 and a +inf in row 8 (rows 3, 5, 7 and 9 are their clean neighbours): the direct and the ``bl_subtract`` variants
of a pair read ``waveform``, the slice variant reads ``waveform_f``.  ``bl`` is a float32 column.  The constants come through ``db_dict``: the
9 taps of ``gaussian_filter1d(1, 4)``, a 1000 x 8 weight matrix with its bias, the mean and variance of a normalisation, and 64 integer taps for
the long-FIR route.

A case is a recipe, its outputs, the kernels its processors own (one launch each) and a function that computes the expected outputs: the
project's CPU models applied link by link in float32, each fed the previous link's result.  ``psd`` and the layers have models with an error
bound and no bit-exact result; for those links the expected value is the device gufunc on the model-made source rows (so ``expected`` of
such a case needs a device).  A pair whose shapes the consumer refuses holds the refusal's text instead.

The four families that fuse processors into one launch -- the pile-up finder (rc_cr2, the bi-level walk), the pulse picker
(peak_snr_threshold, multi_a_filter), the decay-tail fitter (log_check, poly_fit, poly_diff, poly_exp_rms) and the aligner (inl_correction,
get_wf_centroid, wf_alignment, wf_correction) -- are links of their families' own emulations (pileup_cases, pulse_cases, align_cases: bit
for bit; tailfit_cases: the device gufunc on the model-made rows, and within that family's bounds of its long-double sums).  They add a
producer per kind of result and a consumer per family, which asks for all its outputs.  ``waveform_n`` holds the float32 rows with the NaN
and no infinity: rc_cr2 makes an infinity a DSPFatal, so where the +inf of ``waveform_f`` would reach it a pair's slice variant reads
``waveform_n``, and the fatal row is a case of its own (``fatal_cases``: the DSPFatal at ``execute``, naming that one row).  inl_correction
reads an integer column of the table and nothing else: its other two variants are refusals."""
import re

import numpy as np

import align_cases as ac
import extrema_cases as xc
import histogram_cases as hc
import interp_cases as ic
import pileup_cases as pc
import pulse_cases as uc
import reflect_cases as rc
import tailfit_cases as fc
import threshold_cases as tc

M = "dspeed.processors"
ROWS, N = 13, 1000
NAN_ROW, INF_ROW, CONSTANT_ROW = 4, 8, 11
NAN_AT, INF_AT = 300, 700
F32 = np.float32

K_REFLECT, K_HIST, K_EXTREMA, K_THRESH = rc.KERNEL, "dsp_hist_kernel", "dsp_extrema_kernel", "dsp_thresh_kernel"
K_PSD, K_SORT, K_INTERP, K_DENSE = "dsp_spectrum_kernel", "dsp_sort_kernel", ic.KERNEL, "dsp_dense_kernel"
K_FIR = "dsp_fir_f16_kernel"  # a convolve_wf of STAGE_MIN_TAPS taps or more
K_PILEUP, K_PULSES, K_TAILFIT, K_ALIGN = pc.KERNEL, uc.KERNEL, fc.KERNEL, ac.KERNEL
OWN_KERNELS = (K_REFLECT, K_HIST, K_EXTREMA, K_THRESH, K_PSD, K_SORT, K_INTERP, K_DENSE, K_FIR, K_PILEUP, K_PULSES, K_TAILFIT, K_ALIGN)

THRESHOLDS = [0.5, 3.5, 20.5, 100.0, 600.0, 10100.0, 10600.0, 1.0e6]  # counts of a histogram, baseline-subtracted and raw samples, a spectrum
STEP_THRESHOLDS = [100.0 + 50 * k for k in range(8)]  # a producer's: the step (500 at the least) crosses every one, so its row of times is finite
OVER = 100.0
EXTREMA = (15, 15, 0, -1.0e30, 1.0e30)  # a_delta_max, a_delta_min, search_direction, a_abs_max, a_abs_min: any height
BINS, C_BINS, LISTS, LAG, LAYER = 64, 32, 20, 5, 8
LONG_TAPS = 64  # (compiler.STAGE_MIN_TAPS, asserted by the CPU test)
FIR_TOL = 1e-6  # of the row's filtered peak: fir_tile_cases.TOL, the bound of rows with more than float16's 11 significant bits
TAU, WALK_AT, GATE, WALK_LISTS = 20, 25.0, 200, 6  # rc_cr2's t_tau in samples; a walk's thresholds +-WALK_AT: every row of the table but the constant one crosses them more than WALK_LISTS times
CANDS, WIDTH, RATIO = 4, 2, 0.9995  # a picker's list, half its window, its ratio: of the raw rows' candidates some pass and some do not
FRACTION_ROW = 6  # the row of ``cands_half`` that holds a position that is no whole number
FIT_DEG, C_FIT_DEG = 3, 1  # a producer's fit, a consumer's (which also reads rows of two and three samples)
SHIFT, CENTROID = 8, 300.0  # get_wf_centroid's and wf_alignment's shift; the constant centroid
SIZE, CORRECT = 200, (20, 120)  # a producer's window and what of it is corrected
C_SIZE, C_CORRECT = 32, (4, 24)  # a consumer's
TEMPLATE = 100
FATAL_FILTER, FATAL_CENTROID = "RC-CR\\^2 filter produced nans in output\\.", "centroid is nan"
FATAL_FRACTION = "fixed_time_pickoff requires integer t_in when using mode 'i'"


# ---------------------------------------------------------------------------------------------------------------- the table and the constants
def rows():
    """(uint16 rows, the same in float32 with the NaN and the +inf, bl)"""
    rng = np.random.default_rng(0x5C)
    w = (10000 + rng.integers(-20, 21, (ROWS, N)) + (np.arange(N) >= 600) * rng.integers(500, 5000, (ROWS, 1))).astype(np.uint16)
    w[CONSTANT_ROW] = 10007
    f = w.astype(F32)
    f[NAN_ROW, NAN_AT], f[INF_ROW, INF_AT] = np.nan, np.inf
    return w, f, rng.uniform(9990, 10010, ROWS).astype(F32)


def table():
    """... and ``waveform_n``, the float32 rows with the NaN and no infinity (rc_cr2 makes an infinity a DSPFatal); ``cands``, whole positions
    inside the shortest row a picker reads here (five of a walk's six times), a NaN and a position outside the row among them; ``cands_half``,
    the same with one position of row FRACTION_ROW that is no whole number"""
    w, f, bl = rows()
    n = f.copy()
    n[INF_ROW, INF_AT] = w[INF_ROW, INF_AT]
    cands = np.random.default_rng(0xCA).integers(0, 5, (ROWS, CANDS)).astype(F32)
    cands[2, 1], cands[9, 3] = np.nan, 1.0e4
    half = cands.copy()
    half[FRACTION_ROW, 2] = 2.5
    return {"waveform": w, "waveform_f": f, "waveform_n": n, "bl": bl, "cands": cands, "cands_half": half}


def constants():
    from dspeed_amd.processors import gaussian_filter1d

    rng = np.random.default_rng(0xDB)
    return {"kernel": gaussian_filter1d(F32(1), F32(4), np.empty(9, F32)),
            "weights": (rng.integers(-8, 9, (N, LAYER)) / 64).astype(F32), "bias": rng.integers(-4, 5, LAYER).astype(F32),
            "mean": rng.uniform(9000, 11000, N).astype(F32), "variance": rng.uniform(50, 500, N).astype(F32),
            "long_kernel": rc.asymmetric(LONG_TAPS).astype(F32), "inl": ac.inl_table("f32", 1 << 16), "tpl": ac.template("f32", TEMPLATE)}


# ---------------------------------------------------------------------------------------------------------------- sort's total order
def total_order_sort(x):
    """np.sort of each float32 row in the total order of the bit patterns (-0.0 ahead of +0.0); a row that holds a NaN: NaNs"""
    x = np.ascontiguousarray(x, dtype=F32)
    bits = x.view(np.int32)
    key = bits ^ ((bits >> 31) & 0x7FFFFFFF)
    out = np.take_along_axis(x, np.argsort(key, axis=1, kind="stable"), axis=1)
    out[np.isnan(x).any(axis=1)] = np.nan
    return out


# ---------------------------------------------------------------------------------------------------------------- a recipe and its model, link by link
_SOURCE = re.compile(r"^(\w+)(?:\[(-?\d*):(-?\d*)\])?$")
_MEMO = {}  # what a link computes from the table, by its description: shared between the cases, never written to


class Recipe:
    """processors added one by one, each with the model of its link; ``length`` and ``made`` follow every waveform variable"""

    def __init__(self, name, group):
        self.name, self.group = name, group
        self.procs, self.outputs, self.kernels, self.links = {}, [], [], []
        self.refusal, self.refused_at = None, None  # the text of a refusal, and where it is raised: "build" or "execute"
        self.refused_for = None  # what the refusal is a limit of: "the consumer's shapes" or "the producer's source"
        self.psd_links, self.fir_links = [], []  # (source, spectrum) of every psd; the outputs of a long FIR: held to a bound, not to bits
        self.fir_sources = {}  # the output of a long FIR -> what it filters
        self.fir_cancelling = {}  # the output of a long FIR -> the rows whose products cancel to a small part of themselves (the GPU test's _check)
        self.same_as = None  # the case with the intermediate rows among its outputs, whose results this one's equal bit for bit
        self.tail_links = []  # (processor, source, coefficients or None, its outputs, degree) of every decay-tail link: held to the family's bounds
        self.fatal = None  # (the text of the DSPFatal ``execute`` raises, the one row it names): a row a model calls fatal
        self.nan_counts, self.nan_values = [], []  # per-event outputs that are 0 and NaN for a row of NaNs
        self.near_candidates = {}  # a picker's outputs -> its source: it looks at the samples around its candidates, not at the row, so a lone NaN far from them shows nowhere
        self.of_device_rows = None  # (an output held to a bound or None, the outputs behind it): ``after_long_fir`` of the device's own row, or ``same_as``'s
        self.length = {"waveform": N, "waveform_f": N, "waveform_n": N, "cands": CANDS, "cands_half": CANDS}
        self.made = {k: k for k in self.length}  # variable -> how it is made from the table

    # -- sources
    def _parse(self, src):
        name, a, b = _SOURCE.match(src).groups()
        return name, (int(a) if a else None), (int(b) if b else None)

    def len_of(self, src):
        name, a, b = self._parse(src)
        return len(range(self.length[name])[a:b])

    def _take(self, env, src):
        name, a, b = self._parse(src)
        return np.ascontiguousarray(env[name][:, a:b])

    def _describe(self, src):
        name, a, b = self._parse(src)
        return self.made[name] + src[len(name):]

    def _link(self, fn, src, outs, lengths, params, model, kernel, also=()):
        """``also``: what the link reads besides ``src`` (a list, coefficients, a per-event operand); a model may return, behind its
        outputs, the rows it calls fatal"""
        what = f"{fn}{params}({', '.join(self._describe(a) for a in (src, *also))})"
        for k, (o, n) in enumerate(zip(outs, lengths)):
            self.length[o], self.made[o] = n, f"{what}.{k}"
        if kernel is not None:
            self.kernels.append(kernel)

        def run(env):
            if what not in _MEMO:
                res = model(self._take(env, src), env)
                _MEMO[what] = tuple(np.asarray(r) for r in (res if isinstance(res, tuple) else (res,)))
                for r in _MEMO[what]:
                    r.setflags(write=False)
            env.update(zip(outs, _MEMO[what]))
            env["fatal"] += [(fn, int(r)) for fatal in _MEMO[what][len(outs):] for r in np.flatnonzero(fatal)]

        self.links.append(run)
        return outs[0]

    # -- processors
    def bl_subtract(self, src, out="wf_blsub"):
        self.procs[out] = {"function": "bl_subtract", "module": M, "args": [src, "bl", out]}
        return self._link("bl_subtract", src, [out], [self.len_of(src)], "", lambda x, env: (x - env["bl"][:, None]).astype(F32), None)

    def reflect(self, src, out="wf_gaus", current=None):
        """``current``: the name of an avg_current of the filtered row, which joins the launch"""
        n = self.len_of(src)
        self.procs[out] = {"function": "reflected_convolve_wf", "module": f"{M}.convolutions", "args": [src, "db.kernel", out]}
        self._link("reflect", src, [out], [n], "", lambda x, env: rc.emulate(x, env["db"]["kernel"], F32), K_REFLECT)
        if current is None:
            return out
        self.procs[current] = {"function": "avg_current", "module": f"{M}.moving_windows", "args": [out, LAG, f"{current}({n - LAG})"]}
        return self._link("avg_current", out, [current], [n - LAG], "", lambda g, env: rc.avg_current(g, LAG), None)

    def histogram(self, src, weights="wf_hw", borders="wf_hb", bins=BINS, stats=None):
        """``stats``: the names of (mode, max, fwhm) of a histogram_stats that joins the launch"""
        def model(x, env):
            both = [hc.model_histogram(row, bins, F32, 1) for row in x]
            return np.stack([w for w, _b in both]), np.stack([b for _w, b in both])

        self.procs[f"{weights}, {borders}"] = {"function": "histogram", "module": f"{M}.histogram", "args": [src, f"{weights}({bins})", f"{borders}({bins + 1})"]}
        self._link("histogram", src, [weights, borders], [bins, bins + 1], f"[{bins}]", model, K_HIST)
        if stats is not None:
            def model_stats(wts, env):
                res = np.array([hc.model_stats(wts[r], env[borders][r], np.nan, F32) for r in range(len(wts))], dtype=F32)
                return res[:, 0], res[:, 1], res[:, 2]

            self.procs[", ".join(stats)] = {"function": "histogram_stats", "module": f"{M}.histogram", "args": [weights, borders, *stats, "np.nan"]}
            self._link("histogram_stats", weights, list(stats), [None] * 3, "", model_stats, None)
        return weights

    def extrema(self, src, prefix="c", a_abs_max=None):
        """``a_abs_max``: a per-event operand (``_operand``) in the place of EXTREMA's constant"""
        names = [f"wf_{prefix}_vmax", f"wf_{prefix}_vmin", f"{prefix}_n_max", f"{prefix}_n_min"]
        text, reads, worth = self._operand(EXTREMA[3] if a_abs_max is None else a_abs_max)

        def model(x, env):
            top = np.broadcast_to(np.asarray(worth(env), dtype=F32), (len(x),))
            res = [xc.model(row, *EXTREMA[:3], top[k], EXTREMA[4], LISTS, F32, 1) for k, row in enumerate(x)]
            return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], dtype=np.uint32),
                    np.array([r[3] for r in res], dtype=np.uint32))

        self.procs[", ".join(names)] = {"function": "get_multi_local_extrema", "module": f"{M}.get_multi_local_extrema",
                                        "args": [src, *EXTREMA[:3], text, EXTREMA[4], f"{names[0]}({LISTS})", f"{names[1]}({LISTS})", names[2], names[3]]}
        self._link("extrema", src, names, [LISTS, LISTS, None, None], "" if a_abs_max is None else f"[{text}]", model, K_EXTREMA, also=reads)
        return names

    def multi_thresh(self, src, out="wf_tp", thresholds=THRESHOLDS):
        n, m = self.len_of(src), len(thresholds)
        ts = n // 2
        self.procs[out] = {"function": "multi_time_point_thresh", "module": f"{M}.time_point_thresh",
                           "args": [src, str(thresholds), float(ts), 1, "'l'", f"{out}({m})"]}
        return self._link("multi_time_point_thresh", src, [out], [m], f"[{ts}, {thresholds[0]}..]",
                          lambda x, env: np.stack([tc.model(row, F32(thresholds), ts, 1, "l", F32) for row in x]), K_THRESH)

    def time_over(self, src, out="n_over", over=OVER):
        """``over``: the threshold, a number or a per-event operand (``_operand``)"""
        text, reads, worth = self._operand(over)

        def model(x, env):
            level = np.broadcast_to(np.asarray(worth(env), dtype=F32), (len(x),))
            return np.array([tc.model_time_over_threshold(row, level[k], F32) for k, row in enumerate(x)], dtype=F32)

        self.procs[out] = {"function": "time_over_threshold", "module": f"{M}.time_over_threshold", "args": [src, text, out]}
        return self._link("time_over_threshold", src, [out], [None], "" if over == OVER else f"[{text}]", model, K_THRESH, also=reads)

    def psd(self, src, out="wf_psd"):
        def model(x, env):  # (the device gufunc on the model-made rows: test_gpu_spectrum.py's rule)
            from dspeed_amd.processors import psd

            return psd(x, np.empty((len(x), x.shape[1] // 2 + 1), F32))

        n = self.len_of(src)
        self.procs[out] = {"function": "psd", "module": f"{M}.fft", "args": [src, f"{out}({n // 2 + 1})"]}
        self.psd_links.append((src, out))
        return self._link("psd", src, [out], [n // 2 + 1], "", model, K_PSD)

    def sort(self, src, out="wf_sorted"):
        self.procs[out] = {"function": "sort", "module": f"{M}.sort", "args": [src, out]}
        return self._link("sort", src, [out], [self.len_of(src)], "", lambda x, env: total_order_sort(x), K_SORT)

    def interp(self, src, out="wf_up", mode="l", factor=4):
        m = factor * self.len_of(src)
        self.procs[out] = {"function": "interpolating_upsampler", "module": f"{M}.upsampler", "args": [src, f"'{mode}'", f"{out}({m})"]}
        return self._link("interp", src, [out], [m], f"[{mode}{factor}]", lambda x, env: ic.emulate(x, mode, m), K_INTERP)

    def dense(self, src, out="wf_y"):
        def model(x, env):
            from dspeed_amd.processors import dense_layer_with_bias

            return dense_layer_with_bias(x, env["db"]["weights"], env["db"]["bias"], "r")

        self.procs[out] = {"function": "dense_layer_with_bias", "module": f"{M}.ml", "args": [src, "db.weights", "db.bias", "'r'", out]}
        return self._link("dense", src, [out], [LAYER], "", model, K_DENSE)

    def normalise(self, src, out="wf_norm", launch=True):
        """``launch``: False where only layers read it and the recipe does not ask for it -- folded into their launches"""
        def model(x, env):
            from dspeed_amd.processors import normalisation_layer

            return normalisation_layer(x, env["db"]["mean"], env["db"]["variance"])

        self.procs[out] = {"function": "normalisation_layer", "module": f"{M}.ml", "args": [src, "db.mean", "db.variance", out]}
        return self._link("normalise", src, [out], [self.len_of(src)], "", model, K_DENSE if launch else None)

    def long_fir(self, src, out="wf_fir"):
        def model(x, env):  # (the float64 convolution: the matrix-core FIR is held to FIR_TOL of the row's filtered peak, as in its own suite)
            k = env["db"]["long_kernel"].astype(np.float64)
            return np.stack([np.convolve(row.astype(np.float64), k, "valid") for row in x])

        n = self.len_of(src) - LONG_TAPS + 1
        self.procs[out] = {"function": "convolve_wf", "module": M, "args": [src, "db.long_kernel", "'v'", f"{out}({n})"]}
        self.fir_links.append(out)
        self.fir_sources[out] = src
        return self._link("long_fir", src, [out], [n], "", model, K_FIR)

    # -- the four families that fuse: each processor a link of its own, the launches as the families' suites have them
    @staticmethod
    def _operand(a):
        """a per-event operand: a number, or (its text in the recipe, the variables it reads, what it is worth given ``env``)"""
        return (a, (), lambda env: a) if isinstance(a, (int, float)) else a

    def rc_cr2(self, src, out="wf_rc", launch=True):
        """``launch``: False where a walk of exactly this row follows -- it takes the filter into its launch"""
        self.procs[out] = {"function": "rc_cr2", "module": f"{M}.rc_cr2", "args": [src, TAU, out]}
        return self._link("rc_cr2", src, [out], [self.len_of(src)], f"[{TAU}]", lambda x, env: pc.emulate_rc_cr2(x, TAU, F32, cube="product", exp="libm"),
                          K_PILEUP if launch else None)

    def walk(self, src, prefix="w", at=WALK_AT):
        """-> (count, polarity, times), thresholds at +-``at``"""
        names = [f"{prefix}_n", f"wf_{prefix}_pol", f"wf_{prefix}_tt"]
        text, reads, worth = self._operand(at)

        def model(x, env):
            pos = np.broadcast_to(np.asarray(worth(env), dtype=F32), (len(x),))
            return pc.emulate_walk(x, pos, -pos, GATE, 0, WALK_LISTS, F32)

        self.procs[", ".join(names)] = {"function": "bi_level_zero_crossing_time_points", "module": f"{M}.time_point_thresh",
                                        "args": [src, text, f"-{text}", GATE, 0, names[0], *(f"{v}({WALK_LISTS}, vector_len={names[0]})" for v in names[1:])]}
        self.nan_counts.append(names[0])
        self._link("walk", src, names, [None, WALK_LISTS, WALK_LISTS], f"[{text}]", model, K_PILEUP, also=reads)
        return names

    def picker(self, src, lst="cands", prefix="k", ratio=RATIO):
        """-> (positions, count)"""
        names = [f"wf_{prefix}_pos", f"{prefix}_n"]
        text, reads, worth = self._operand(ratio)
        self.procs[", ".join(names)] = {"function": "peak_snr_threshold", "module": f"{M}.peak_snr_threshold",
                                        "args": [src, lst, text, WIDTH, f"{names[0]}(vector_len={names[1]})", names[1]]}
        self.nan_counts.append(names[1])
        self.near_candidates.update(dict.fromkeys(names, src))
        self._link("picker", src, names, [self.len_of(lst), None], f"[{text}, {WIDTH}]", lambda x, env: uc.emulate_picker(x, env[lst], worth(env), WIDTH, F32)[:2], K_PULSES,
                   also=(lst, *reads))
        return names

    def pickoff(self, src, lst, out="wf_k_en", launch=True):
        """``launch``: False where ``lst`` is a picker's list of the same variable, whole: multi_a_filter joins the picker's launch"""
        self.procs[out] = {"function": "multi_a_filter", "module": f"{M}.multi_a_filter", "args": [src, lst, f"{out}(vector_len=len({lst}))"]}
        return self._link("pickoff", src, [out], [self.len_of(lst)], "", lambda x, env: uc.emulate_pickoff(x, env[lst], F32), K_PULSES if launch else None, also=(lst,))

    def log_check(self, src, out="wf_log", launch=True):
        """``launch``: False where a poly_fit of exactly this row follows"""
        def model(x, env):  # (the device gufunc on the model-made rows, as for psd; held to log_bound by the GPU test)
            from dspeed_amd.processors import log_check

            return log_check(x, np.empty_like(x))

        self.procs[out] = {"function": "log_check", "module": M, "args": [src, out]}
        self.tail_links.append(("log_check", src, None, [out], None))
        return self._link("log_check", src, [out], [self.len_of(src)], "", model, K_TAILFIT if launch else None)

    def poly_fit(self, src, out="wf_pars", deg=FIT_DEG, launch=True):
        """``launch``: False where a residual of this fit and of the rows it was made of follows"""
        n = self.len_of(src)

        def model(x, env):
            from dspeed_amd.processors import poly_fit

            return poly_fit(n, deg)(x, np.empty((len(x), deg + 1), F32))

        self.procs[out] = {"function": f"{M}.poly_fit", "args": [src, f"{out}(shape={deg + 1})"], "init_args": [n, deg]}
        self.tail_links.append(("poly_fit", src, None, [out], deg))
        return self._link("poly_fit", src, [out], [deg + 1], f"[{deg}]", model, K_TAILFIT if launch else None)

    def residual(self, src, pars, names=("tm", "tr"), exp=True):
        """poly_exp_rms, or poly_diff with ``exp`` false -> (mean, rms)"""
        fn = "poly_exp_rms" if exp else "poly_diff"

        def model(x, env):
            from dspeed_amd import processors

            return getattr(processors, fn)(x, self._take(env, pars), np.empty(len(x), F32), np.empty(len(x), F32))

        self.procs[", ".join(names)] = {"function": fn, "module": f"{M}.poly_fit", "args": [src, pars, *names]}
        self.tail_links.append((fn, src, pars, list(names), None))
        self.nan_values += names
        self._link(fn, src, list(names), [None, None], "", model, K_TAILFIT, also=(pars,))
        return list(names)

    def inl(self, src, out="wf_inl"):
        self.procs[out] = {"function": "inl_correction", "module": M, "args": [src, "db.inl", out]}
        return self._link("inl", src, [out], [self.len_of(src)], "", lambda x, env: ac.emulate_inl(x.astype(np.int64), env["db"]["inl"], F32)[0], K_ALIGN)

    def centroid(self, src, out="cen"):
        self.procs[out] = {"function": "get_wf_centroid", "module": M, "args": [src, SHIFT, out]}
        self.nan_values.append(out)
        return self._link("centroid", src, [out], [None], f"[{SHIFT}]", lambda x, env: ac.emulate_centroid(x, SHIFT, F32)[0], K_ALIGN)

    def align(self, src, out="wf_al", centroid=CENTROID, size=SIZE, launch=True):
        """``launch``: False where a wf_correction of exactly this window follows -- it takes the alignment into its launch"""
        text, reads, worth = self._operand(centroid)

        def model(x, env):
            win, status = ac.emulate_alignment(x, worth(env), SHIFT, size, F32)
            return win, status == ac.FATAL

        self.procs[out] = {"function": "wf_alignment", "module": M, "args": [src, text, SHIFT, size, f"{out}({size})"]}
        return self._link("align", src, [out], [size], f"[{text}, {SHIFT}, {size}]", model, K_ALIGN if launch else None, also=reads)

    def correct(self, src, out="wf_corr", window=CORRECT):
        self.procs[out] = {"function": "wf_correction", "module": M, "args": [src, "db.tpl", *window, out]}
        return self._link("correct", src, [out], [self.len_of(src)], f"{list(window)}", lambda x, env: ac.emulate_correction(x, env["db"]["tpl"], *window, F32), K_ALIGN)

    def expect_fatal(self, text, row):
        self.fatal = (text, row)
        return self

    # -- the case
    def out(self, *names):
        self.outputs += [n for n in names if n not in self.outputs]
        return self

    def recipe(self):
        return {"outputs": list(self.outputs), "processors": dict(self.procs)}

    def take(self, env, src):
        """the rows a processor reads as ``src``, out of ``expected``'s second result"""
        return self._take(env, src)

    def expected(self):
        """({output: the expected array}, every variable of the recipe): the models applied link by link to the table (``psd`` and layer
        links call the device)"""
        env = self._run()
        assert not env["fatal"], (self.name, env["fatal"])  # (a case whose models call a row fatal says so: ``fatal``, ``fatal_rows``)
        return {o: env[o] for o in self.outputs}, env

    def _run(self):
        env = dict(table(), db=constants(), fatal=[])
        env["waveform"] = env["waveform"].astype(F32)
        for run in self.links:
            run(env)
        return env

    def fatal_rows(self):
        """the rows the models call fatal, in the order of the links: [(link, row)]"""
        return self._run()["fatal"]


# ---------------------------------------------------------------------------------------------------------------- producers and consumers
# producer: (how it is added, the slice of its row a consumer reads in the slice variant)
PRODUCERS = {
    "reflect": (lambda r, s: r.reflect(s), "[100:900]"),
    "current": (lambda r, s: r.reflect(s, current="wf_cur"), "[100:900]"),
    "histogram": (lambda r, s: r.histogram(s), "[8:56]"),
    "multi_thresh": (lambda r, s: r.multi_thresh(s, thresholds=[t + (0 if s == "wf_blsub" else 10000) for t in STEP_THRESHOLDS]), "[1:7]"),
    "psd": (lambda r, s: r.psd(s), "[1:]"),
    "sort": (lambda r, s: r.sort(s), "[200:]"),  # (the +inf of a sorted row is its last sample)
    "interp": (lambda r, s: r.interp(s), "[:1000]"),
    "dense": (lambda r, s: r.dense(s), "[1:7]"),
    "normalise": (lambda r, s: r.normalise(s), "[100:900]"),
}


def _consume_reflect(r, s):
    r.out(r.reflect(s, out="wf_c_gaus"))


def _consume_histogram(r, s):
    stats = ("c_mode", "c_max", "c_fwhm")
    r.histogram(s, "wf_c_hw", "wf_c_hb", bins=C_BINS, stats=stats)
    r.out("wf_c_hw", "wf_c_hb", *stats)


def _consume_extrema(r, s):
    r.out(*r.extrema(s))


def _consume_thresholds(r, s):
    r.out(r.multi_thresh(s, out="wf_c_tp"), r.time_over(s, out="c_n_over"))


def _consume_psd(r, s):
    r.out(r.psd(s, out="wf_c_psd"))


def _consume_sort(r, s):
    r.out(r.sort(s, out="wf_c_sorted"))


def _consume_interp(r, s):
    r.out(r.interp(s, out="wf_c_up"))


def _consume_ml(r, s):
    r.out(r.dense(s, out="wf_c_y"))


def _consume_pileup(r, s):
    flt = r.rc_cr2(s, out="wf_c_rc", launch=False)
    r.out(flt, *r.walk(flt, prefix="c"))


def _consume_pulses(r, s):
    pos, count = r.picker(s, prefix="c")
    r.out(pos, count, r.pickoff(s, pos, out="wf_c_en", launch="[" in s))  # (two slices of a row are two arguments: the launches stay apart)


def _consume_tailfit(r, s):
    pars = r.poly_fit(r.log_check(s, out="wf_c_log", launch=False), out="wf_c_pars", deg=C_FIT_DEG, launch=False)
    r.out("wf_c_log", pars, *r.residual(s, pars, names=("c_tm", "c_tr")))


def _consume_align(r, s):
    r.out(r.centroid(s, out="c_cen"), r.align(s, out="wf_c_al", size=C_SIZE, launch=False), r.correct("wf_c_al", out="wf_c_corr", window=C_CORRECT))


CONSUMERS = {"reflect": _consume_reflect, "histogram": _consume_histogram, "extrema": _consume_extrema, "thresholds": _consume_thresholds,
             "psd": _consume_psd, "sort": _consume_sort, "interp": _consume_interp, "ml": _consume_ml,
             "pileup": _consume_pileup, "pulses": _consume_pulses, "tailfit": _consume_tailfit, "align": _consume_align}
OLD_PRODUCERS = tuple(PRODUCERS)
PRODUCERS.update({
    "rc_cr2": (lambda r, s: r.rc_cr2(s), "[100:900]"),
    "walk": (lambda r, s: r.walk(r.rc_cr2(s, launch=False))[2], "[1:]"),  # the trig_times of a walk fused with its filter
    "energies": (lambda r, s: r.pickoff(s, r.picker(s)[0], launch=False), "[1:]"),  # of a picker fused with multi_a_filter
    "logged": (lambda r, s: r.log_check(s), "[100:900]"),
    "pars": (lambda r, s: r.poly_fit(r.log_check(s, launch=False)), "[1:]"),  # the coefficients of a fused log_check + poly_fit
    "inl": (lambda r, s: r.inl(s), "[100:900]"),
    "aligned": (lambda r, s: r.align(s), "[50:150]"),
    "corrected": (lambda r, s: r.correct(r.align(s, launch=False)), "[50:150]"),  # of the fused alignment and correction
})
NEW_CONSUMERS = ("pileup", "pulses", "tailfit", "align")
VARIANTS = ("direct", "slice", "blsub")
#: the producers that make the +inf of ``waveform_f`` a DSPFatal of rc_cr2 -- their own, or the consumer's, which finds an infinity (and no NaN
#: beside it) ahead of the last sample of the slice it reads: their slice variant reads ``waveform_n``, and ``fatal_cases`` holds ``waveform_f``
STARTS_WITH_FILTER = ("rc_cr2", "walk")
INF_TO_FILTER = ("reflect", "normalise", "logged")


def _refusal(consumer, n):
    """(the text with which a consumer is refused on a row of ``n`` samples, where it is raised), or (None, None): it takes the row.  The
    peak finder's is the reference body's own check of its arguments, raised as a DSPFatal when the stage is planned, at the first ``execute``;
    all others are raised by ``build_processing_chain``: the filter's and the layer's as the processors are read, the four fusing families'
    (processors.check_rc_cr2, check_pulse_list, check_alignment: the reference's words) as their stages are made."""
    if consumer == "reflect" and n < 9:
        return "The filter is longer than the input waveform", "build"
    if consumer == "ml" and n != N:
        return f"dense_layer_with_bias \\(wf_c_y\\): '.*' holds {n} samples, kernel has shape \\({N}, {LAYER}\\)", "build"
    if consumer == "extrema" and n <= LISTS:
        return "The length of your return array must be smaller than the length of your waveform", "execute"
    if consumer == "pileup" and n <= 3:
        return "The length of the waveform must be larger than 3 for the filter to work safely", "build"
    if consumer == "pulses" and n <= CANDS:
        return "The length of your return array must be smaller than the length of your waveform", "build"
    if consumer == "align" and (SHIFT > n or C_SIZE > n):
        return ("shift" if SHIFT > n else "size") + " must be shorter than input waveform size", "build"
    return None, None


def _pair(producer, consumer, variant):
    add, cut = PRODUCERS[producer]
    r = Recipe(f"{producer}->{consumer}/{variant}", "pair")
    clean = producer in STARTS_WITH_FILTER or (consumer == "pileup" and producer in INF_TO_FILTER)
    src = {"direct": "waveform", "slice": "waveform_n" if clean else "waveform_f"}.get(variant) or r.bl_subtract("waveform")
    made = add(r, src)
    if producer == "normalise" and consumer == "ml" and variant != "slice":
        r.kernels.remove(K_DENSE)  # (a normalisation that only a layer reads whole runs inside the layer's launch)
    r.read = read = made + (cut if variant == "slice" else "")
    r.refusal, r.refused_at = _refusal(consumer, r.len_of(read))
    r.refused_for = "the consumer's shapes" if r.refusal else None
    if producer == "inl" and variant != "direct" and r.refused_at != "build":  # (inl_correction reads ADC codes: an integer column of the table)
        r.refusal, r.refused_at, r.refused_for = f"inl_correction \\(wf_inl\\): '{src}' is not an integer input column", "build", "the producer's source"
    CONSUMERS[consumer](r, read)
    return r


def pairs():
    """the old producers with every consumer (the old ones first: their cases are the ones they were), then the new ones"""
    return [_pair(p, c, v) for p in PRODUCERS for c in CONSUMERS for v in VARIANTS]


def _between():
    """interpreter ops between two row kernels"""
    out = []
    r = Recipe("psd(bl_subtract(sort))", "between")
    out.append(r.out(r.psd(r.bl_subtract(r.sort("waveform_f")))))
    r = Recipe("sort(bl_subtract(sort))", "between")
    out.append(r.out(r.sort(r.bl_subtract(r.sort("waveform_f")), out="wf_c_sorted")))
    r = Recipe("histogram(bl_subtract(interp))", "between")
    r.histogram(r.bl_subtract(r.interp("waveform")))
    out.append(r.out("wf_hw", "wf_hb"))
    return out


def _deep():
    """depth three and fan-out, each with the intermediate rows among the outputs and without"""
    out = []
    for keep in (False, True):
        tag = "+rows" if keep else ""
        r = Recipe("multi_thresh(interp(reflect(bl_subtract)))" + tag, "deep")
        r.out(r.multi_thresh(r.interp(r.reflect(r.bl_subtract("waveform")))))
        out.append(r.out("wf_blsub", "wf_gaus", "wf_up") if keep else r)
        r = Recipe("time_over(dense(interp[:1000]))" + tag, "deep")
        r.out(r.time_over(r.dense(r.interp("waveform") + "[:1000]")))
        out.append(r.out("wf_up", "wf_y") if keep else r)
        r = Recipe("sort(psd(interp)[1:])" + tag, "deep")
        r.out(r.sort(r.psd(r.interp("waveform_f")) + "[1:]", out="wf_c_sorted"))
        out.append(r.out("wf_up", "wf_psd") if keep else r)
        r = Recipe("histogram+sort(interp)" + tag, "fan-out")  # one producer, two consumers of different families
        up = r.interp("waveform_f")
        r.histogram(up, stats=("h_mode", "h_max", "h_fwhm"))
        r.out("h_mode", "h_max", "h_fwhm", r.sort(up))
        out.append(r.out("wf_up", "wf_hw", "wf_hb") if keep else r)
    r = Recipe("sort(interp['s'])", "deep")  # the spline mode of the upsampler, once
    out.append(r.out(r.sort(r.interp("waveform", mode="s"))))
    return out


def _long_fir():
    """a convolve_wf of STAGE_MIN_TAPS constant taps whose input another row kernel makes; 64 integer taps that are no few runs of equal ones, so
    the filter goes to the matrix cores, not to the prefix sums"""
    out = []
    r = Recipe("long_fir(sort)", "long-fir")
    out.append(r.out(r.long_fir(r.sort("waveform"))))
    r = Recipe("long_fir(interp)", "long-fir")
    out.append(r.out(r.long_fir(r.interp("waveform"))))
    return out


def _times(factor, name):
    """the per-event operand ``factor * name``, as the small program of its own evaluates it: one float32 product"""
    return f"{factor}*{name}", (name,), lambda env: F32(factor) * env[name]


def _value(name):
    return name, (name,), lambda env: env[name]


def _fused_families():
    """the pile-up finder, the pulse picker, the decay-tail fitter and the aligner between, below and beside the other row kernels, each
    with the intermediate rows among the outputs and without; the group says which shape a case has"""
    out = []
    stats = ("h_mode", "h_max", "h_fwhm")
    for keep in (False, True):
        tag = "+rows" if keep else ""
        r = Recipe("walk(rc_cr2(reflect))" + tag, "deep")
        r.out(*r.walk(r.rc_cr2(r.reflect("waveform_n"), launch=False)))
        out.append(r.out("wf_gaus", "wf_rc") if keep else r)
        r = Recipe("pickoff(picker(extrema(rc_cr2)))" + tag, "deep")  # one filtered row read by the peak finder, the picker and multi_a_filter
        flt = r.rc_cr2("waveform_n")
        peaks = r.extrema(flt, prefix="x")
        pos, count = r.picker(flt, lst=peaks[0])
        r.out(count, r.pickoff(flt, pos, launch=False))
        out.append(r.out("wf_rc", *peaks, pos) if keep else r)
        r = Recipe("poly_diff(psd[1:])" + tag, "deep")  # with its fit, in one launch
        spectrum = r.psd("waveform") + "[1:]"
        r.out(*r.residual(spectrum, r.poly_fit(spectrum, launch=False), exp=False))
        out.append(r.out("wf_psd", "wf_pars") if keep else r)
        r = Recipe("walk+centroid+align(rc_cr2)" + tag, "fan-out")
        flt = r.rc_cr2(r.bl_subtract("waveform"), launch=False)
        r.out(*r.walk(flt), r.centroid(flt), r.align(flt))
        out.append(r.out("wf_blsub", "wf_rc") if keep else r)
        r = Recipe("psd(correct(align(inl)))" + tag, "deep")
        r.out(r.psd(r.correct(r.align(r.inl("waveform"), launch=False))))
        out.append(r.out("wf_inl", "wf_al", "wf_corr") if keep else r)
        r = Recipe("walk(rc_cr2)@3*fwhm(histogram(rc_cr2))" + tag, "fan-out")  # the filter runs ahead of the histogram, the walk behind it: two launches
        flt = r.rc_cr2("waveform_n")
        r.histogram(flt, stats=stats)
        r.out(*r.walk(flt, at=_times(3, "h_fwhm")))
        out.append(r.out("wf_rc", "wf_hw", "wf_hb", *stats) if keep else r)
        r = Recipe("extrema@3*tr+picker@tr(tailfit)" + tag, "deep")  # a threshold and a ratio off the residual of the fit: the three in one launch, first
        tr = r.residual("waveform", r.poly_fit(r.log_check("waveform", launch=False), launch=False))[1]
        peaks = r.extrema("waveform", prefix="x", a_abs_max=_times(3, tr))
        pos, count = r.picker("waveform", lst=peaks[0], ratio=_times(0.001, tr))
        r.out(*peaks, pos, count, r.pickoff("waveform", pos, launch=False))
        out.append(r.out("wf_log", "wf_pars", "tm", tr) if keep else r)
        r = Recipe("align@mode(histogram)" + tag, "deep")
        r.histogram("waveform", stats=stats)
        r.out(r.align("waveform", centroid=_value("h_mode")))
        out.append(r.out("wf_hw", "wf_hb", *stats) if keep else r)
        r = Recipe("walk+walk(rc_cr2)" + tag, "fan-out")  # the first walk takes the filter along and writes its row for the second
        flt = r.rc_cr2("waveform_n", launch=False)
        r.out(*r.walk(flt), *r.walk(flt, prefix="v", at=100.0))
        out.append(r.out("wf_rc") if keep else r)
        r = Recipe("walk(rc_cr2[100:900])" + tag, "deep")  # a slice of the filtered row is not the filtered row: two launches
        r.out(*r.walk(r.rc_cr2("waveform_n") + "[100:900]"))
        out.append(r.out("wf_rc") if keep else r)
        r = Recipe("correct(align[50:150])" + tag, "deep")  # likewise
        r.out(r.correct(r.align("waveform_n") + "[50:150]", window=C_CORRECT))
        out.append(r.out("wf_al") if keep else r)
        # The FIR of the constant row's filtered row is outside the filter's 1e-6 bar: that row is nothing but rc_cr2's start-up transient,
        # smooth, and the taps (their sum -17 of 497 in magnitude) cancel it: the products are 79 times the peak they leave, against 9 to 21
        # on the other rows, so one float32 rounding of a partial sum is 2**-24 * 79 = 4.7e-6 of the peak.  NumPy's float32 convolution errs
        # by 1.0e-6 of the peak there and the device, which keeps 22 bits of each float32 sample, by 1.07e-6; the other rows are at 0.3e-6.
        # That row is held to the FIR suite's rule for the cancelling regime (test_gpu_fir_mfma.py's pedestal test: a multiple of the
        # reference's own float32 error); the GPU test asserts the premise on it, and every other row is held to the bar.
        r = Recipe("long_fir(rc_cr2)" + tag, "long-fir")
        r.out(r.long_fir(r.rc_cr2("waveform")))
        r.fir_cancelling["wf_fir"] = [CONSTANT_ROW]
        out.append(r.out("wf_rc") if keep else r)
    # a long FIR ahead of the filter: the FIR is held to a bound, so what follows it is held, bit for bit, to the models of the row the
    # device made -- with that row among the outputs; without the rows, to what the chain with them gave (``same_as``)
    with_rows = Recipe("walk(rc_cr2(long_fir))+rows", "long-fir")
    flt = with_rows.rc_cr2(with_rows.long_fir("waveform"), launch=False)
    with_rows.of_device_rows = ("wf_fir", [flt, *with_rows.walk(flt)])
    with_rows.out("wf_fir", *with_rows.of_device_rows[1])
    r = Recipe("walk(rc_cr2(long_fir))", "long-fir")
    r.of_device_rows = (None, r.walk(r.rc_cr2(r.long_fir("waveform"), launch=False)))
    r.same_as = with_rows
    return out + [r.out(*r.of_device_rows[1]), with_rows]


def after_long_fir(rows):
    """(the filtered row, count, polarity, times) of ``walk(rc_cr2(long_fir))``'s links behind the FIR, on the rows the device's FIR made"""
    flt, fatal = pc.emulate_rc_cr2(rows, TAU, F32, cube="product", exp="libm")
    assert not fatal.any()
    return (flt, *pc.emulate_walk(flt, WALK_AT, -WALK_AT, GATE, 0, WALK_LISTS, F32))


def fatal_cases():
    """Rows a model calls fatal: the case expects the DSPFatal at ``execute``, naming that one row.  The +inf of row INF_ROW inside what
    rc_cr2 reads -- of the table's row, and behind every producer of INF_TO_FILTER, whose pair reads ``waveform_n`` for that reason --; the
    centroid of the constant row, which the reference leaves undefined and the device makes a NaN, reaching wf_alignment; a position that
    is no whole number reaching multi_a_filter through the picker that keeps it."""
    out = []
    r = Recipe("walk(rc_cr2(waveform_f))", "fatal")
    out.append(r.out(*r.walk(r.rc_cr2("waveform_f", launch=False))).expect_fatal(FATAL_FILTER, INF_ROW))
    for producer in INF_TO_FILTER:
        add, cut = PRODUCERS[producer]
        r = Recipe(f"{producer}->pileup/slice of waveform_f", "fatal")
        _consume_pileup(r, add(r, "waveform_f") + cut)
        out.append(r.expect_fatal(FATAL_FILTER, INF_ROW))
    r = Recipe("align@centroid(bl_subtract)", "fatal")
    rows = r.bl_subtract("waveform")
    out.append(r.out(r.align(rows, centroid=_value(r.centroid(rows)))).expect_fatal(FATAL_CENTROID, CONSTANT_ROW))
    r = Recipe("pickoff(picker(cands_half))", "fatal")
    pos, count = r.picker("waveform", lst="cands_half", ratio=2.0)
    out.append(r.out(count, r.pickoff("waveform", pos, launch=False)).expect_fatal(FATAL_FRACTION, FRACTION_ROW))
    return out


def cases():
    return pairs() + _between() + _deep() + _long_fir() + _fused_families() + fatal_cases()

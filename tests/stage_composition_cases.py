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
such a case needs a device).  A pair whose shapes the consumer refuses holds the refusal's text instead."""
import re

import numpy as np

import extrema_cases as xc
import histogram_cases as hc
import interp_cases as ic
import reflect_cases as rc
import threshold_cases as tc

M = "dspeed.processors"
ROWS, N = 13, 1000
NAN_ROW, INF_ROW, CONSTANT_ROW = 4, 8, 11
NAN_AT, INF_AT = 300, 700
F32 = np.float32

K_REFLECT, K_HIST, K_EXTREMA, K_THRESH = rc.KERNEL, "dsp_hist_kernel", "dsp_extrema_kernel", "dsp_thresh_kernel"
K_PSD, K_SORT, K_INTERP, K_DENSE = "dsp_spectrum_kernel", "dsp_sort_kernel", ic.KERNEL, "dsp_dense_kernel"
K_FIR = "dsp_fir_f16_kernel"  # a convolve_wf of STAGE_MIN_TAPS taps or more
OWN_KERNELS = (K_REFLECT, K_HIST, K_EXTREMA, K_THRESH, K_PSD, K_SORT, K_INTERP, K_DENSE, K_FIR)

THRESHOLDS = [0.5, 3.5, 20.5, 100.0, 600.0, 10100.0, 10600.0, 1.0e6]  # counts of a histogram, baseline-subtracted and raw samples, a spectrum
STEP_THRESHOLDS = [100.0 + 50 * k for k in range(8)]  # a producer's: the step (500 at the least) crosses every one, so its row of times is finite
OVER = 100.0
EXTREMA = (15, 15, 0, -1.0e30, 1.0e30)  # a_delta_max, a_delta_min, search_direction, a_abs_max, a_abs_min: any height
BINS, C_BINS, LISTS, LAG, LAYER = 64, 32, 20, 5, 8
LONG_TAPS = 64  # (compiler.STAGE_MIN_TAPS, asserted by the CPU test)
FIR_TOL = 1e-6  # of the row's filtered peak: fir_tile_cases.TOL, the bound of rows with more than float16's 11 significant bits


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
    w, f, bl = rows()
    return {"waveform": w, "waveform_f": f, "bl": bl}


def constants():
    from dspeed_amd.processors import gaussian_filter1d

    rng = np.random.default_rng(0xDB)
    return {"kernel": gaussian_filter1d(F32(1), F32(4), np.empty(9, F32)),
            "weights": (rng.integers(-8, 9, (N, LAYER)) / 64).astype(F32), "bias": rng.integers(-4, 5, LAYER).astype(F32),
            "mean": rng.uniform(9000, 11000, N).astype(F32), "variance": rng.uniform(50, 500, N).astype(F32),
            "long_kernel": rc.asymmetric(LONG_TAPS).astype(F32)}


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
        self.psd_links, self.fir_links = [], []  # (source, spectrum) of every psd; the outputs of a long FIR: held to a bound, not to bits
        self.length = {"waveform": N, "waveform_f": N}
        self.made = {"waveform": "waveform", "waveform_f": "waveform_f"}  # variable -> how it is made from the table

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

    def _link(self, fn, src, outs, lengths, params, model, kernel):
        what = f"{fn}{params}({self._describe(src)})"
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

    def extrema(self, src, prefix="c"):
        names = [f"wf_{prefix}_vmax", f"wf_{prefix}_vmin", f"{prefix}_n_max", f"{prefix}_n_min"]

        def model(x, env):
            res = [xc.model(row, *EXTREMA, LISTS, F32, 1) for row in x]
            return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], dtype=np.uint32),
                    np.array([r[3] for r in res], dtype=np.uint32))

        self.procs[", ".join(names)] = {"function": "get_multi_local_extrema", "module": f"{M}.get_multi_local_extrema",
                                        "args": [src, *EXTREMA, f"{names[0]}({LISTS})", f"{names[1]}({LISTS})", names[2], names[3]]}
        self._link("extrema", src, names, [LISTS, LISTS, None, None], "", model, K_EXTREMA)
        return names

    def multi_thresh(self, src, out="wf_tp", thresholds=THRESHOLDS):
        n, m = self.len_of(src), len(thresholds)
        ts = n // 2
        self.procs[out] = {"function": "multi_time_point_thresh", "module": f"{M}.time_point_thresh",
                           "args": [src, str(thresholds), float(ts), 1, "'l'", f"{out}({m})"]}
        return self._link("multi_time_point_thresh", src, [out], [m], f"[{ts}, {thresholds[0]}..]",
                          lambda x, env: np.stack([tc.model(row, F32(thresholds), ts, 1, "l", F32) for row in x]), K_THRESH)

    def time_over(self, src, out="n_over"):
        self.procs[out] = {"function": "time_over_threshold", "module": f"{M}.time_over_threshold", "args": [src, OVER, out]}
        return self._link("time_over_threshold", src, [out], [None], "",
                          lambda x, env: np.array([tc.model_time_over_threshold(row, OVER, F32) for row in x], dtype=F32), K_THRESH)

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
        return self._link("long_fir", src, [out], [n], "", model, K_FIR)

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
        env = dict(table(), db=constants())
        env["waveform"] = env["waveform"].astype(F32)
        for run in self.links:
            run(env)
        return {o: env[o] for o in self.outputs}, env


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


CONSUMERS = {"reflect": _consume_reflect, "histogram": _consume_histogram, "extrema": _consume_extrema, "thresholds": _consume_thresholds,
             "psd": _consume_psd, "sort": _consume_sort, "interp": _consume_interp, "ml": _consume_ml}
VARIANTS = ("direct", "slice", "blsub")


def _refusal(consumer, n):
    """(the text with which a consumer is refused on a row of ``n`` samples, where it is raised), or (None, None): it takes the row.  The
    filter's and the layer's are raised by ``build_processing_chain``; the peak finder's is the reference body's own check of its arguments,
    raised as a DSPFatal when the stage is planned, at the first ``execute``."""
    if consumer == "reflect" and n < 9:
        return "The filter is longer than the input waveform", "build"
    if consumer == "ml" and n != N:
        return f"dense_layer_with_bias \\(wf_c_y\\): '.*' holds {n} samples, kernel has shape \\({N}, {LAYER}\\)", "build"
    if consumer == "extrema" and n <= LISTS:
        return "The length of your return array must be smaller than the length of your waveform", "execute"
    return None, None


def _pair(producer, consumer, variant):
    add, cut = PRODUCERS[producer]
    r = Recipe(f"{producer}->{consumer}/{variant}", "pair")
    src = {"direct": "waveform", "slice": "waveform_f"}.get(variant) or r.bl_subtract("waveform")
    made = add(r, src)
    if producer == "normalise" and consumer == "ml" and variant != "slice":
        r.kernels.remove(K_DENSE)  # (a normalisation that only a layer reads whole runs inside the layer's launch)
    read = made + (cut if variant == "slice" else "")
    r.refusal, r.refused_at = _refusal(consumer, r.len_of(read))
    CONSUMERS[consumer](r, read)
    return r


def pairs():
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


def cases():
    return pairs() + _between() + _deep() + _long_fir()

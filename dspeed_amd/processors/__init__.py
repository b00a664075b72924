"""Processor registry: the same names as ``dspeed.processors`` (reference processors/__init__.py:66-172) for the
hot-path processors, each a :class:`~dspeed_amd.gufunc.HipGUFunc` with the reference's gufunc layout and type
strings, executed by hand-written HIP kernels through the C ABI.

A dspeed JSON recipe that says ``"module": "dspeed.processors"`` resolves to this module in
``dspeed_amd.processing_chain`` (the reference's own Python never runs on the GPU box).

A regular processor -- rows in, rows or a value per row out -- is one ``_device(...)`` description beside its ``HipGUFunc`` line: the entry
point, the kind of every input after the rows and the shape rule of every output.  The irregular ones have a body of their own inside the
same frame (``device_call``).
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..device import DeviceArray
from ..errors import DSPFatal
from ..gufunc import HipGUFunc, device_call, dtype_of, run


def _split(g, args):
    """Split positional arguments into inputs and (optional) in-place outputs, as NumPy gufuncs do."""
    if len(args) == g.nargs:
        return list(args[: g.nin]), list(args[g.nin:])
    if len(args) == g.nin:
        return list(args), [None] * g.nout
    raise TypeError(f"{g.__name__}() takes {g.nin} inputs and {g.nout} outputs ({len(args)} given)")


def _as_int(v, what):
    a = np.asarray(v)
    if a.size != 1:
        raise NotImplementedError(f"{what}: per-waveform integer parameters are not supported on the device")
    f = float(a.reshape(-1)[0])
    if np.isnan(f):
        raise NotImplementedError(f"{what}: NaN integer parameter")
    return int(f)


def _mode_char(m):
    if isinstance(m, str):
        return ord(m)
    a = np.asarray(m)
    if a.dtype.kind in "SU":
        return ord(str(a.reshape(-1)[0])[0])
    return int(a.reshape(-1)[0])


# --------------------------------------------------------------------------------------------------- the kinds of a '()' input
# each turns the caller's value into the C arguments it stands for
def COL(c, v):
    """one value per row or one for all of them: (device column or NULL, constant)"""
    return c.col(v)


def INT(c, v):
    """an integer constant of the launch (one value per row is taken apart by HipGUFunc before it gets here)"""
    return [_as_int(v, c.what)]


def CONST(c, v):
    """a float constant of the launch"""
    return [float(np.asarray(v).reshape(-1)[0])]


def INT64(c, v):
    return [int(np.asarray(v).reshape(-1)[0])]


def MODE(c, v):
    """a mode character"""
    return [_mode_char(v)]


def HAAR(c, v):
    """the wavelet's name: checked, not passed on"""
    if _mode_char(v) not in (ord("h"), ord("d")):
        raise NotImplementedError("only the Haar wavelet ('h' / 'd' = db1) is implemented")
    return []


def _device(name, ins=(), outs=("n",), must_pass=None, f64_rows_only=False):
    """Implementation of a regular processor from its description: ``dsp_<name>_<loop>`` takes the rows, then what the kinds ``ins`` make
    of the inputs after the rows, then the outputs by their shape rules ``outs`` ("" a value per row, "n" a row like the input's, "m" a row as
    long as the array passed for it).  ``must_pass``: the TypeError text of a processor whose outputs cannot be left out, because their
    length is an argument.  ``f64_rows_only``: the float64 loop takes no int32 / uint32 rows."""

    def impl(g, *args):
        if must_pass is None:
            given, passed = _split(g, args)
        elif len(args) != 1 + len(ins) + len(outs):
            raise TypeError(must_pass)
        else:
            given, passed = args[: 1 + len(ins)], args[1 + len(ins):]
        with device_call(g.__name__, given[0], f64_rows_only) as c:
            cargs = [a for kind, v in zip(ins, given[1:]) for a in kind(c, v)]
            for rule, o in zip(outs, passed):
                cargs += c.out(o, rule)
            return c.launch(name, *c.rows_args, *cargs)

    return impl


# --------------------------------------------------------------------------------------------------- waveform -> waveform
bl_subtract = HipGUFunc("bl_subtract", "(n),()->(n)", ["ff->f", "dd->d"], _device("bl_subtract", [COL]),
                        "w_out = w_in - a_baseline (reference processors/bl_subtract.py:11-46)")
min_max_norm = HipGUFunc("min_max_norm", "(n),(),()->(n)", ["fff->f", "ddd->d"], _device("min_max_norm", [COL, COL]),
                         "waveform over the larger of |a_min|, |a_max| (reference processors/min_max.py:85-140)")
pole_zero = HipGUFunc("pole_zero", "(n),()->(n)", ["ff->f", "dd->d"], _device("pole_zero_col", [COL]),
                      "single pole-zero cancellation (reference processors/pole_zero.py:24-77)")
double_pole_zero = HipGUFunc("double_pole_zero", "(n),(),(),()->(n)", ["ffff->f", "dddd->d"], _device("double_pole_zero_col", [COL, COL, COL]),
                             "double pole-zero cancellation (reference processors/pole_zero.py:82-198)")
trap_filter = HipGUFunc("trap_filter", "(n),(),()->(n)", ["fii->f", "dii->d"], _device("trap_filter", [INT, INT]),
                        "symmetric trapezoidal filter (reference processors/trap_filters.py:12-76)")
trap_norm = HipGUFunc("trap_norm", "(n),(),()->(n)", ["fii->f", "dii->d"], _device("trap_norm", [INT, INT]),
                      "normalised trapezoidal filter (reference processors/trap_filters.py:79-149)")
asym_trap_filter = HipGUFunc("asym_trap_filter", "(n),(),(),()->(n)", ["fiii->f", "diii->d"], _device("asym_trap_filter", [INT, INT, INT]),
                             "asymmetric trapezoidal filter (reference processors/trap_filters.py:152-227)")


# --------------------------------------------------------------------------------------------------- waveform -> scalars
def _constant_of_call(v, what, name):
    a = np.asarray(v)
    if a.size != 1:
        raise NotImplementedError(f"{what}: {name} is a constant of the call on the device, not a per-event value")
    return a.reshape(-1)[0]


def _multi_time_point_thresh(g, *args):
    ins, outs = _split(g, args)
    w_in, a_threshold, t_start, polarity, mode_in = ins
    what = g.__name__
    # polarity and mode are constants, checked for every row (the reference raises on the rows that get that far)
    pol = float(_constant_of_call(polarity, what, "polarity"))
    if not (pol > 0 or pol < 0):
        raise DSPFatal("polarity cannot be 0")
    mode = _mode_char(_constant_of_call(mode_in, what, "mode_in"))
    if not 0 < mode < 128 or chr(mode) not in "iafbcrnl":
        raise DSPFatal("Unrecognized interpolation mode")
    with device_call(what, w_in, f64_rows_only=True) as c:
        if isinstance(a_threshold, DeviceArray):
            if a_threshold.dtype != np.dtype(c.ft):
                raise TypeError(f"{what}: thresholds on the device have the loop's type, {np.dtype(c.ft)}")
            thr, shape = a_threshold, tuple(a_threshold.shape)
        else:
            host = np.ascontiguousarray(np.asarray(a_threshold), dtype=c.ft)
            shape = host.shape
            thr = None
        if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] != c.n_wf):
            raise ValueError(f"{what}: a_threshold has shape {shape}, expected (m,) or ({c.n_wf}, m)")
        m = int(shape[-1])
        if m > _lib.THRESH_MAX:
            raise NotImplementedError(f"{what}: at most {_lib.THRESH_MAX} thresholds ({m} given): a wavefront keeps one per lane")
        oshape = (m,) if c.one_d else (c.n_wf, m)
        if m == 0:
            return outs[0] if outs[0] is not None else np.empty(oshape, dtype=c.ft)
        if thr is None:
            thr = DeviceArray.from_numpy(host)
            c.st.keep.append(thr)
        tp, tv = c.col(t_start)
        optr, res = c.st.out(outs[0], oshape, c.ft)
        c.results.append(res)
        return c.launch("multi_time_point_thresh", *c.rows_args, thr.ptr, m, m if len(shape) == 2 else 0, tp, tv, pol, mode, optr, m)


fixed_time_pickoff = HipGUFunc("fixed_time_pickoff", "(n),(),()->()", ["ffb->f", "ddb->d"], _device("fixed_time_pickoff", [COL, MODE], [""]),
                               "value at a (fractional) sample index, modes i n f c l h (reference processors/fixed_time_pickoff.py:12-125)")
time_point_thresh = HipGUFunc("time_point_thresh", "(n),(),(),()->()", ["ffff->f", "dddd->d"], _device("time_point_thresh", [COL, COL, CONST], [""]),
                              "first threshold crossing walking forward/backward (reference processors/time_point_thresh.py:12-92)")
interpolated_time_point_thresh = HipGUFunc("interpolated_time_point_thresh", "(n),(),(),(),()->()", ["ffflb->f", "dddlb->d"],
                                           _device("interpolated_time_point_thresh", [COL, COL, INT64, MODE], [""]),
                                           "threshold crossing placed between samples, modes i b c a f r n l (reference processors/time_point_thresh.py:95-222)")
multi_time_point_thresh = HipGUFunc("multi_time_point_thresh", "(n),(m),(),(),()->(m)", ["ffffb->f", "ddddb->d"], _multi_time_point_thresh,
                                    "the times at which a row crosses m thresholds (m <= 64), found from one starting sample: upwards with the polarity, "
                                    "downwards against it; modes i a f b c r n l; polarity and mode are constants of the call "
                                    "(reference processors/time_point_thresh.py:225-401)")
time_over_threshold = HipGUFunc("time_over_threshold", "(n),()->()", ["ff->f", "dd->d"], _device("time_over_threshold", [COL], [""], f64_rows_only=True),
                                "the number of samples above a threshold (reference processors/time_over_threshold.py:11-48)")
linear_slope_fit = HipGUFunc("linear_slope_fit", "(n)->(),(),(),()", ["f->ffff", "d->dddd"], _device("linear_slope_fit", [], ["", "", "", ""]),
                             "Welford mean / standard deviation and least-squares slope / intercept (reference processors/linear_slope_fit.py:11-91)")
mean_below_threshold = HipGUFunc("mean_below_threshold", "(n),()->()", ["ff->f", "dd->d"], _device("mean_below_threshold", [COL], [""]),
                                 "mean of the samples below a threshold (reference processors/arithmetic.py:9-62)")
min_max = HipGUFunc("min_max", "(n)->(),(),(),()", ["f->ffff", "d->dddd"], _device("min_max", [], ["", "", "", ""]),
                    "first-occurrence argmin/argmax and values (reference processors/min_max.py:11-82)")


# --------------------------------------------------------------------------------------------------- '(n),...,(m)' in-place outputs
def _get_multi_local_extrema(g, *args):
    if len(args) not in (8, 10):
        raise TypeError("get_multi_local_extrema(w_in, a_delta_max_in, a_delta_min_in, search_direction, a_abs_max_in, a_abs_min_in, vt_max_out, "
                        "vt_min_out[, n_max_out, n_min_out]): vt_max_out and vt_min_out must be passed (their length is the number of extrema kept)")
    w_in, d_max, d_min, direction, a_max, a_min, vt_max, vt_min = args[:8]
    n_max, n_min = args[8:] if len(args) == 10 else (None, None)
    with device_call(g.__name__, w_in) as c:
        m = vt_max.shape[-1]
        if vt_min.shape[-1] != m:
            raise ValueError("get_multi_local_extrema: vt_max_out and vt_min_out share the dimension m")
        cols = [c.col(v) for v in (d_max, d_min, a_max, a_min)]
        pmax, pmin = c.out(vt_max, "m")[0], c.out(vt_min, "m")[0]
        pnmax, pnmin = c.out(n_max, "", np.uint32)[0], c.out(n_min, "", np.uint32)[0]
        return c.launch("get_multi_local_extrema", *c.rows_args, *cols[0], *cols[1], _as_int(direction, g.__name__), *cols[2], *cols[3],
                        pmax, pmin, m, m, pnmax, pnmin)


def _histogram_stats(g, *args):
    if len(args) != 6:
        raise TypeError("histogram_stats(weights_in, edges_in, mode_out, max_out, fwhm_out, max_in): the three outputs stand in the middle, "
                        "as in the reference; pass None to have them allocated")
    weights, edges, mode_out, max_out, fwhm_out, max_in = args
    with device_call(g.__name__) as c:
        if np.dtype(dtype_of(weights)) not in (np.dtype(np.float32), np.dtype(np.float64)) or dtype_of(edges) != dtype_of(weights):
            raise TypeError("histogram_stats: weights_in and edges_in are float32 (the float32 loop) or float64 rows of one type")
        c.rows(weights)
        pe, _, n_e, p, e_stride, _ = c.st.wf_in(edges)
        if n_e != c.n_wf:
            raise ValueError("histogram_stats: weights_in and edges_in hold the same number of rows")
        col = c.col(max_in)
        outs = [c.out(o)[0] for o in (mode_out, max_out, fwhm_out)]
        return c.launch("histogram_stats", c.ptr, c.n_wf, c.n, c.stride, pe, p, e_stride, *col, *outs)


def _convolve(g, *args):
    if len(args) != 4:
        raise TypeError(f"{g.__name__}(w_in, kernel, mode_in, w_out): w_out must be passed (its length selects the output size)")
    w_in, kernel, mode_in, w_out = args
    with device_call(g.__name__, w_in) as c:
        if isinstance(kernel, DeviceArray):
            kd = kernel
        else:
            k = np.ascontiguousarray(kernel, dtype=c.ft)
            if k.ndim != 1:
                raise NotImplementedError("per-waveform kernels are not supported")
            kd = DeviceArray.from_numpy(k)
            c.st.keep.append(kd)
        out = c.out(w_out, "m")
        return c.launch("convolve_wf", *c.rows_args, kd.ptr, kd.shape[-1], _mode_char(mode_in), *out)


discrete_wavelet_transform = HipGUFunc("discrete_wavelet_transform", "(n),(),(),(),(m)", ["fibbf", "dlbbd"],
                                       _device("dwt_haar", [INT, HAAR, MODE], ["m"], must_pass="discrete_wavelet_transform(w_in, level, wave_type, coeff, w_out): "
                                               "w_out must be passed (its length is the output size)"),
                                       "Haar DWT approximation/detail coefficients (reference processors/dwt.py:13-81)")
convolve_wf = HipGUFunc("convolve_wf", "(n),(m),(),(p)", ["ffbf", "ddbd"], _convolve,
                        "FIR filter, np.convolve semantics, modes f v s (reference processors/convolutions.py:14-72)")
fft_convolve_wf = HipGUFunc("fft_convolve_wf", "(n),(m),(),(p)", ["ffbf", "ddbd"], _convolve,
                            "same filter as convolve_wf (the reference routes it through scipy fftconvolve, "
                            "processors/convolutions.py:75-119); evaluated in direct form on the device")


# --------------------------------------------------------------------------------------------------- kernel generators (host, run once)
def _check_kernel_params(sigma, flat, decay):
    # messages and order: reference processors/energy_kernels.py:51-61 / :115-125
    if sigma < 0:
        raise DSPFatal("The curvature parameter must be positive")
    if flat < 0:
        raise DSPFatal("The length of the flat section must be positive")
    if np.floor(flat) != flat:
        raise DSPFatal("The length of the flat section must be an integer")
    if decay < 0:
        raise DSPFatal("The decay constant must be positive")


def _scalar_for(kernel, v):
    # the reference's object-mode gufunc boxes float32 scalars into Python floats carrying the float32 value
    return float(np.float32(v)) if kernel.dtype == np.float32 else float(v)


def _cusp_shape(length, sigma, flat):
    """float64 cusp with flat top: sinh(i/sigma)/sinh(lt/sigma) rising, 1 on [lt, lt+flat], mirrored falling edge."""
    lt = int((length - flat) / 2)
    fl = int(flat)
    ind = np.arange(length, dtype=np.float64)
    cusp = np.zeros(length, dtype=np.float64)
    den = np.sinh(lt / sigma)
    cusp[:lt] = np.sinh(ind[:lt] / sigma) / den
    cusp[lt: lt + fl + 1] = 1.0
    cusp[lt + fl + 1:] = np.sinh((length - ind[lt + fl + 1:]) / sigma) / den
    return cusp, lt, fl


def _cusp_filter(g, sigma, flat, decay, kernel):
    sigma, flat, decay = (_scalar_for(kernel, v) for v in (sigma, flat, decay))
    _check_kernel_params(sigma, flat, decay)
    n = len(kernel)
    cusp, _, _ = _cusp_shape(n, sigma, flat)
    k = cusp.astype(kernel.dtype)  # the reference builds the cusp inside the output array (energy_kernels.py:63-70)
    kernel[:] = np.convolve(k, [1, -np.exp(-1 / decay)], "same")
    return kernel


def _zac_filter(g, sigma, flat, decay, kernel):
    sigma, flat, decay = (_scalar_for(kernel, v) for v in (sigma, flat, decay))
    _check_kernel_params(sigma, flat, decay)
    n = len(kernel)
    cusp, lt, fl = _cusp_shape(n, sigma, flat)
    ind = np.arange(n, dtype=np.float64)
    par = np.zeros(n, dtype=np.float64)
    par[:lt] = np.power(ind[:lt] - lt / 2, 2) - np.power(lt / 2, 2)
    par[lt + fl + 1:] = np.power(n - ind[lt + fl + 1:] - lt / 2, 2) - np.power(lt / 2, 2)
    areapar = areacusp = 0.0
    for a, b in zip(par.tolist(), cusp.tolist()):  # sequential sums, as the reference accumulates them (energy_kernels.py:146-149)
        areapar += a
        areacusp += b
    zac = cusp + (-par / areapar * areacusp)
    kernel[:] = np.convolve(zac, [1, -np.exp(-1 / decay)], "same")
    return kernel


windower = HipGUFunc("windower", "(n),(),(m)", ["fff", "ddd"],
                     _device("windower", [COL], ["m"], must_pass="windower(w_in, t0_in, w_out): w_out must be passed (its length is the window size)"),
                     "window of len(w_out) samples starting at int(t0_in), NaN outside the input (reference processors/windower.py:12-54)")
get_multi_local_extrema = HipGUFunc("get_multi_local_extrema", "(n),(),(),(),(),(),(m),(m),(),()", ["ffffffffII", "ddddddddII"], _get_multi_local_extrema,
                                    "lists of the local maxima and minima, len(vt_max_out) of each at most, NaN-padded, and their counts; search_direction 0, 1 "
                                    "or 3 (reference processors/get_multi_local_extrema.py:12-306)")
histogram = HipGUFunc("histogram", "(n),(m),(p)", ["fff", "ddd"],
                      _device("histogram", [], ["m", "m"], f64_rows_only=True,
                              must_pass="histogram(w_in, weights_out, borders_out): both outputs must be passed (len(weights_out) is the number of bins)"),
                      "histogram of the row between its extremes: len(weights_out) bins, len(weights_out) + 1 borders; the maximum is not counted "
                      "(reference processors/histogram.py:14-89)")
histogram_stats = HipGUFunc("histogram_stats", "(n),(m),(),(),(),()", ["ffffff", "dddddd"], _histogram_stats,
                            "index and left edge of a histogram's mode (or of the edge nearest max_in) and the half width at half maximum "
                            "(reference processors/histogram_stats.py:157-261)")
avg_current = HipGUFunc("avg_current", "(n),(),(m)", ["fff", "ddd"],
                        _device("avg_current", [CONST], ["m"], must_pass="avg_current(w_in, length, w_out): w_out must be passed (len(w_in) - int(length) samples)"),
                        "(w_in[L:] - w_in[:-L]) / length (reference processors/moving_windows.py:206-249)")
upsampler = HipGUFunc("upsampler", "(n),(),(m)", ["fff", "ddd"],
                      _device("upsampler", [CONST], ["m"], must_pass="upsampler(w_in, upsample, w_out): w_out must be passed (its length is the output size)"),
                      "every sample repeated int(upsample) times (reference processors/upsampler.py:13-56)")
moving_window_multi = HipGUFunc("moving_window_multi", "(n),(),(),()->(n)", ["fffi->f", "dddi->d"], _device("moving_window_multi", [CONST, CONST, INT]),
                                "moving averages applied alternately from the left and the right (reference processors/moving_windows.py:117-204)")
trap_pickoff = HipGUFunc("trap_pickoff", "(n),(),(),()->()", ["fiif->f", "diid->d"], _device("trap_pickoff", [INT, INT, COL], [""]),
                         "normalised difference of two rise-long window sums at an integer pick-off sample (reference processors/trap_filters.py:230-293)")
def _t0_filter(g, rise, fall, kernel):
    """t0 kernel: a ramp of weights 2 (r - i) / (r (r + 1)), i = 0 .. r - 1 (they sum to 1), followed by the plateau -1 / fall.
    Evaluated in float64 and rounded once into the kernel (the reference's generator runs in object mode on Python floats,
    processors/kernels.py:12-61); the three parameter checks keep the reference's order and texts."""
    rise, fall = _scalar_for(kernel, rise), _scalar_for(kernel, fall)
    for value, what in ((rise, "rise"), (fall, "fall")):
        if value < 0:
            raise DSPFatal(f"The length of the {what} section must be positive")
    if len(kernel) != rise + fall:
        raise DSPFatal("The length of the output kernel must equal rise+fall")
    r = int(rise)
    if r > 0:
        ramp = 2.0 * np.arange(r, 0, -1, dtype=np.float64)  # 2 (r - i): exact integers
        kernel[:r] = ramp / (rise * (rise + 1))
    if len(kernel) > r:  # (an empty section divides by nothing)
        kernel[r:] = -1.0 / fall
    return kernel


def _moving_slope(g, kernel):
    """Least-squares slope of n equidistant samples as FIR weights, w_j = (n j - S1) / (n S2 - S1^2) for j = n .. 1 (the order a
    convolution wants), S1 = sum j, S2 = sum j^2.  Numerator and denominator are rounded to the kernel's type before the division,
    which is where the reference's in-place array arithmetic rounds (processors/kernels.py:69-100)."""
    n = len(kernel)
    s1 = n * (n + 1) / 2
    s2 = n * (n + 1) * (2 * n + 1) / 6
    numer = (n * np.arange(n, 0, -1, dtype=np.float64) - s1).astype(kernel.dtype)
    kernel[:] = numer / kernel.dtype.type(n * s2 - s1 * s1)
    return kernel


t0_filter = HipGUFunc("t0_filter", "(),(),(n)", ["fff", "ddd"], _t0_filter,
                      "t0 kernel generator (asymmetric trapezoid weights), host, once (reference processors/kernels.py:12-66)")
moving_slope = HipGUFunc("moving_slope", "(n)", ["f", "d"], _moving_slope,
                         "moving-slope kernel generator, host, once (reference processors/kernels.py:69-98)")
cusp_filter = HipGUFunc("cusp_filter", "(),(),(),(n)", ["ffff", "dddd"], _cusp_filter,
                        "CUSP kernel generator, evaluated once on the host at chain build (reference processors/energy_kernels.py:12-73)")
zac_filter = HipGUFunc("zac_filter", "(),(),(),(n)", ["ffff", "dddd"], _zac_filter,
                       "zero-area CUSP kernel generator, host, once (reference processors/energy_kernels.py:76-157)")

# --------------------------------------------------------------------------------------------------- spectra
def spectrum_limits(loop_dtype):
    """(longest power-of-two row, longest row of any other length) of psd / fft in a loop: the transform lives in 64 KiB of LDS"""
    half = 2 if np.dtype(loop_dtype) == np.dtype(np.float64) else 1
    return _lib.SPECTRUM_F32_POW2_MAX // half, _lib.SPECTRUM_F32_ANY_MAX // half


def check_spectrum_length(what, n, loop_dtype):
    pow2_max, any_max = spectrum_limits(loop_dtype)
    if n > (pow2_max if n & (n - 1) == 0 else any_max):
        raise NotImplementedError(f"{what}: the {np.dtype(loop_dtype).name} loop takes rows of a power of two up to {pow2_max} samples and of any other "
                                  f"length up to {any_max} ({n} given): a row's transform lives in 64 KiB of LDS")


def _spectrum(complex_out):
    """psd / fft: one C entry for both loops (``dsp_psd`` / ``dsp_fft`` take the loop's type).  fft's output is complex64 / complex128 to the
    caller and (re, im) pairs of the loop's type to the device: the same bytes."""

    def impl(g, *args):
        name = g.__name__
        if len(args) != 2 or args[1] is None:
            raise TypeError(f"{name}(w_in, {name}_out): {name}_out must be passed (len(w_in)//2 + 1 bins)")
        w_in, out = args
        with device_call(name, w_in, f64_rows_only=True) as c:
            m = c.n // 2 + 1
            ct = np.dtype(np.complex64 if c.ft is np.float32 else np.complex128) if complex_out else np.dtype(c.ft)
            if not isinstance(out, (np.ndarray, DeviceArray)):
                raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
            if out.shape[-1] != m:
                raise DSPFatal(f"Size of {name} must be len(w_in)//2+1 = {m}")
            if np.dtype(out.dtype) != ct:
                raise TypeError(f"{name}: {name}_out is {ct.name} in the {np.dtype(c.ft).name} loop ({np.dtype(out.dtype).name} given)")
            check_spectrum_length(name, c.n, c.ft)
            ptr, res = c.st.out(out, (m,) if c.one_d else (c.n_wf, m), ct)
            c.results.append(res)
            width = 2 * m if complex_out else m
            run(getattr(_lib.lib(), f"dsp_{name}"), name, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, ptr, m, width)
            c.st.finish()
            return res

    return impl


psd = HipGUFunc("psd", "(n),(m)", ["ff", "dd"], _spectrum(False),
                "power spectrum (re^2 + im^2) / n of a real row, len(w_in)//2 + 1 bins; a row with a NaN or an infinity: NaN bins "
                "(reference processors/fft.py:92-126)")
fft = HipGUFunc("fft", "(n),(m)", ["fF", "dD"], _spectrum(True),
                "spectrum of a real row, NumPy's rfft: len(w_in)//2 + 1 complex bins; a row with a NaN or an infinity: bins NaN + 0j "
                "(reference processors/fft.py:12-46)")

# The spectral processors are attributes of this module -- "module": "dspeed.processors" resolves them -- and are listed here, not in
# __all__: tests/test_gufunc_calls_cpu.py holds a call record for every name of __all__, and these two have theirs in a file of their own
# (tests/test_spectrum_plan_cpu.py).
SPECTRAL = ("fft", "psd")


# --------------------------------------------------------------------------------------------------- order statistics
def sort_limit(loop_dtype):
    """longest row of sort in a loop: the row's keys live in 64 KiB of LDS"""
    return _lib.SORT_F32_MAX // (2 if np.dtype(loop_dtype) == np.dtype(np.float64) else 1)


def check_sort_length(what, n, loop_dtype):
    """(both limits are named whichever loop runs: the planner's text)"""
    if n > sort_limit(loop_dtype):
        raise NotImplementedError(f"{what}: rows of up to {_lib.SORT_F32_MAX} samples in the float32 loop and {_lib.SORT_F32_MAX // 2} in the float64 loop "
                                  f"({n} given): a row's keys live in 64 KiB of LDS")


def _sort(g, *args):
    """one C entry for both loops, like psd's (``dsp_sort_rows`` takes the loop's type); the output may be left out"""
    (w_in,), (out,) = _split(g, args)
    with device_call(g.__name__, w_in, f64_rows_only=True) as c:
        check_sort_length(g.__name__, c.n, c.ft)
        ptr, stride = c.out(out, "n")
        run(getattr(_lib.lib(), "dsp_sort_rows"), g.__name__, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, ptr, stride)
        c.st.finish()
        return c.results[0]


sort = HipGUFunc("sort", "(n)->(n)", ["f->f", "d->d"], _sort,
                 "rows in ascending order, -inf first and +inf last, -0.0 before +0.0; a row with a NaN: NaNs (reference processors/sort.py:10-42)")

# Listed here and not in __all__, like the spectral processors: its call record is tests/test_sort_plan_cpu.py's.
ORDER = ("sort",)


# --------------------------------------------------------------------------------------------------- resampling
INTERP_MODES = "infclhs"


def interp_limit(mode, loop_dtype):
    """longest row of interpolating_upsampler in a mode and loop: the row (and the spline's second derivatives) live in 64 KiB of LDS"""
    f64 = np.dtype(loop_dtype) == np.dtype(np.float64)
    if mode == "s":
        return _lib.INTERP_SPLINE_F64_MAX if f64 else _lib.INTERP_SPLINE_F32_MAX
    return _lib.INTERP_F32_MAX // (2 if f64 else 1)


def check_interp(what, mode, n, m, loop_dtype):
    """what the planner checks, in its words (and the reference's, where it has them): ``mode`` is the character's code"""
    if not 0 < mode < 128 or chr(mode) not in INTERP_MODES:
        raise DSPFatal("Unrecognized interpolation mode")
    mode = chr(mode)
    if m < 1:
        raise ValueError(f"{what}: the output holds at least one sample ({m} given)")
    if mode == "i" and m % n:
        raise DSPFatal("interpolating_upsampler requires len(w_out) to be an integer multiple of len(w_in) for mode 'i'")
    if mode == "h" and n < 2:
        raise NotImplementedError(f"{what}: mode 'h' takes rows of at least 2 samples ({n} given): the reference reads an unbound variable there")
    if n > interp_limit(mode, loop_dtype):
        if mode == "s":
            raise NotImplementedError(f"{what}: mode 's' takes rows of up to {_lib.INTERP_SPLINE_F32_MAX} samples in the float32 loop and "
                                      f"{_lib.INTERP_SPLINE_F64_MAX} in the float64 loop ({n} given): the row and its second derivatives live in 64 KiB of LDS")
        raise NotImplementedError(f"{what}: rows of up to {_lib.INTERP_F32_MAX} samples in the float32 loop and {_lib.INTERP_F32_MAX // 2} in the float64 loop "
                                  f"({n} given): a row lives in 64 KiB of LDS")


def _interpolating_upsampler(g, *args):
    """one C entry for both loops, like psd's (``dsp_interp_upsample_rows`` takes the loop's type).  The mode is a constant of the call,
    checked here for every row (the reference raises on the rows that get that far)."""
    what = g.__name__
    if len(args) != 3 or args[2] is None:
        raise TypeError(f"{what}(w_in, mode_in, w_out): w_out must be passed (its length is the output size)")
    w_in, mode_in, w_out = args
    mode = _mode_char(_constant_of_call(mode_in, what, "mode_in"))
    with device_call(what, w_in, f64_rows_only=True) as c:
        if not isinstance(w_out, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
        if np.dtype(w_out.dtype) != np.dtype(c.ft):
            raise TypeError(f"{what}: w_out is {np.dtype(c.ft).name} in the {np.dtype(c.ft).name} loop ({np.dtype(w_out.dtype).name} given)")
        m = int(w_out.shape[-1]) if len(w_out.shape) else 0
        check_interp(what, mode, c.n, m, c.ft)
        ptr, res = c.st.out(w_out, (m,) if c.one_d else (c.n_wf, m), c.ft)
        c.results.append(res)
        run(getattr(_lib.lib(), "dsp_interp_upsample_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, mode, ptr, m, m)
        c.st.finish()
        return res


interpolating_upsampler = HipGUFunc("interpolating_upsampler", "(n),(),(m)", ["fbf", "dbd"], _interpolating_upsampler,
                                    "the row resampled to len(w_out) samples: 'i' zero-stuffing, 'n' nearest, 'f' floor, 'c' ceiling, 'l' linear, 'h' Hermite "
                                    "cubic, 's' natural cubic spline; a row with a NaN: NaNs (reference processors/upsampler.py:52-216)")

# Listed here and not in __all__, like the spectral processors and sort: its call record is tests/test_interp_plan_cpu.py's.
RESAMPLING = ("interpolating_upsampler",)


# --------------------------------------------------------------------------------------------------- neural-network layers
ML_ACTIVATIONS = "srlmt"  # sigmoid, relu, leaky relu, softplus ("softmax" in the reference), tanh; any other character: NaN outputs, no error
DENSE_LIMITS = f"layers of up to {_lib.DENSE_N_MAX} inputs and {_lib.DENSE_M_MAX} outputs"  # (DSP_DENSE_LIMITS_TEXT, dsp_program.h)


def check_dense(what, n, m):
    """what the planner checks, in its words"""
    if n > _lib.DENSE_N_MAX or m > _lib.DENSE_M_MAX:
        raise NotImplementedError(f"{what}: {DENSE_LIMITS} (n = {n}, m = {m} given)")


def _layer_constant(c, v, what, name):
    """weights, bias, means or variances: one constant array for every row, on the device in the loop's type -> (DeviceArray, shape)"""
    if isinstance(v, DeviceArray):
        if v.dtype != np.dtype(c.ft):
            raise TypeError(f"{what}: {name} on the device has the loop's type, {np.dtype(c.ft)}")
        return v, tuple(v.shape)
    host = np.ascontiguousarray(np.asarray(v), dtype=c.ft)
    if host.size < 1:
        raise ValueError(f"{what}: {name} is empty")
    d = DeviceArray.from_numpy(host if host.ndim else host.reshape(1))
    c.st.keep.append(d)
    return d, host.shape


def _dense(classify, with_bias):
    """dense_layer_* (an (n, m) kernel, m outputs a row) and classification_layer_* (an (n) kernel, one value a row): one C entry for both
    loops, ``dsp_dense_rows``.  Kernel and bias are constants of the call; so is the activation."""

    def impl(g, *args):
        what = g.__name__
        ins, outs = _split(g, args)
        w_in, kernel, bias = ins[0], ins[1], ins[2] if with_bias else None
        act = _mode_char(_constant_of_call(ins[-1], what, "activation_func"))
        with device_call(what, w_in, f64_rows_only=True) as c:
            wd, wshape = _layer_constant(c, kernel, what, "kernel")
            if classify:
                if wshape not in ((c.n,), (c.n, 1)):
                    raise ValueError(f"{what}: kernel has shape {wshape}, expected ({c.n},)")
                m = 1
            else:
                if len(wshape) != 2 or wshape[0] != c.n:
                    raise ValueError(f"{what}: kernel has shape {wshape}, expected ({c.n}, m)")
                m = int(wshape[1])
            check_dense(what, c.n, m)
            bptr = None
            if with_bias:
                bd, bshape = _layer_constant(c, bias, what, "bias")
                if int(np.prod(bshape)) != m or len(bshape) > 1:
                    raise (NotImplementedError(f"{what}: bias is a constant of the call on the device, not a per-event value") if classify else
                           ValueError(f"{what}: bias has shape {bshape}, expected ({m},)"))
                bptr = bd.ptr
            shape = () if classify else (m,)
            ptr, res = c.st.out(outs[0], shape if c.one_d else (c.n_wf, *shape), c.ft)
            run(getattr(_lib.lib(), "dsp_dense_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, wd.ptr, bptr, act, ptr,
                0 if classify else m, m)
            c.st.finish()
            return res[()] if isinstance(res, np.ndarray) and res.ndim == 0 else res

    return impl


def _normalisation_layer(g, *args):
    what = g.__name__
    (w_in, means, variances), outs = _split(g, args)
    with device_call(what, w_in, f64_rows_only=True) as c:
        check_dense(what, c.n, 1)
        consts = []
        for v, name in ((means, "means"), (variances, "variances")):
            d, shape = _layer_constant(c, v, what, name)
            if shape != (c.n,):
                raise ValueError(f"{what}: {name} has shape {shape}, expected ({c.n},)")
            consts.append(d.ptr)
        ptr, res = c.st.out(outs[0], (c.n,) if c.one_d else (c.n_wf, c.n), c.ft)
        run(getattr(_lib.lib(), "dsp_normalisation_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, *consts, ptr, c.n)
        c.st.finish()
        return res


_LAYER_DOC = ("activation(x_in . kernel{}) on the matrix cores, one fused multiply-add chain per output in ascending k; activations s r l m t as the "
              "reference writes them, any other character: NaN outputs; a row with a NaN: NaN outputs (reference processors/ml.py:{})")
normalisation_layer = HipGUFunc("normalisation_layer", "(n),(n),(n)->(n)", ["fff->f", "ddd->d"], _normalisation_layer,
                                "(x_in - means) / sqrt(variances), every step in the loop's type (reference processors/ml.py:349-390)")
dense_layer_no_bias = HipGUFunc("dense_layer_no_bias", "(n),(n,m),()->(m)", ["ffb->f", "ddb->d"], _dense(False, False), _LAYER_DOC.format("", "83-141"))
dense_layer_with_bias = HipGUFunc("dense_layer_with_bias", "(n),(n,m),(m),()->(m)", ["fffb->f", "dddb->d"], _dense(False, True),
                                  _LAYER_DOC.format(" + bias", "144-209"))
classification_layer_no_bias = HipGUFunc("classification_layer_no_bias", "(n),(n),()->()", ["ffb->f", "ddb->d"], _dense(True, False),
                                         _LAYER_DOC.format("", "212-274").replace("per output", "per row"))
classification_layer_with_bias = HipGUFunc("classification_layer_with_bias", "(n),(n),(),()->()", ["fffb->f", "dddb->d"], _dense(True, True),
                                           _LAYER_DOC.format(" + bias", "277-346").replace("per output", "per row"))

# Listed here and not in __all__, like the spectral processors, sort and the resampler: their call records are tests/test_ml_plan_cpu.py's.
ML = ("normalisation_layer", "dense_layer_no_bias", "dense_layer_with_bias", "classification_layer_no_bias", "classification_layer_with_bias")


# --------------------------------------------------------------------------------------------------- smoothing
def reflect_limit(loop_dtype):
    """longest staged row of reflected_convolve_wf in a loop, len(w_in) + len(kernel) - 1: the row and its mirrored margins live in 64 KiB of LDS"""
    return _lib.REFLECT_F64_MAX if np.dtype(loop_dtype) == np.dtype(np.float64) else _lib.REFLECT_F32_MAX


def check_reflect(what, n, m, loop_dtype):
    """what the planner checks, in its words (and the reference's, where it has them).  A kernel longer than the rows is refused for the
    whole call, even where every row holds a NaN (the reference raises on the rows that get that far)."""
    if m < 1:
        raise ValueError(f"{what}: the kernel holds at least one tap ({m} given)")
    if m > n:
        raise DSPFatal("The filter is longer than the input waveform")
    if n + m - 1 > reflect_limit(loop_dtype):
        raise NotImplementedError(f"{what}: len(w_in) + len(kernel) - 1 of up to {_lib.REFLECT_F32_MAX} in the float32 loop and {_lib.REFLECT_F64_MAX} in the "
                                  f"float64 loop (len(w_in) = {n}, len(kernel) = {m} given): a row and its mirrored margins live in 64 KiB of LDS")


def _reflected_convolve_wf(g, *args):
    """one C entry for both loops, like psd's (``dsp_reflected_convolve_rows`` takes the loop's type).  The kernel is one constant array for
    all rows, handled as convolve_wf's; ``w_out`` may be left out: its length is the input's."""
    what = g.__name__
    if len(args) not in (2, 3):
        raise TypeError(f"{what}(w_in, kernel[, w_out]) takes 2 or 3 arguments ({len(args)} given)")
    w_in, kernel = args[:2]
    w_out = args[2] if len(args) == 3 else None
    with device_call(what, w_in, f64_rows_only=True) as c:
        if isinstance(kernel, DeviceArray):
            if np.dtype(kernel.dtype) != np.dtype(c.ft) or len(kernel.shape) != 1:
                raise TypeError(f"{what}: a kernel on the device is one row of {np.dtype(c.ft).name} values in the {np.dtype(c.ft).name} loop")
            kd = kernel
        else:
            k = np.ascontiguousarray(kernel, dtype=c.ft)
            if k.ndim != 1:
                raise NotImplementedError("per-waveform kernels are not supported")
            kd = DeviceArray.from_numpy(k) if k.size else None
            if kd is not None:
                c.st.keep.append(kd)
        m = int(kd.shape[-1]) if kd is not None else 0
        if w_out is not None:
            if not isinstance(w_out, (np.ndarray, DeviceArray)):
                raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
            p = int(w_out.shape[-1]) if len(w_out.shape) else 0
            if p != c.n:
                raise ValueError(f"{what}: the output has the length of the input (len(w_in) = {c.n}, len(w_out) = {p})")
        check_reflect(what, c.n, m, c.ft)
        ptr, stride = c.out(w_out, "n")
        run(getattr(_lib.lib(), "dsp_reflected_convolve_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, kd.ptr, m, ptr, stride)
        c.st.finish()
        return c.results[0]


reflected_convolve_wf = HipGUFunc("reflected_convolve_wf", "(n),(m),(p)", ["fff", "ddd"], _reflected_convolve_wf,
                                  "FIR filter with mirrored edges: np.convolve of the row padded by reflection, cut back to len(w_in) samples; float64 "
                                  "accumulators; a row or a kernel with a NaN: NaNs (reference processors/convolutions.py:122-182)")


def _gaussian_filter1d(g, sigma, truncate, weights):
    """Gaussian weights exp(-x^2 / (2 sigma^2)) over x = -lw .. lw, lw = int(truncate * sigma + 0.5), normalised to sum 1: evaluated in
    float64 and rounded once into the array (the reference's generator runs in object mode on Python floats,
    processors/gaussian_filter1d.py:56-82).  Stricter than the reference in two places: it fails in NumPy's broadcast when the array has
    another length than 2 lw + 1, and divides by zero for sigma == 0."""
    sigma, truncate = _scalar_for(weights, sigma), _scalar_for(weights, truncate)
    if not sigma > 0:
        raise ValueError(f"gaussian_filter1d: sigma must be positive ({sigma} given)")
    lw = int(truncate * sigma + 0.5)
    if len(weights) != 2 * lw + 1:
        raise ValueError(f"gaussian_filter1d: weights holds 2 * int(truncate * sigma + 0.5) + 1 = {2 * lw + 1} values ({len(weights)} given)")
    x = np.arange(-lw, lw + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x**2)
    weights[:] = phi / phi.sum()
    return weights


gaussian_filter1d = HipGUFunc("gaussian_filter1d", "(),(),(n)", ["fff", "ddd"], _gaussian_filter1d,
                              "Gaussian kernel generator for reflected_convolve_wf, host, once (reference processors/gaussian_filter1d.py:56-82)")

# Listed here and not in __all__, like the spectral processors and sort: their call records are tests/test_reflect_plan_cpu.py's.
SMOOTHING = ("reflected_convolve_wf", "gaussian_filter1d")


# --------------------------------------------------------------------------------------------------- pile-up
def check_rc_cr2(what, n, m=None):
    """what the planner checks, in the reference's words where it has them"""
    if n <= 3:
        raise DSPFatal("The length of the waveform must be larger than 3 for the filter to work safely")
    if m is not None and m != n:
        raise ValueError(f"{what}: the output has the length of the input (len(w_in) = {n}, len(w_out) = {m})")


def check_bi_level_lists(what, m_polarity, m_times):
    if m_polarity != m_times:
        raise ValueError(f"{what}: polarity_out and t_trig_times_out share the dimension m ({m_polarity} and {m_times} given)")
    if m_polarity < 1:
        raise ValueError(f"{what}: polarity_out and t_trig_times_out hold at least one entry")


def _rc_cr2(g, *args):
    """one C entry for both loops, like sort's (``dsp_rc_cr2_rows`` takes the loop's type).  t_tau is a constant of the call: the filter's
    coefficients are formed on the host, in float64, from the value the loop receives; ``w_out`` may be left out."""
    what = g.__name__
    (w_in, t_tau), (out,) = _split(g, args)
    tau = float(_constant_of_call(t_tau, what, "t_tau"))
    with device_call(what, w_in, f64_rows_only=True) as c:
        if out is not None and not isinstance(out, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
        check_rc_cr2(what, c.n, None if out is None else (int(out.shape[-1]) if len(out.shape) else 0))
        ptr, stride = c.out(out, "n")
        run(getattr(_lib.lib(), "dsp_rc_cr2_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, tau, ptr, stride)
        c.st.finish()
        return c.results[0]


def _bi_level_zero_crossing_time_points(g, *args):
    """one C entry for both loops.  The two lists must be passed: their length is m; the count may be ``None``.  Thresholds, gate and start
    are each one value or a value per row."""
    what = g.__name__
    if len(args) != 8:
        raise TypeError(f"{what}(w_in, a_pos_threshold_in, a_neg_threshold_in, gate_time_in, t_start_in, n_crossings_out, polarity_out, "
                        "t_trig_times_out): polarity_out and t_trig_times_out must be passed (their length is the number of crossings kept); "
                        "n_crossings_out may be None")
    w_in, pos, neg, gate, t_start, n_out, polarity, times = args
    for o in (polarity, times):
        if not isinstance(o, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
    with device_call(what, w_in, f64_rows_only=True) as c:
        m = int(polarity.shape[-1]) if len(polarity.shape) else 0
        check_bi_level_lists(what, m, int(times.shape[-1]) if len(times.shape) else 0)
        if np.size(gate) == 1 and not isinstance(gate, DeviceArray) and not np.isfinite(float(np.asarray(gate).reshape(-1)[0])):
            raise ValueError(f"{what}: gate_time_in is a finite number of samples")
        cols = [c.col(v) for v in (pos, neg, gate, t_start)]
        pn = c.out(n_out, "", np.uint32)[0]
        pp, pt = c.out(polarity, "m")[0], c.out(times, "m")[0]
        run(getattr(_lib.lib(), "dsp_bi_level_zero_crossing_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64,
            *cols[0], *cols[1], *cols[2], *cols[3], pn, pp, pt, m, m)
        c.st.finish()
        return tuple(c.results)


rc_cr2 = HipGUFunc("rc_cr2", "(n),()->(n)", ["ff->f", "dd->d"], _rc_cr2,
                   "RC-CR^2 shaper with the time constant t_tau (a constant of the call): a third-order recursion with a float64 state, one "
                   "rounding at the store; a row with a NaN: NaNs (reference processors/rc_cr2.py:12-94)")
bi_level_zero_crossing_time_points = HipGUFunc("bi_level_zero_crossing_time_points", "(n),(),(),(),(),(),(m),(m)", ["fffffIff", "dddddIdd"],
                                               _bi_level_zero_crossing_time_points,
                                               "the zero crossings between a crossing of one threshold and, within the gate, of the other: count, "
                                               "polarities and NaN-padded indices (reference processors/time_point_thresh.py:404-532)")

# Listed here and not in __all__, like the smoothing processors: their call records are tests/test_pileup_plan_cpu.py's.
PILEUP = ("rc_cr2", "bi_level_zero_crossing_time_points")


# --------------------------------------------------------------------------------------------------- pulses
def check_pulse_list(what, n, m, m_out=None, pickoff=False):
    """what the planner checks of a list of ``m`` entries on rows of ``n`` samples, in the reference's words where it has them"""
    if m_out is not None and m_out != m:
        raise ValueError(f"{what}: the output has the length of the list ({m} entries, {m_out} given)")
    if m > _lib.PEAKS_MAX:
        raise NotImplementedError(f"{what}: at most {_lib.PEAKS_MAX} list entries ({m} given): a wavefront keeps one per lane")
    if pickoff and not m < n:
        raise DSPFatal("The length of your return array must be smaller than the length of your waveform")


def check_pulse_width(what, width):
    """width_in as the kernel takes it: one non-negative, finite number of samples"""
    a = np.asarray(width.magnitude if hasattr(width, "magnitude") else width)
    if a.size != 1:
        raise NotImplementedError(f"{what}: per-waveform integer parameters are not supported on the device")
    w = float(a.reshape(-1)[0])
    if not (w >= 0 and np.isfinite(w)):
        raise ValueError(f"{what}: width_in is a non-negative number of samples")
    return w


def _pulse_list(c, what, v, name):
    """a '(m)' input on the device: (array, m, row stride); one list is repeated for every row"""
    if isinstance(v, DeviceArray):
        if v.dtype != np.dtype(c.ft):
            raise TypeError(f"{what}: {name} on the device has the loop's type, {np.dtype(c.ft)}")
        shape, dev = tuple(v.shape), v
    else:
        host = np.ascontiguousarray(np.asarray(v), dtype=c.ft)
        shape, dev = host.shape, None
    if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] != c.n_wf) or (dev is not None and len(shape) == 1 and c.n_wf != 1):
        raise ValueError(f"{what}: {name} has shape {shape}, expected ({c.n_wf}, m)" + ("" if dev is not None else " or (m,)"))
    m = int(shape[-1])
    if dev is None and m > 0 and m <= _lib.PEAKS_MAX:
        dev = DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(host, (c.n_wf, m))))
        c.st.keep.append(dev)
    return dev, m, m


def _pulse_out(c, given, m, dtype=None):
    """an output of m values a row (``m`` None: a value a row), the caller's or a new one"""
    if given is not None and not isinstance(given, (np.ndarray, DeviceArray)):
        raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
    shape = () if m is None else (m,)
    ptr, res = c.st.out(given, shape if c.one_d else (c.n_wf, *shape), dtype or c.ft)
    c.results.append(res)
    return ptr


def _results(c):
    res = [r[()] if isinstance(r, np.ndarray) and r.ndim == 0 else r for r in c.results]
    return res[0] if len(res) == 1 else tuple(res)


def _peak_snr_threshold(g, *args):
    """one C entry for both loops, like sort's.  ``width_in`` is a constant of the call, ``ratio_in`` one value or a value per row; the
    outputs may be left out: their length is that of ``idx_in``."""
    what = g.__name__
    (w_in, idx_in, ratio, width), (idx_out, n_out) = _split(g, args)
    width = check_pulse_width(what, width)
    with device_call(what, w_in, f64_rows_only=True) as c:
        lst, m, stride = _pulse_list(c, what, idx_in, "idx_in")
        check_pulse_list(what, c.n, m, None if idx_out is None else (int(idx_out.shape[-1]) if len(idx_out.shape) else 0))
        col = c.col(ratio)
        if m == 0:  # no candidate: nothing to launch, the counts are 0
            zeros = np.zeros(() if c.one_d else (c.n_wf,), np.uint32)
            if isinstance(n_out, DeviceArray):
                n_out.copy_from(zeros.reshape(n_out.shape))
            elif n_out is not None:
                n_out[...] = 0
            return (idx_out if idx_out is not None else np.empty((0,) if c.one_d else (c.n_wf, 0), c.ft)), (n_out if n_out is not None else zeros[()])
        po, pn = _pulse_out(c, idx_out, m), _pulse_out(c, n_out, None, np.uint32)
        run(getattr(_lib.lib(), "dsp_peak_snr_threshold_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, lst.ptr, m, stride, *col,
            width, po, m, pn)
        c.st.finish()
        return _results(c)


def _multi_a_filter(g, *args):
    """one C entry for both loops; ``va_max_out`` may be left out: its length is that of ``vt_maxs_in``"""
    what = g.__name__
    (w_in, vt), (out,) = _split(g, args)
    with device_call(what, w_in, f64_rows_only=True) as c:
        lst, m, stride = _pulse_list(c, what, vt, "vt_maxs_in")
        check_pulse_list(what, c.n, m, None if out is None else (int(out.shape[-1]) if len(out.shape) else 0), pickoff=True)
        if m == 0:
            return out if out is not None else np.empty((0,) if c.one_d else (c.n_wf, 0), c.ft)
        po = _pulse_out(c, out, m)
        run(getattr(_lib.lib(), "dsp_multi_a_filter_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, lst.ptr, m, stride, po, m)
        c.st.finish()
        return _results(c)


peak_snr_threshold = HipGUFunc("peak_snr_threshold", "(n),(m),(),()->(m),()", ["ffff->fI", "dddd->dI"], _peak_snr_threshold,
                               "of the candidates idx_in those whose window [c - width, c + width) -- clamped to the row, its upper end excluded -- "
                               "goes down to less than ratio_in of the sample at c: packed to the front, NaN-padded, and their number; m <= 64, "
                               "width_in a constant of the call (reference processors/peak_snr_threshold.py:19-71)")
multi_a_filter = HipGUFunc("multi_a_filter", "(n),(m)->(m)", ["ff->f", "dd->d"], _multi_a_filter,
                           "the row's samples at the whole-numbered positions vt_maxs_in, NaN for a NaN position or one outside the row; a row with "
                           "a NaN: NaNs; m <= 64 and m < n (reference processors/multi_a_filter.py:20-57)")

# Listed here and not in __all__, like the pile-up processors: their call records are tests/test_pulse_plan_cpu.py's.
PULSES = ("peak_snr_threshold", "multi_a_filter")


# --------------------------------------------------------------------------------------------------- decay-tail fit
def check_poly(what, n, m):
    """what the planner checks of ``m`` coefficients on rows of ``n`` samples, in its words"""
    if m < 1:
        raise ValueError(f"{what}: at least one coefficient")
    if m > _lib.POLY_MAX:
        raise NotImplementedError(f"{what}: at most {_lib.POLY_MAX} coefficients ({m} given): a lane keeps one float64 accumulator each")
    if max(n - 1, 0) ** (m - 1) >= 2 ** 63:
        raise NotImplementedError(f"{what}: (n - 1)**(m - 1) must stay below 2**63 (n = {n} samples, m = {m} coefficients): beyond it the "
                                  "reference's int64 power i**j wraps silently")


def check_poly_fit_init(what, length, deg):
    """``init_args`` of poly_fit: two non-negative integer constants -> (length, deg)"""
    out = []
    for name, v in (("length", length), ("deg", deg)):
        a = np.asarray(v.magnitude if hasattr(v, "magnitude") else v)
        if a.size != 1:
            raise NotImplementedError(f"{what}: {name} is a constant of the call on the device, not a per-event value")
        f = float(a.reshape(-1)[0])
        if not (f >= 0 and f == int(f)):
            raise ValueError(f"{what}: {name} is a non-negative integer ({v} given)")
        out.append(int(f))
    return tuple(out)


def poly_fit_inverse(length, deg):
    """The factory's matrix (reference processors/poly_fit.py:50-61, as written): the power sums over ``range(length)`` in float64, inverted
    once on the host with ``np.linalg.inv``.  A singular matrix (``length <= deg``) raises as it does there."""
    vals_array = np.zeros(2 * deg + 1, dtype="float64")
    for i in range(length):
        for j in range(2 * deg + 1):
            vals_array[j] += i**j
    mat = np.zeros((deg + 1, deg + 1), dtype="float")
    for i in range(deg + 1):
        mat[i, :] = vals_array[i: deg + 1 + i]
    return np.linalg.inv(mat)


def _log_check(g, *args):
    """one C entry for both loops, like sort's; ``w_log`` may be left out"""
    what = g.__name__
    (w_in,), (out,) = _split(g, args)
    with device_call(what, w_in, f64_rows_only=True) as c:
        if out is not None and not isinstance(out, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
        if out is not None and (int(out.shape[-1]) if len(out.shape) else 0) != c.n:
            raise ValueError(f"{what}: the output has the length of the input (len(w_in) = {c.n}, len(w_log) = {int(out.shape[-1]) if len(out.shape) else 0})")
        ptr, stride = c.out(out, "n")
        run(getattr(_lib.lib(), "dsp_log_check_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, ptr, stride)
        c.st.finish()
        return _results(c)


def poly_fit(length, deg):
    """The reference's factory (processors/poly_fit.py:35-71): the gufunc ``poly_fitter``, ``(n),(m)``, that fits rows to a polynomial of order
    ``deg`` over ``range(length)``.  The inverted matrix is formed here, once, and travels with every call; ``poly_pars`` (``deg + 1``
    coefficients a row) is written in place, or returned where it is left out."""
    length, deg = check_poly_fit_init("poly_fit", length, deg)
    check_poly("poly_fit", length, deg + 1)
    inv = np.ascontiguousarray(poly_fit_inverse(length, deg), dtype=np.float64)
    m = deg + 1

    def impl(g, *args):
        what = g.__name__
        if len(args) not in (1, 2):
            raise TypeError(f"{what}() takes w_in and poly_pars ({len(args)} given)")
        w_in, out = args[0], (args[1] if len(args) == 2 else None)
        with device_call(what, w_in, f64_rows_only=True) as c:
            if out is not None and not isinstance(out, (np.ndarray, DeviceArray)):
                raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
            m_out = m if out is None else (int(out.shape[-1]) if len(out.shape) else 0)
            if m_out != m:
                raise ValueError(f"{what}: poly_pars holds deg + 1 = {m} coefficients ({m_out} given)")
            check_poly(what, c.n, m)
            dev = DeviceArray.from_numpy(inv)
            c.st.keep.append(dev)
            po = _pulse_out(c, out, m)
            run(getattr(_lib.lib(), "dsp_poly_fit_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, dev.ptr, m, po, m)
            c.st.finish()
            return _results(c)

    g = HipGUFunc("poly_fitter", "(n),(m)", ["ff", "dd"], impl, f"Fit w_in to order {deg} polynomial.")
    g.inv = inv
    return g


def _poly_pars(c, what, v):
    """the '(m)' input of the residuals on the device: (array, m, row stride); one row of coefficients is repeated for every row"""
    if isinstance(v, DeviceArray):
        if v.dtype != np.dtype(c.ft):
            raise TypeError(f"{what}: poly_pars on the device has the loop's type, {np.dtype(c.ft)}")
        shape, dev = tuple(v.shape), v
    else:
        host = np.ascontiguousarray(np.asarray(v), dtype=c.ft)
        shape, dev = host.shape, None
    if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] != c.n_wf) or (dev is not None and len(shape) == 1 and c.n_wf != 1):
        raise ValueError(f"{what}: poly_pars has shape {shape}, expected ({c.n_wf}, m)" + ("" if dev is not None else " or (m,)"))
    m = int(shape[-1])
    check_poly(what, c.n, m)
    if dev is None:
        dev = DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(host, (c.n_wf, m))))
        c.st.keep.append(dev)
    return dev, m, m


def _poly_residual(exp_rms):
    def impl(g, *args):
        """one C entry for both processors and both loops; ``mean`` and ``rms`` may be left out"""
        what = g.__name__
        (w_in, pars), (mean, rms) = _split(g, args)
        with device_call(what, w_in, f64_rows_only=True) as c:
            dev, m, stride = _poly_pars(c, what, pars)
            pm, pr = _pulse_out(c, mean, None), _pulse_out(c, rms, None)
            run(getattr(_lib.lib(), "dsp_poly_residual_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, exp_rms, dev.ptr, m, stride, pm, pr)
            c.st.finish()
            return _results(c)

    return impl


log_check = HipGUFunc("log_check", "(n)->(n)", ["f->f", "d->d"], _log_check,
                      "the logarithm of a row that is positive throughout; a row with a NaN or a sample <= 0: NaNs (reference "
                      "processors/log_check.py:11-48)")
poly_diff = HipGUFunc("poly_diff", "(n),(m)->(),()", ["ff->ff", "dd->dd"], _poly_residual(0),
                      "of the residuals r_i = w_in[i] - sum_j poly_pars[j] i**j (float64): sum r_i / (i + 1) and sqrt(sum r_i^2 / (n - 1)), both "
                      "rounded to the loop's type after every sample; m <= 8 (reference processors/poly_fit.py:74-108)")
poly_exp_rms = HipGUFunc("poly_exp_rms", "(n),(m)->(),()", ["ff->ff", "dd->dd"], _poly_residual(1),
                         "poly_diff against the exponential of the polynomial, r_i = w_in[i] - exp(sum_j poly_pars[j] i**j) (reference "
                         "processors/poly_fit.py:111-141)")

# Listed here and not in __all__, like the pulse picker's processors: their call records are tests/test_tailfit_plan_cpu.py's.
TAILFIT = ("log_check", "poly_fit", "poly_diff", "poly_exp_rms")


# --------------------------------------------------------------------------------------------------- waveform aligner
_INL_ROWS = (np.dtype(np.int16), np.dtype(np.uint16), np.dtype(np.int32), np.dtype(np.uint32))


def _one_value(what, name, v):
    """a parameter that is a constant of the call -> its value as a Python float"""
    if isinstance(v, DeviceArray):
        raise NotImplementedError(f"{what}: {name} is a constant of the call on the device, not a per-event value")
    return float(_constant_of_call(v.magnitude if hasattr(v, "magnitude") else v, what, name))


def check_centroid_shift(what, n, shift, loop_dtype=np.float32):
    """get_wf_centroid.py:55-60 for rows of ``n`` samples: checked once for the call, in the reference's order and words -> shift as the loop receives it"""
    shift = float(np.dtype(loop_dtype).type(_one_value(what, "shift", shift)))
    if np.isnan(shift):
        raise DSPFatal("shift is nan")
    if shift < 0:
        raise DSPFatal("shift must be positive")
    if shift > n - 1:
        raise DSPFatal("shift must be shorter than input waveform size")
    return shift


def check_alignment(what, n, shift, size, m_out, loop_dtype=np.float32):
    """wf_alignment.py:66-78 for rows of ``n`` samples and an output of ``m_out``, in the reference's order and words; then the rule the
    reference leaves to NumPy's broadcast: ``size`` is a whole number and equals ``len(w_out)`` -> (shift, size) as the loop receives them"""
    ft = np.dtype(loop_dtype).type
    shift, size = float(ft(_one_value(what, "shift", shift))), float(ft(_one_value(what, "size", size)))
    if np.isnan(shift):
        raise DSPFatal("shift is nan")
    if shift < 0:
        raise DSPFatal("shift must be positive")
    if shift > n:
        raise DSPFatal("shift must be shorter than input waveform size")
    if np.isnan(size):
        raise DSPFatal("size is nan")
    if size <= 0:
        raise DSPFatal("size must be positive")
    if size > n:
        raise DSPFatal("size must be shorter than input waveform size")
    if size != m_out:
        raise ValueError(f"{what}: size is a whole number and equals len(w_out) (size = {size:g}, len(w_out) = {m_out})")
    return shift, size


def check_correction(what, n, m, start_idx, stop_idx):
    """wf_correction.py:64-77 for rows of ``n`` samples and a template of ``m``, in the reference's order and words -> (start, stop)"""
    start, stop = (_as_int(_one_value(what, name, v), what) for name, v in (("start_idx", start_idx), ("stop_idx", stop_idx)))
    if m < 1:
        raise ValueError(f"{what}: w_corr holds at least one sample")
    if start < 0:
        raise DSPFatal("start_idx must be positive")
    if start > n:
        raise DSPFatal("start_idx must be shorter than input waveform size")
    if stop <= 0:
        raise DSPFatal("stop_idx must be positive")
    if stop > n:
        raise DSPFatal("stop_idx must be shorter than input waveform size")
    if start >= stop:
        raise DSPFatal("start_idx must be smaller than stop_idx")
    if stop - start > m:
        raise DSPFatal("stop_idx - start_idx must be smaller than len(w_corr)")
    return start, stop


def inl_range_error(row, p):
    """the reference's text for the first sample of ``row`` outside ``[0, p)`` (inl_correction.py:59-61)"""
    codes = np.asarray(row).astype(np.int64).reshape(-1)
    bad = np.flatnonzero((codes < 0) | (codes >= p))
    return DSPFatal(f"ADC code {int(codes[bad[0]]) if bad.size else '?'} out of range for INL array of length {p}")


def _constant_array(c, what, name, v, ft):
    """a '(p)' input that is one constant array for all rows -> (DeviceArray, length)"""
    if isinstance(v, DeviceArray):
        if np.dtype(v.dtype) != np.dtype(ft) or len(v.shape) != 1:
            raise TypeError(f"{what}: {name} on the device is one row of {np.dtype(ft).name} values in the {np.dtype(ft).name} loop")
        return v, int(v.shape[-1])
    a = np.asarray(v.magnitude if hasattr(v, "magnitude") else v)
    if a.ndim != 1:
        raise NotImplementedError(f"{what}: {name} is one constant array of the call on the device, not an array per event")
    if a.size == 0:
        raise ValueError(f"{what}: {name} holds at least one value")
    dev = DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=ft))
    c.st.keep.append(dev)
    return dev, int(a.size)


def _out_len(out):
    return int(out.shape[-1]) if len(out.shape) else 0


def _inl_correction(g, *args):
    """one C entry for both loops; the table's type selects the loop (``if->f``, ``id->d``), the rows are integers.  ``w_out`` may be left out."""
    what = g.__name__
    (w_in, inl), (out,) = _split(g, args)
    if np.dtype(dtype_of(w_in)) not in _INL_ROWS:
        raise TypeError(f"{what}: w_in holds int16, uint16, int32 or uint32 ADC codes ({np.dtype(dtype_of(w_in))} given): the reference has no loop for anything else")
    with device_call(what) as c:
        c.ptr, c.code, c.n_wf, c.n, c.stride, c.one_d = c.st.wf_in(w_in)
        c.ft = np.float64 if np.dtype(dtype_of(inl)) == np.dtype(np.float64) else np.float32
        if out is not None and not isinstance(out, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
        if out is not None and _out_len(out) != c.n:
            raise ValueError(f"{what}: the output has the length of the input (len(w_in) = {c.n}, len(w_out) = {_out_len(out)})")
        table, p = _constant_array(c, what, "inl", inl, c.ft)
        ptr, stride = c.out(out, "n")
        row = _lib.C.c_int64(-1)
        rc = _lib.lib().dsp_inl_correction_rows(*c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, table.ptr, p, ptr, stride, None, _lib.C.byref(row))
        if rc == _lib.E_INL_RANGE and row.value >= 0:
            # the error word holds a code and a row: that row is read back and its first offending sample named
            r = int(row.value)
            if isinstance(w_in, DeviceArray):  # (that row alone comes back)
                codes = DeviceArray.from_ptr(w_in.ptr + r * c.n * np.dtype(w_in.dtype).itemsize, (c.n,), w_in.dtype).to_numpy()
            else:
                codes = np.asarray(w_in).reshape(c.n_wf, c.n)[r]
            err = inl_range_error(codes, p)
            err.wf_range, err.processor = range(r, r + 1), what
            raise err
        _lib.check(rc, row=row.value if row.value >= 0 else None, what=what)
        c.st.finish()
        return _results(c)


def _get_wf_centroid(g, *args):
    """one C entry for both loops; ``shift`` is a constant of the call, ``centroid`` may be left out"""
    what = g.__name__
    (w_in, shift), (out,) = _split(g, args)
    with device_call(what, w_in, f64_rows_only=True) as c:
        shift = check_centroid_shift(what, c.n, shift, c.ft)
        po = _pulse_out(c, out, None)
        run(getattr(_lib.lib(), "dsp_wf_centroid_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, shift, po)
        c.st.finish()
        return _results(c)


def _wf_alignment(g, *args):
    """one C entry for both loops; ``centroid`` is one value or a value per row, ``shift`` and ``size`` constants of the call; ``w_out`` must
    be passed: its length is ``size``.  Integer rows take their loop like any rows: (u)int16 the float32 one, (u)int32 the float64 one."""
    what = g.__name__
    if len(args) != 5:
        raise TypeError(f"{what}(w_in, centroid, shift, size, w_out): w_out must be passed, its length is an argument ({len(args)} given)")
    w_in, centroid, shift, size, out = args
    if not isinstance(out, (np.ndarray, DeviceArray)):
        raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
    with device_call(what, w_in) as c:
        shift, size = check_alignment(what, c.n, shift, size, _out_len(out), c.ft)
        col = c.col(centroid)
        if col[0] is None and np.isnan(col[1]):
            raise DSPFatal("centroid is nan")
        m = int(size)
        po = _pulse_out(c, out, m)
        run(getattr(_lib.lib(), "dsp_wf_alignment_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, *col, shift, size, po, m, m)
        c.st.finish()
        return _results(c)


def _wf_correction(g, *args):
    """one C entry for both loops; ``w_corr`` is one constant array, the indices constants of the call; ``w_out`` may be left out"""
    what = g.__name__
    (w_in, w_corr, start_idx, stop_idx), (out,) = _split(g, args)
    with device_call(what, w_in, f64_rows_only=True) as c:
        if out is not None and not isinstance(out, (np.ndarray, DeviceArray)):
            raise TypeError("output arguments must be NumPy arrays or DeviceArrays")
        if out is not None and _out_len(out) != c.n:
            raise ValueError(f"{what}: the output has the length of the input (len(w_in) = {c.n}, len(w_out) = {_out_len(out)})")
        if not isinstance(w_corr, DeviceArray) and np.ndim(w_corr.magnitude if hasattr(w_corr, "magnitude") else w_corr) != 1:
            raise NotImplementedError(f"{what}: w_corr is one constant array of the call on the device, not an array per event")
        m = int(w_corr.shape[-1]) if isinstance(w_corr, DeviceArray) else int(np.size(w_corr.magnitude if hasattr(w_corr, "magnitude") else w_corr))
        start, stop = check_correction(what, c.n, m, start_idx, stop_idx)
        table, m = _constant_array(c, what, "w_corr", w_corr, c.ft)
        ptr, stride = c.out(out, "n")
        run(getattr(_lib.lib(), "dsp_wf_correction_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, table.ptr, m, start, stop, ptr, stride)
        c.st.finish()
        return _results(c)


def _step(g, weight_pos, kernel):
    """+1 on the middle half of the kernel, -1 on its outer quarters: ``len / 4 <= i < 3 len / 4`` as comparisons of real numbers.  ``weight_pos``
    is accepted and not used, as in the reference (processors/kernels.py:103-142)."""
    n = len(kernel)
    x = np.arange(n)
    kernel[:] = np.where((x >= n / 4) & (x < 3 * n / 4), 1, -1)
    return kernel


inl_correction = HipGUFunc("inl_correction", "(n),(p)->(n)", ["if->f", "id->d"], _inl_correction,
                           "w_out[i] = w_in[i] + inl[w_in[i]], a float64 sum rounded once; integer rows; a NaN in inl: NaN rows; a sample outside the "
                           "table: DSPFatal with the code (reference processors/inl_correction.py:12-61)")
get_wf_centroid = HipGUFunc("get_wf_centroid", "(n),()->()", ["ff->f", "dd->d"], _get_wf_centroid,
                            "the rounded middle (half to even) of the first positive and the last negative sample between the row's first minimum "
                            "and first maximum, plus shift; NaN for a row with a NaN and where the reference defines nothing (reference "
                            "processors/get_wf_centroid.py:12-69)")
wf_alignment = HipGUFunc("wf_alignment", "(n),(),(),(),(m)", ["fffff", "ddddd"], _wf_alignment,
                         "the window of size samples centred on the centroid, padded with w_in[0] near the start of the row, w_in[:size] otherwise; "
                         "shift and size constants of the call (reference processors/wf_alignment.py:12-87)")
wf_correction = HipGUFunc("wf_correction", "(n),(m),(),()->(n)", ["ffii->f", "ddii->d"], _wf_correction,
                          "w_in with w_corr[: stop_idx - start_idx] subtracted on [start_idx, stop_idx); a NaN in the row or in w_corr: NaNs "
                          "(reference processors/wf_correction.py:10-83)")
step = HipGUFunc("step", "(),(n)", ["ff", "dd"], _step, "step kernel generator, host, once (reference processors/kernels.py:103-142)")

# Listed here and not in __all__, like the decay-tail fitter's processors: their call records are tests/test_align_plan_cpu.py's.
ALIGNMENT = ("inl_correction", "get_wf_centroid", "wf_alignment", "wf_correction", "step")


# --------------------------------------------------------------------------------------------------- data cleaning
SVM_KERNELS = ("rbf", "linear")  # kernel_kind 0 and 1 of dsp_svm_rows
SVM_LIMITS = f"rows of up to {_lib.DENSE_N_MAX} samples and models of up to {_lib.SVM_CLASSES_MAX} classes"  # (DSP_SVM_LIMITS_TEXT, dsp_program.h)
_SVM_FIELDS = ("kernel", "gamma", "support_vectors", "n_support", "dual_coef", "intercept", "classes")


def check_svm(what, n, n_classes, n_sv=None):
    """what the planner and the C entry check, in their words: rows and classes; with ``n_sv``, the size of the model as well"""
    if n > _lib.DENSE_N_MAX or n_classes > _lib.SVM_CLASSES_MAX:
        raise NotImplementedError(f"{what}: {SVM_LIMITS} (n = {n}, {n_classes} classes given)")
    pairs = n_classes * (n_classes - 1) // 2
    if n_sv is not None and (n_sv < 1 or n < 1 or n_sv * n > _lib.SVM_MODEL_MAX or n_sv * pairs > _lib.SVM_MODEL_MAX):
        raise NotImplementedError(f"{what}: at least one support vector, and at most {_lib.SVM_MODEL_MAX} support-vector samples and coefficients "
                                  f"({n_sv} support vectors of {n} samples, {pairs} pairs of classes given)")


def svm_model_arrays(svc):
    """The constant arrays a fitted ``sklearn.svm.SVC`` predicts with, as a dict: ``kernel``, ``gamma``, ``support_vectors`` (n_sv, n),
    ``n_support`` (k,), ``dual_coef`` and ``intercept`` (the UNDERSCORED attributes ``_dual_coef_`` and ``_intercept_``: for two classes the
    public ones carry the opposite sign) and ``classes``.  Needs nothing of scikit-learn but the object."""
    if type(svc).__name__ != "SVC" or not hasattr(svc, "support_vectors_") or not hasattr(svc, "_dual_coef_"):
        raise TypeError(f"svm_predict: {type(svc).__name__!r} is no fitted sklearn.svm.SVC")
    kernel = svc.kernel
    if kernel not in SVM_KERNELS:
        raise NotImplementedError(f"svm_predict: the kernel function {kernel if isinstance(kernel, str) else 'given as a callable'!r} is not "
                                  "implemented on the device: 'rbf' and 'linear' are")
    if getattr(svc, "break_ties", False):
        raise NotImplementedError("svm_predict: break_ties=True is not implemented on the device (the vote's first maximum wins)")
    classes = np.asarray(svc.classes_)
    if classes.dtype.kind not in "fiub":
        raise TypeError(f"svm_predict: the class labels are {classes.dtype.name}; the label of a row is a number (float32 in the reference)")
    sv = svc.support_vectors_
    if hasattr(sv, "toarray"):
        raise NotImplementedError("svm_predict: sparse support vectors are not implemented on the device")
    return _checked_svm_model({"kernel": kernel, "gamma": float(svc._gamma), "support_vectors": sv, "n_support": svc.n_support_,
                               "dual_coef": svc._dual_coef_, "intercept": svc._intercept_, "classes": classes})


def _checked_svm_model(m):
    """the dict of ``svm_model_arrays`` -- from an SVC or from a file -- with its arrays in their types and its shapes checked"""
    missing = [f for f in _SVM_FIELDS if f not in m]
    if missing:
        raise ValueError(f"svm_predict: the model lacks {', '.join(missing)}")
    kernel = str(np.asarray(m["kernel"]).reshape(-1)[0]) if not isinstance(m["kernel"], str) else m["kernel"]
    if kernel not in SVM_KERNELS:
        raise NotImplementedError(f"svm_predict: the kernel function {kernel!r} is not implemented on the device: 'rbf' and 'linear' are")
    classes = np.asarray(m["classes"])
    if classes.dtype.kind not in "fiub":
        raise TypeError(f"svm_predict: the class labels are {classes.dtype.name}; the label of a row is a number (float32 in the reference)")
    out = {"kernel": kernel, "gamma": float(np.asarray(m["gamma"]).reshape(-1)[0]),
           "support_vectors": np.ascontiguousarray(m["support_vectors"], dtype=np.float64), "n_support": np.asarray(m["n_support"], dtype=np.int32).reshape(-1),
           "dual_coef": np.ascontiguousarray(m["dual_coef"], dtype=np.float64), "intercept": np.asarray(m["intercept"], dtype=np.float64).reshape(-1),
           "classes": classes.astype(np.float64).reshape(-1)}
    k, sv = out["classes"].size, out["support_vectors"]
    if (k < 2 or sv.ndim != 2 or sv.shape[0] < 1 or out["n_support"].size != k or int(out["n_support"].sum()) != sv.shape[0] or (out["n_support"] < 0).any()
            or out["dual_coef"].shape != (k - 1, sv.shape[0]) or out["intercept"].size != k * (k - 1) // 2):
        raise ValueError(f"svm_predict: the model's arrays do not fit each other ({k} classes, support_vectors {sv.shape}, n_support {out['n_support'].shape}, "
                         f"dual_coef {out['dual_coef'].shape}, intercept {out['intercept'].shape})")
    return out


def svm_device_arrays(model):
    """what ``dsp_svm_rows`` takes of a model, float64 and contiguous on the host: the support vectors, their squared norms, D (n_sv, P) --
    the coefficient of support vector s in pair p = (i, j) of classes, ``dual_coef[j - 1, s]`` for a support vector of class i and
    ``dual_coef[i, s]`` for one of class j, 0 elsewhere; the pairs in the order (0,1), (0,2) .. (k-2,k-1) --, the intercepts and the classes"""
    sv, k = model["support_vectors"], model["classes"].size
    cls = np.repeat(np.arange(k), model["n_support"])
    D = np.zeros((sv.shape[0], k * (k - 1) // 2))
    p = 0
    for i in range(k):
        for j in range(i + 1, k):
            D[cls == i, p] = model["dual_coef"][j - 1, cls == i]
            D[cls == j, p] = model["dual_coef"][i, cls == j]
            p += 1
    return sv, np.ascontiguousarray((sv * sv).sum(axis=1)), D, model["intercept"], model["classes"]


def save_svm_model(path, svc):
    """``svm_model_arrays(svc)`` as an ``.npz`` file: what ``svm_predict(path)`` reads where scikit-learn is not installed"""
    np.savez(path, **svm_model_arrays(svc))


def load_svm_model(svm_file):
    """the model behind ``svm_predict``'s argument: a fitted SVC, a dict of its arrays, an ``.npz`` of them, or a pickle of the SVC"""
    if isinstance(svm_file, dict):
        return _checked_svm_model(svm_file)
    if isinstance(svm_file, (str, bytes)) or hasattr(svm_file, "__fspath__"):
        import os

        path = os.fspath(svm_file)
        path = path.decode() if isinstance(path, bytes) else path
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as f:
                return _checked_svm_model({name: f[name] for name in f.files})
        try:
            import sklearn.svm  # noqa: F401  (the pickle names its classes)
        except ImportError:
            raise ImportError(f"svm_predict: '{path}' is a pickle of a scikit-learn SVC, and scikit-learn is not installed where the chain is built; "
                              "write the model's arrays with dspeed_amd.processors.save_svm_model(path.npz, svc) where it is") from None
        import pickle

        with open(path, "rb") as f:
            return svm_model_arrays(pickle.load(f))
    return svm_model_arrays(svm_file)


def _null_svm(g, *args):
    """``svm_predict(0)``: NaN for every row, nothing launched (reference processors/svm.py:45-51)"""
    if len(args) not in (1, 2):
        raise TypeError(f"{g.__name__}() takes w_in and label_out ({len(args)} given)")
    w_in, out = args[0], (args[1] if len(args) == 2 else None)
    shape, dt = tuple(w_in.shape), np.dtype(dtype_of(w_in))
    ft = np.float64 if dt == np.dtype(np.float64) else np.float32
    if out is None:
        return np.full(shape[:-1], np.nan, dtype=ft)[()] if len(shape) == 1 else np.full(shape[:-1], np.nan, dtype=ft)
    if isinstance(out, DeviceArray):
        out.copy_from(np.full(tuple(out.shape), np.nan, dtype=out.dtype))
    else:
        out[...] = np.nan
    return out


def svm_predict(svm_file):
    """The reference's factory (processors/svm.py:13-71): the gufunc ``svm_out``, ``(n)->()``, that gives every row the class label of a fitted
    scikit-learn ``SVC``.  ``svm_file`` is 0 (the null processor: NaN for every row, nothing launched), the path of a pickle of the SVC (needs
    scikit-learn importable here; UNPICKLING RUNS WHAT THE FILE SAYS, as in the reference: open files you trust), a path ending in ``.npz`` holding
    ``svm_model_arrays`` (``save_svm_model``; needs no scikit-learn), or the fitted ``SVC`` itself.  Nothing of scikit-learn runs per row: the
    model's arrays are taken out here, once, go to the device at the first call and stay with the returned processor.  "rbf" and "linear"
    kernel functions; a row with a NaN -- or, unlike the reference, which raises scikit-learn's ValueError, with an infinite sample -- gives
    NaN.  The float64 loop is this project's addition."""
    doc = "the class label of a fitted sklearn.svm.SVC (rbf or linear, one-vs-one) for every row; a row with a NaN or an infinity: NaN (reference processors/svm.py:13-71)"
    if isinstance(svm_file, (int, np.integer, float)) and not isinstance(svm_file, bool) and svm_file == 0:
        g = HipGUFunc("svm_out", "(n)->()", ["f->f", "d->d"], _null_svm, doc)
        g.model = None
        return g
    model = load_svm_model(svm_file)
    host = svm_device_arrays(model)
    n_sv, n = model["support_vectors"].shape
    k = model["classes"].size
    check_svm("svm_predict", n, k, n_sv)
    kind = SVM_KERNELS.index(model["kernel"])
    held = []  # the model on the device: made at the first call, kept

    def impl(g, *args):
        what = "svm_predict"
        if len(args) not in (1, 2):
            raise TypeError(f"{what}() takes w_in and label_out ({len(args)} given)")
        w_in, out = args[0], (args[1] if len(args) == 2 else None)
        if np.dtype(dtype_of(w_in)) not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise NotImplementedError(f"{what}: float32 rows (the float32 loop) or float64 rows (the float64 loop), not {np.dtype(dtype_of(w_in)).name}")
        with device_call(what, w_in) as c:
            if c.n != n:
                raise ValueError(f"{what}: the rows hold {c.n} samples, the model's support vectors {n}")
            check_svm(what, c.n, k, n_sv)
            if not held:
                held.extend(DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) for a in host)
            (ptr,) = c.out(out)
            run(getattr(_lib.lib(), "dsp_svm_rows"), what, *c.rows_args, _lib.F32 if c.ft is np.float32 else _lib.F64, *(d.ptr for d in held), n_sv, k, kind,
                float(model["gamma"]), ptr, None, 0)  # (no decisions: the label alone)
            c.st.finish()
            res = c.results[0]
            return res[()] if isinstance(res, np.ndarray) and res.ndim == 0 else res

    g = HipGUFunc("svm_out", "(n)->()", ["f->f", "d->d"], impl, doc)
    g.model, g.device_arrays = model, held
    return g


# Listed here and not in __all__, like the aligner's processors: its call record is tests/test_svm_plan_cpu.py's.
CLEANING = ("svm_predict",)

__all__ = ["bl_subtract", "pole_zero", "double_pole_zero", "trap_filter", "trap_norm", "asym_trap_filter", "fixed_time_pickoff",
           "time_point_thresh", "interpolated_time_point_thresh", "min_max", "min_max_norm", "linear_slope_fit", "mean_below_threshold", "windower", "avg_current", "upsampler", "moving_window_multi", "trap_pickoff", "discrete_wavelet_transform", "convolve_wf", "fft_convolve_wf", "cusp_filter", "zac_filter", "t0_filter", "moving_slope", "get_multi_local_extrema", "histogram", "histogram_stats", "multi_time_point_thresh", "time_over_threshold"]

"""From the steps of a recipe to device programs (``dsp_chain_create``).  ``_add_step`` resolves one recipe entry into a step (the role of
ProcessorManager.__init__, reference src/dspeed/processing_chain.py:1527-1775, and of the processor loop of build_processing_chain,
:2655-2823); ``_compile`` runs the passes over the steps, in this order:

``_int_island``          per-event integer arithmetic into the integer program ahead of everything
``_extract_fits``        linear_slope_fit onto the rows of the batch, ahead of the chain
``_extract_stages``      what the planner gives to specialised kernels ahead of the program (``_Stager``: ``_stage_long_firs``,
                         ``_stage_short_traps``, ``_stage_current_branch``, ``_stage_row_reductions``)
``_schedule``            the remaining processors ordered for short waveform lifetimes
``_push_down_slices``, ``_last_uses``    an element-wise result read through one slice computed on it alone; who reads what last
``_Emitter``             the steps into ops: slots, registers, bindings, fusions (a method per processor family: ``_EMIT``, ``_READ_OFF``)
``_emit_outputs``, ``_fit_descriptors``  the stores of the outputs; what the runtime launches for the fits
``_split_scalar_tail``, ``_split_scalar_head``, ``_split_walks``    arithmetic behind / ahead of the waveform ops and the threshold walks
                         leave the program for kernels with a row per lane or wavefront
"""
from __future__ import annotations

import ast
import copy
import os
from types import SimpleNamespace

import numpy as np

from . import _lib
from .chain import Program, Scalar
from .device import dtype_code
from .errors import DSPFatal, ProcessingChainError
from .gufunc import loop_suffix
from .language import (Char, Grid, Quantity, SExpr, Var, View, _Builder, _GENERATORS, _MODULES, _NUMPY_BINARY, module_accepted, _SIGS, _column, _grid_of, _is_int_dtype,
                       _is_scalar, _is_wf, _resolve, _roles, _time_unit_ns)

# processors whose output waveform has the input's dimension name in the gufunc signature ("(n),...->(n)") and therefore its
# coordinate grid (reference :1601-1619, 1700); the others' outputs have no grid unless the recipe declares one
_MULTI_EXTREMA = "get_multi_local_extrema"
_HISTOGRAM, _HISTOGRAM_STATS = "histogram", "histogram_stats"
_MULTI_TPT, _TIME_OVER = "multi_time_point_thresh", "time_over_threshold"
_PSD, _SORT, _INTERP, _REFLECT = "psd", "sort", "interpolating_upsampler", "reflected_convolve_wf"
_RC_CR2, _BI_LEVEL = "rc_cr2", "bi_level_zero_crossing_time_points"
_PEAK_SNR, _MULTI_A = "peak_snr_threshold", "multi_a_filter"
_LOG_CHECK, _POLY_FIT, _POLY_DIFF, _POLY_EXP_RMS = "log_check", "poly_fit", "poly_diff", "poly_exp_rms"
_TAILFIT = (_LOG_CHECK, _POLY_FIT, _POLY_DIFF, _POLY_EXP_RMS)
_INL, _WF_CENTROID, _WF_ALIGN, _WF_CORR = "inl_correction", "get_wf_centroid", "wf_alignment", "wf_correction"
_ALIGN = (_INL, _WF_CENTROID, _WF_ALIGN, _WF_CORR)
_NORMALISE = "normalisation_layer"
_DENSE_LAYERS = ("dense_layer_no_bias", "dense_layer_with_bias", "classification_layer_no_bias", "classification_layer_with_bias")
_ML = (_NORMALISE,) + _DENSE_LAYERS
_SVM = "svm_predict"
_OWN_KERNEL = (_MULTI_EXTREMA, _HISTOGRAM, _HISTOGRAM_STATS, _MULTI_TPT, _TIME_OVER, _PSD, _SORT, _INTERP, _REFLECT, _RC_CR2, _BI_LEVEL, _PEAK_SNR, _MULTI_A) + _TAILFIT + _ALIGN + _ML + (_SVM,)  # processors that run as stages ahead of the program, on kernels of their own
_SAME_DIM = ("bl_subtract", "numpy_subtract", "numpy_add", "min_max_norm", "pole_zero", "double_pole_zero", "trap_filter", "trap_norm", "asym_trap_filter", "moving_window_multi", _SORT, _NORMALISE, _REFLECT, _RC_CR2, _LOG_CHECK, _INL, _WF_CORR)
# processors whose result may take the place of their source waveform
_IN_PLACE = ("bl_subtract", "numpy_subtract", "numpy_add", "min_max_norm", "pole_zero", "double_pole_zero")


def _add_step(b: _Builder, key, node, new_vars, proc_strings):
    module, function = node["module"], node["function"]
    b.cur_key = key
    if module is None:  # inline expression: alias / constant / the result of operators and functions of the language (reference :2676-2696)
        val = b.eval_arg(node["args"][0])
        if isinstance(val, Char):
            raise ProcessingChainError(f"'{key}': {val!r} is not a value")
        if isinstance(val, (Var, SExpr, View)):
            if isinstance(val, (Var, SExpr)) and "#" in val.name and not val.is_input:
                val.name = new_vars[0]  # (an expression's result takes the name the recipe gives it)
            if "unit" in node and isinstance(val, (Var, SExpr)) and val.unit is None and isinstance(node["unit"], str):
                val.unit = node["unit"]
            b.vars[new_vars[0]] = val
        else:
            b.vars[new_vars[0]] = Var(new_vars[0], "const", const=val)
        return
    if not module_accepted(module, function):
        raise NotImplementedError(f"module '{module}' is not available on the device path (processor {module}.{function})")
    if module in ("numpy", "np") and function == "copyto":
        # numpy.copyto(dst, src) as a processor: the copy of a (variable-length) array into a declared output (reference
        # tests/test_processing_chain.py:656-674)
        args = [b.eval_arg(a, new_vars) for a in node["args"]]
        if len(args) != 2 or not isinstance(args[0], Var) or args[0].length is None or not _is_wf(args[1]):
            raise ProcessingChainError(f"numpy.copyto takes a declared output array and an array for parameter {key}")
        dst, src = args
        if src.length < dst.length:
            raise ProcessingChainError(f"numpy.copyto for parameter {key}: the output holds {dst.length} samples, the source only {src.length}")
        dst.kind = "wf"
        dst.dtype = dst.dtype if dst.dtype is not None else np.dtype(np.float32)
        lo = src.lo if isinstance(src, View) else 0
        b._step("slice", [src if src.length == dst.length else View(src.base, lo, lo + dst.length), 0, 1, dst], "wiiW")
        return
    if module in ("numpy", "np") and function not in ("amax",) + tuple(_NUMPY_BINARY):
        raise NotImplementedError(f"numpy.{function} is not available on the device path")
    if "unit" in node:  # "unit": one string, or one per new variable (reference :2705-2711)
        for i, name in enumerate(new_vars):
            unit = node["unit"][i] if isinstance(node["unit"], (list, tuple)) else node["unit"]
            v = b.vars.get(name)
            if v is None:
                b.vars[name] = Var(name, None, unit=unit)
            elif isinstance(v, Var) and v.unit is None:
                v.unit = unit
    args = [b.eval_arg(a, new_vars) for a in node["args"]]
    if module in ("numpy", "np") and function in _NUMPY_BINARY:
        # a NumPy binary ufunc as a processor (numpy.subtract(waveform, bl_mean, wf_blsub), numpy.divide(A_max, trapEmax, AoE)):
        # between per-event values it is the same scalar op the operators make; waveform -/+ per-event value is the subtraction of
        # bl_subtract without its NaN rule (a NaN sample stays a NaN sample)
        if len(args) != 3 or not isinstance(args[2], Var):
            raise ProcessingChainError(f"numpy.{function} takes two operands and an output variable for parameter {key}")
        x, y, out = args
        if _is_wf(x) and not _is_wf(y) and function in ("subtract", "add"):
            function = "numpy_subtract" if function == "subtract" else "numpy_add"
        elif _is_wf(x) or _is_wf(y):
            # the ufunc on waveforms, as the operator of the language makes it (one NumPy loop per sample); the declared output names the result
            val = b._wf_binop(_NUMPY_BINARY[function](), x, y, f"numpy.{function}({', '.join(map(str, node['args']))})")
            if out.length is not None and out.length != val.length:
                raise ProcessingChainError(f"failed to broadcast array dimensions for {function}: '{out.name}' holds {out.length} samples, the operands {val.length}")
            val.name = out.name
            val.unit = out.unit if out.unit is not None else val.unit
            val.grid = out.grid if out.grid is not None else val.grid
            b.vars[new_vars[0]] = val
            return
        else:
            b.vars[new_vars[0]] = b._scalar_binop(_NUMPY_BINARY[function](), x, y, str(node["args"]), declared=out)
            return
    if function in _GENERATORS:
        _fold_generator(b, function, args, new_vars)
        return
    if function == "fft":
        raise NotImplementedError(f"processor 'fft' ({key}): complex variables are not in the recipe language; the gufunc dspeed_amd.processors.fft "
                                  "and the C entry dsp_fft are the interface (psd runs in recipes)")
    if function not in _SIGS or (function in (_PEAK_SNR, _MULTI_A) and module in _MODULES):
        # (peak_snr_threshold and multi_a_filter are reached through their files' module strings, dspeed.processors.peak_snr_threshold and
        # dspeed.processors.multi_a_filter, as the SiPM configs write them; under the package's string they stay refused, in these words:
        # tests/test_histogram_plan_cpu.py and the recorded translations hold that -- as they hold gaussian_filter1d's refusal)
        raise NotImplementedError(f"processor '{function}' is not implemented on the device path")
    if "init_args" in node and function not in (_POLY_FIT, _SVM):
        raise NotImplementedError(f"{function} ({key}): init_args builds a processor from a factory; on the device path only poly_fit is one")
    roles = _SIGS[function]
    if len(args) != len(roles):
        raise ProcessingChainError(f"{function} takes {len(roles)} arguments ({len(args)} given) for parameter {key}")
    # give the variables this processor creates their type now, so later recipe entries can slice / measure them
    src_len = None
    for a, r in zip(args, roles):
        if r == "w" and isinstance(a, (Var, View)):
            src_len = a.length
    for a, r in zip(args, roles):
        if r == "W" and isinstance(a, Var):
            if a.kind is None:
                a.kind = "wf"
            if a.length is None and function in _SAME_DIM:
                a.length = src_len
            a.dtype = np.dtype(np.float32)
            a.is_coord = False
    if function == _MULTI_EXTREMA:
        # its lists hold sample indices of the input: with a time unit they are coordinates on its grid, written in that unit like tp_max of
        # min_max (reference :1990-2014); its counts are uint32 (the gufunc's "II")
        for a in args[6:8]:
            if isinstance(a, Var) and _time_unit_ns(a.unit) is not None and _grid_of(args[0]) is not None:
                a.is_coord, a.grid = True, _grid_of(args[0])
        for a in args[8:10]:
            if isinstance(a, Var):
                a.out_dtype = np.dtype(np.uint32)
    if function == _BI_LEVEL:
        # its times are sample indices of the input, like the peak finder's lists; its count is uint32 (the gufunc's "I")
        if isinstance(args[7], Var) and _time_unit_ns(args[7].unit) is not None and _grid_of(args[0]) is not None:
            args[7].is_coord, args[7].grid = True, _grid_of(args[0])
        if isinstance(args[5], Var):
            args[5].out_dtype = np.dtype(np.uint32)
    if function in (_PEAK_SNR, _MULTI_A):
        # the output list is as long as the list read (the reference's ProcessorManager deduces m: the config declares no length); the
        # picker's list holds sample indices of the input, like the peak finder's; its count is uint32 (the gufunc's "I")
        lst, out = args[1], args[4 if function == _PEAK_SNR else 2]
        if isinstance(out, Var) and out.kind == "wf" and _is_wf(lst):
            if out.length is None:
                out.length = lst.length
            if function == _PEAK_SNR and _time_unit_ns(out.unit) is not None and _grid_of(args[0]) is not None:
                out.is_coord, out.grid = True, _grid_of(args[0])
        if function == _PEAK_SNR and isinstance(args[5], Var):
            args[5].out_dtype = np.dtype(np.uint32)
    inverse = _poly_fit_inverse(b, node, args, key) if function == _POLY_FIT else None
    svm = _svm_model(b, node, args, key) if function == _SVM else None
    if function == _SVM and svm is None:  # svm_file = 0: the label is the constant NaN, as the reference's null processor leaves it
        loop = np.float64 if loop_suffix(args[0].dtype if args[0].dtype is not None else np.float32) == "f64" else np.float32  # (the type the staged label would have)
        b.vars[args[1].name] = Var(args[1].name, "const", const=loop(np.nan))
        return
    if function == _MULTI_TPT:
        # its thresholds are one constant list, or a list per event read from rows in memory; its times are sample indices of the input:
        # with a time unit they are coordinates on its grid, written in that unit like the peak finder's lists
        args[1] = _as_threshold_list(b, args[1], key)
        t_out = args[5]
        if isinstance(t_out, Var) and t_out.kind == "wf":
            if t_out.length is None:
                t_out.length = args[1].length
            if _time_unit_ns(t_out.unit) is not None and _grid_of(args[0]) is not None:
                t_out.is_coord, t_out.grid = True, _grid_of(args[0])
    if function in _ML:
        args = _layer_arguments(b, function, args, key)
    if function in (_INL, _WF_CORR):
        args = _table_argument(b, function, args, key)
    if function == _WF_ALIGN:
        _alignment_output(args, key)
    args = [_as_taps(b, a, function) if r == "t" else a for a, r in zip(args, roles)]
    args = [_group_constant(b, a, function, key) if r == "i" and isinstance(a, (Var, SExpr)) else a for a, r in zip(args, roles)]
    _, args = _resolve(b, roles, args, same_dim_out=function in _SAME_DIM)
    if inverse is not None:
        args = list(args) + [inverse]  # (behind the arguments the roles name: a constant of the step)
    if svm is not None:
        args = list(args) + svm  # (likewise: the model's five arrays, gamma and the kernel function)
    b.steps.append((function, args, key))
    proc_strings.append(f"{function}({', '.join(str(a.name if isinstance(a, (Var, SExpr)) else a) for a in args)})")


def _poly_fit_inverse(b: _Builder, node, args, key):
    """``poly_fit`` is a factory in the reference: ``init_args`` -- (length, deg), each an expression of the language, ``len(wf_logged)`` among
    them -- builds the gufunc (processing_chain.py:2723-2773).  Both are constants of the chain; the inverted matrix is formed here, once, and
    travels as a constant array behind the step's arguments: returned.  The coefficients are a row of ``deg + 1``: that is their length where the declaration
    gives none, and must be where it gives one."""
    from .processors import check_poly, check_poly_fit_init, poly_fit_inverse

    what = f"{_POLY_FIT} ({key})"
    init = node.get("init_args")
    if not isinstance(init, (list, tuple)) or len(init) != 2:
        raise ProcessingChainError(f"{what}: init_args holds length and deg, as the factory takes them")
    vals = []
    for name, a in zip(("length", "deg"), init):
        v = b.eval_arg(a) if isinstance(a, str) else a
        if isinstance(v, Var) and v.kind == "const":
            v = v.const
        if isinstance(v, (Var, SExpr, View)):
            raise NotImplementedError(f"{what}: {name} is a constant of the call on the device, not a per-event value")
        vals.append(v)
    try:
        length, deg = check_poly_fit_init(what, *vals)
    except ValueError as e:
        raise ProcessingChainError(str(e)) from None
    src, out = args
    if not _is_wf(src):
        raise ProcessingChainError(f"{what}: '{src}' is not a waveform")
    if not isinstance(out, Var):
        raise ProcessingChainError(f"{what}: the coefficients are a variable name")
    if out.length is None:
        out.length = deg + 1
    if out.length != deg + 1:
        raise ProcessingChainError(f"{what}: poly_pars holds deg + 1 = {deg + 1} coefficients ({out.length} declared)")
    check_poly(what, max(length, src.length), deg + 1)
    try:
        inv = poly_fit_inverse(length, deg)
    except np.linalg.LinAlgError as e:  # (length <= deg: the reference's factory raises there too)
        raise ProcessingChainError(f"{what}: the matrix of power sums over range({length}) cannot be inverted for deg = {deg} ({e})") from None
    return Var(f"inv#{out.name}", "taps", (deg + 1) ** 2, np.float64, const=np.ascontiguousarray(inv, dtype=np.float64))


def _svm_model(b: _Builder, node, args, key):
    """``svm_predict`` is a factory in the reference: ``init_args`` -- the file of the pickled SVC, a character constant or a ``db.`` value, or 0
    -- builds the gufunc (processing_chain.py:2723-2773).  The model is read here, once, at chain build (``processors.load_svm_model``): its
    arrays travel as float64 constants behind the step's arguments, with gamma and the kernel function: returned."""
    from .processors import SVM_KERNELS, check_svm, load_svm_model, svm_device_arrays

    what = f"{_SVM} ({key})"
    init = node.get("init_args")
    if not isinstance(init, (list, tuple)) or len(init) != 1:
        raise ProcessingChainError(f"{what}: init_args holds the file of the fitted SVC (or 0), as the factory takes it")
    src, out = args
    if not _is_wf(src):
        raise ProcessingChainError(f"{what}: '{src}' is not a waveform")
    if not isinstance(out, Var):
        raise ProcessingChainError(f"{what}: name the label")
    file = init[0]
    if isinstance(file, str):
        text = file.strip()
        file = text[1:-1] if len(text) >= 2 and text[0] == text[-1] and text[0] in "'\"" else (0 if text == "0" else text)
    if _is_number(file) and file == 0:
        return None  # (the null processor: NaN for every row, nothing launched)
    if isinstance(file, (Var, SExpr, View)) or _is_number(file):
        raise ProcessingChainError(f"{what}: init_args holds the file of the fitted SVC (or 0), as the factory takes it")
    model = load_svm_model(file)
    n_sv, n = model["support_vectors"].shape
    check_svm(what, max(n, src.length), model["classes"].size, n_sv)
    if src.length != n:
        raise ProcessingChainError(f"{what}: '{src.name if hasattr(src, 'name') else src}' holds {src.length} samples, the model's support vectors {n}")
    consts = []
    for name, arr in zip(("support_vectors", "sv_norms", "coefficients", "intercepts", "classes"), svm_device_arrays(model)):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        consts.append(Var(f"{name}#{out.name}", "taps", int(arr.size), np.float64, const=arr))
    return consts + [float(model["gamma"]), SVM_KERNELS.index(model["kernel"])]


class _PerEventInteger(Exception):
    """an integer parameter of a processor is a column of the input table: the chain is built per value of it (GroupedProcessingChain)"""

    def __init__(self, column):
        super().__init__(column)
        self.column = column


def _group_constant(b: _Builder, a, function, key):
    """An INTEGER parameter of a processor (the rise and flat times of a trapezoid, a wavelet level, the number of moving windows) given as
    a per-event variable.  The reference broadcasts the variable's buffer into the gufunc's "()" slot, if its type can be cast to the
    signature's (:1565-1572, 1702-1745).  The device program holds such parameters as constants -- they size loops and LDS --, so the rows
    are grouped by the column's value and each group runs a chain built for it: here the column is replaced by the value of the group this
    chain is for, or reported to ``build_processing_chain``, which then returns a GroupedProcessingChain."""
    if isinstance(a, Var) and a.kind == "const":
        return a.const
    if not (isinstance(a, Var) and a.kind == "scalar" and a.is_input and a.source is not None and a.ext_key is None):
        raise NotImplementedError(f"{function} ({key}): the integer parameter '{a.name}' is computed per event inside the recipe; the device "
                                  "programs take integer parameters as constants or as columns of the input table (rows grouped by value)")
    if not np.can_cast(a.dtype, np.int32):  # ("fii->f" and the like: the column must cast to the signature's 'i', reference :1565-1572)
        raise ProcessingChainError(f"could not find a type signature matching the types of the variables given for {function} ({a.name} is {a.dtype})")
    if a.source not in b.group_values:
        raise _PerEventInteger(a.source)
    return int(b.group_values[a.source])


def _as_taps(b: _Builder, a, function):
    """A constant array given where a processor takes its kernel -- a list literal, loadlh5(...), or a recipe entry holding one -- becomes
    the same kind of variable a kernel generator leaves.  The reference passes the array itself, and its type takes part in the choice of
    the loop (:1565-1572): a float64 or integer array selects the processor's float64 loop, which the float32 chain does not run."""
    arr = a.const if isinstance(a, Var) and a.kind == "const" and isinstance(a.const, np.ndarray) else a
    if not isinstance(arr, np.ndarray):
        return a
    if arr.ndim != 1 or arr.size < 1:
        raise ProcessingChainError(f"{function}: the kernel must be a one-dimensional array, not one of shape {arr.shape}")
    if not np.can_cast(arr.dtype, np.float32):
        raise NotImplementedError(f"{function}: a {arr.dtype.name} kernel selects the float64 loop of the processor in the reference; give it "
                                  "as float32 values")
    b._anon += 1
    name = a.name if isinstance(a, Var) else f"kernel#{b._anon}"
    return Var(name, "taps", int(arr.size), np.float32, const=np.ascontiguousarray(arr, dtype=np.float32))


def _as_threshold_list(b: _Builder, a, key):
    """The thresholds of ``multi_time_point_thresh``: a constant array (a list literal, a database array, loadlh5(...), or a recipe entry
    holding one) becomes one list for every row, in the loop's float32; a two-dimensional input column or a stage's waveform stays what it
    is: a list per event, in memory.  (The reference hands a float64 list to the float64 loop of the gufunc: here the list is cast.)"""
    fn = _MULTI_TPT
    arr = a.const if isinstance(a, Var) and a.kind in ("const", "taps") and isinstance(a.const, np.ndarray) else a
    if isinstance(arr, np.ndarray):
        if arr.ndim != 1 or arr.size < 1 or arr.dtype.kind not in "fiu":
            raise ProcessingChainError(f"{fn} ({key}): the thresholds are a one-dimensional array of numbers, not {arr.dtype.name} of shape {arr.shape}")
        if arr.size > _lib.THRESH_MAX:
            raise NotImplementedError(f"{fn} ({key}): at most {_lib.THRESH_MAX} thresholds ({arr.size} given): a wavefront keeps one per lane")
        b._anon += 1
        name = a.name if isinstance(a, Var) else f"thresholds#{b._anon}"
        return Var(name, "taps", int(arr.size), np.float32, const=np.ascontiguousarray(arr, dtype=np.float32))
    if _is_wf(a):
        if a.length > _lib.THRESH_MAX:
            raise NotImplementedError(f"{fn} ({key}): at most {_lib.THRESH_MAX} thresholds ({a.length} given): a wavefront keeps one per lane")
        return a
    raise ProcessingChainError(f"{fn} ({key}): the thresholds are a constant array or an array per event, not {a!r}")


def _layer_arguments(b: _Builder, function, args, key):
    """The constant arrays of a neural-network layer (ml.py): weights, bias, means and variances are a ``db.`` value, a list literal,
    loadlh5(...), or a recipe entry holding one -- one array for every row, cast to the loop's float32 once, here (the reference hands a
    float64 array to the float64 loop of the gufunc, like a float64 threshold list).  The weights of a dense layer are two-dimensional and
    give an undeclared output its length; a classification layer's are one-dimensional, its bias one number."""
    classify = function.startswith("classification")
    names = {_NORMALISE: ("means", "variances")}.get(function, ("kernel", "bias"))
    dims = {_NORMALISE: (1, 1)}.get(function, (1 if classify else 2, 0 if classify else 1))
    args = list(args)
    for k, (name, ndim) in enumerate(zip(names, dims), start=1):
        if _SIGS[function][k] != "a":
            break
        a = args[k]
        arr = a.const if isinstance(a, Var) and a.kind in ("const", "taps") and a.const is not None else a
        if isinstance(arr, (list, tuple)) or (ndim == 0 and _is_number(arr)):
            arr = np.asarray(arr)
        if not isinstance(arr, np.ndarray):
            raise NotImplementedError(f"{function} ({key}): {name} is a constant array -- a db. value, a list, loadlh5(...) or a recipe entry holding "
                                      f"one --, not a per-event value ({a!r})")
        if arr.ndim != ndim or arr.size < 1 or arr.dtype.kind not in "fiu":
            raise ProcessingChainError(f"{function} ({key}): {name} is {'a number' if ndim == 0 else f'a {ndim}-dimensional array of numbers'}, "
                                       f"not {arr.dtype.name} of shape {arr.shape}")
        b._anon += 1
        args[k] = Var(a.name if isinstance(a, Var) else f"{name}#{b._anon}", "taps", int(arr.size), np.float32, const=np.ascontiguousarray(arr, dtype=np.float32))
    src, out = args[0], args[-1]
    if _is_wf(src):
        n = src.length
        if function == _NORMALISE:
            wrong = next((f"{nm} holds {a.length} values" for nm, a in zip(names, args[1:3]) if a.length != n), None)
        else:
            wrong = None if args[1].const.shape[0] == n else f"kernel has shape {args[1].const.shape}"
            if wrong is None and len(names) > 1 and _SIGS[function][2] == "a" and args[2].length != (1 if classify else args[1].const.shape[1]):
                wrong = f"bias holds {args[2].length} values"
        if wrong:
            raise ProcessingChainError(f"{function} ({key}): '{src.name}' holds {n} samples, {wrong}")
        if not classify and function != _NORMALISE and isinstance(out, Var) and out.kind in (None, "wf"):
            m = int(args[1].const.shape[1])
            if out.length is None:
                out.kind, out.length = "wf", m
            elif out.length != m:
                raise ProcessingChainError(f"{function} ({key}): '{out.name}' holds {out.length} samples, the kernel has {m} columns")
    return args


def _table_argument(b: _Builder, function, args, key):
    """The constant array of ``inl_correction`` (inl) and ``wf_correction`` (w_corr): a ``db.`` value, a list literal, loadlh5(...) or a recipe
    entry holding one -- one array for every row, cast to the loop's float32 once, here, as the layers' weights are."""
    name = "inl" if function == _INL else "w_corr"
    args = list(args)
    a = args[1]
    arr = a.const if isinstance(a, Var) and a.kind in ("const", "taps") and a.const is not None else a
    if isinstance(arr, (list, tuple)):
        arr = np.asarray(arr)
    if not isinstance(arr, np.ndarray):
        raise NotImplementedError(f"{function} ({key}): {name} is one constant array of the call on the device, not an array per event ({a!r})")
    if arr.ndim != 1 or arr.size < 1 or arr.dtype.kind not in "fiu":
        raise ProcessingChainError(f"{function} ({key}): {name} is a one-dimensional array of numbers, not {arr.dtype.name} of shape {arr.shape}")
    b._anon += 1
    args[1] = Var(a.name if isinstance(a, Var) else f"{name}#{b._anon}", "taps", int(arr.size), np.float32, const=np.ascontiguousarray(arr, dtype=np.float32))
    return args


def _alignment_output(args, key):
    """``wf_alignment`` writes ``size`` samples: that is the output's length where the declaration gives none"""
    size, out = args[3], args[4]
    if isinstance(size, Var) and size.kind == "const":
        size = size.const
    if isinstance(out, Var) and out.kind == "wf" and out.length is None and _is_number(size) and float(size) == int(float(size)) and size > 0:
        out.length = int(size)


def _fold_generator(b: _Builder, function, args, new_vars):
    """Kernel generators (cusp_filter, zac_filter, t0_filter, moving_slope) with constant arguments run once, here, on the host
    (reference :2797-2813)."""
    from . import processors as P

    *scal, out = args
    if not isinstance(out, Var) or out.length is None:
        raise ProcessingChainError(f"{function}: the kernel argument must be declared as name(length, 'f')")
    period = b.default_period
    vals = []
    for s in scal:
        if isinstance(s, Quantity):
            if period is None:
                raise ProcessingChainError(f"{function}: time quantity without a sampling period")
            s = float(s) / period
        if isinstance(s, (Var, View, Char)):
            raise NotImplementedError(f"{function} with per-event arguments is not supported")
        vals.append(float(s))
    k = np.zeros(out.length, dtype=np.float32)
    getattr(P, function)(*vals, k)
    out.kind, out.const, out.dtype = "taps", k, np.dtype(np.float32)


# ----------------------------------------------------------------------------------------------------------------
# program generation
# ----------------------------------------------------------------------------------------------------------------
def _loop_dtype(b: _Builder):
    """float32 loop unless an input selects the float64 one (first castable signature wins, reference :1565-1572, 1654-1664):
    float64 / int32 / uint32 waveforms or float64 scalar columns cannot be cast to float32."""
    for v in b.vars.values():
        if isinstance(v, Var) and v.is_input and v.dtype is not None:
            if v.source is not None and v.source.endswith(".t0"):
                continue  # the time of sample 0 is a coordinate offset, not a processor argument: a float64 t0 column (what LH5 files hold)
                # does not make the processors run their float64 loops (the value enters coordinate conversions in the loop's type)
            if v.kind == "wf" and v.dtype in (np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.uint32)):
                return np.dtype(np.float64)
            if v.kind == "scalar" and v.dtype == np.dtype(np.float64):
                return np.dtype(np.float64)
    return np.dtype(np.float32)

# ----------------------------------------------------------------------------------------------------------------
# steps: (processor name, arguments, recipe key); what every pass asks of them
# ----------------------------------------------------------------------------------------------------------------
def _is_number(x) -> bool:
    """a plain number: not a bool, not a ``Quantity``"""
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, Quantity))


def _is_integral(x) -> bool:
    return _is_number(x) and float(x) == int(float(x))


def _leaves(a, acc):
    """the variables an argument is made of (an expression's operands, the waveform under a slice), appended to ``acc``"""
    if isinstance(a, SExpr):
        for x in a.args:
            _leaves(x, acc)
    elif isinstance(a, (Var, View)):
        acc.append(a.base)
    return acc


def _base_of(a):
    """the waveform variable of an argument, whole or under a slice (None: not a waveform argument)"""
    return a.base if isinstance(a, (Var, View)) else None


def _outputs_of(step):
    return [a for a, r in zip(step[1], _roles(step[0])) if r in "WS"]


def _inputs_of(step):
    return [a for a, r in zip(step[1], _roles(step[0])) if r not in "WS"]


def _reads(step, v) -> bool:
    """does the step read the waveform v, whole or through a slice"""
    return any(_base_of(a) is v for a in _inputs_of(step))


def _without(steps, gone):
    return [x for x in steps if not any(x is g for g in gone)]


def _live_steps(b: _Builder, steps, out_pars):
    """the steps the outputs depend on, in their order"""
    needed = {id(v) for o in out_pars for v in _leaves(b.vars.get(o), [])}
    live = []
    for st in reversed(steps):
        if any(id(v) in needed for a in _outputs_of(st) for v in _leaves(a, [])):
            live.append(st)
            for a in _inputs_of(st):
                needed.update(id(v) for v in _leaves(a, []))
    return live[::-1]


def _schedule(steps):
    """Order the processors so that few waveforms are alive at a time -- every waveform variable of a chain lives in LDS, and the
    LDS a waveform needs decides how many run per compute unit.  The reference's order (depth-first from the outputs,
    processing_chain.py:2601-2651) is one valid order of a dependency graph; the processors are pure, so any other valid order
    computes the same values.  List scheduling with two rules: a processor that only reduces waveforms to numbers runs as soon as its
    operands exist (it can only end lifetimes); among the ones that create a waveform, the one reading the oldest waveform goes
    first (finish with a waveform before starting on newer ones), an element-wise or recursive filter that may then take its place
    last; a processor whose result could not be consumed yet (a consumer waits for another operand) yields to the others."""
    producer = {}
    ins, creates = [], []
    for j, st in enumerate(steps):
        ins.append([v for a in _inputs_of(st) for v in _leaves(a, [])])
        creates.append("W" in _roles(st[0]))
        for a in _outputs_of(st):
            for v in _leaves(a, []):
                producer.setdefault(id(v), j)
    deps = [{producer[id(v)] for v in reads if id(v) in producer and producer[id(v)] != j} for j, reads in enumerate(ins)]
    consumers = [[] for _ in steps]
    for c, d in enumerate(deps):
        for j in d:
            consumers[j].append(c)
    born = {}  # waveform -> position in the new order of the processor that made it (inputs: -1)
    order, done = [], set()
    while len(order) < len(steps):
        ready = [j for j in range(len(steps)) if j not in done and deps[j] <= done]
        if not ready:  # (cannot happen for steps that came out of the dependency resolution; keep the given order)
            return steps
        reducers = [j for j in ready if not creates[j]]
        if reducers:
            j = reducers[0]
        else:
            def age(j):
                wfs = [born.get(id(v), -1) for v in ins[j] if v.kind == "wf"]
                return min(wfs) if wfs else len(steps)
            def waits(j):  # a consumer of what j makes still lacks an operand that does not itself come from j: j's waveform
                family, todo = {j}, [j]  # would sit in LDS until that arrives
                while todo:
                    for c in consumers[todo.pop()]:
                        if c not in family:
                            family.add(c)
                            todo.append(c)
                return any(deps[c] - done - family for c in consumers[j])
            # (same oldest waveform: the one that could overwrite it in place waits until the others have read it)
            j = min(ready, key=lambda j: (waits(j), age(j), steps[j][0].startswith("ew:") or steps[j][0] in _IN_PLACE, j))
        for a, r in zip(steps[j][1], _roles(steps[j][0])):
            if r == "W" and isinstance(a, Var):
                born[id(a)] = len(order)
        order.append(j)
        done.add(j)
    return [steps[j] for j in order]


#: taps from which a convolve_wf / fft_convolve_wf goes to the matrix-core FIR kernels ahead of the program (dsp_fir_mfma.hip needs 64)
STAGE_MIN_TAPS = 64


#: what the run-length FIR kernel takes (DSP_FIR_RUNS_MAX / DSP_FIR_RUNS_MAX_TAPS of csrc/dsp_program.h)
FIR_RUNS_MAX, FIR_RUNS_MAX_TAPS = 24, 512


def _piecewise_constant(taps) -> bool:
    """Is the kernel a few runs of equal taps (``t0_filter``: a ramp of 8 and a plateau of 125; moving averages)?  Then convolve_wf is a
    handful of differences of prefix sums per output instead of a multiply-add per tap (csrc/dsp_fir_runs.hip)."""
    k = np.asarray(taps, dtype=np.float32)
    if k.ndim != 1 or not 1 <= k.size <= FIR_RUNS_MAX_TAPS or not np.isfinite(k).all():
        return False
    edges = np.concatenate([[np.float32(0)], k, [np.float32(0)]])
    return int(np.count_nonzero(edges[1:] != edges[:-1])) <= FIR_RUNS_MAX + 1


def _stage_record(what, program, consts, in_vars, alias, outs, **more):
    """a program that runs ahead of the main one, as the runtime reads it: ``outs`` are (its binding, the binding later programs read the
    buffer under, samples or None for a column); the device chain and the buffers are made on first use"""
    return {"what": what, "program": program, "consts": consts, "in_vars": in_vars, "alias": alias, "outs": outs, **more, "chain": None, "bufs": {}}


#: how many of each the reductions kernels take in one program (dsp_reduce.hip, and dsp_fir_runs.hip on the waveform it has just filtered)
_REDUCTIONS_MAX = {"min_max": 1, "amax": 1, "fixed_time_pickoff": 4, "time_point_thresh": 2}


def _within_reductions_max(group) -> bool:
    by_fn = [g[0] for g in group]
    return all(by_fn.count(fn) <= most for fn, most in _REDUCTIONS_MAX.items())


class _Stager:
    """What the stage families of ``_extract_stages`` share: the steps still left to the program, the stages made so far in launch order,
    the names of the recipe's outputs, and the questions they ask of the steps."""

    def __init__(self, b: _Builder, steps, out_pars, n_rows, ft):
        self.b, self.steps, self.n_rows, self.ft = b, steps, n_rows, ft
        self.stages = []
        self.out_names = set(out_pars)
        for o in out_pars:
            self.out_names.update(v.name for v in _leaves(b.vars.get(o), []))

    def has(self, st) -> bool:
        return any(st is x for x in self.steps)

    def steps_of(self, fn, only=None):
        """the steps of processor ``fn`` that are still in the program when their turn comes (an earlier one's stage may have taken them, or
        a reader of theirs that was staged first: ``_stage_producers``); ``only``: that step alone"""
        for st in list(self.steps):
            if st[0] == fn and self.has(st) and (only is None or st is only):
                yield st

    def replace(self, old, new):
        """the step ``new`` in the place of ``old``; returns it"""
        self.steps = [new if x is old else x for x in self.steps]
        return new

    def producer_of(self, v):
        for st in self.steps:
            if any(a is v for a in _outputs_of(st)):
                return st
        return None

    def users_of(self, v, but=None):
        return [x for x in self.steps if x is not but and _reads(x, v)]

    def only_user(self, v, fn_name):
        users = self.users_of(v)
        return users[0] if len(users) == 1 and users[0][0] == fn_name and users[0][1][0] is v and v.name not in self.out_names else None

    @staticmethod
    def plain_scalar(x) -> bool:  # a constant, a per-event input column or a fit / stage result: in HBM before the stage runs
        if isinstance(x, Var):
            return x.kind == "scalar" and x.sreg is None and ((x.is_input and x.source is not None) or x.ext_key is not None)
        if isinstance(x, SExpr):  # (an expression a stage of its own has evaluated: stage_expression)
            return x.op == "ext" and x.ext_key is not None
        return _is_number(x)

    @staticmethod
    def row_input(v) -> bool:  # rows of the input table or of an earlier stage
        return isinstance(v, Var) and v.kind == "wf" and ((v.is_input and v.source is not None) or v.ext_key is not None)

    def ancestors(self, v):
        """steps that compute v from inputs and earlier results, in order"""
        want, todo = [], [v]
        seen = set()
        while todo:
            x = todo.pop()
            if id(x) in seen or self.row_input(x):
                continue
            seen.add(id(x))
            st = self.producer_of(x)
            if st is None:
                continue
            if not any(st is w for w in want):
                want.append(st)
            for a in _inputs_of(st):
                todo.extend(_leaves(a, []))
        return [st for st in self.steps if any(st is w for w in want)]

    def rows_steps(self, v):
        """steps that read only the rows v and per-event values already in HBM and make per-event values only; in order, closed under
        their own results"""
        made, picked = set(), []
        for st in self.steps:
            ins, outs = _inputs_of(st), _outputs_of(st)
            if not outs or "W" in _roles(st[0]) or not any(a is v for a in ins if isinstance(a, Var)):
                continue
            others = [a for a in ins if a is not v and isinstance(a, (Var, SExpr, View))]
            if all(isinstance(a, Var) and (self.plain_scalar(a) or id(a) in made) for a in others) and all(isinstance(o, Var) for o in outs):
                picked.append(st)
                made.update(id(o) for o in outs)
        return picked

    def reads_off_row(self, st, extremes=()) -> bool:
        """what the reductions kernels read off a row (dsp_reduce.hip; dsp_fir_runs.hip off the waveform it has just filtered): min_max,
        numpy.amax, a sample at a constant integral time, time_point_thresh from a constant sample -- or from one of ``extremes``, the t_min /
        t_max of a min_max in the same launch"""
        if st[0] in ("min_max", "amax"):
            return True
        if st[0] == "fixed_time_pickoff":
            return _is_integral(st[1][1])
        if st[0] == "time_point_thresh":
            _w, thr, start, walk, _o = st[1]
            return ((_is_number(thr) or self.plain_scalar(thr)) and _is_number(walk) and float(walk) in (0.0, 1.0)
                    and (_is_integral(start) or any(start is o for o in extremes)))
        return False

    def stage(self, group, scalars, what, wf=None, drop=None, wfs=(), rows_first=False):
        """Compile the steps ``group`` (on copies of the variables) into a program of its own that writes the per-event values ``scalars``
        and the waveforms ``wf`` / ``wfs`` (stored ahead of the per-event values with ``rows_first``); from here on these are columns / rows
        in HBM, and the steps ``drop`` (default: the group) leave the program.  A per-event value with an ``out_dtype`` travels in that type."""
        rows = ([wf] if wf is not None else []) + list(wfs)
        b, outs = self.b, (rows + list(scalars)) if rows_first else (list(scalars) + rows)
        vars2, steps2 = copy.deepcopy((b.vars, group))
        b2 = copy.copy(b)
        b2.vars, b2.steps, b2._conversions, b2.stage_ft = vars2, list(steps2), {}, self.ft
        for v in vars2.values():
            if isinstance(v, Var) and v.aux_io is not None:
                v.aux_io = None  # (an index into the main program's bindings; the stage binds the fit's column by its name)
        pc, _tb = _compile(b2, [o.name for o in outs], self.n_rows, [], stage_mode=True)
        self.stages.append(_stage_record(what, pc._program, pc._consts, pc._in_vars, pc._ext_alias,
                                         [(f"out:{o.name}", f"in:{o.name}", o.length if o.kind == "wf" else None) for o in outs],
                                         out_dtypes={f"in:{o.name}": o.out_dtype for o in outs if o.out_dtype is not None}))
        for o in outs:
            if o.kind == "wf":  # pole_zero returns an all-NaN waveform for an input with a NaN and DSPFatal for a NaN of its own making
                made_by = self.producer_of(o)
                o.nan_uniform = made_by is not None and made_by[0] == "pole_zero"
            o.ext_key, o.is_input, o.slot, o.sreg = f"in:{o.name}", True, None, None
            if o.kind == "wf":
                o.ext_len, o.offset, o.dtype = o.length, 0, np.dtype(np.float32)
        for o in scalars:
            o.kind = "scalar"
            if o.out_dtype is not None:
                o.ext_dtype = o.out_dtype
        self.steps = _without(self.steps, group if drop is None else drop)

    def stage_expression(self, a, what):
        """A per-event operand of a kernel that reads its operands as float32 columns, evaluated by a small program of its own: an expression
        between values that are in HBM (0.5 * bl_std), or a column of another type.  Returns the operand as the kernel's stage reads it."""
        if not isinstance(a, SExpr):
            a = SExpr("func", (_lib.FN_COPY, a), f"float32({a.name})", a.unit, a.is_coord, a.grid)
        self.b.vars[a.name] = a  # (an output of the small program, by its name)
        self.stage([], [a], what)
        del self.b.vars[a.name]
        a.op, a.args, a.ext_dtype, a.io = "ext", (), self.ft, None
        return a

    def move_ahead(self, operands) -> bool:
        """What computes these per-event operands from rows in HBM (min_max of the t0-filtered waveform, the t0 estimate) moves ahead of the
        program, as a small program of its own on the same rows.  False, and nothing moved, if one of them is not computed that way."""
        movers = []
        for a in operands:
            pst = self.producer_of(a) if isinstance(a, Var) else None
            rows_v = next((x for x in _inputs_of(pst) if isinstance(x, Var) and self.row_input(x)), None) if pst else None
            group = self.rows_steps(rows_v) if rows_v is not None else []
            if pst is None or not any(pst is g for g in group):
                return False
            movers.append((rows_v, group))
        for rows_v, group in movers:
            group = [g for g in group if self.has(g)]  # (two operands off the same rows: moved with the first)
            if group:
                self.stage(group, [o for g in group for o in _outputs_of(g)], f"per-event values of {rows_v.name}")
        return True


def _fir_input_as_rows(cx: _Stager, base):
    """The FIR kernels read rows from HBM.  Returns what joins the filter's own stage ahead of it: nothing for a chain input or what a
    stage wrote (made here, if need be, by a small program that writes the filter's input to HBM), the bl_subtract of an input that is done
    while staging; None if the input cannot become rows."""
    _stage_producers(cx, base)
    if cx.row_input(base):
        return []
    pst = cx.producer_of(base)
    if (pst is not None and pst[0] == "bl_subtract" and cx.row_input(_base_of(pst[1][0])) and cx.plain_scalar(pst[1][1])
            and base.name not in cx.out_names):
        return [pst]
    anc = cx.ancestors(base)
    if not anc or any(a[0] in ("convolve_wf", "fft_convolve_wf") for a in anc):
        return None
    # min_max of the raw rows goes along: the pole-zero rows kernel streams them anyway (dsp_pz.hip), a launch of the
    # reductions kernel would read them once more
    extra, made = [], []
    raw = _base_of(anc[0][1][0]) if anc[0][0] in ("bl_subtract", "pole_zero") else None
    if (cx.ft == np.dtype(np.float32) and isinstance(raw, Var) and cx.row_input(raw) and [a[0] for a in anc] in (["bl_subtract", "pole_zero"], ["pole_zero"])
            and os.environ.get("DSPEED_HIP_NO_ROW_REDUCTIONS") != "1"):
        mm = [g for g in cx.rows_steps(raw) if g[0] == "min_max" and g[1][0] is raw]
        if len(mm) == 1:
            extra, made = mm, list(mm[0][1][1:5])
    cx.stage(extra + anc, made, f"{base.name} -> HBM" + (f" + min_max of {raw.name}" if extra else ""), wf=base, drop=extra)
    return []


def _stage_long_firs(cx: _Stager):
    """Each ``convolve_wf`` with a constant kernel of STAGE_MIN_TAPS or more taps, with its input as rows."""
    for st in list(cx.steps):
        fn, args, key = st
        if fn not in ("convolve_wf", "fft_convolve_wf") or not cx.has(st):
            continue
        taps, out = args[1], args[3]
        if not (isinstance(taps, Var) and taps.kind == "taps" and taps.const is not None and isinstance(out, Var) and out.length):
            continue
        m = int(taps.length)
        base, n_in = _base_of(args[0]), args[0].length
        if base is None or n_in is None or m < STAGE_MIN_TAPS or m > n_in or not np.isfinite(taps.const).all():
            continue
        mode = args[2].value[0] if isinstance(args[2], Char) else (chr(args[2]) if isinstance(args[2], (int, np.integer)) else None)
        want_len = {"v": n_in - m + 1, "s": n_in, "f": n_in + m - 1}.get(mode)
        if want_len is None or want_len != out.length:
            continue  # (the program's own op reports it)
        pre = _fir_input_as_rows(cx, base)
        if pre is None:
            continue
        # --- the filter itself; numpy.amax goes along when it is the only reader
        users = cx.users_of(out, but=st)
        if (len(users) == 1 and users[0][0] == "amax" and users[0][1][0] is out and out.name not in cx.out_names and isinstance(users[0][1][2], Var)
                and mode == "v" and out.length <= 320):  # (what the amax form of the kernel takes; else the filtered waveform is kept)
            cx.stage(pre + [st, users[0]], [users[0][1][2]], f"{fn} {key} + amax", drop=[st, users[0]])
            continue
        # a piecewise-constant kernel (the t0 filter) on float32 rows: prefix sums instead of products, and what the recipe reads off
        # the filtered waveform -- min_max, the threshold walk of the t0 estimate -- in the same pass; a filtered waveform that nothing
        # else reads then never reaches HBM (csrc/dsp_fir_runs.hip)
        group = []
        if (cx.ft == np.dtype(np.float32) and not pre and isinstance(args[0], Var) and cx.row_input(args[0]) and np.dtype(args[0].dtype) == np.dtype(np.float32)
                and n_in % 8 == 0 and _piecewise_constant(taps.const) and os.environ.get("DSPEED_HIP_NO_FIR_RUNS") != "1"):
            for g in cx.rows_steps(out):
                if g[1][0] is out and cx.reads_off_row(g, extremes=[o for x in group if x[0] == "min_max" for o in x[1][1:3]]):
                    group.append(g)
            if not _within_reductions_max(group):
                group = []
        if group:
            keep = out.name in cx.out_names or any(not any(x is g for g in group) for x in users)
            cx.stage([st] + group, [o for g in group for o in _outputs_of(g)], f"{fn} {key} on prefix sums + per-event values of {out.name}",
                     wf=out if keep else None)
        else:
            cx.stage(pre + [st], [], f"{fn} {key}", wf=out, drop=[st])


def _stage_short_traps(cx: _Stager):
    """Short trapezoids that only feed min_max / time_point_thresh, on rows: the lane-per-waveform kernel (dsp_rows.hip) runs the
    reference's recurrence as it is, 64 waveforms per instruction, where the program replays it twice per waveform (the t0 chain of the
    Ge recipes, asym_trap_filter -> time_point_thresh: a fifth of the program).  The kernel reads rows, so the trapezoid's input must
    be rows (an input or what a stage above wrote) and every per-event operand a column in HBM: what such an operand depends on --
    min_max of the t0-filtered waveform -- moves ahead of the program as well, as a small program of its own on the same rows."""
    for st in list(cx.steps):
        fn, args, key = st
        if fn not in ("trap_filter", "trap_norm", "asym_trap_filter") or not cx.has(st):
            continue
        src, dst = args[0], args[-1]
        ints = args[1:-1]
        if not (isinstance(src, Var) and cx.row_input(src) and isinstance(dst, Var) and dst.name not in cx.out_names and src.length and src.length % 8 == 0
                and src.length >= 16 and all(_is_integral(x) for x in ints)):
            continue
        iv = [int(x) for x in ints]
        lags = (iv[0], iv[0] + iv[1], iv[0] + iv[1] + iv[2]) if fn == "asym_trap_filter" else (iv[0], iv[0] + iv[1], 2 * iv[0] + iv[1])
        if min(lags) < 8 or (((max(lags) + 8 + 7) // 8) * 8 + 8) * 256 > 80 * 1024:
            continue
        users = cx.users_of(dst, but=st)
        kinds = sorted(x[0] for x in users)
        if kinds not in (["min_max"], ["time_point_thresh"], ["min_max", "time_point_thresh"]) or not all(x[1][0] is dst for x in users):
            continue
        mm_outs = [o for x in users if x[0] == "min_max" for o in x[1][1:5]]
        # per-event operands of the walk: in HBM already, the reduction's own t_min / t_max, or movable ahead of the program
        need = [a for x in users if x[0] == "time_point_thresh" for a in x[1][1:4] if isinstance(a, (Var, SExpr))]
        if not cx.move_ahead([a for a in need if not (isinstance(a, Var) and (cx.plain_scalar(a) or any(a is o for o in mm_outs)))]):
            continue
        cx.stage([st] + users, [o for x in users for o in _outputs_of(x)], f"{fn} {key} on rows")


def _stage_current_branch(cx: _Stager):
    """The current branch (windower -> avg_current -> upsampler -> moving_window_multi -> min_max, the A/E part of the Ge recipes) on
    rows: three moving averages that alternate direction are float32 recurrences over 4784 samples each -- 30 % of the program, which
    replays their rounding twice per pass.  dsp_current.hip gives every waveform a lane and runs them as written (bit-exact), keeping
    checkpoints instead of the intermediate waveforms.  Needs the window's source as rows in HBM and its start as a column there."""
    for st in list(cx.steps):
        if st[0] != "windower" or not cx.has(st):
            continue
        src, start, w_le = st[1]
        if not (isinstance(src, Var) and cx.row_input(src) and np.dtype(src.dtype) == np.dtype(np.float32) and isinstance(w_le, Var)):
            continue
        # the window's start (tp_0_est) is computed by the program from rows in HBM (the t0-filtered waveform): what computes it moves ahead
        # as a small program of its own on those rows, like the operands of the t0 chain's walk above
        if not cx.plain_scalar(start) and not cx.move_ahead([start]):
            continue
        chain_steps, v = [st], w_le
        for fn_name in ("avg_current", "upsampler", "moving_window_multi", "min_max"):
            nxt = cx.only_user(v, fn_name)
            if nxt is None:
                break
            chain_steps.append(nxt)
            v = nxt[1][-1]
        outs = list(chain_steps[-1][1][1:5])
        if len(chain_steps) == 5 and all(isinstance(o, Var) for o in outs):
            cx.stage(chain_steps, outs, f"current branch of {src.name} on rows")


def _stage_row_reductions(cx: _Stager):
    """Per-event values read straight off rows in HBM: min_max, numpy.amax and a sample at a constant integral time of an input or of a
    stage's waveform, a walk from a constant sample (from an extreme of the same rows: what the t0 chain above moves).  In the program they
    cost a LOAD of the whole row into LDS and a pass over it, at the occupancy the longest waveform leaves (one wavefront per SIMD for 8192
    samples); dsp_reduce.hip streams the row through registers once."""
    for v in [x for x in list(cx.b.vars.values()) if cx.row_input(x)]:
        if np.dtype(v.dtype) not in (np.dtype(np.float32), np.dtype(np.int16), np.dtype(np.uint16)):
            continue
        group = [g for g in cx.rows_steps(v) if cx.reads_off_row(g) and g[1][0] is v]
        if not group or not _within_reductions_max(group):
            continue
        rest = _without(cx.steps, group)
        if any(_reads(x, v) for x in rest):
            continue  # (the program loads these rows for something else as well: there the reduction is one more pass over LDS, no row traffic)
        if not any(r in "wW" for x in rest for r in _roles(x[0])):
            continue  # (the program would be left without a waveform: nothing gained by a launch of its own)
        cx.stage(group, [o for g in group for o in _outputs_of(g)], f"per-event values of {v.name} off its rows")


def _stage_multi_extrema(cx: _Stager, only=None):
    """``get_multi_local_extrema`` runs on dsp_extrema.hip and nowhere else (the interpreter has no such op), on rows in HBM: this stage is
    mandatory.  Rows that are chain inputs or a stage's waveform are read as they are; any other source is written to HBM first by a small
    program of its own, as a long filter's input is.  Per-event operands: constants, float32 columns of the input table, fit and stage
    results; what the program would compute off rows in HBM moves ahead of it (``move_ahead``); expressions of those and columns of other
    types go through a small program of their own (``stage_expression``)."""
    fn = _MULTI_EXTREMA
    for st in cx.steps_of(fn, only):
        args, key = list(st[1]), st[2]
        src, direction, lists, counts = args[0], args[3], args[6:8], args[8:10]
        if not _is_integral(direction):
            raise NotImplementedError(f"{fn} ({key}): search_direction must be a constant integer")
        if int(direction) == 2:
            raise NotImplementedError(f"{fn} ({key}): search_direction 2 (extrema found in both directions) is not implemented: the reference's "
                                      "branch reads the maxima with the minima's mask and defines no result to agree with")
        if not all(isinstance(v, Var) and v.kind == "wf" and v.length for v in lists) or not all(isinstance(v, Var) for v in counts):
            raise ProcessingChainError(f"{fn} ({key}): declare the lists as name(length) and name the counts")
        if int(direction) == 3 and lists[0].length > 64:
            raise NotImplementedError(f"{fn} ({key}): search_direction 3 takes lists of at most 64 entries ({lists[0].length} declared)")
        _rows_in_memory(cx, src, fn, key)
        for k in (1, 2, 4, 5):
            args[k] = _operand_in_memory(cx, args[k], fn, key)
        step = cx.replace(st, (fn, args, key))
        cx.stage([step], counts, f"{fn} {key} on rows", wfs=lists, rows_first=True)


def _operand_in_memory(cx: _Stager, a, fn, key, written_first=False):
    """A per-event operand of a kernel that reads its operands as constants or float32 columns (``_stage_multi_extrema`` says which it
    takes): returns it as the kernel's stage reads it, after moving ahead or evaluating what has to be.  ``written_first`` (the threshold
    kernel's operands) admits one more source: a per-event value that the program would read off a waveform it computes itself (the maximum
    of the baseline-subtracted waveform, for a threshold at half of it) is written to HBM first, with the other results of its processor,
    by a small program of its own -- as a source waveform is."""
    if not isinstance(a, (Var, SExpr)):
        if not (_is_number(a) or isinstance(a, Quantity)):
            raise NotImplementedError(f"{fn} ({key}): operand {a!r} is neither a number nor a per-event value")
        return a
    for leaf in _leaves(a, []):
        _stage_producers(cx, leaf)
    for leaf in _leaves(a, []) if written_first else ():
        pst = cx.producer_of(leaf) if isinstance(leaf, Var) and leaf.kind == "scalar" and not cx.plain_scalar(leaf) else None
        if pst is None or any(isinstance(x, Var) and cx.row_input(x) for x in _inputs_of(pst)):
            continue  # (in memory already, or read off rows in memory: ``move_ahead`` takes it)
        outs = _outputs_of(pst)
        if all(isinstance(o, Var) and o.kind == "scalar" for o in outs):
            cx.stage(cx.ancestors(leaf), outs, f"{leaf.name} -> HBM", drop=[])
    for leaf in _leaves(a, []):  # what the program would compute off rows in HBM moves ahead of it
        if not cx.plain_scalar(leaf) and not (leaf.kind == "scalar" and cx.move_ahead([leaf])):
            raise NotImplementedError(f"{fn} ({key}): operand '{a.name}' depends on '{leaf.name}', which is neither a constant, an input column, "
                                      "a fit or stage result nor computed off rows in memory")
    is_f32_column = isinstance(a, Var) and (a.ext_key is not None
                                            or np.dtype(_column(cx.b.tb_in, a.source).dtype) == np.dtype(np.float32))
    if not is_f32_column and not (isinstance(a, SExpr) and cx.plain_scalar(a)):
        return cx.stage_expression(a, f"{a.name} for {fn} {key}")
    return a


def _folded_normalisation(cx: _Stager, st) -> bool:
    """a normalisation that only dense or classification layers read, and the recipe does not ask for: it runs inside their launches"""
    out = st[1][3]
    return out.name not in cx.out_names and all(u[0] in _DENSE_LAYERS and u[1][0] is out for u in cx.users_of(out))


def _stage_producers(cx: _Stager, v):
    """Stages are made in the order the data flows.  Whatever ``v`` is computed from that runs on a kernel of its own is staged here, by its
    own family, before a reader of ``v`` is: the first such processor among ``v``'s ancestors has none above it, its stage takes it out of
    the program and makes its result rows in memory, where ``ancestors`` ends -- so every one of them is staged once, a producer ahead of
    its readers, and what is then left between them and ``v`` is work of the interpreter.  (A folded normalisation goes with its layer.)
    A family asked for a step that begins a fused group -- an ``rc_cr2``, a ``log_check``, a ``poly_fit`` -- stages the launch the step would
    have joined in the family's own turn, so a reader staged first costs no fusion."""
    while True:
        own = next((a for a in cx.ancestors(v) if a[0] in _OWN_KERNEL and not (a[0] == _NORMALISE and _folded_normalisation(cx, a))), None)
        if own is None:
            return
        _FAMILY_OF[own[0]](cx, only=own)
        if cx.has(own):
            raise NotImplementedError(f"{own[0]} ({own[2]}): cannot be staged ahead of what reads '{v.name}'")


def _rows_in_memory(cx: _Stager, src, fn, key):
    """the source of a kernel that reads rows in HBM: a chain input or a stage's waveform as it is, anything else written there first --
    behind the stages of the processors it comes from that own a kernel (``_stage_producers``)"""
    base = _base_of(src)
    if base is None:
        raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
    _stage_producers(cx, base)
    if not cx.row_input(base):
        anc = cx.ancestors(base)
        if not anc:
            raise NotImplementedError(f"{fn} ({key}): its source '{base.name}' cannot be written to rows in memory")
        cx.stage(anc, [], f"{base.name} -> HBM", wf=base, drop=[])


def _stage_histogram(cx: _Stager, only=None):
    """``histogram`` and ``histogram_stats`` run on dsp_hist.hip and nowhere else, on rows in HBM: mandatory stages, like the peak finder's.
    A ``histogram_stats`` that reads exactly a histogram's weights and borders joins its launch; weights and borders are then written only
    if something else reads them or the recipe asks for them.  Any other ``histogram_stats`` reads weights and edges as rows in memory."""
    for st in cx.steps_of(_HISTOGRAM, only):
        args, key = list(st[1]), st[2]
        weights, borders = args[1:3]
        if not all(isinstance(v, Var) and v.kind == "wf" and v.length for v in (weights, borders)):
            raise ProcessingChainError(f"{_HISTOGRAM} ({key}): declare the outputs as name(length): weights(bins), borders(bins + 1)")
        if borders.length != weights.length + 1:
            raise DSPFatal("length borders_out must be exactly 1 + length of weights_out")
        if weights.length > _lib.HIST_MAX_BINS:
            raise NotImplementedError(f"{_HISTOGRAM} ({key}): at most {_lib.HIST_MAX_BINS} bins ({weights.length} declared)")
        _rows_in_memory(cx, args[0], _HISTOGRAM, key)
        stats = next((x for x in cx.steps if x[0] == _HISTOGRAM_STATS and x[1][0] is weights and x[1][1] is borders), None)
        group, scalars = [st], []
        if stats is not None:
            sargs = list(stats[1])
            sargs[5] = _operand_in_memory(cx, sargs[5], _HISTOGRAM_STATS, stats[2])
            fused = cx.replace(stats, (_HISTOGRAM_STATS, sargs, stats[2]))
            group, scalars = [st, fused], sargs[2:5]
            if not all(isinstance(v, Var) for v in scalars):
                raise ProcessingChainError(f"{_HISTOGRAM_STATS} ({stats[2]}): name the three outputs")
        rows_wanted = any(v.name in cx.out_names or [u for u in cx.users_of(v) if not any(u is g for g in group)] for v in (weights, borders))
        cx.stage(group, scalars, f"{_HISTOGRAM} {key}" + (f" + {_HISTOGRAM_STATS} {stats[2]} in one launch" if stats is not None else "") + " on rows",
                 wfs=[weights, borders] if rows_wanted or stats is None else [], rows_first=True)
    for st in cx.steps_of(_HISTOGRAM_STATS, only):
        args, key = list(st[1]), st[2]
        for a in args[:2]:
            if not (isinstance(a, Var) and a.kind == "wf" and a.length):
                raise ProcessingChainError(f"{_HISTOGRAM_STATS} ({key}): weights_in and edges_in are whole arrays of a declared length")
        if args[1].length != args[0].length + 1:
            raise DSPFatal("length edges_in must be exactly 1 + length of weights_in")
        for a in args[:2]:
            _rows_in_memory(cx, a, _HISTOGRAM_STATS, key)
        args[5] = _operand_in_memory(cx, args[5], _HISTOGRAM_STATS, key)
        step = cx.replace(st, (_HISTOGRAM_STATS, args, key))
        cx.stage([step], args[2:5], f"{_HISTOGRAM_STATS} {key} on rows")


def _stage_thresholds(cx: _Stager, only=None):
    """``multi_time_point_thresh`` and ``time_over_threshold`` run on dsp_thresh.hip and nowhere else, on rows in HBM: mandatory stages, like
    the peak finder's.  Polarity and mode are constants, checked here for every row; t_start and time_over_threshold's threshold are
    per-event operands (``_operand_in_memory``); the thresholds are one constant list or rows in memory -- a two-dimensional input column
    or a stage's waveform --, not something the program would compute per event."""
    for st in cx.steps_of(_MULTI_TPT, only):
        fn, args, key = st[0], list(st[1]), st[2]
        src, thr, _t_start, polarity, mode, t_out = args
        if isinstance(polarity, Var) and polarity.kind == "const":
            polarity = polarity.const
        if not _is_number(polarity):
            raise NotImplementedError(f"{fn} ({key}): the polarity is a constant of the kernel, not a per-event value")
        if not (polarity > 0 or polarity < 0):
            raise DSPFatal("polarity cannot be 0")
        if not isinstance(mode, (Char, int, np.integer)):
            raise NotImplementedError(f"{fn} ({key}): the interpolation mode is a constant of the kernel, not a per-event value")
        code = _Emitter.char_of(mode)
        if not 0 < code < 128 or chr(code) not in "iafbcrnl":
            raise DSPFatal("Unrecognized interpolation mode")
        m = thr.length
        if not (isinstance(t_out, Var) and t_out.kind == "wf" and t_out.length == m):
            raise ProcessingChainError(f"{fn} ({key}): t_out holds a time per threshold: declare it as name({m})")
        _rows_in_memory(cx, src, fn, key)
        if not (isinstance(thr, Var) and thr.kind == "taps"):
            base = _base_of(thr)
            if base is None or not cx.row_input(base):
                raise NotImplementedError(f"{fn} ({key}): a threshold list computed per event inside the recipe is not supported: the thresholds "
                                          "are a constant array, a two-dimensional input column or a stage's waveform")
        args[2] = _operand_in_memory(cx, args[2], fn, key, written_first=True)
        args[3] = float(polarity)
        step = cx.replace(st, (fn, args, key))
        cx.stage([step], [], f"{fn} {key} on rows", wfs=[t_out], rows_first=True)
    for st in cx.steps_of(_TIME_OVER, only):
        fn, args, key = st[0], list(st[1]), st[2]
        if not isinstance(args[2], Var):
            raise ProcessingChainError(f"{fn} ({key}): name the output")
        _rows_in_memory(cx, args[0], fn, key)
        args[1] = _operand_in_memory(cx, args[1], fn, key, written_first=True)
        step = cx.replace(st, (fn, args, key))
        cx.stage([step], [args[2]], f"{fn} {key} on rows")


def _stage_spectrum(cx: _Stager, only=None):
    """``psd`` runs on dsp_spectrum.hip and nowhere else, on rows in HBM: a mandatory stage, like the peak finder's.  The source is a chain
    input, a stage's waveform, a slice of either, or a waveform the program computes, written to HBM first; the spectrum is an ordinary
    waveform variable of the program."""
    from .processors import check_spectrum_length

    fn = _PSD
    for st in cx.steps_of(fn, only):
        args, key = list(st[1]), st[2]
        src, out = args
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        m = src.length // 2 + 1
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): declare the output as name(len(w_in)//2+1): {m} bins")
        if out.length != m:
            raise DSPFatal(f"Size of psd must be len(w_in)//2+1 = {m}")
        check_spectrum_length(f"{fn} ({key})", src.length, np.float32)
        _rows_in_memory(cx, src, fn, key)
        cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)


def _stage_sort(cx: _Stager, only=None):
    """``sort`` runs on dsp_sort.hip and nowhere else, on rows in HBM: a mandatory stage, like the spectrum's.  The source is a chain input,
    a stage's waveform, a slice of either, or a waveform the program computes, written to HBM first; the sorted row is an ordinary waveform
    variable of the program, with the source's length and grid."""
    from .processors import check_sort_length

    fn = _SORT
    for st in cx.steps_of(fn, only):
        args, key = list(st[1]), st[2]
        src, out = args
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): the output is a waveform variable")
        if out.length != src.length:
            raise ProcessingChainError(f"{fn} ({key}): '{out.name}' holds {out.length} samples, the source {src.length}")
        check_sort_length(f"{fn} ({key})", src.length, np.float32)
        _rows_in_memory(cx, src, fn, key)
        cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)


def _stage_interp_upsampler(cx: _Stager, only=None):
    """``interpolating_upsampler`` runs on dsp_interp.hip and nowhere else, on rows in HBM: a mandatory stage, like sort's.  The source is
    a chain input, a stage's waveform, a slice of either, or a waveform the program computes, written to HBM first; the resampled row is an
    ordinary waveform variable of the program, declared with its length (and ``period=``: the finer grid).  The mode is a constant of the
    kernel, checked here for every row."""
    from .processors import check_interp

    fn = _INTERP
    for st in cx.steps_of(fn, only):
        args, key = list(st[1]), st[2]
        src, mode, out = args
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not isinstance(mode, (Char, int, np.integer)):
            raise NotImplementedError(f"{fn} ({key}): the interpolation mode is a constant of the kernel, not a per-event value")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): declare the output with its length, as in wf_up(len(wf)*10, period=wf.period/10)")
        check_interp(f"{fn} ({key})", _Emitter.char_of(mode), src.length, out.length, np.float32)
        _rows_in_memory(cx, src, fn, key)
        cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)


def _stage_reflected_convolve(cx: _Stager, only=None):
    """``reflected_convolve_wf`` runs on dsp_reflect.hip and nowhere else, on rows in HBM: a mandatory stage, like sort's, made ahead of the
    others (the histogram and the peak finder of the SiPM recipes read what it feeds).  The source is a chain input, a stage's waveform, a
    slice of either, or a waveform the program computes, written to HBM first; the kernel is constant taps in any form convolve_wf's takes;
    the filtered row is an ordinary waveform variable of the program, with the source's length and grid.  An ``avg_current`` that reads
    exactly the filtered waveform, with a constant length, joins the launch; the filtered waveform is then written only if something else
    reads it or the recipe asks for it (``_stage_histogram``'s rule for weights and borders)."""
    from .processors import check_reflect

    fn = _REFLECT
    for st in cx.steps_of(fn, only):
        args, key = list(st[1]), st[2]
        src, taps, out = args
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not (isinstance(taps, Var) and taps.kind == "taps"):
            raise NotImplementedError(f"{fn} ({key}): the kernel is one constant array for every row (a database array, a list, loadlh5 or a kernel "
                                      "generator's output), not a per-event value")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): the output is a waveform variable")
        if out.length != src.length:
            raise ValueError(f"{fn} ({key}): the output has the length of the input (len(w_in) = {src.length}, len(w_out) = {out.length})")
        check_reflect(f"{fn} ({key})", src.length, taps.length, np.float32)
        _rows_in_memory(cx, src, fn, key)
        def joins(x):  # an avg_current of exactly the filtered row, with a constant length DSP_OP_AVG_CURRENT accepts
            length = x[1][1].const if isinstance(x[1][1], Var) and x[1][1].kind == "const" else x[1][1]
            return (x[0] == "avg_current" and x[1][0] is out and _is_number(length) and isinstance(x[1][2], Var) and bool(x[1][2].length)
                    and 0 < int(length) < out.length and x[1][2].length == out.length - int(length))

        cur = next((x for x in cx.users_of(out) if joins(x)), None)
        if cur is None:
            cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)
            continue
        row_wanted = out.name in cx.out_names or any(u is not cur for u in cx.users_of(out))
        cx.stage([st, cur], [], f"{fn} {key} + avg_current {cur[2]} in one launch on rows", wfs=([out] if row_wanted else []) + [cur[1][2]], rows_first=True)


def _pileup_rows(cx: _Stager, src, fn, key, reader):
    """The rows the pile-up kernel reads: a chain input or a stage's waveform as it is (behind the stages of what it comes from).  A
    ``bl_subtract`` of a chain input by a per-event value in memory, whose result only ``reader`` (a step, or a list of them: the steps of one
    launch) reads and the recipe does not ask for, joins
    the launch -- one float subtraction as the rows are read, as ``_fir_input_as_rows`` has it for the long filters: returned, for the
    stage's group.  Anything else is written to memory first."""
    base = _base_of(src)
    if base is None:
        raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
    _stage_producers(cx, base)
    pst = cx.producer_of(base) if not cx.row_input(base) else None
    if (pst is not None and src is base and pst[0] == "bl_subtract" and isinstance(pst[1][0], Var) and cx.row_input(pst[1][0])
            and base.name not in cx.out_names and all(any(u is r for r in (reader if isinstance(reader, list) else [reader])) for u in cx.users_of(base))
            and (_is_number(pst[1][1]) or all(cx.plain_scalar(leaf) for leaf in _leaves(pst[1][1], [])))):
        bargs = list(pst[1])
        bargs[1] = _operand_in_memory(cx, bargs[1], "bl_subtract", pst[2])
        return [cx.replace(pst, ("bl_subtract", bargs, pst[2]))]
    _rows_in_memory(cx, src, fn, key)
    return []


def _stage_pileup(cx: _Stager, only=None):
    """``rc_cr2`` and ``bi_level_zero_crossing_time_points`` run on dsp_pileup.hip and nowhere else, on rows in HBM: mandatory stages, like
    the threshold kernel's.  A walk that reads exactly an ``rc_cr2``'s output takes the filter into its launch; the filtered waveform is then
    written only if something else reads it or the recipe asks for it (``_stage_histogram``'s rule for weights and borders).  t_tau is a
    constant -- the filter's coefficients are formed on the host --; thresholds, gate and start are per-event operands
    (``_operand_in_memory``); the lists are declared with their length, ``name(20, vector_len=n_crossings)``."""
    from .processors import check_bi_level_lists, check_rc_cr2

    def filter_checked(st):
        fn, (src, tau, out), key = st
        if isinstance(tau, Var) and tau.kind == "const":
            tau = tau.const
        if not (_is_number(tau) or isinstance(tau, Quantity)):
            raise NotImplementedError(f"{fn} ({key}): t_tau is a constant of the kernel, not a per-event value: its coefficients are formed on the host")
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): the output is a waveform variable")
        check_rc_cr2(f"{fn} ({key})", src.length, out.length)
        return src, out

    def filter_of(walk):
        """the ``rc_cr2`` a walk takes into its launch: it reads exactly the filtered row, and none of its operands is computed from that row
        (a threshold at 3*fwhm of the filtered row's histogram: the filter runs first, on its own)"""
        src = walk[1][0]
        flt = cx.producer_of(src) if isinstance(src, Var) else None
        if flt is None or flt[0] != _RC_CR2 or not cx.has(flt):
            return None
        operands = [leaf for a in walk[1][1:5] for leaf in _leaves(a, [])]
        return None if any(flt is x for leaf in operands for x in cx.ancestors(leaf)) else flt

    if only is not None and only[0] == _RC_CR2:  # (asked for a filter: the launch it would have joined when the family's turn came)
        only = next((w for w in cx.steps_of(_BI_LEVEL) if filter_of(w) is only), only)
    for st in cx.steps_of(_BI_LEVEL, only):
        fn, args, key = st[0], list(st[1]), st[2]
        src, gate, count, polarity, times = args[0], args[3], args[5], args[6], args[7]
        if not all(isinstance(v, Var) and v.kind == "wf" and v.length for v in (polarity, times)) or not isinstance(count, Var):
            raise ProcessingChainError(f"{fn} ({key}): declare the lists as name(length, vector_len=<the count>) and name the count")
        check_bi_level_lists(f"{fn} ({key})", polarity.length, times.length)
        if isinstance(gate, Var) and gate.kind == "const":
            gate = gate.const
        if _is_number(gate) and not np.isfinite(float(gate)):
            raise ValueError(f"{fn} ({key}): gate_time_in is a finite number of samples")
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        flt = filter_of(st)
        rows, out = filter_checked(flt) if flt is not None else (src, None)
        pre = _pileup_rows(cx, rows, fn if flt is None else _RC_CR2, key if flt is None else flt[2], st if flt is None else flt)
        for k in (1, 2, 3, 4):
            args[k] = _operand_in_memory(cx, args[k], fn, key, written_first=True)
        step = cx.replace(st, (fn, args, key))
        if flt is None:
            cx.stage(pre + [step], [count], f"{fn} {key} on rows", wfs=[polarity, times], rows_first=True)
            continue
        row_wanted = out.name in cx.out_names or any(u is not step for u in cx.users_of(out))
        cx.stage(pre + [flt, step], [count], f"{_RC_CR2} {flt[2]} + {fn} {key} in one launch on rows", wfs=([out] if row_wanted else []) + [polarity, times],
                 rows_first=True)
    for st in cx.steps_of(_RC_CR2, only):
        src, out = filter_checked(st)
        pre = _pileup_rows(cx, src, st[0], st[2], st)
        cx.stage(pre + [st], [], f"{st[0]} {st[2]} on rows", wfs=[out], rows_first=True)


def _stage_pulses(cx: _Stager, only=None):
    """``peak_snr_threshold`` and ``multi_a_filter`` run on dsp_pulses.hip and nowhere else, on rows in HBM: mandatory stages, like the
    threshold kernel's.  The list is a stage's list in memory (the peak finder's, a picker's) or a two-dimensional input column; the ratio is
    a per-event operand (``_operand_in_memory``), the width a constant.  A ``multi_a_filter`` that reads exactly a picker's ``idx_out``, on
    the same waveform, joins its launch; the list is then written only if something else reads it or the recipe asks for it
    (``_stage_histogram``'s rule for weights and borders).  The outputs' length is that of the list read."""
    from .processors import check_pulse_list, check_pulse_width

    def list_in_memory(fn, key, lst, out, pickoff, n):
        if not _is_wf(lst) or not lst.length:
            raise ProcessingChainError(f"{fn} ({key}): the list is an array per event: a stage's list or a two-dimensional input column, not {lst!r}")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{fn} ({key}): the output is an array variable (its length is that of the list read)")
        check_pulse_list(f"{fn} ({key})", n, lst.length, out.length, pickoff=pickoff)

    for st in cx.steps_of(_PEAK_SNR, only):
        fn, args, key = st[0], list(st[1]), st[2]
        src, lst, _ratio, width, out, count = args
        if isinstance(width, Var) and width.kind == "const":
            width = width.const
        if not (_is_number(width) or isinstance(width, Quantity)):
            raise NotImplementedError(f"{fn} ({key}): per-waveform integer parameters are not supported on the device")
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not isinstance(count, Var):
            raise ProcessingChainError(f"{fn} ({key}): name the count")
        if not isinstance(width, Quantity):
            args[3] = check_pulse_width(f"{fn} ({key})", width)
        list_in_memory(fn, key, lst, out, False, src.length)
        _rows_in_memory(cx, src, fn, key)
        _rows_in_memory(cx, lst, fn, key)
        args[2] = _operand_in_memory(cx, args[2], fn, key, written_first=True)
        step = cx.replace(st, (fn, args, key))
        amp = next((x for x in cx.steps if x[0] == _MULTI_A and x[1][1] is out and x[1][0] is src), None)
        if amp is None:
            cx.stage([step], [count], f"{fn} {key} on rows", wfs=[out], rows_first=True)
            continue
        list_in_memory(_MULTI_A, amp[2], out, amp[1][2], True, src.length)
        list_wanted = out.name in cx.out_names or any(u is not amp for u in cx.users_of(out))
        cx.stage([step, amp], [count], f"{fn} {key} + {_MULTI_A} {amp[2]} in one launch on rows", wfs=([out] if list_wanted else []) + [amp[1][2]],
                 rows_first=True)
    for st in cx.steps_of(_MULTI_A, only):
        fn, (src, lst, out), key = st
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        list_in_memory(fn, key, lst, out, True, src.length)
        _rows_in_memory(cx, lst, fn, key)  # (a picker's list: its stage first, and with it this step, if it reads the same waveform)
        if not cx.has(st):
            continue
        _rows_in_memory(cx, src, fn, key)
        cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)


def _same_rows(a, b) -> bool:
    """the same variable, or the same slice of the same variable"""
    return a is b or (isinstance(a, View) and a == b)


def _stage_tailfit(cx: _Stager, only=None):
    """``log_check``, ``poly_fit``, ``poly_diff`` and ``poly_exp_rms`` run on dsp_tailfit.hip and nowhere else, on rows in HBM: mandatory stages,
    like the pile-up kernel's.  Each owns one launch: a ``poly_diff`` / ``poly_exp_rms`` that reads exactly a ``poly_fit``'s coefficients, and
    the rows that fit was made of (or their logarithm), takes the fit into its launch, and the fit a ``log_check`` whose result it reads; the
    logged row and the coefficients are then written only if something else reads them or the recipe asks for them (``_stage_histogram``'s
    rule for weights and borders).  A ``bl_subtract`` nothing else reads joins as in ``_pileup_rows``.  ``mean`` and ``rms`` are per-event
    values, the coefficients a row of m."""
    from .processors import check_poly

    def producer(v, fn):
        st = cx.producer_of(v) if isinstance(v, Var) else None
        return st if st is not None and st[0] == fn and cx.has(st) else None

    def fit_checked(st):
        fn, (src, out, _inv), key = st
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        check_poly(f"{fn} ({key})", src.length, out.length)
        return src, out

    def log_checked(st):
        fn, (src, out), key = st
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length == src.length):
            raise ProcessingChainError(f"{fn} ({key}): the output is a waveform variable of the source's {src.length} samples")
        return src, out

    def wanted(v, group):
        return v.name in cx.out_names or any(not any(u is g for g in group) for u in cx.users_of(v))

    def fit_group(ft, checked=True):
        """the fit with the log_check it reads, if there is one: (steps, rows, the logged row or None, the coefficients); ``checked``
        false: only looked at, the shapes' errors are left to the step's own turn"""
        src, pars = fit_checked(ft) if checked else ft[1][:2]
        lg = producer(src, _LOG_CHECK)
        if lg is None:
            return [ft], src, None, pars
        rows, logged = log_checked(lg) if checked else lg[1]
        return [lg, ft], rows, logged, pars

    def fuses(st):
        """the steps a ``poly_diff`` / ``poly_exp_rms`` would take into its launch, or None: it runs on coefficients in memory"""
        ft = producer(st[1][1], _POLY_FIT)
        if ft is None:
            return None
        group, rows, logged, _ = fit_group(ft, checked=False)
        return group if _same_rows(st[1][0], rows) or (logged is not None and st[1][0] is logged) else None

    if only is not None and only[0] in (_LOG_CHECK, _POLY_FIT):  # (asked for a group's head: the launch it would have joined in the family's turn)
        joined = [st for fn in (_POLY_DIFF, _POLY_EXP_RMS) for st in cx.steps_of(fn) if any(g is only for g in fuses(st) or [])]
        joined += [ft for ft in cx.steps_of(_POLY_FIT) if producer(ft[1][0], _LOG_CHECK) is only]
        only = joined[0] if joined else only
    for fn in (_POLY_DIFF, _POLY_EXP_RMS):
        for st in cx.steps_of(fn, only):
            (src, pars, mean, rms), key = st[1], st[2]
            if _base_of(src) is None:
                raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
            if not _is_wf(pars) or not pars.length:
                raise ProcessingChainError(f"{fn} ({key}): the coefficients are an array per event: a poly_fit's or a two-dimensional input column, not {pars!r}")
            if not (isinstance(mean, Var) and isinstance(rms, Var)):
                raise ProcessingChainError(f"{fn} ({key}): name the two outputs")
            check_poly(f"{fn} ({key})", src.length, pars.length)
            ft = producer(pars, _POLY_FIT)
            if ft is not None:
                group, rows, logged, _ = fit_group(ft)
                if _same_rows(src, rows) or (logged is not None and src is logged):
                    group = group + [st]
                    pre = _pileup_rows(cx, rows, group[0][0], group[0][2], group)
                    wfs = ([logged] if logged is not None and wanted(logged, group) else []) + ([pars] if wanted(pars, group) else [])
                    cx.stage(pre + group, [mean, rms], " + ".join(f"{g[0]} {g[2]}" for g in group) + " in one launch on rows", wfs=wfs, rows_first=True)
                    continue
            _rows_in_memory(cx, pars, fn, key)  # (a fit's coefficients: its stage first)
            pre = _pileup_rows(cx, src, fn, key, st)
            cx.stage(pre + [st], [mean, rms], f"{fn} {key} on rows", rows_first=True)
    for st in cx.steps_of(_POLY_FIT, only):
        group, rows, logged, pars = fit_group(st)
        pre = _pileup_rows(cx, rows, group[0][0], group[0][2], group)
        wfs = ([logged] if logged is not None and wanted(logged, group) else []) + [pars]
        cx.stage(pre + group, [], " + ".join(f"{g[0]} {g[2]}" for g in group) + (" in one launch" if len(group) > 1 else "") + " on rows", wfs=wfs, rows_first=True)
    for st in cx.steps_of(_LOG_CHECK, only):
        src, out = log_checked(st)
        pre = _pileup_rows(cx, src, st[0], st[2], st)
        cx.stage(pre + [st], [], f"{st[0]} {st[2]} on rows", wfs=[out], rows_first=True)


def _stage_align(cx: _Stager, only=None):
    """``inl_correction``, ``get_wf_centroid``, ``wf_alignment`` and ``wf_correction`` run on dsp_align.hip and nowhere else, on rows in HBM:
    mandatory stages, like the decay-tail fitter's.  Each owns one launch; a ``wf_correction`` that reads exactly a ``wf_alignment``'s output
    takes it into its launch, and the aligned row is then written only if something else reads it or the recipe asks for it
    (``_stage_histogram``'s rule for weights and borders).  ``shift``, ``size`` and the indices are constants, checked here for every row in
    the reference's order and words; the centroid is a constant, an input column or a stage's result (``_operand_in_memory``); ``inl`` and
    ``w_corr`` are constant arrays; ``inl_correction`` reads an integer input column."""
    from .processors import check_alignment, check_centroid_shift, check_correction

    def constant(what, name, v):
        if isinstance(v, Var) and v.kind == "const":
            v = v.const
        if not _is_number(v):
            raise NotImplementedError(f"{what}: {name} is a constant of the call on the device, not a per-event value")
        return float(v)

    def rows_out(what, src, out, length):
        if _base_of(src) is None:
            raise ProcessingChainError(f"{what}: '{src}' is not a waveform")
        if not (isinstance(out, Var) and out.kind == "wf" and out.length):
            raise ProcessingChainError(f"{what}: the output is a waveform variable" + ("" if length else ", declared with its length: name(size)"))
        if length and out.length != length:
            raise ProcessingChainError(f"{what}: '{out.name}' holds {out.length} samples, the source {length}")

    def corr_checked(st):
        fn, args, key = st[0], list(st[1]), st[2]
        what = f"{fn} ({key})"
        src, tpl, start, stop, out = args
        rows_out(what, src, out, src.length if _base_of(src) is not None else None)
        try:
            args[2], args[3] = check_correction(what, src.length, tpl.length, constant(what, "start_idx", start), constant(what, "stop_idx", stop))
        except ValueError as e:
            raise ProcessingChainError(str(e)) from None
        return cx.replace(st, (fn, args, key))

    for st in cx.steps_of(_WF_ALIGN, only):
        fn, args, key = st[0], list(st[1]), st[2]
        what = f"{fn} ({key})"
        src, centroid, shift, size, out = args
        rows_out(what, src, out, None)
        try:
            args[2], args[3] = check_alignment(what, src.length, constant(what, "shift", shift), constant(what, "size", size), out.length)
        except ValueError as e:
            raise ProcessingChainError(str(e)) from None
        if isinstance(centroid, Var) and centroid.kind == "const":
            centroid = args[1] = centroid.const
        if _is_number(centroid) and np.isnan(centroid):
            raise DSPFatal("centroid is nan")
        _rows_in_memory(cx, src, fn, key)
        args[1] = _operand_in_memory(cx, args[1], fn, key, written_first=True)
        step = cx.replace(st, (fn, args, key))
        corr = next((x for x in cx.steps if x[0] == _WF_CORR and x[1][0] is out), None)
        if corr is None:
            cx.stage([step], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)
            continue
        corr = corr_checked(corr)
        wanted = out.name in cx.out_names or any(u is not corr for u in cx.users_of(out))
        cx.stage([step, corr], [], f"{fn} {key} + {_WF_CORR} {corr[2]} in one launch on rows", wfs=([out] if wanted else []) + [corr[1][4]], rows_first=True)
    for st in cx.steps_of(_WF_CORR, only):
        src = st[1][0]
        if _base_of(src) is not None:
            _rows_in_memory(cx, src, st[0], st[2])  # (an alignment's window: its stage first, and with it this step)
        if not cx.has(st):
            continue
        st = corr_checked(st)
        cx.stage([st], [], f"{st[0]} {st[2]} on rows", wfs=[st[1][4]], rows_first=True)
    for st in cx.steps_of(_WF_CENTROID, only):
        fn, args, key = st[0], list(st[1]), st[2]
        what = f"{fn} ({key})"
        src, shift, out = args
        if _base_of(src) is None:
            raise ProcessingChainError(f"{what}: '{src}' is not a waveform")
        if not isinstance(out, Var):
            raise ProcessingChainError(f"{what}: name the centroid")
        args[1] = check_centroid_shift(what, src.length, constant(what, "shift", shift))
        _rows_in_memory(cx, src, fn, key)
        cx.stage([cx.replace(st, (fn, args, key))], [out], f"{fn} {key} on rows")
    for st in cx.steps_of(_INL, only):
        fn, (src, _table, out), key = st
        what = f"{fn} ({key})"
        rows_out(what, src, out, src.length if _base_of(src) is not None else None)
        base = _base_of(src)
        if not (base.is_input and base.source is not None and base.ext_key is None and _is_int_dtype(base)):
            raise NotImplementedError(f"{what}: '{base.name}' is not an integer input column: inl_correction reads ADC codes, int16 or uint16 rows of the input table")
        cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)


def _stage_ml_layers(cx: _Stager, only=None):
    """The neural-network layers (ml.py) run on dsp_dense.hip and nowhere else, on rows in HBM: mandatory stages, like sort's.  Each dense or
    classification layer is a launch on rows in memory -- a chain input, a stage's waveform (the layer before it), or a waveform the program
    computes, written to HBM first.  A ``normalisation_layer`` whose result only dense or classification layers read, and which is not an
    output of the recipe, is folded into their loads (the kernel normalises while it stages a row); otherwise it is a launch of its own.
    The activation is a constant of the kernel."""
    from .processors import check_dense

    def folded(st):  # (a normalisation whose layers are all staged already has no reader left: it ran with them)
        return _folded_normalisation(cx, st)

    for st in [x for x in cx.steps if x[0] in _ML and (only is None or x is only)]:
        if not cx.has(st):
            continue
        fn, args, key = st[0], list(st[1]), st[2]
        src, out = args[0], args[-1]
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        if fn == _NORMALISE:
            if not (isinstance(out, Var) and out.kind == "wf" and out.length == src.length):
                raise ProcessingChainError(f"{fn} ({key}): the output is a waveform variable of the source's {src.length} samples")
            check_dense(f"{fn} ({key})", src.length, 1)
            if not folded(st):
                _rows_in_memory(cx, src, fn, key)
                cx.stage([st], [], f"{fn} {key} on rows", wfs=[out], rows_first=True)
            continue
        if not isinstance(args[-2], (Char, int, np.integer)):
            raise NotImplementedError(f"{fn} ({key}): the activation function is a constant of the kernel, not a per-event value")
        classify = fn.startswith("classification")
        check_dense(f"{fn} ({key})", src.length, 1 if classify else int(args[1].const.shape[1]))
        if not isinstance(out, Var) or (not classify and not (out.kind == "wf" and out.length)):
            raise ProcessingChainError(f"{fn} ({key}): name the output")
        norm = cx.producer_of(src) if isinstance(src, Var) else None
        if norm is not None and norm[0] == _NORMALISE and cx.has(norm) and folded(norm):
            _rows_in_memory(cx, norm[1][0], _NORMALISE, norm[2])
            group, what = [norm, st], f"{_NORMALISE} {norm[2]} + {fn} {key} in one launch on rows"
        else:
            _rows_in_memory(cx, src, fn, key)
            group, what = [st], f"{fn} {key} on rows"
        if classify:
            cx.stage(group, [out], what, drop=[st])
        else:
            cx.stage(group, [], what, wfs=[out], rows_first=True, drop=[st])


def _stage_svm(cx: _Stager, only=None):
    """``svm_predict`` runs on dsp_svm.hip and nowhere else, on rows in HBM: a mandatory stage, like a classification layer's.  Its rows are a
    chain input, a stage's waveform (the normalisation before it), or a waveform the program computes, written to HBM first; its label is a
    per-event value of the later entries."""
    for st in cx.steps_of(_SVM, only):
        fn, args, key = st
        src, out = args[0], args[1]
        if _base_of(src) is None:
            raise ProcessingChainError(f"{fn} ({key}): '{src}' is not a waveform")
        _rows_in_memory(cx, src, fn, key)
        cx.stage([st], [out], f"{fn} {key} on rows")


#: the family that stages each processor with a kernel of its own (``_stage_producers`` asks it for one step)
_FAMILY_OF = {_REFLECT: _stage_reflected_convolve, _RC_CR2: _stage_pileup, _BI_LEVEL: _stage_pileup, _PEAK_SNR: _stage_pulses, _MULTI_A: _stage_pulses, **dict.fromkeys(_TAILFIT, _stage_tailfit), **dict.fromkeys(_ALIGN, _stage_align), _HISTOGRAM: _stage_histogram, _HISTOGRAM_STATS: _stage_histogram,
              _MULTI_EXTREMA: _stage_multi_extrema, _MULTI_TPT: _stage_thresholds, _TIME_OVER: _stage_thresholds, _PSD: _stage_spectrum,
              _SORT: _stage_sort, _INTERP: _stage_interp_upsampler, **dict.fromkeys(_ML, _stage_ml_layers), _SVM: _stage_svm}


def _extract_stages(b: _Builder, steps, out_pars, n_rows, ft):
    """Long FIRs leave the program: each ``convolve_wf`` with a constant kernel of STAGE_MIN_TAPS or more taps becomes a launch of the
    matrix-core FIR kernels ahead of the program (one waveform per wavefront is the wrong shape for 133 x 8192 or 5792 x 301
    multiply-adds per waveform; 64 waveforms x 320 outputs per workgroup on the MFMA units is 4 - 40 times faster, and the filter's
    input and output slots leave the program's LDS).  The FIR kernels read rows from HBM, so a filter's input is a chain input, the
    input minus a per-event value (bl_subtract: done while staging), or -- anything else, the pole-zero corrected waveform of the Ge
    recipes -- a waveform that a small program of its own writes to HBM first (32 kB per waveform: noise at a recipe's rate).  What a
    stage wrote is an input of the later stages and of the program; processors that only fed a stage drop out of the program.  With rows
    in HBM, the other stage families follow: short trapezoids, the current branch, reductions read off rows.
    Returns (steps left to the program, stages in launch order)."""
    if all(st[0] in ("convolve_wf", "fft_convolve_wf", "amax", "bl_subtract", "alias") for st in steps):
        return steps, []  # the program is nothing but filters (BASELINE configs[2]): dsp_chain_create gives it the FIR kernel as a whole
    cx = _Stager(b, steps, out_pars, n_rows, ft)
    _stage_long_firs(cx)
    fir_staged = bool(cx.stages)
    has_peaks = any(st[0] in _OWN_KERNEL for st in cx.steps)
    if not cx.stages and not has_peaks:
        return cx.steps, cx.stages
    if fir_staged:  # (the optional families follow the long filters, as before; the peak finder's stage is made with or without them)
        _stage_short_traps(cx)
        _stage_current_branch(cx)
    _stage_reflected_convolve(cx)  # (ahead of everything that may read the smoothed rows or their current)
    _stage_histogram(cx)  # (ahead of the peak finder: its thresholds may be arithmetic of these results, "3*fwhm")
    _stage_multi_extrema(cx)
    _stage_thresholds(cx)
    _stage_pileup(cx)
    _stage_pulses(cx)
    _stage_tailfit(cx)
    _stage_align(cx)
    _stage_spectrum(cx)
    _stage_sort(cx)
    _stage_interp_upsampler(cx)
    _stage_ml_layers(cx)
    _stage_svm(cx)
    # what the stages' results replaced is not computed any more: producers of staged variables, and whatever only fed them
    staged = {id(v) for v in b.vars.values() if isinstance(v, Var) and v.ext_key is not None and v.aux_io is None}
    cx.steps = _live_steps(b, [x for x in cx.steps if not any(id(a) in staged for a in _outputs_of(x))], out_pars)
    if ft == np.dtype(np.float32) and os.environ.get("DSPEED_HIP_NO_ROW_REDUCTIONS") != "1" and fir_staged:
        _stage_row_reductions(cx)
    return cx.steps, cx.stages


def _column_dtype(dt):
    """type of the column an integer value travels in (the 8-bit integer types have no column type of their own: 16 bits hold them)"""
    dt = np.dtype(dt)
    return {np.dtype(np.int8): np.dtype(np.int16), np.dtype(np.uint8): np.dtype(np.uint16)}.get(dt, dt)


def _int_dtype_of(x):
    """the integer (or bool) type of a per-event column or of an expression between such values; None: not one"""
    dt = getattr(x, "dtype", None)
    if (isinstance(x, SExpr) and x.op == "func") or (isinstance(x, Var) and x.kind == "scalar"):
        return np.dtype(dt) if dt is not None and np.dtype(dt).kind in "iub" else None
    return None


def _is_table_column(x) -> bool:  # a column of the input table: in HBM before any program runs
    return isinstance(x, Var) and x.kind == "scalar" and x.is_input and x.source is not None and x.sreg is None and x.ext_key is None


def _expressions(b: _Builder, steps, out_pars):
    """every expression between per-event values that the steps or the outputs read, operands first"""
    nodes, seen = [], set()

    def visit(x):
        if isinstance(x, SExpr) and id(x) not in seen:
            seen.add(id(x))
            for y in x.args:
                visit(y)
            nodes.append(x)

    for _fn, args, _key in steps:
        for a in args:
            visit(a)
    for o in out_pars:
        visit(b.vars.get(o))
    return nodes


def _int_island(b: _Builder, steps, out_pars, ft):
    """Per-event INTEGER arithmetic that no float register holds -- NumPy's 64-bit loops ('ll->l', 'QQ->Q': int64 / uint64 columns, int32
    beside uint32; reference :1565-1572), comparisons, ``where`` and casts of their results, and in a float32 chain the 32-bit loops too -- leaves
    the programs: it becomes an *integer program* (``dsp_chain_create(..., DSP_I64)``: 64-bit integer registers, NumPy's wrap-around bit
    for bit, dsp_scalar.hip) that runs ahead of everything else on the input table's integer columns.  What the recipe's outputs or the
    other programs read of it arrives as a column of the value's own type (``SExpr.op == 'ext'``).  Operands must be columns of the input
    table, constants or such arithmetic itself: a 64-bit loop on a value a processor computes is refused by name (a 32-bit one then stays
    where it was: the float operation, exact below 2^24).  Returns the stage's description (None: nothing to do) and {output: dtype} of the
    recipe outputs it writes itself."""
    nodes = _expressions(b, steps, out_pars)
    wide = lambda dt: dt is not None and dt.itemsize == 8 and dt.kind in "iu"  # noqa: E731
    eligible = {}

    def ok(x):  # computable ahead of the programs, in integers
        if _is_number(x) or isinstance(x, bool):
            return True
        if _is_table_column(x):
            return _int_dtype_of(x) is not None
        if isinstance(x, SExpr):
            if id(x) not in eligible:
                eligible[id(x)] = x.op == "func" and _int_dtype_of(x) is not None and all(ok(y) for y in x.args[1:])
            return eligible[id(x)]
        return False

    need = []
    for n in nodes:
        if n.op != "func":
            continue
        opn = [x for x in n.args[1:] if isinstance(x, (Var, SExpr))]
        is_wide = wide(_int_dtype_of(n)) or any(wide(_int_dtype_of(x)) for x in opn)
        narrow32 = ((int(n.args[0]) >> 8) & 0xff) == 32 and ft != np.dtype(np.float64) and _int_dtype_of(n) is not None
        if is_wide:
            if _int_dtype_of(n) is None or not ok(n):
                raise NotImplementedError(f"'{n.name}': 64-bit integers reach the device as columns of the input table and arithmetic between them; "
                                          "here they meet a value a processor computes, or leave as a float (astype of a 64-bit integer)")
            need.append(n)
        elif narrow32 and ok(n):
            need.append(n)
    if not need:
        return None, {}
    island = {}

    def take(x):
        if isinstance(x, SExpr) and id(x) not in island:
            for y in x.args[1:]:
                take(y)
            island[id(x)] = x

    for n in need:
        take(n)
    members = [n for n in nodes if id(n) in island]  # (operands first)

    # who reads a member from outside: a processor, an expression that stays behind, an output of the recipe
    outside = set()
    for _fn, args, _key in steps:
        outside.update(id(a) for a in args if isinstance(a, SExpr) and id(a) in island)
    for n in nodes:
        if id(n) not in island:
            outside.update(id(y) for y in n.args if isinstance(y, SExpr) and id(y) in island)
    direct = {}
    for o in out_pars:
        v = b.vars.get(o)
        if isinstance(v, SExpr) and id(v) in island and not (v.is_coord is True and _time_unit_ns(v.unit) is not None):
            direct.setdefault(id(v), []).append(o)
        elif isinstance(v, SExpr) and id(v) in island:
            outside.add(id(v))

    t = Program()
    in_vars, leaf_io = {}, {}

    def opnd(x):
        if isinstance(x, SExpr):
            return Scalar.reg(x.sreg)
        if isinstance(x, Var):
            if id(x) not in leaf_io:
                name = f"in:{x.name}"
                leaf_io[id(x)] = t.add_io(name, _lib.IO_SCALAR_IN, np.dtype(x.dtype))
                in_vars[name] = x
            return Scalar.input(leaf_io[id(x)])
        return Scalar.const(float(x))

    outs, out_dtypes, direct_out = [], {}, {}
    for k, n in enumerate(members):
        n.sreg = t.add_sregs(1)
        sp = [opnd(x) for x in n.args[1:]]
        t.add_op(_lib.OP_SCALAR_FUNC, dst=n.sreg, ip=(int(n.args[0]),), sp=tuple(sp + [Scalar.const(0.0)] * (3 - len(sp))))
    for k, n in enumerate(members):
        nat = _int_dtype_of(n)
        is_u64 = int(nat == np.dtype(np.uint64))
        for o in direct.get(id(n), ()):
            t.add_op(_lib.OP_STORE_SCALAR, io=t.add_io(f"out:{o}", _lib.IO_SCALAR_OUT, _column_dtype(nat)), ip=(n.sreg, is_u64))
            direct_out[o] = (nat, _column_dtype(nat))
        if id(n) in outside:
            key = f"in:isl{k}"
            t.add_op(_lib.OP_STORE_SCALAR, io=t.add_io(f"out:isl{k}", _lib.IO_SCALAR_OUT, _column_dtype(nat)), ip=(n.sreg, is_u64))
            outs.append((f"out:isl{k}", key, None))
            out_dtypes[key] = _column_dtype(nat)
            n.ext_key = key
    for n in members:  # from here on a member is a column in HBM to everybody else
        n.ext_dtype = _column_dtype(_int_dtype_of(n))
        n.op, n.args, n.sreg = "ext", (), None
    if len(t.ops) > _lib.MAX_OPS or len(t.io) > _lib.MAX_IO or t.n_sregs > _lib.MAX_SREGS:
        raise NotImplementedError("the recipe's integer arithmetic is too large for one device program (ops/bindings/registers limit)")
    stage = _stage_record("integer arithmetic between per-event columns (64-bit registers)", t, {}, in_vars, {}, outs,
                          out_dtypes=out_dtypes, compute=np.dtype(np.int64))
    return stage, direct_out


def _extract_fits(b: _Builder, steps, out_pars, p: Program, ft):
    """linear_slope_fit on the rows of the batch (dsp_linear_slope_fit_rows: one waveform per lane) instead of inside the program,
    where its sequential float32 recurrences cost a third of a LEGEND recipe: a fit whose waveform is an input, the input minus a
    per-event input / constant (bl_subtract or numpy.subtract), or the pole_zero of that (constant tau), read whole or through a
    constant slice.  The kernel runs ahead of the chain on the same stream; the chain reads its results as per-event inputs.
    Returns (one group per (input waveform, subtraction, pole-zero) pipeline = launch, the steps that remain)."""
    producer = {}
    for fn, args, _k in steps:
        for a, r in zip(args, _roles(fn)):
            if r == "W" and isinstance(a, Var):
                producer[a.name] = (fn, args)

    def plain_scalar(x):  # a constant or a per-event input column (known before the chain runs)
        if isinstance(x, Var):
            return x.kind == "scalar" and x.is_input and x.sreg is None
        return _is_number(x)

    def pipeline_of(v):
        """(input wf Var, first sample, length, sub operand, sub mode, tau) of waveform v, or None"""
        tau = None
        if not v.is_input and v.name in producer and producer[v.name][0] == "pole_zero":
            _fn, a = producer[v.name]
            if not isinstance(a[0], Var) or isinstance(a[1], (Var, SExpr, Quantity, View, Char)):
                return None
            tau, v = float(a[1]), a[0]
        sub, mode = None, 0
        src = v
        if not v.is_input:
            if v.name not in producer or producer[v.name][0] not in ("bl_subtract", "numpy_subtract"):
                return None
            fn2, a = producer[v.name]
            if not plain_scalar(a[1]):
                return None
            sub, mode, src = a[1], (1 if fn2 == "bl_subtract" else 2), a[0]
        lo, n = 0, None
        if isinstance(src, View):
            src, lo, n = src.base, src.lo, src.length
        if not (isinstance(src, Var) and src.is_input and src.kind == "wf" and src.offset == 0):
            return None
        return src, lo, (src.length if n is None else n), sub, mode, tau

    aux, kept = [], []
    for st in steps:
        fn, args, _key = st
        kept.append(st)
        if fn != "linear_slope_fit" or not all(isinstance(a, Var) for a in args[1:5]):
            continue
        a0, first, count = args[0], 0, None
        if isinstance(a0, View):
            a0, first, count = a0.base, a0.lo, a0.length
        pl = pipeline_of(a0) if isinstance(a0, Var) else None
        if pl is None:
            continue
        src, lo, n, sub, mode, tau = pl
        count = n - first if count is None else count
        if not (0 <= first and first + count <= n and count >= 1):
            continue
        gkey = (src.name, lo, n, id(sub) if isinstance(sub, Var) else ("c", sub), mode)
        grp = next((g for g in aux if g["key"] == gkey and len(g["fits"]) < _lib.FIT_MAX
                    and (g["tau"] == tau or tau is None or g["tau"] is None)), None)
        if grp is None:
            grp = {"key": gkey, "src": src, "lo": lo, "len": n, "sub": sub, "mode": mode, "tau": tau, "fits": [], "outs": []}
            aux.append(grp)
        if tau is not None:
            grp["tau"] = tau
        grp["fits"].append((1 if tau is not None else 0, first, count))
        grp["outs"].append(list(args[1:5]))
        kept.pop()  # (the fit leaves the program)
    if aux:  # what only fed those fits is not computed any more
        kept = _live_steps(b, kept, out_pars)
    for gi, g in enumerate(aux):  # the chain reads the results as per-event input columns
        for k, outs in enumerate(g["outs"]):
            for q, o in enumerate(outs):
                o.kind = "scalar"
                o.aux_io = p.add_io(f"aux:{gi}:{4 * k + q}", _lib.IO_SCALAR_IN, ft)
                o.ext_key = f"aux:{gi}:{4 * k + q}"
    return aux, kept


def _push_down_slices(steps, out_names):
    """Slice push-down: an element-wise result (bl_subtract) that is read ONLY through one constant slice [lo:hi] -- the
    long-FIR recipes do that, icpc-dsp-config.json:160-239 -- is computed on that slice alone: a 6092-sample slot instead of
    an 8192-sample one plus a copy.  Same values: the op is per sample.  ``steps`` is changed in place; returns
    {sliced-input variable: (samples before, samples after) the slice that a LOAD screens for NaN}."""
    whole_nan_rule = {}
    for si, (fn, args, key) in enumerate(steps):
        if fn != "bl_subtract" or not isinstance(args[0], Var) or not isinstance(args[-1], Var) or args[-1].name in out_names:
            continue
        src_v, dst_v = args[0], args[-1]
        found = {(x.lo, x.hi) for _fn, a2, _k in steps for x in a2 if isinstance(x, View) and x.base is dst_v}
        uses_of_dst = sum(1 for _fn, a2, _k in steps for x in a2 if x is dst_v)  # the producing step itself counts once
        if len(found) != 1 or uses_of_dst != 1 or not src_v.is_input or src_v.kind != "wf":
            continue
        (lo, hi), = found
        if not (0 <= lo < hi <= (src_v.length or 0)):
            continue
        # ... except for bl_subtract's NaN rule, which looks at the WHOLE waveform (bl_subtract.py:41-44): the load of the slice also screens
        # the samples outside it (LOAD ip[0..1]); another processor reading the same slice of the input as a plain view must not see that
        pushed = View(src_v, lo, hi)
        if any(isinstance(x, View) and x == pushed for _f, a2, _k in steps for x in a2):
            continue
        whole_nan_rule[pushed.name] = (lo, src_v.length - hi)
        new_args = list(args)
        new_args[0] = pushed
        steps[si] = (fn, new_args, key)
        dst_v.length = hi - lo
        for sj, (fn2, a2, k2) in enumerate(steps):
            if sj != si:
                steps[sj] = (fn2, [dst_v if (isinstance(x, View) and x.base is dst_v) else x for x in a2], k2)
    return whole_nan_rule


def _last_uses(b: _Builder, steps, out_pars):
    """which step reads which variable last (slot reuse, in-place decisions, fusions); an output lives beyond the last step"""
    last_use = {}
    for si, (fn, args, _) in enumerate(steps):
        for a, r in zip(args, _roles(fn)):
            v = _base_of(a)
            if v is not None and r in "wts":
                last_use[v.name] = si
    for o in out_pars:  # (a variable may be known by another name than the output's: an alias, a named slice)
        last_use[o] = len(steps) + 1
        v = _base_of(b.vars.get(o))
        if v is not None:
            last_use[v.name] = len(steps) + 1
    return last_use


_TRAP_OPS = {"trap_filter": _lib.OP_TRAP_FILTER, "trap_norm": _lib.OP_TRAP_NORM, "asym_trap_filter": _lib.OP_ASYM_TRAP}
_WINDOW_OPS = {"windower": _lib.OP_WINDOWER, "avg_current": _lib.OP_AVG_CURRENT, "upsampler": _lib.OP_UPSAMPLER}


class _Emitter:
    """The steps of a program, in their scheduled order, into ops: waveforms get slots, per-event values registers, inputs bindings.  The order
    in which these are handed out is visible in the program; each processor family is a method (``_EMIT``)."""

    def __init__(self, b: _Builder, p: Program, ft, steps, out_names, whole_nan_rule, last_use):
        self.b, self.p, self.ft, self.steps, self.out_names = b, p, ft, steps, out_names
        self.whole_nan_rule, self.last_use = whole_nan_rule, last_use
        self.in_bind, self.consts = {}, {}
        self.ext_alias = {}  # binding name -> name of the buffer a fit / stage ahead of the program filled (a slice of it has a name of its own)
        self.free_slots, self.slot_len = [], []
        self.skip = set()  # steps a fusion has emitted together with an earlier one
        self.pending_reduce = {}  # trapezoid output name -> what its fused min_max / time_point_thresh op needs

    def run(self):
        for si, (fn, args, key) in enumerate(self.steps):
            if si in self.skip or fn == "alias":
                continue
            what = f"{fn} ({key})"
            if fn in ("min_max", "time_point_thresh", "amax", "fixed_time_pickoff") and isinstance(args[0], Var) and args[0].name in self.pending_reduce:
                self.fused_reduction(si, fn, args, what)
            elif fn in _READ_OFF:
                self.read_off(si, fn, args, what)
            elif fn.startswith("ew:"):
                self.elementwise(si, fn, args, what)
            elif fn in _EMIT:
                _EMIT[fn](self, si, fn, args, what)
            else:
                raise NotImplementedError(f"processor '{fn}' is not implemented on the device path")

    # --- slots, registers, operands
    def new_slot(self, length):
        # one slot per waveform variable: dsp_chain_create packs slots with disjoint lifetimes into the same LDS, whatever their
        # lengths.  Only a recipe with more variables than slot ids goes back to an id whose variable is dead.
        if len(self.slot_len) >= _lib.MAX_SLOTS:
            for s in self.free_slots:
                if self.slot_len[s] == length:
                    self.free_slots.remove(s)
                    return s
        self.slot_len.append(int(length))
        return len(self.slot_len) - 1

    def free(self, slot):
        if slot not in self.free_slots:
            self.free_slots.append(slot)

    def dead_after(self, v, si) -> bool:
        return self.last_use.get(v.name, -1) <= si

    def release(self, v, si):
        if v.slot is not None and self.dead_after(v, si) and v.kind == "wf":
            self.free(v.slot)

    def period_of(self, args):
        for a in args:
            v = _base_of(a)
            if v is not None and v.period is not None:
                return v.period
        return self.b.default_period

    def ensure_loaded(self, a, si):
        """Waveform operand -> slot.  Chain inputs are loaded on first use (a constant slice of an input is free)."""
        b, p = self.b, self.p
        if isinstance(a, View):
            base, lo, hi, key = a.base, a.lo, a.hi, a.name
            v = b.vars.get(key)
            if base.is_input:
                if v is None:
                    v = Var(key, "wf", hi - lo, base.dtype, source=base.source, offset=lo, grid=a.grid, is_coord=False)
                    v.is_input = True
                    v.ext_key, v.ext_len = base.ext_key, base.ext_len  # (a waveform a stage wrote: same buffer, first sample lo)
                    b.vars[key] = v
                    self.last_use[key] = self.last_use.get(base.name, si)
                return self.ensure_loaded(v, si)
            if v is not None and v.slot is not None:
                return v  # the same slice was materialised for an earlier processor and is still alive
            src = self.ensure_loaded(base, si)
            v = Var(key, "wf", hi - lo, np.float32, grid=a.grid, is_coord=False)
            v.slot = self.new_slot(v.length)
            p.add_op(_lib.OP_COPY, dst=v.slot, src=src.slot, ip=(lo,))
            b.vars[key] = v
            self.last_use[key] = max((sj for sj, (_, a2, _k) in enumerate(self.steps) for x in a2 if isinstance(x, View) and x == a), default=si)
            return v
        v = a
        if v.kind != "wf":
            raise ProcessingChainError(f"'{v.name}' is not a waveform")
        if v.slot is None:
            if not v.is_input:
                raise ProcessingChainError(f"waveform '{v.name}' is used before it is computed")
            if v.ext_key is not None:  # written by a stage ahead of the program: float32 rows of the variable's length
                io = p.add_io(f"in:{v.name}", _lib.IO_WF_IN, np.float32, v.length, v.offset, v.ext_len)
                self.ext_alias[f"in:{v.name}"] = v.ext_key
            else:
                col = _column(b.tb_in, v.source)
                io = p.add_io(f"in:{v.name}", _lib.IO_WF_IN, col.dtype, v.length, v.offset, col.shape[1])
                self.in_bind[f"in:{v.name}"] = v
            v.slot = self.new_slot(v.length)
            screens = self.whole_nan_rule.get(v.name, ())
            if v.nan_uniform:  # rows a stage wrote with pole_zero's rule: all NaN or free of NaN (DSP_OP_LOAD ip[2])
                screens = (*(screens or (0, 0)), 1)
            p.add_op(_lib.OP_LOAD, dst=v.slot, io=io, ip=screens)
        return v

    def expression(self, a: SExpr, args, what):
        """the register of an expression between per-event values; its first reader emits the op (its operands were computed by earlier
        processors)"""
        p, ft = self.p, self.ft
        if a.sreg is not None:
            return Scalar.reg(a.sreg)

        def opnd(x):
            return self.scalar_operand(x, args, what=what) if isinstance(x, (Var, SExpr)) else Scalar.const(float(x))

        r = p.add_sregs(1)
        if a.op in ("affine", "div"):
            p.add_op(_lib.OP_SCALAR_AFFINE if a.op == "affine" else _lib.OP_SCALAR_DIV, dst=r, sp=tuple(opnd(x) for x in a.args))
        elif a.op == "func":
            code, *xs = a.args
            if code == _lib.FN_COPY and a.want_dtype not in (None, ft):
                raise NotImplementedError(f"{what}: astype to {a.want_dtype} in a chain whose loop type is {ft}")
            if (code >> 8) & 0xff == 32 and ft != np.dtype(np.float64):
                # a 32-bit integer loop between per-event values of a float32 chain (len(v) // 2, eventnumber + 1): the registers are
                # float32, so the operation is the float one -- the same integer as long as operands and result stay below 2**24
                float_fn = {_lib.FN_IADD: _lib.FN_ADD, _lib.FN_ISUB: _lib.FN_SUB, _lib.FN_IMUL: _lib.FN_MUL, _lib.FN_IFLOORDIV: _lib.FN_FLOORDIV}
                if code & 0xff not in float_fn:
                    raise NotImplementedError(f"{what}: astype to a 32-bit integer in a chain whose loop type is {ft}")
                code = float_fn[code & 0xff]
            sp = [opnd(x) for x in xs] + [Scalar.const(0.0)] * (3 - len(xs))
            p.add_op(_lib.OP_SCALAR_FUNC, dst=r, ip=(code,), sp=tuple(sp))
        elif a.op == "convert":
            x, off_in, off_out, ratio = a.args
            p.add_op(_lib.OP_SCALAR_CONVERT, dst=r, ip=(a.mode,), sp=(opnd(x), opnd(off_in), opnd(off_out), Scalar.const(ratio)))
        else:
            raise ProcessingChainError(f"{what}: cannot evaluate '{a.name}'")
        a.sreg = r
        return Scalar.reg(a.sreg)

    def column(self, a, name, dtype, buffer=None, var=None):
        """a per-event value that is in HBM before the program runs, bound on first use: a column of the input table (``var``), or one a fit,
        a stage or the integer program ahead of this one wrote (``buffer``)"""
        if a.io is None:
            a.io = self.p.add_io(name, _lib.IO_SCALAR_IN, dtype)
            if var is not None:
                self.in_bind[name] = var
            else:
                self.ext_alias[name] = buffer
        return Scalar.input(a.io)

    def scalar_operand(self, a, args, integer=False, what=""):
        """Scalar argument -> Scalar (const / input column / register)."""
        if isinstance(a, SExpr) and a.op == "ext":  # a column the integer program ahead of this one wrote (_int_island)
            if a.ext_key is None:
                raise ProcessingChainError(f"{what}: '{a.name}' is written by the integer program as an output only")
            return self.column(a, a.ext_key, a.ext_dtype, buffer=a.ext_key)
        if isinstance(a, SExpr):
            return self.expression(a, args, what)
        if isinstance(a, Var):
            if a.kind == "const":
                a = a.const
            elif a.kind == "scalar":
                if a.sreg is not None:
                    return Scalar.reg(a.sreg)
                if a.aux_io is not None:  # a fit done ahead of the chain
                    return Scalar.input(a.aux_io)
                if a.ext_key is not None:  # a fit or a stage ahead of this program
                    return self.column(a, f"in:{a.name}", self.ft if a.ext_dtype is None else a.ext_dtype, buffer=a.ext_key)
                if a.is_input:
                    return self.column(a, f"in:{a.name}", _column(self.b.tb_in, a.source).dtype, var=a)
                raise ProcessingChainError(f"scalar '{a.name}' is used before it is computed")
            else:
                raise ProcessingChainError(f"{what}: '{a.name}' is not a scalar")
        if isinstance(a, Quantity):  # (no grid on this processor: the reference refuses; the input's sampling period is used)
            per = self.period_of(args)
            if per is None:
                raise ProcessingChainError(f"{what}: time quantity without a sampling period (wrap the input in WaveformInput)")
            a = float(a) / per
        if isinstance(a, (View, Char, Grid)):
            raise ProcessingChainError(f"{what}: expected a number or a per-event variable, got {a!r}")
        if integer:  # reference :1767-1768: integer parameters are rounded after the unit conversion
            return int(a) if isinstance(a, (int, np.integer)) else int(np.rint(float(a)))
        return Scalar.const(float(a))

    @staticmethod
    def char_of(a):
        if isinstance(a, Char):
            return ord(a.value[0])
        if isinstance(a, (int, np.integer)):
            return int(a)
        raise ProcessingChainError(f"expected a character argument, got {a!r}")

    @staticmethod
    def out_wf(a, length, fn=None):
        """the waveform a processor writes, ``length`` samples if nothing declared it (None: it must be declared)"""
        if not isinstance(a, Var):
            raise ProcessingChainError("output argument must be a variable name")
        if a.kind is None:
            a.kind, a.length = "wf", length
        if a.kind != "wf":
            raise ProcessingChainError(f"'{a.name}' is not a waveform output")
        if a.length is None:
            a.length = length
        a.dtype = np.dtype(np.float32)
        if a.length is None:
            raise ProcessingChainError(f"{fn}: declare the output as name(length, 'f')")
        return a

    def out_scalar(self, a):
        if not isinstance(a, Var):
            raise ProcessingChainError("output argument must be a variable name")
        if a.kind is None:
            a.kind = "scalar"
        if a.sreg is None:
            a.sreg = self.p.add_sregs(1)
        return a

    def out_row(self, outs, refusal):
        """registers in a row for the named results of one op: min_max, linear_slope_fit, the peak finder's counts, histogram_stats"""
        first = self.p.add_sregs(len(outs))
        for k, a in enumerate(outs):
            if not isinstance(a, Var):
                raise ProcessingChainError(refusal)
            a.kind, a.sreg = "scalar", first + k
        return first

    # --- the processor families
    def read_off(self, si, fn, args, what):
        """one per-event value read off a waveform: load the source, make the output's register, emit one op, release (``_READ_OFF``)"""
        opcode, out, operands, operands_first = _READ_OFF[fn]
        so = lambda a, **kw: self.scalar_operand(a, args, what=what, **kw)  # noqa: E731
        src = self.ensure_loaded(args[0], si)
        if operands_first:
            ip, sp = operands(self, args, so)
        o = self.out_scalar(args[out])
        if not operands_first:
            ip, sp = operands(self, args, so)
        self.p.add_op(opcode, dst=o.sreg, src=src.slot, ip=ip, sp=sp)
        self.release(src, si)

    def in_place(self, si, fn, args, what):
        """a result that may take its source's place: the subtractions, min_max_norm, the pole-zero corrections"""
        p = self.p
        src = self.ensure_loaded(args[0], si)
        dst = self.out_wf(args[-1], src.length)
        inplace = self.dead_after(src, si)
        dst.slot = src.slot if inplace else self.new_slot(src.length)
        if fn == "bl_subtract":
            p.add_op(_lib.OP_BL_SUBTRACT, dst=dst.slot, src=src.slot, sp=(self.scalar_operand(args[1], args, what=what),))
        elif fn in ("numpy_subtract", "numpy_add"):
            y = args[1]
            if fn == "numpy_add":  # w + y = w - (-y), exactly
                y = SExpr("affine", (y, -1.0, -0.0), "(-...)", None, False, None) if isinstance(y, (Var, SExpr)) else -float(y)
            p.add_op(_lib.OP_BL_SUBTRACT, dst=dst.slot, src=src.slot, ip=(1,), sp=(self.scalar_operand(y, args, what=what),))
        else:
            opcode = {"min_max_norm": _lib.OP_MIN_MAX_NORM, "pole_zero": _lib.OP_POLE_ZERO, "double_pole_zero": _lib.OP_DOUBLE_POLE_ZERO}[fn]
            p.add_op(opcode, dst=dst.slot, src=src.slot, sp=tuple(self.scalar_operand(a, args, what=what) for a in args[1:-1]))
        if not inplace:
            self.release(src, si)

    def elementwise(self, si, fn, args, what):
        code, *opn, dst = args
        if code == _lib.FN_COPY and dst.want_dtype not in (None, self.ft):
            raise NotImplementedError(f"{what}: astype to {dst.want_dtype} in a chain whose loop type is {self.ft}")
        if (code >> 8) & 0xff == 32 and self.ft != np.dtype(np.float64):
            raise NotImplementedError(f"{what}: a 32-bit integer loop on waveforms in a chain whose loop type is {self.ft} (its values do not hold every "
                                      "32-bit integer); make one operand a float (astype)")
        slots, sps, srcs = [], [], []
        for x, r in zip(opn, fn[3:]):
            if r == "w":
                v = self.ensure_loaded(x, si)
                slots.append(v.slot)
                sps.append(Scalar.const(0.0))
                srcs.append(v)
            else:
                slots.append(-1)
                sps.append(self.scalar_operand(x, args, what=what) if r == "s" else Scalar.const(0.0))
        dead = next((v for v in srcs if self.dead_after(v, si)), None)  # the result may take the place of an operand nobody reads again
        dst.slot = dead.slot if dead is not None else self.new_slot(dst.length)
        self.p.add_op(_lib.OP_ELEMENTWISE, dst=dst.slot, src=slots[0], ip=(code, slots[1], slots[2]), sp=tuple(sps))
        for v in srcs:
            if v is not dead and v.slot != dst.slot:
                self.release(v, si)

    def multi_extrema(self, si, fn, args, what):
        """the whole program of the peak finder's stage: LOAD, MULTI_EXTREMA; the stores of its lists and counts follow (``_emit_outputs``)"""
        src = self.ensure_loaded(args[0], si)
        sp = tuple(self.scalar_operand(args[k], args, what=what) for k in (1, 2, 4, 5))
        direction = self.scalar_operand(args[3], args, integer=True, what=what)
        vt_max, vt_min = self.out_wf(args[6], None, fn), self.out_wf(args[7], None, fn)
        if vt_max.length != vt_min.length:
            raise ProcessingChainError(f"{what}: the two lists share one length ({vt_max.length} and {vt_min.length} declared)")
        vt_max.slot, vt_min.slot = self.new_slot(vt_max.length), self.new_slot(vt_min.length)
        first = self.out_row(args[8:10], f"{what}: the counts must be variable names")
        self.p.add_op(_lib.OP_MULTI_EXTREMA, dst=vt_max.slot, src=src.slot, ip=(direction, vt_min.slot, first), sp=sp)
        self.release(src, si)

    def histogram(self, si, fn, args, what):
        """LOAD, HISTOGRAM of the histogram's stage; a fused histogram_stats and the stores follow"""
        src = self.ensure_loaded(args[0], si)
        weights, borders = self.out_wf(args[1], None, fn), self.out_wf(args[2], None, fn)
        weights.slot, borders.slot = self.new_slot(weights.length), self.new_slot(borders.length)
        self.p.add_op(_lib.OP_HISTOGRAM, dst=weights.slot, src=src.slot, ip=(borders.slot,))
        self.release(src, si)

    def histogram_stats(self, si, fn, args, what):
        """HISTOGRAM_STATS on the slots of a histogram in the same program, or on weights and edges loaded from rows in memory"""
        weights, edges = self.ensure_loaded(args[0], si), self.ensure_loaded(args[1], si)
        max_in = self.scalar_operand(args[5], args, what=what)
        first = self.out_row(args[2:5], f"{what}: mode_out, max_out and fwhm_out must be variable names")
        self.p.add_op(_lib.OP_HISTOGRAM_STATS, src=weights.slot, ip=(edges.slot, first), sp=(max_in,))

    def multi_time_point_thresh(self, si, fn, args, what):
        """the whole program of the stage: LOAD, [LOAD of a list per event,] MULTI_TIME_POINT_THRESH; the store of t_out follows"""
        src, thr = self.ensure_loaded(args[0], si), args[1]
        if isinstance(thr, Var) and thr.kind == "taps":  # one list for every row: a constant vector of the program
            if thr.io is None:
                thr.io = self.p.add_io(f"taps:{thr.name}", _lib.IO_TAPS, self.ft, thr.length, 0, 0)
                self.consts[f"taps:{thr.name}"] = thr.const.astype(self.ft)
            io, lists, m = thr.io, -1, thr.length
        else:
            tv = self.ensure_loaded(thr, si)
            io, lists, m = 0, tv.slot, tv.length
        t_start = self.scalar_operand(args[2], args, what=what)
        t_out = self.out_wf(args[5], m, fn)
        t_out.slot = self.new_slot(m)
        self.p.add_op(_lib.OP_MULTI_TIME_POINT_THRESH, dst=t_out.slot, src=src.slot, io=io, ip=(self.char_of(args[4]), lists),
                      sp=(t_start, Scalar.const(float(args[3]))))
        self.release(src, si)

    def psd(self, si, fn, args, what):
        """the whole program of the stage: LOAD, PSD; the store of the spectrum follows"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[1], src.length // 2 + 1, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_PSD, dst=out.slot, src=src.slot)
        self.release(src, si)

    def sort(self, si, fn, args, what):
        """the whole program of the stage: LOAD, SORT; the store of the sorted row follows"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[1], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_SORT, dst=out.slot, src=src.slot)
        self.release(src, si)

    def interpolating_upsampler(self, si, fn, args, what):
        """the whole program of the stage: LOAD, INTERP_UPSAMPLE; the store of the resampled row follows"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[2], None, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_INTERP_UPSAMPLE, dst=out.slot, src=src.slot, ip=(self.char_of(args[1]),))
        self.release(src, si)

    def reflected_convolve(self, si, fn, args, what):
        """the whole program of the stage: LOAD, REFLECTED_CONVOLVE; an avg_current of the filtered row may follow, then the stores"""
        src = self.ensure_loaded(args[0], si)
        taps = args[1]
        out = self.out_wf(args[2], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_REFLECTED_CONVOLVE, dst=out.slot, src=src.slot, io=self.taps_io(taps), ip=(int(np.isnan(taps.const).any()),))
        self.release(src, si)

    def rc_cr2(self, si, fn, args, what):
        """LOAD, [BL_SUBTRACT,] RC_CR2 of the pile-up stage; the walk of the filtered row may follow, then the stores"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[2], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_RC_CR2, dst=out.slot, src=src.slot, sp=(self.scalar_operand(args[1], args, what=what),))
        self.release(src, si)

    def bi_level_zero_crossing(self, si, fn, args, what):
        """BI_LEVEL_ZERO_CROSSING on the rows of the stage, or on the filtered row of the same program; the stores of its lists and count follow"""
        src = self.ensure_loaded(args[0], si)
        sp = tuple(self.scalar_operand(args[k], args, what=what) for k in (1, 2, 3, 4))
        polarity, times = self.out_wf(args[6], None, fn), self.out_wf(args[7], None, fn)
        polarity.slot, times.slot = self.new_slot(polarity.length), self.new_slot(times.length)
        first = self.out_row(args[5:6], f"{what}: the count must be a variable name")
        self.p.add_op(_lib.OP_BI_LEVEL_ZERO_CROSSING, dst=polarity.slot, src=src.slot, ip=(times.slot, first), sp=sp)
        self.release(src, si)

    def peak_snr_threshold(self, si, fn, args, what):
        """LOAD, LOAD of the candidates, PEAK_SNR_THRESHOLD of the picker's stage; a multi_a_filter of the packed list may follow, then the stores"""
        src, lst = self.ensure_loaded(args[0], si), self.ensure_loaded(args[1], si)
        sp = (self.scalar_operand(args[2], args, what=what), self.scalar_operand(args[3], args, what=what))
        out = self.out_wf(args[4], lst.length, fn)
        out.slot = self.new_slot(out.length)
        first = self.out_row(args[5:6], f"{what}: the count must be a variable name")
        self.p.add_op(_lib.OP_PEAK_SNR_THRESHOLD, dst=out.slot, src=src.slot, ip=(lst.slot, first), sp=sp)
        self.release(lst, si)
        self.release(src, si)

    def multi_a_filter(self, si, fn, args, what):
        """MULTI_A_FILTER on rows and a list loaded from memory, or on the rows and the packed list of a picker in the same program"""
        src, lst = self.ensure_loaded(args[0], si), self.ensure_loaded(args[1], si)
        out = self.out_wf(args[2], lst.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_MULTI_A_FILTER, dst=out.slot, src=src.slot, ip=(lst.slot,))
        self.release(lst, si)
        self.release(src, si)

    def log_check(self, si, fn, args, what):
        """LOAD, [BL_SUBTRACT,] LOG_CHECK of the tail-fit stage; a poly_fit of the logged row may follow, then the stores"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[1], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_LOG_CHECK, dst=out.slot, src=src.slot)
        self.release(src, si)

    def poly_fit(self, si, fn, args, what):
        """POLY_FIT on the rows of the stage, or on the logged row of the same program; the inverted matrix is a float64 binding in both loops"""
        src, inv = self.ensure_loaded(args[0], si), args[2]
        out = self.out_wf(args[1], None, fn)
        out.slot = self.new_slot(out.length)
        if inv.io is None:
            inv.io = self.p.add_io(f"taps:{inv.name}", _lib.IO_TAPS, np.float64, inv.length, 0, 0)
            self.consts[f"taps:{inv.name}"] = np.ascontiguousarray(inv.const, dtype=np.float64).reshape(-1)
        self.p.add_op(_lib.OP_POLY_FIT, dst=out.slot, src=src.slot, io=inv.io)
        self.release(src, si)

    def poly_residual(self, si, fn, args, what):
        """POLY_DIFF / POLY_EXP_RMS on rows and coefficients loaded from memory, or on the rows (or the logged row) and the coefficients of a
        poly_fit in the same program; the stores of its two results follow"""
        src, pars = self.ensure_loaded(args[0], si), self.ensure_loaded(args[1], si)
        first = self.out_row(args[2:4], f"{what}: mean and rms must be variable names")
        self.p.add_op(_lib.OP_POLY_DIFF if fn == _POLY_DIFF else _lib.OP_POLY_EXP_RMS, dst=first, src=src.slot, ip=(pars.slot,))
        self.release(pars, si)
        self.release(src, si)

    def inl_correction(self, si, fn, args, what):
        """the whole program of the stage: LOAD of the integer rows, INL_CORRECTION; the store of the corrected row follows"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[2], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_INL_CORRECTION, dst=out.slot, src=src.slot, io=self.taps_io(args[1]))
        self.release(src, si)

    def get_wf_centroid(self, si, fn, args, what):
        """the whole program of the stage: LOAD, WF_CENTROID; the store of the centroid follows"""
        src = self.ensure_loaded(args[0], si)
        o = self.out_scalar(args[2])
        self.p.add_op(_lib.OP_WF_CENTROID, dst=o.sreg, src=src.slot, sp=(self.scalar_operand(args[1], args, what=what),))
        self.release(src, si)

    def wf_alignment(self, si, fn, args, what):
        """LOAD, WF_ALIGNMENT of the aligner's stage; a wf_correction of the window may follow, then the stores"""
        src = self.ensure_loaded(args[0], si)
        sp = tuple(self.scalar_operand(args[k], args, what=what) for k in (1, 2, 3))
        out = self.out_wf(args[4], None, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_WF_ALIGNMENT, dst=out.slot, src=src.slot, sp=sp)
        self.release(src, si)

    def wf_correction(self, si, fn, args, what):
        """WF_CORRECTION on rows loaded from memory, or on the window of an alignment in the same program"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[4], src.length, fn)
        out.slot = self.new_slot(out.length)
        self.p.add_op(_lib.OP_WF_CORRECTION, dst=out.slot, src=src.slot, io=self.taps_io(args[1]), ip=(int(args[2]), int(args[3])))
        self.release(src, si)

    def taps_io(self, v):
        """the binding of a constant array, made at its first use"""
        if v.io is None:
            v.io = self.p.add_io(f"taps:{v.name}", _lib.IO_TAPS, self.ft, v.length, 0, 0)
            self.consts[f"taps:{v.name}"] = np.ascontiguousarray(v.const, dtype=self.ft).reshape(-1)
        return v.io

    def normalisation_layer(self, si, fn, args, what):
        """LOAD, NORMALISE in place; a dense layer of the same stage or the store of the normalised row follows"""
        src = self.ensure_loaded(args[0], si)
        out = self.out_wf(args[3], src.length, fn)
        out.slot = src.slot
        self.p.add_op(_lib.OP_NORMALISE, dst=src.slot, src=src.slot, io=self.taps_io(args[1]), ip=(self.taps_io(args[2]),))

    def dense_layer(self, si, fn, args, what):
        """[LOAD,] DENSE; the store of the m outputs -- of the one value, for a classification layer -- follows"""
        classify = fn.startswith("classification")
        src = self.ensure_loaded(args[0], si)
        io_w = self.taps_io(args[1])
        io_b = self.taps_io(args[2]) if fn.endswith("with_bias") else -1
        act = self.char_of(args[-2])
        if classify:
            o = self.out_scalar(args[-1])
            self.p.add_op(_lib.OP_DENSE, dst=o.sreg, src=src.slot, io=io_w, ip=(act, io_b, src.length, 0))
        else:
            m = int(args[1].const.shape[1])
            out = self.out_wf(args[-1], m, fn)
            out.slot = self.new_slot(m)
            self.p.add_op(_lib.OP_DENSE, dst=out.slot, src=src.slot, io=io_w, ip=(act, io_b, src.length, m))
        self.release(src, si)

    def svm_predict(self, si, fn, args, what):
        """the whole program of the stage: LOAD, SVM_PREDICT; the store of the label follows.  The model is float64 bindings in both loops"""
        src = self.ensure_loaded(args[0], si)
        ios = []
        for v in args[2:7]:
            if v.io is None:
                v.io = self.p.add_io(f"taps:{v.name}", _lib.IO_TAPS, np.float64, v.length, 0, 0)
                self.consts[f"taps:{v.name}"] = np.ascontiguousarray(v.const, dtype=np.float64).reshape(-1)
            ios.append(v.io)
        o = self.out_scalar(args[1])
        self.p.add_op(_lib.OP_SVM_PREDICT, dst=o.sreg, src=src.slot, io=ios[0], ip=tuple(ios[1:]),
                      sp=(Scalar.const(float(args[7])), Scalar.const(float(args[8])), Scalar.const(-1.0)))
        self.release(src, si)

    def copy_slice(self, si, fn, args, what):
        src = self.ensure_loaded(args[0], si)
        dst = args[3]
        dst.slot = self.new_slot(dst.length)
        self.p.add_op(_lib.OP_COPY, dst=dst.slot, src=src.slot, ip=(int(args[1]), int(args[2])))
        self.release(src, si)

    def trapezoid(self, si, fn, args, what):
        p, steps, last_use, char_of = self.p, self.steps, self.last_use, self.char_of
        src = self.ensure_loaded(args[0], si)
        ints = [self.scalar_operand(a, args, integer=True, what=what) for a in args[1:-1]]
        ints += [0] * (3 - len(ints))
        dst = self.out_wf(args[-1], src.length)
        # fusion: the trapezoid's only consumer is the next fixed_time_pickoff and it is not an output
        nxt = steps[si + 1] if si + 1 < len(steps) else None
        if (nxt and nxt[0] == "fixed_time_pickoff" and _base_of(nxt[1][0]) is dst and last_use.get(dst.name) == si + 1
                and dst.name not in self.out_names and char_of(nxt[1][2]) != ord("s")):
            t_in = self.scalar_operand(nxt[1][1], nxt[1], what=what)
            o = self.out_scalar(nxt[1][3])
            p.add_op(_lib.OP_TRAP_PICKOFF, dst=o.sreg, src=src.slot, io=char_of(nxt[1][2]), ip=(*ints, _TRAP_OPS[fn]), sp=(t_in,))
            self.skip.add(si + 1)
            self.release(src, si + 1)
            return
        # fusion: the trapezoid only feeds one min_max and / or one time_point_thresh (the t0 chain of the LEGEND recipes:
        # asym_trap_filter -> min_max -> time_point_thresh) and is not an output -> it is never stored.  The fused op is emitted
        # where the last of the two stands, so their scalar operands (a threshold computed in between) are ready
        users = [sj for sj, (f2, a2, _k) in enumerate(steps) if sj > si and sj not in self.skip and any(_base_of(x) is dst for x in a2)]
        kinds = [steps[sj][0] for sj in users]
        plain = all(steps[sj][1][0] is dst for sj in users)  # (not through a slice)
        pick_ok = all(char_of(steps[sj][1][2]) != ord("s") for sj in users if steps[sj][0] == "fixed_time_pickoff")
        if (users and plain and pick_ok and dst.name not in self.out_names
                and sorted(kinds) in (["min_max"], ["time_point_thresh"], ["min_max", "time_point_thresh"], ["amax"], ["amax", "fixed_time_pickoff"])
                and not any(isinstance(x, View) and x.base is dst for _f, a2, _k in steps for x in a2)):
            self.pending_reduce[dst.name] = {"src": src, "ints": ints, "kind": _TRAP_OPS[fn], "emit_at": max(users), "mm_first": -1}
            last_use[src.name] = max(last_use.get(src.name, si), max(users))
            return
        dst.slot = self.new_slot(src.length)
        p.add_op(_TRAP_OPS[fn], dst=dst.slot, src=src.slot, ip=ints)
        self.release(src, si)

    def fused_reduction(self, si, fn, args, what):
        """a reader of a trapezoid that is never stored (``trapezoid``): its part of the fused op, which the last reader emits"""
        p = self.p
        pr = self.pending_reduce[args[0].name]
        if fn == "fixed_time_pickoff":  # trapEftp beside trapEmax: the samples around the pick-off time are captured in the same pass
            pr["pick"] = (self.scalar_operand(args[1], args, what=what), self.char_of(args[2]), self.out_scalar(args[3]))
        elif fn == "amax":  # numpy.amax of a trapezoid (trapEmax): the a_max of the same reduction (NaN in, NaN out in both)
            pr["mm_first"] = p.add_sregs(4)
            pr["amax_only"] = pr["kind"] != _lib.OP_ASYM_TRAP
            if not isinstance(args[2], Var):
                raise ProcessingChainError("numpy.amax output must be a variable name")
            args[2].kind, args[2].sreg = "scalar", pr["mm_first"] + 3
        elif fn == "min_max":
            pr["mm_first"] = self.out_row(args[1:5], "min_max outputs must be variable names")
        else:
            pr["tpt"] = (tuple(self.scalar_operand(a, args, what=what) for a in args[1:4]), self.out_scalar(args[4]))
        if si == pr["emit_at"]:
            sp, o = pr.get("tpt", ((), None))
            code = pr["kind"] | ((1 << 30) if pr.get("amax_only") else 0)
            if "pick" in pr:
                t_in, mode, po = pr["pick"]
                code |= (mode << 8) | ((po.sreg + 1) << 16)
                sp = tuple(sp) + (Scalar.const(0.0),) * (3 - len(sp)) + (t_in,)
            p.add_op(_lib.OP_TRAP_REDUCE, dst=pr["mm_first"], src=pr["src"].slot, io=(o.sreg if o is not None else -1),
                     ip=(*pr["ints"], code), sp=sp)
            self.release(pr["src"], si)
            del self.pending_reduce[args[0].name]

    def four_values(self, si, fn, args, what):
        """min_max, and linear_slope_fit where it stayed in the program"""
        a0, view = args[0], ()
        if fn == "linear_slope_fit":
            view = (0, 0)
            if isinstance(a0, View) and not a0.is_input:  # a window of an intermediate: read in place
                a0, view = a0.base, (a0.lo, a0.length)
        src = self.ensure_loaded(a0, si)
        first = self.out_row(args[1:5], f"{fn} outputs must be variable names")
        self.p.add_op(_lib.OP_MIN_MAX if fn == "min_max" else _lib.OP_LINEAR_SLOPE_FIT, dst=first, src=src.slot, ip=view)
        self.release(src, si)

    def window(self, si, fn, args, what):
        """windower, avg_current, upsampler: a declared output of another length, one per-event operand"""
        src = self.ensure_loaded(args[0], si)
        dst = self.out_wf(args[2], None, fn)
        dst.slot = self.new_slot(dst.length)
        self.p.add_op(_WINDOW_OPS[fn], dst=dst.slot, src=src.slot, sp=(self.scalar_operand(args[1], args, what=what),))
        self.release(src, si)

    def moving_window_multi(self, si, fn, args, what):
        p = self.p
        src = self.ensure_loaded(args[0], si)
        num = self.scalar_operand(args[2], args, integer=True, what=what)
        typ = self.scalar_operand(args[3], args, integer=True, what=what)
        dst = self.out_wf(args[4], src.length)
        win = args[1]
        chunk = -(-(-(-src.length // 64)) // 16) * 16  # samples of a waveform per lane (dsp_chain_create: a multiple of 16)
        if (self.dead_after(src, si) and num >= 1 and (_is_number(win) or win is True) and float(win) == int(win) and 1 <= int(win) <= chunk):
            # in place: a source nobody reads again is overwritten pass by pass; only the ends of the lanes' chunks (64 x window
            # samples) are kept aside.  One waveform instead of two in LDS for the averaged current of the Ge recipes (22 + 13 kB
            # instead of 43): with that the whole recipe fits four times into a CU instead of three
            dst.slot = src.slot
            side = self.new_slot(64 * int(win))
            p.add_op(_lib.OP_MOVING_WINDOW_MULTI, dst=dst.slot, src=src.slot, ip=(typ, num, side, 1), sp=(self.scalar_operand(win, args, what=what),))
            self.free(side)
            return
        dst.slot = self.new_slot(src.length)
        # ping-pong target of the passes before the last: with an odd number of windows the first pass goes source -> target, so a
        # source nobody reads again serves
        own = num > 1 and not (num % 2 == 1 and self.dead_after(src, si))
        tmp = self.new_slot(src.length) if own else (src.slot if num > 1 else dst.slot)
        p.add_op(_lib.OP_MOVING_WINDOW_MULTI, dst=dst.slot, src=src.slot, ip=(typ, num, tmp), sp=(self.scalar_operand(args[1], args, what=what),))
        if own:
            self.free(tmp)
        self.release(src, si)

    def wavelet(self, si, fn, args, what):
        src = self.ensure_loaded(args[0], si)
        level = self.scalar_operand(args[1], args, integer=True, what=what)
        wt, part = self.char_of(args[2]), self.char_of(args[3])
        if wt not in (ord("h"), ord("d")):
            raise NotImplementedError("only the Haar wavelet ('h' / 'd') is implemented on the device")
        dst = self.out_wf(args[4], None, fn)
        dead = self.dead_after(src, si)
        scratch = src.slot if dead else self.new_slot(src.length)
        dst.slot = self.new_slot(dst.length)
        self.p.add_op(_lib.OP_DWT_HAAR, dst=dst.slot, src=src.slot, ip=(level, part, scratch))
        if dead:
            self.release(src, si)
        else:
            self.free(scratch)

    def convolve(self, si, fn, args, what):
        p, steps = self.p, self.steps
        src = self.ensure_loaded(args[0], si)
        taps = args[1]
        if not (isinstance(taps, Var) and taps.kind == "taps"):
            raise NotImplementedError(f"{fn}: the kernel must be a constant computed in the recipe (cusp_filter / zac_filter)")
        if taps.io is None:  # (zeros after the taps up to a multiple of the FIR op's tap block: its fast path then covers every tap)
            padded = -(-taps.length // 16) * 16
            taps.io = p.add_io(f"taps:{taps.name}", _lib.IO_TAPS, self.ft, padded, 0, 0)
            self.consts[f"taps:{taps.name}"] = np.concatenate([taps.const.astype(self.ft), np.zeros(padded - taps.length, dtype=self.ft)])
        dst = self.out_wf(args[3], None, fn)
        has_nan = int(np.isnan(taps.const).any()) | (2 if np.isinf(taps.const).any() else 0)  # (bit 1: an infinite tap)
        # fusion: the filtered waveform's only consumer is one numpy.amax and it is not an output -> it is never stored
        users = [sj for sj, (f2, a2, _k) in enumerate(steps) if sj != si and any(_base_of(x) is dst for x in a2)]
        if (len(users) == 1 and steps[users[0]][0] == "amax" and steps[users[0]][1][0] is dst and dst.name not in self.out_names
                and users[0] > si and users[0] not in self.skip):
            o = self.out_scalar(steps[users[0]][1][2])
            p.add_op(_lib.OP_CONVOLVE_AMAX, dst=o.sreg, src=src.slot, io=taps.io, ip=(self.char_of(args[2]), has_nan, int(dst.length), int(taps.length)))
            self.skip.add(users[0])
            self.last_use[src.name] = max(self.last_use.get(src.name, si), si)
            self.release(src, si)
            return
        dst.slot = self.new_slot(dst.length)
        p.add_op(_lib.OP_CONVOLVE, dst=dst.slot, src=src.slot, io=taps.io,
                 ip=(self.char_of(args[2]), has_nan, int(_piecewise_constant(taps.const)), int(taps.length)))
        self.release(src, si)


#: processors that read one per-event value off a waveform (``_Emitter.read_off``): name -> (op, index of the output argument, (emitter,
#: arguments, ``so``: a scalar argument as an operand) -> (ip, sp) of the op, are the operands resolved before the output's register is made?)
_READ_OFF = {
    "sample": (_lib.OP_PICKOFF, 2, lambda e, a, so: ((ord("n"), 1), (Scalar.const(float(a[1])),)), False),
    "get": (_lib.OP_PICKOFF, 2, lambda e, a, so: ((ord("n"), 2), (so(a[1]), Scalar.const(float("nan")))), False),
    "fixed_time_pickoff": (_lib.OP_PICKOFF, 3, lambda e, a, so: ((e.char_of(a[2]),), (so(a[1]),)), False),
    "time_point_thresh": (_lib.OP_TIME_POINT_THRESH, 4, lambda e, a, so: ((), tuple(so(x) for x in a[1:4])), True),
    "interpolated_time_point_thresh": (_lib.OP_INTERP_TIME_POINT_THRESH, 5, lambda e, a, so: (
        (e.char_of(a[4]),), (so(a[1]), so(a[2]), Scalar.const(float(so(a[3], integer=True))))), True),
    "amax": (_lib.OP_AMAX, 2, lambda e, a, so: ((), ()), False),
    "mean_below_threshold": (_lib.OP_MEAN_BELOW, 2, lambda e, a, so: ((), (so(a[1]),)), False),
    _TIME_OVER: (_lib.OP_TIME_OVER_THRESHOLD, 2, lambda e, a, so: ((), (so(a[1]),)), False),
    "trap_pickoff": (_lib.OP_TRAP_WINDOW_PICKOFF, 4, lambda e, a, so: (tuple(so(x, integer=True) for x in a[1:3]), (so(a[3]),)), False),
}
#: the other processors -> the method of ``_Emitter`` that emits their family
_EMIT = {**dict.fromkeys(_IN_PLACE, _Emitter.in_place), **dict.fromkeys(_TRAP_OPS, _Emitter.trapezoid), **dict.fromkeys(_WINDOW_OPS, _Emitter.window),
         "slice": _Emitter.copy_slice, "min_max": _Emitter.four_values, "linear_slope_fit": _Emitter.four_values,
         "moving_window_multi": _Emitter.moving_window_multi, "discrete_wavelet_transform": _Emitter.wavelet,
         "convolve_wf": _Emitter.convolve, "fft_convolve_wf": _Emitter.convolve, _MULTI_EXTREMA: _Emitter.multi_extrema,
         _HISTOGRAM: _Emitter.histogram, _HISTOGRAM_STATS: _Emitter.histogram_stats, _MULTI_TPT: _Emitter.multi_time_point_thresh,
         _PSD: _Emitter.psd, _SORT: _Emitter.sort, _INTERP: _Emitter.interpolating_upsampler, _REFLECT: _Emitter.reflected_convolve, _RC_CR2: _Emitter.rc_cr2,
         _BI_LEVEL: _Emitter.bi_level_zero_crossing, _PEAK_SNR: _Emitter.peak_snr_threshold, _MULTI_A: _Emitter.multi_a_filter,
         _INL: _Emitter.inl_correction, _WF_CENTROID: _Emitter.get_wf_centroid, _WF_ALIGN: _Emitter.wf_alignment, _WF_CORR: _Emitter.wf_correction,
         _LOG_CHECK: _Emitter.log_check, _POLY_FIT: _Emitter.poly_fit, _POLY_DIFF: _Emitter.poly_residual, _POLY_EXP_RMS: _Emitter.poly_residual,
         _NORMALISE: _Emitter.normalisation_layer, **dict.fromkeys(_DENSE_LAYERS, _Emitter.dense_layer), _SVM: _Emitter.svm_predict}


def _emit_outputs(e: _Emitter, out_pars, island_out, n_rows, stage_mode):
    """The stores of the recipe's outputs, behind the last processor.  Returns (the output table, the output bindings, {variable-length
    output: the input column that holds its per-event lengths})."""
    b, p, ft = e.b, e.p, e.ft
    tb_out, out_bind, vector_lens = {}, {}, {}
    for o in out_pars:
        v = b.vars.get(o)
        if o in island_out:  # written by the integer program, in its own type
            nat, col_dt = island_out[o]
            out_bind[f"out:{o}"] = (SimpleNamespace(name=o, dtype=col_dt), None)
            tb_out[o] = np.empty(n_rows, dtype=nat)
            continue
        if isinstance(v, View):  # a named slice: of an input it is read straight from the rows, else copied out of its waveform
            v = e.ensure_loaded(v, len(e.steps))
        if v is None or v.kind in (None,):
            raise ProcessingChainError(f"output '{o}' was never computed")
        if v.kind == "const":
            c = np.asarray(v.const)  # a number, or a constant array ("a1": "[1, 2, 3]"): every row holds it
            tb_out[o] = np.broadcast_to(c, (n_rows, *c.shape)).copy()
            continue
        if v.kind == "taps":
            tb_out[o] = np.broadcast_to(v.const, (n_rows, v.length)).copy()
            continue
        if v.kind == "wf":
            if v.slot is None and v.is_input:  # (an input under another name, or astype of nothing: load it to store it)
                v = e.ensure_loaded(v, len(e.steps))
            if v.slot is None:
                raise ProcessingChainError(f"output waveform '{o}' was never computed")
            odt = np.dtype(np.bool_) if v.dtype == np.dtype(np.bool_) else ft
            unit_ns = _time_unit_ns(v.unit)
            src_slot = v.slot
            if v.is_coord is True and v.grid is not None and unit_ns is not None and not stage_mode:
                # a list of sample indices (get_multi_local_extrema) written in its time unit: (index + grid offset) * period, sample by sample,
                # in the chain's float type (exact while the times are integers below 2^24; the reference forms them in float64)
                off_in = b.offset_in_periods(v.grid, v.grid.period)
                off_in = e.scalar_operand(off_in, [], what=f"output {o}") if isinstance(off_in, (Var, SExpr)) else Scalar.const(float(off_in))
                src_slot = e.new_slot(v.length)
                p.add_op(_lib.OP_ELEMENTWISE, dst=src_slot, src=v.slot, ip=(_lib.FN_ADD, -1, -1), sp=(Scalar.const(0.0), off_in, Scalar.const(0.0)))
                p.add_op(_lib.OP_ELEMENTWISE, dst=src_slot, src=src_slot, ip=(_lib.FN_MUL, -1, -1),
                         sp=(Scalar.const(0.0), Scalar.const(v.grid.period / unit_ns), Scalar.const(0.0)))
            io = p.add_io(f"out:{o}", _lib.IO_WF_OUT, odt, v.length)
            p.add_op(_lib.OP_STORE, src=src_slot, io=io)
            out_bind[f"out:{o}"] = (SimpleNamespace(name=o, dtype=odt), v.length)
            if v.vector_len is not None and not stage_mode:  # (a stage hands on whole rows: the lengths leave with the recipe's outputs)
                vl = v.vector_len
                if isinstance(vl, Var) and vl.is_input and vl.source is not None:
                    vector_lens[o] = vl.source  # a column of the input table
                elif isinstance(vl, Var) and vl.name in out_pars:
                    vector_lens[o] = vl.name    # a per-event value the recipe computes: an output (a hidden one if the recipe does not ask for it)
                else:
                    raise NotImplementedError(f"output '{o}': vector_len must be the length of an input array or a per-event variable the recipe computes")
            tb_out[o] = np.empty((n_rows, v.length), dtype=v.dtype if _is_int_dtype(v) and v.dtype.kind != "b" else odt)
            continue
        # a time coordinate is written in its unit, not in samples: (index + grid offset) * period (reference :1990-2014, get_buffer(unit))
        unit_ns = _time_unit_ns(v.unit)
        if v.is_coord is True and v.grid is not None and unit_ns is not None and not stage_mode:  # (a stage hands on sample indices)
            v = b.converted(v, Grid(unit_ns))
        if isinstance(v, Var) and v.sreg is None and (v.aux_io is not None or v.ext_key is not None):
            src_op = e.scalar_operand(v, [], what=f"output {o}")  # (stores read registers)
            v.sreg = p.add_sregs(1)
            p.add_op(_lib.OP_SCALAR_FUNC, dst=v.sreg, ip=(_lib.FN_COPY,), sp=(src_op, Scalar.const(0.0), Scalar.const(0.0)))
        if isinstance(v, Var) and v.sreg is None:
            if v.is_input:
                tb_out[o] = _column(b.tb_in, v.source)
                continue
            raise ProcessingChainError(f"output '{o}' was never computed")
        reg = e.scalar_operand(v, [], what=f"output {o}")
        odt = np.dtype(np.bool_) if getattr(v, "dtype", None) == np.dtype(np.bool_) else ft
        as_dt = v.out_dtype  # (a count of get_multi_local_extrema: uint32 -- as its stage writes it, and as the table holds it)
        if stage_mode and as_dt is not None:
            odt = np.dtype(as_dt)
        io = p.add_io(f"out:{o}", _lib.IO_SCALAR_OUT, odt)
        p.add_op(_lib.OP_STORE_SCALAR, io=io, ip=(reg.index,))
        out_bind[f"out:{o}"] = (SimpleNamespace(name=o, dtype=odt, table_dtype=None if stage_mode or as_dt is None else np.dtype(as_dt)), None)
        tb_out[o] = np.empty(n_rows, dtype=v.dtype if isinstance(v, SExpr) and _is_int_dtype(v) and v.dtype.kind != "b" else (as_dt or odt))
    return tb_out, out_bind, vector_lens


def _fit_descriptors(e: _Emitter, aux):
    """what the runtime launches for the fits that ``_extract_fits`` took out, with the program's bindings of their rows and subtrahends"""
    b, p = e.b, e.p
    aux_desc = []
    for gi, g in enumerate(aux):
        src = g["src"]
        col = _column(b.tb_in, src.source)
        wf_bind = next((nm for nm, v in e.in_bind.items() if isinstance(v, Var) and v.kind == "wf" and v.source == src.source and v.offset == 0
                        and v.length == src.length), None)
        if wf_bind is None:  # (nothing in the program reads the whole row: bind it for the fit alone)
            wf_bind = f"in:{src.name}:fit{gi}"
            p.add_io(wf_bind, _lib.IO_WF_IN, col.dtype, src.length, 0, col.shape[1])
            e.in_bind[wf_bind] = src
        sub_bind, sub_const, sub_code = None, 0.0, _lib.F32
        if isinstance(g["sub"], Var):
            sub_bind = p.io[e.scalar_operand(g["sub"], [], what="linear_slope_fit").index][0]
            sub_code = dtype_code(_column(b.tb_in, g["sub"].source).dtype)
        elif g["sub"] is not None:
            sub_const = float(g["sub"])
        aux_desc.append({"wf": wf_bind, "dtype": dtype_code(col.dtype), "itemsize": np.dtype(col.dtype).itemsize, "lo": g["lo"], "len": g["len"],
                         "stride": col.shape[1], "sub": sub_bind, "sub_dtype": sub_code, "sub_const": sub_const, "mode": g["mode"],
                         "tau": g["tau"], "fits": list(g["fits"]), "names": [f"aux:{gi}:{j}" for j in range(4 * len(g["fits"]))]})
    return aux_desc


def _compile(b: _Builder, out_pars, n_rows, proc_strings, stage_mode=False):
    """The passes, in order.  ``stage_mode``: the program of a stage that runs ahead of the main program (_extract_stages): the integer
    program, fits and other stages are not taken out of it again; their results arrive as bindings (``Var.ext_key``)."""
    p = Program()
    ft = b.stage_ft if stage_mode else _loop_dtype(b)
    main = not stage_mode
    off = lambda switch: os.environ.get(switch) == "1"  # noqa: E731
    steps = b.steps
    hidden = []
    if main:
        out_pars = list(out_pars)
        for o in list(out_pars):  # the computed length of a variable-length output leaves with it: a hidden output if the recipe does not ask for it
            vl = getattr(b.vars.get(o), "vector_len", None)
            if isinstance(vl, Var) and not vl.is_input and vl.name not in out_pars and b.vars.get(vl.name) is vl:
                out_pars.append(vl.name)
                hidden.append(vl.name)
        for own in _OWN_KERNEL:
            if not any(st[0] == own for st in steps):
                continue
            if off("DSPEED_HIP_NO_STAGES"):
                raise NotImplementedError(f"{own} runs as a stage ahead of the program, on a kernel of its own: not with DSPEED_HIP_NO_STAGES=1")
            if ft != np.dtype(np.float32):
                raise NotImplementedError(f"{own} in a recipe whose loop type is {ft}: the stages ahead of the program hand on float32 rows")
    island, island_out = _int_island(b, steps, out_pars, ft) if main else (None, {})
    aux, stages = [], []
    if main and not off("DSPEED_HIP_FIT_IN_CHAIN"):
        aux, steps = _extract_fits(b, steps, out_pars, p, ft)
    # long FIRs on the matrix cores, ahead of the program: their results are bindings of the program
    if main and ft == np.dtype(np.float32) and not off("DSPEED_HIP_NO_STAGES"):
        steps, stages = _extract_stages(b, steps, out_pars, n_rows, ft)
    if island is not None:
        stages = [island] + stages
    steps = b.steps = _schedule(steps)
    out_names = set(out_pars)  # names of the variables that are outputs (a variable may have another name than the output: alias, named slice)
    out_names.update(v.name for v in (_base_of(b.vars.get(o)) for o in out_pars) if v is not None)
    whole_nan_rule = _push_down_slices(steps, out_names)
    e = _Emitter(b, p, ft, steps, out_names, whole_nan_rule, _last_uses(b, steps, out_pars))
    e.run()
    tb_out, out_bind, vector_lens = _emit_outputs(e, out_pars, island_out, n_rows, stage_mode)
    aux_desc = _fit_descriptors(e, aux)
    p.slots = e.slot_len
    if not p.ops:  # (every output is written by the integer program or handed through: the program is a placeholder)
        p.add_op(_lib.OP_SCALAR_AFFINE, dst=p.add_sregs(1), sp=(Scalar.const(0.0), Scalar.const(0.0), Scalar.const(0.0)))
    if len(p.ops) > _lib.MAX_OPS or len(p.slots) > _lib.MAX_SLOTS or len(p.io) > _lib.MAX_IO or p.n_sregs > _lib.MAX_SREGS:
        raise NotImplementedError("recipe is too large for one device chain (ops/slots/bindings limit)")
    for st in stages:  # columns of the input table that only a stage reads are linked like the program's own
        for nm, v in st["in_vars"].items():
            e.in_bind.setdefault(nm, v)
    tail = _split_scalar_tail(p, ft) if main and not off("DSPEED_HIP_NO_SCALAR_TAIL") else None
    if main and not off("DSPEED_HIP_NO_SCALAR_HEAD"):  # (behind the tail's cut: what is only stored is the tail's)
        head = _split_scalar_head(p, ft, e.ext_alias)
        if head is not None:
            stages.append(head)
    walks = _split_walks(p, ft) if main and not off("DSPEED_HIP_NO_WALKS_BEHIND") else None
    from .processing_chain import ProcessingChain  # (the runtime imports this module)

    chain = ProcessingChain(p, e.in_bind, out_bind, e.consts, n_rows, proc_strings, ft, aux_desc, stages=stages, ext_alias=e.ext_alias, tail=tail, walks=walks)
    chain.vector_lens = vector_lens  # variable-length outputs -> the input column, or the output, that holds their per-event lengths
    chain.hidden_outputs = hidden    # outputs the recipe did not ask for: the computed lengths of variable-length outputs
    return chain, tb_out


_SCALAR_OPS = (_lib.OP_SCALAR_AFFINE, _lib.OP_SCALAR_DIV, _lib.OP_SCALAR_CONVERT, _lib.OP_SCALAR_FUNC, _lib.OP_STORE_SCALAR)


def _reads_of(op):
    """the registers an op reads"""
    opcode, _dst, _src, _io, ip, sp = op
    return [a.index for a in sp if a.kind == _lib.ARG_REG] + ([ip[0]] if opcode == _lib.OP_STORE_SCALAR else [])


def _writes_of(op):
    """the registers an op writes"""
    opcode, dst, _src, io, ip, _sp = op
    if opcode in (_lib.OP_STORE_SCALAR, _lib.OP_LOAD, _lib.OP_STORE):
        return []
    if opcode == _lib.OP_MIN_MAX:
        return [dst + k for k in range(4)]
    if opcode == _lib.OP_TRAP_REDUCE:  # (its extremes, the maximum alone, a pick-off of the same trapezoid: include/dspeed_hip.h)
        w = [dst + k for k in range(4)] if dst >= 0 else []
        if io >= 0:
            w.append(io)
        if ((ip[3] >> 16) & 0x3fff) - 1 >= 0:
            w.append(((ip[3] >> 16) & 0x3fff) - 1)
        return w
    return [dst]


def _split_off(p: Program, slots=False):
    """an empty program with the registers of ``p``, and the function that gives a binding of ``p`` its place in it (copied on first use)"""
    q = Program()
    q.n_sregs = p.n_sregs
    if slots:
        q.slots = list(p.slots)
    io_map = {}

    def binding(idx):
        if idx not in io_map:
            io_map[idx] = q.add_io(*p.io[idx])
        return io_map[idx]

    return q, binding


#: a tail is cut off when it has at least this many ops (a launch and a column per handed-over register have to pay for themselves)
SCALAR_TAIL_MIN_OPS = 8


#: a head is split off when it takes at least this many ops out of the program
SCALAR_HEAD_MIN_OPS = 2


def _split_scalar_head(p: Program, ft, ext_alias: dict):
    """The counterpart of the scalar tail at the other end: arithmetic between per-event values that needs nothing the program computes --
    pick-off times from the t0 estimate a stage left in HBM, thresholds from fit results -- leaves the program and runs ahead of it with a row
    per lane (dsp_scalar.hip), as one more stage; the program reads the results as columns.  On the interpreter an op costs a row's wavefront
    about 1 700 cycles whatever it computes (a lone wavefront issues its ~ 150 dispatch instructions one per ~ 12 cycles: measured 45 us per
    op and 65 536 rows), and a program of 8192-sample rows holds one row per SIMD.  ``p`` is changed in place; returns the stage's description or
    None.  Registers may be reused along the program: what an op reads is tracked by position."""
    if not p.slots:
        return None  # (no waveform: the program is a row-per-lane program already)
    from_head = {}          # register -> (column name, index into `made`) while the register's current value comes from a head op
    head_ops, made = [], []  # made: [column name, register, read by the program?]
    new_ops = []
    for op in p.ops:
        opcode, dst, src, io, ip, sp = op
        is_head = (opcode in _SCALAR_OPS and opcode != _lib.OP_STORE_SCALAR
                   and all(a.kind in (_lib.ARG_CONST, _lib.ARG_INPUT) or (a.kind == _lib.ARG_REG and a.index in from_head) for a in sp))
        if is_head:
            head_ops.append(op)
            made.append([f"head:r{dst}.{len(made)}", dst, False])
            from_head[dst] = len(made) - 1
            continue
        # an op that stays: what it reads of the head's results arrives as a column
        sp2 = []
        for a in sp:
            if a.kind == _lib.ARG_REG and a.index in from_head:
                made[from_head[a.index]][2] = True
                sp2.append(("head", from_head[a.index]))
            else:
                sp2.append(a)
        if opcode == _lib.OP_STORE_SCALAR and ip[0] in from_head:  # a stored value needs its register: a copy of the column
            made[from_head[ip[0]]][2] = True
            new_ops.append(("copy", ip[0], from_head[ip[0]]))
            del from_head[ip[0]]
        new_ops.append((opcode, dst, src, io, ip, tuple(sp2)))
        for r in _writes_of(op):
            from_head.pop(r, None)
    if len(head_ops) < SCALAR_HEAD_MIN_OPS or not any(m[2] for m in made):
        return None
    h, head_io = _split_off(p)
    for (opcode, dst, src, io, ip, sp), (name, r, used) in zip(head_ops, made):
        h.add_op(opcode, dst=dst, src=src, io=io, ip=ip, sp=tuple(Scalar.input(head_io(a.index)) if a.kind == _lib.ARG_INPUT else a for a in sp))
        if used:  # (stored right behind the op that made it: the head may write the register again)
            h.add_op(_lib.OP_STORE_SCALAR, io=h.add_io("out:" + name, _lib.IO_SCALAR_OUT, ft), ip=(r,))
    col_io = {}

    def column(j):
        if j not in col_io:
            col_io[j] = p.add_io("in:" + made[j][0], _lib.IO_SCALAR_IN, ft)
            ext_alias["in:" + made[j][0]] = "in:" + made[j][0]
        return col_io[j]

    del p.ops[:]
    for entry in new_ops:
        if entry[0] == "copy":
            _c, r, j = entry
            p.add_op(_lib.OP_SCALAR_FUNC, dst=r, ip=(_lib.FN_COPY,), sp=(Scalar.input(column(j)), Scalar.const(0.0), Scalar.const(0.0)))
            continue
        opcode, dst, src, io, ip, sp = entry
        p.add_op(opcode, dst=dst, src=src, io=io, ip=ip, sp=tuple(Scalar.input(column(a[1])) if isinstance(a, tuple) else a for a in sp))
    if len(p.io) > _lib.MAX_IO or len(h.io) > _lib.MAX_IO:
        raise NotImplementedError("recipe is too large for one device chain (ops/slots/bindings limit)")
    names = [io[0] for io in h.io if io[1] == _lib.IO_SCALAR_IN]
    return _stage_record("per-event arithmetic ahead of the program", h, {}, {}, {n: ext_alias.get(n, n) for n in names},
                         [("out:" + name, "in:" + name, None) for name, _r, used in made if used])


#: the rise-time walks leave a program whose waveform has at least this many samples (LDS then holds a handful of rows per CU)
WALKS_BEHIND_MIN_SAMPLES = 4096
#: walks the reductions kernel takes in one program (DSP_REDUCE_WALKS of csrc/dsp_program.h)
WALKS_BEHIND_MAX = 6


def _split_walks(p: Program, ft):
    """The threshold walks of a program that only reads its one long waveform -- the rise times of the Ge recipes: time_point_thresh at 0.99 /
    0.9 / 0.5 / 0.1 of the trapezoid's maximum, each from where the one before ended -- run behind the program as a launch of their own
    (dsp_reduce.hip: a wavefront per row straight off HBM, thousands of rows in flight) instead of in it, where LDS holds four 8192-sample
    rows per CU and the row's wavefronts wait for the chain *trapezoid -> maximum -> walks* (2.1 of 14.2 ms of the Ge recipe's pass on the
    synthetic rows, whose tp_100 walk runs to the end of the waveform; 0.6 - 0.9 on pulses with a rise time).  The per-event values the walks
    start from or scale (the maximum) are handed over as columns (``walk:r<k>``); the stores of the walks' results move along.  ``p`` is
    changed in place; returns {"program", "handover"} or None."""
    from .chain import plan

    ops = p.ops
    if len(p.slots) != 1 or not ops or ops[0][0] != _lib.OP_LOAD or p.slots[0] < WALKS_BEHIND_MIN_SAMPLES:
        return None
    slot = ops[0][1]
    TPT, AFF, STS = _lib.OP_TIME_POINT_THRESH, _lib.OP_SCALAR_AFFINE, _lib.OP_STORE_SCALAR

    n_writes = {}
    for op in ops:
        for r in _writes_of(op):
            n_writes[r] = n_writes.get(r, 0) + 1
    writer = {r: k for k, op in enumerate(ops) for r in _writes_of(op)}

    def readers(r):
        return [(k, j) for k, op in enumerate(ops) for j, a in enumerate(op[5]) if a.kind == _lib.ARG_REG and a.index == r] + \
               [(k, -1) for k, op in enumerate(ops) if op[0] == STS and op[4][0] == r]

    number = lambda a: a.kind == _lib.ARG_CONST  # noqa: E731
    walks = [k for k, op in enumerate(ops) if op[0] == TPT and op[2] == slot and number(op[5][2]) and op[5][2].value in (0.0, 1.0)]
    scales = set()
    changed = True
    while changed:  # a walk stays if its result is read by anything but a store or a moving walk's start; a fraction if anything else reads it
        changed = False
        for k in list(walks):
            d = ops[k][1]
            fine = n_writes.get(d, 0) == 1 and all(j == -1 or (kk in walks and j == 1) for kk, j in readers(d))
            for j in (0, 1):  # threshold, start
                a = ops[k][5][j]
                if a.kind != _lib.ARG_REG:
                    continue
                src = writer.get(a.index)
                if src is None or n_writes.get(a.index, 0) != 1 or src > k:
                    fine = False
                elif ops[src][0] == TPT and src in walks:
                    fine = fine and j == 1
                elif (j == 0 and ops[src][0] == AFF and number(ops[src][5][1]) and number(ops[src][5][2]) and ops[src][5][2].value == 0.0
                      and ops[src][5][0].kind in (_lib.ARG_REG, _lib.ARG_INPUT) and all(kk in walks and jj == 0 for kk, jj in readers(a.index))):
                    x = ops[src][5][0]
                    if x.kind == _lib.ARG_REG and (n_writes.get(x.index, 0) != 1 or writer[x.index] > src or ops[writer[x.index]][0] in (TPT, AFF)):
                        fine = False
                elif ops[src][0] in (TPT, AFF):
                    fine = False  # (a walk that stays, or arithmetic of another form: the program's)
            if not fine:
                walks.remove(k)
                changed = True
    if not 2 <= len(walks) <= WALKS_BEHIND_MAX:
        return None
    for k in walks:
        a = ops[k][5][0]
        if a.kind == _lib.ARG_REG and ops[writer[a.index]][0] == AFF:
            scales.add(writer[a.index])
    moved = set(walks) | scales
    walk_regs = {ops[k][1] for k in walks}
    stores = [k for k, op in enumerate(ops) if op[0] == STS and op[4][0] in walk_regs]
    # what the walks read of the program: registers made by ops that stay -> columns
    handed = []
    for k in sorted(moved):
        for a in ops[k][5][:2] if ops[k][0] == TPT else ops[k][5][:1]:
            if a.kind == _lib.ARG_REG and writer[a.index] not in moved and a.index not in handed:
                handed.append(a.index)
    w, w_io = _split_off(p, slots=True)
    col = {r: w.add_io(f"walk:r{r}", _lib.IO_SCALAR_IN, ft) for r in handed}

    def operand(a):
        if a.kind == _lib.ARG_INPUT:
            return Scalar.input(w_io(a.index))
        if a.kind == _lib.ARG_REG and a.index in col:
            return Scalar.input(col[a.index])
        return a

    ld = ops[0]
    w.add_op(_lib.OP_LOAD, dst=ld[1], src=ld[2], io=w_io(ld[3]), ip=ld[4], sp=ld[5])
    for k in sorted(moved):
        opcode, dst, src, io, ip, sp = ops[k]
        w.add_op(opcode, dst=dst, src=src, io=io, ip=ip, sp=tuple(operand(a) for a in sp))
    for k in stores:
        opcode, dst, src, io, ip, sp = ops[k]
        w.add_op(opcode, dst=dst, src=src, io=w_io(io), ip=ip, sp=sp)
    try:
        if "dsp_reduce_kernel" not in plan(w, ft)["kernel"]:
            return None
    except Exception:  # noqa: BLE001  (a form the planner refuses: the walks stay where they were)
        return None
    gone = moved | set(stores)
    kept = [op for k, op in enumerate(ops) if k not in gone]
    if not any(op[0] not in (_lib.OP_LOAD, STS) for op in kept):
        return None  # (nothing but the walks read the waveform: the program is theirs)
    del ops[:]
    ops.extend(kept)
    handover = []
    for r in handed:
        handover.append(f"walk:r{r}")
        p.add_op(STS, io=p.add_io(f"walk:r{r}", _lib.IO_SCALAR_OUT, ft), ip=(r,))
    if len(p.io) > _lib.MAX_IO or len(w.io) > _lib.MAX_IO:
        raise NotImplementedError("recipe is too large for one device chain (ops/slots/bindings limit)")
    return {"program": w, "handover": handover}


def _split_scalar_tail(p: Program, ft):
    """Cut the all-scalar tail off a program: the ops after the last one that touches a waveform -- arithmetic between per-event values,
    unit conversions, stores; two thirds of a whole recipe's ops -- become a program of their own that ``dsp_chain_create`` gives to the
    row-per-lane kernel (dsp_scalar.hip: 64 rows per interpreter dispatch instead of one).  The head stores every register the tail
    reads and does not make itself into a column (``tail:r<k>``), the tail starts by loading them.  ``p`` is changed in place; returns the
    tail's description ({"program", "handover": [binding names]}) or None when the program has no tail worth a launch."""
    ops = p.ops
    k = len(ops)
    while k > 0 and ops[k - 1][0] in _SCALAR_OPS:
        k -= 1
    if k == 0 or len(ops) - k < SCALAR_TAIL_MIN_OPS:
        return None
    tail_ops = ops[k:]
    written, live_in = set(), []
    for op in tail_ops:
        for r in _reads_of(op):
            if r not in written and r not in live_in:
                live_in.append(r)
        written.update(_writes_of(op))
    t, tail_io = _split_off(p)
    handover = []
    del ops[k:]
    for r in live_in:
        name = f"tail:r{r}"
        handover.append(name)
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, ft), ip=(r,))
        t.add_op(_lib.OP_SCALAR_FUNC, dst=r, ip=(_lib.FN_COPY,),
                 sp=(Scalar.input(t.add_io(name, _lib.IO_SCALAR_IN, ft)), Scalar.const(0.0), Scalar.const(0.0)))
    for opcode, dst, src, io, ip, sp in tail_ops:
        sp2 = tuple(Scalar.input(tail_io(a.index)) if a.kind == _lib.ARG_INPUT else a for a in sp)
        t.add_op(opcode, dst=dst, src=src, io=tail_io(io) if opcode == _lib.OP_STORE_SCALAR else io, ip=ip, sp=sp2)
    if len(t.io) > _lib.MAX_IO or len(p.io) > _lib.MAX_IO or len(p.ops) > _lib.MAX_OPS:
        raise NotImplementedError("recipe is too large for one device chain (ops/slots/bindings limit)")
    return {"program": t, "handover": handover}

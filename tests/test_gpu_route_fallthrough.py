"""A program planned for a specialised kernel, executed on rows that do not start on a 16-byte boundary although their stride keeps them
16 bytes apart: the plan vouches for strides and offsets, only ``dsp_chain_execute`` sees the pointer.  The launch then runs on the next
route that takes the pointer -- the interpreter with its element-wise loads for the energy chain and the run-length FIR, the reduce kernel's
own scalar loads for the reductions -- and gives bit for bit what the same route gives on an aligned copy of the same rows."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
TOL = 1e-6
ROWS = 70


def _off_boundary(w):
    """the rows of ``w`` in device memory, one float32 element past a 16-byte boundary (NaN in front: nothing may read below the rows)"""
    from dspeed_amd.device import DeviceArray

    base = DeviceArray.from_numpy(np.concatenate([np.full(1, np.nan, np.float32), w.ravel(), np.zeros(3, np.float32)]))
    assert base.ptr % 16 == 0
    view = DeviceArray.from_ptr(base.ptr + 4, w.shape, np.float32)
    view._base = base  # (the view keeps the allocation alive)
    return view


def _run(prog, planned, fused, rows_name, rows, inputs, outputs):
    """the program on ``rows`` (a DeviceArray) -> {output: array}; ``outputs``: name -> shape"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray

    ch = Chain(prog, "fall-through", np.float32)
    assert planned in ch.kernel_name, ch.kernel_name
    assert ch.set_fused(fused) == bool(fused)
    bufs = {rows_name: rows, **{name: DeviceArray.from_numpy(a) for name, a in inputs.items()}}
    for name, shape in outputs.items():
        bufs[name] = DeviceArray.zeros(shape, np.float32)
    ch.execute(bufs, ROWS)
    ch.check()
    return {name: bufs[name].to_numpy() for name in outputs}


def _assert_same(got, want):
    for name in want:
        assert np.array_equal(got[name], want[name], equal_nan=True), name


def test_energy_chain_off_boundary_runs_the_interpreter():
    from dspeed_amd.chain import energy_chain_program
    from dspeed_amd.device import DeviceArray

    wf_len, rise, flat = 1024, 64, 16
    rng = np.random.default_rng(wf_len + rise)
    i = np.arange(wf_len, dtype=np.float64)[None, :]
    B = rng.uniform(9000, 11000, (ROWS, 1))
    A = rng.uniform(500, 15000, (ROWS, 1))
    t0 = np.floor(rng.uniform(0.45, 0.55, (ROWS, 1)) * wf_len)
    wf = (B + A * np.exp(-(i - t0) / 1716.28) * (i >= t0) + 5.0 * rng.standard_normal((ROWS, wf_len))).astype(np.float32)
    bl = B[:, 0].astype(np.float32)
    tp = (t0[:, 0] + rise + 0.8 * flat).astype(np.float32)
    wf[11, 17] = np.nan
    bl[14] = np.nan
    tp[15] = np.nan
    prog = energy_chain_program(wf_len, 1716.28, rise, flat, "l")
    inputs, outputs = {"baseline": bl, "t_pick": tp}, {"trapEftp": (ROWS,)}
    got = _run(prog, "dsp_energy_rr_kernel", 1, "waveform", _off_boundary(wf), inputs, outputs)
    vm = _run(prog, "dsp_energy_rr_kernel", 0, "waveform", DeviceArray.from_numpy(wf), inputs, outputs)
    _assert_same(got, vm)
    want, rc = oracle.chain_energy(wf, bl, tp, 1716.28, rise, flat, "l")
    assert rc == 0
    e = got["trapEftp"]
    assert np.array_equal(np.isnan(e), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(e[ok] - want[ok]) / np.abs(want[ok])
    print("energy chain off the boundary vs oracle: max rel", rel.max())
    assert rel.max() <= TOL


def test_run_length_fir_off_boundary_runs_the_interpreter():
    from dspeed_amd.device import DeviceArray
    from test_gpu_fir_runs import _program, _pulses, _taps

    n = 64  # (the smallest rows test_gpu_fir_runs feeds the kernel)
    rng = np.random.default_rng(n)
    taps = _taps("step", rng)
    prog, P, outs = _program(n, 0, n, taps, "f")
    w = _pulses(rng, ROWS, n)
    w[3, n // 2] = np.nan
    w[5, n // 3] = np.inf
    padded = prog.io[1][3]
    inputs = {"taps": np.concatenate([taps, np.zeros(padded - len(taps), np.float32)]), "thr": rng.uniform(5, 200, ROWS).astype(np.float32)}
    outputs = {"filtered": (ROWS, P + 8), **{name: (ROWS,) for name in outs}}
    got = _run(prog, "dsp_fir_runs_kernel", 1, "wf", _off_boundary(w), inputs, outputs)
    vm = _run(prog, "dsp_fir_runs_kernel", 0, "wf", DeviceArray.from_numpy(w), inputs, outputs)
    _assert_same(got, vm)


def test_reductions_off_boundary_stay_on_the_reduce_kernel():
    from dspeed_amd.device import DeviceArray
    from test_gpu_reduce_kernel import _program

    length = 256  # (whole 16-byte vectors a row: planned for the kernel's wide loads, which this launch cannot use)
    rng = np.random.default_rng(length)
    prog, outs = _program(np.float32, length, 0, length, [(0, 0), (length - 1, 0), (length, 0), (2, 1)], walks=[("t_max", 0, None), ("t_min", 1, 1.0)])
    w = rng.normal(0, 1000, (ROWS, length)).astype(np.float32)
    w[1, :] = w[1, 0]
    w[2, [length // 3, length - 1]] = w[2].max()
    w[4, length // 2] = np.nan
    w[5, :] = np.nan
    w[6, length - 1] = np.inf
    w[7, 0] = -np.inf
    thr = rng.uniform(-500, 500, ROWS).astype(np.float32)
    thr[9] = np.nan
    outputs = {name: (ROWS, 2) for name in outs}
    got = _run(prog, "dsp_reduce_kernel", 1, "wf", _off_boundary(w), {"thr": thr}, outputs)
    aligned = _run(prog, "dsp_reduce_kernel", 1, "wf", DeviceArray.from_numpy(w), {"thr": thr}, outputs)
    _assert_same(got, aligned)
    with np.errstate(invalid="ignore"):  # (a_max lives in register 3: column 1 of its interleaved binding; a NaN anywhere: NaN)
        assert np.array_equal(got["a_max"][:, 1], np.max(w, axis=1), equal_nan=True)

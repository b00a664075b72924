#!/usr/bin/env python3
"""Rate of the threshold kernel (dsp_thresh.hip) on a device-resident batch of pulse rows with a rise time, float32 and int16:
multi_time_point_thresh with 3 thresholds (10 / 50 / 90 % of the row's maximum, from the maximum backwards) and with 20, and
time_over_threshold; beside them min_max of the same rows through dsp_reduce.hip -- one streaming pass, the yardstick -- and the same
three times as three time_point_thresh walks of the reductions kernel, as a recipe ran them before.  Device events around a window of at
least a second after two warm-up launches; the forms alternate over `repeats` rounds, every round's figure is kept.
python tools/thresh_rate.py [rows] [samples] [seconds] [repeats] [json file]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain, Program, Scalar  # noqa: E402
from dspeed_amd.device import DeviceArray, Event, Stream, device_info, sync  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
seconds = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 2
out_file = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
FRACTIONS = {3: np.float32([0.1, 0.5, 0.9]), 20: np.linspace(0.05, 0.95, 20).astype(np.float32)}


def min_max_program(dt):
    p = Program()
    p.slots, p.n_sregs = [n], 4
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n))
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
    for r, name in enumerate(("t_min", "t_max", "a_min", "a_max")):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p


def multi_program(dt, m):
    p = Program()
    p.slots = [n, m, m]
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n))
    p.add_op(_lib.OP_LOAD, dst=2, io=p.add_io(f"lists{m}", _lib.IO_WF_IN, np.float32, m))
    ts = Scalar.input(p.add_io("t_max", _lib.IO_SCALAR_IN, np.float32))
    p.add_op(_lib.OP_MULTI_TIME_POINT_THRESH, dst=1, src=0, ip=(ord("l"), 2), sp=(ts, Scalar.const(1.0)))
    p.add_op(_lib.OP_STORE, src=1, io=p.add_io(f"times{m}", _lib.IO_WF_OUT, np.float32, m))
    return p


def over_program(dt):
    p = Program()
    p.slots, p.n_sregs = [n], 1
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n))
    p.add_op(_lib.OP_TIME_OVER_THRESHOLD, dst=0, src=0, sp=(Scalar.input(p.add_io("half", _lib.IO_SCALAR_IN, np.float32)),))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("count", _lib.IO_SCALAR_OUT, np.float32), ip=(0,))
    return p


def walks_program(dt, promise=False):
    """three time_point_thresh walks backwards from the maximum, thresholds and start as columns.  ``promise``: the rows are NaN-free or
    all NaN (LOAD ip[2], what pole_zero writes): the reductions kernel then reads only what the walks visit; int16 rows need none"""
    p = Program()
    p.slots, p.n_sregs = [n], 3
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n), ip=(0, 0, 1) if promise else ())
    ts = Scalar.input(p.add_io("t_max", _lib.IO_SCALAR_IN, np.float32))
    for k in range(3):
        thr = Scalar.input(p.add_io(f"thr{k}", _lib.IO_SCALAR_IN, np.float32))
        p.add_op(_lib.OP_TIME_POINT_THRESH, dst=k, src=0, sp=(thr, ts, Scalar.const(0.0)))
    for k in range(3):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(f"walk{k}", _lib.IO_SCALAR_OUT, np.float32), ip=(k,))
    return p


st = Stream()
device = device_info(0).get("name")
results = []
for dt, code in ((np.float32, _lib.F32), (np.int16, _lib.I16)):
    wf, bl, tp = DeviceArray((rows, n), dt), DeviceArray((rows,), np.float32), DeviceArray((rows,), np.float32)
    _lib.check(_lib.lib().dsp_synth_pulses(wf.ptr, code, rows, n, n, bl.ptr, tp.ptr, 0xD5BEED, 0, 1716.28, 5.0, 625 + 0.8 * 188, -30.0, 30.0,
                                           5000.0, 15000.0, 20.0, 80.0, st.ptr), what="synth")
    sync()
    bufs = {"wf": wf, "count": DeviceArray((rows,), np.float32)}
    bufs.update({k: DeviceArray((rows,), np.float32) for k in ("t_min", "t_max", "a_min", "a_max", "walk0", "walk1", "walk2")})
    mm = Chain(min_max_program(dt), "min_max", np.float32)
    mm.execute({k: bufs[k] for k in mm.io_names}, rows, st)
    sync()
    mm.check(st)
    a_max = bufs["a_max"].to_numpy()
    for m, f in FRACTIONS.items():
        bufs[f"lists{m}"] = DeviceArray.from_numpy(np.ascontiguousarray(a_max[:, None] * f[None, :]))
        bufs[f"times{m}"] = DeviceArray((rows, m), np.float32)
    for k in range(3):
        bufs[f"thr{k}"] = DeviceArray.from_numpy(a_max * FRACTIONS[3][k])
    bufs["half"] = bufs["thr1"]
    forms = [("min_max (dsp_reduce.hip)", min_max_program(dt)), ("multi_time_point_thresh, m = 3", multi_program(dt, 3)),
             ("multi_time_point_thresh, m = 20", multi_program(dt, 20)), ("time_over_threshold", over_program(dt)),
             ("three time_point_thresh walks", walks_program(dt))]
    if dt == np.float32:
        forms.append(("three time_point_thresh walks, rows promised NaN-free", walks_program(dt, promise=True)))
    chains = []
    for name, prog in forms:
        try:
            chains.append((name, Chain(prog, name, np.float32)))
        except Exception as exc:  # (a form the planner does not take is reported, not measured)
            results.append({"form": name, "rows_dtype": np.dtype(dt).name, "error": str(exc)})
    run = lambda ch, k: [ch.execute({x: bufs[x] for x in ch.io_names}, rows, st) for _ in range(k)]  # noqa: E731
    steps = {}
    for name, ch in chains:
        run(ch, 2)
        sync()
        ch.check(st)
        e0, e1 = Event(), Event()
        e0.record(st)
        run(ch, 5)
        e1.record(st)
        sync()
        steps[name] = max(5, int(np.ceil(seconds / max(e0.elapsed_ms(e1) * 1e-3 / 5, 1e-6))))
    times = {name: [] for name, _ in chains}
    for _ in range(repeats):
        for name, ch in chains:
            e0, e1 = Event(), Event()
            e0.record(st)
            run(ch, steps[name])
            e1.record(st)
            sync()
            ch.check(st)
            times[name].append(e0.elapsed_ms(e1) * 1e-3 / steps[name])
    # what was measured: the share of rows with three finite times, and that the walks found the same samples
    t3 = bufs["times3"].to_numpy()[:4096]
    walks = np.stack([bufs[f"walk{k}"].to_numpy()[:4096] for k in range(3)], axis=1)
    floor = float(min(times["min_max (dsp_reduce.hip)"]))
    for name, ch in chains:
        best = min(times[name])
        results.append({"form": name, "rows_dtype": np.dtype(dt).name, "kernel": ch.kernel_name, "rows": rows, "samples": n, "launches_per_window": steps[name],
                        "ms_each_round": [round(t * 1e3, 4) for t in times[name]], "ms_best": round(best * 1e3, 4), "waveforms_per_s": round(rows / best),
                        "row_GBps_one_pass": round(rows * n * np.dtype(dt).itemsize / best / 1e9, 1), "ratio_to_min_max": round(best / floor, 3)})
    results.append({"form": "what the rows gave", "rows_dtype": np.dtype(dt).name, "rows_with_three_times": float(np.isfinite(t3).all(axis=1).mean()),
                    "walks_end_at_the_sample_after_the_times": float(np.mean(np.ceil(t3) == walks)),
                    "mean_samples_from_the_maximum_to_the_10_percent_time": float(np.nanmean(bufs["t_max"].to_numpy()[:4096] - t3[:, 0]))})
    for d in bufs.values():
        d.free()
    bl.free()
    tp.free()
for rec in results:
    print(json.dumps(rec))
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump({"tool": "tools/thresh_rate.py", "device": device, "results": results}, f, indent=1)

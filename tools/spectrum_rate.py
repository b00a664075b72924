#!/usr/bin/env python3
"""Rate of the spectrum kernel (dsp_spectrum.hip): psd of a device-resident batch of synthetic pulse rows -- 8192 samples, float32 and
int16 (the packed transform, a workgroup per row), then 1000 samples (Bluestein, 2048 points) and 1024 (a wavefront per row) -- beside
min_max of the same rows through dsp_reduce.hip, one streaming pass: the yardstick of the other row-streaming kernels.  Device events around
a window of `seconds` after two warm-up launches; the forms alternate over `repeats` rounds, every round's figure is kept.
python tools/spectrum_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]
(with seconds 0: two launches of each form and no timing -- what a counter run wants)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain, Program  # noqa: E402
from dspeed_amd.device import DeviceArray, Event, Stream, device_info, sync  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else None
lengths = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [8192, 1000, 1024]


def min_max_program(dt, n):
    p = Program()
    p.slots, p.n_sregs = [n], 4
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n))
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
    for r, name in enumerate(("t_min", "t_max", "a_min", "a_max")):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p


def psd_program(dt, n):
    p = Program()
    m = n // 2 + 1
    p.slots = [n, m]
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dt, n, 0, n))
    p.add_op(_lib.OP_PSD, dst=1, src=0)
    p.add_op(_lib.OP_STORE, src=1, io=p.add_io("psd", _lib.IO_WF_OUT, np.float32, m))
    return p


st = Stream()
device = device_info(0).get("name")
results = []
for n in lengths:
    for dt, code in ((np.float32, _lib.F32), (np.int16, _lib.I16)) if n == lengths[0] else ((np.float32, _lib.F32),):
        wf, bl, tp = DeviceArray((rows, n), dt), DeviceArray((rows,), np.float32), DeviceArray((rows,), np.float32)
        _lib.check(_lib.lib().dsp_synth_pulses(wf.ptr, code, rows, n, n, bl.ptr, tp.ptr, 0xD5BEED, 0, 1716.28, 5.0, 0.4 * n, -30.0, 30.0,
                                               5000.0, 15000.0, 20.0, 80.0, st.ptr), what="synth")
        sync()
        bufs = {"wf": wf, "psd": DeviceArray((rows, n // 2 + 1), np.float32)}
        bufs.update({k: DeviceArray((rows,), np.float32) for k in ("t_min", "t_max", "a_min", "a_max")})
        chains = [(name, Chain(prog, name, np.float32)) for name, prog in (("min_max (dsp_reduce.hip)", min_max_program(dt, n)), ("psd", psd_program(dt, n)))]
        run = lambda ch, k: [ch.execute({x: bufs[x] for x in ch.io_names}, rows, st) for _ in range(k)]  # noqa: E731
        steps = {}
        for name, ch in chains:
            run(ch, 2)
            sync()
            ch.check(st)
            if seconds > 0:
                e0, e1 = Event(), Event()
                e0.record(st)
                run(ch, 3)
                e1.record(st)
                sync()
                steps[name] = max(3, int(np.ceil(seconds / max(e0.elapsed_ms(e1) * 1e-3 / 3, 1e-6))))
        times = {name: [] for name, _ in chains}
        for _ in range(repeats if seconds > 0 else 0):
            for name, ch in chains:
                e0, e1 = Event(), Event()
                e0.record(st)
                run(ch, steps[name])
                e1.record(st)
                sync()
                ch.check(st)
                times[name].append(e0.elapsed_ms(e1) * 1e-3 / steps[name])
        # what was measured: the first rows' spectra against NumPy's float64 rfft of the same rows
        k = min(rows, 16)
        w = DeviceArray.from_ptr(wf.ptr, (k, n), dt).to_numpy()
        got = DeviceArray.from_ptr(bufs["psd"].ptr, (k, n // 2 + 1), np.float32).to_numpy()
        want = np.abs(np.fft.rfft(w.astype(np.float64), axis=1)) ** 2 / n
        check = float(np.abs(got - want).sum() / want.sum())
        for name, ch in chains:
            rec = {"form": name, "rows_dtype": np.dtype(dt).name, "kernel": ch.kernel_name, "rows": rows, "samples": n, "geometry": ch.geometry(rows)}
            if times[name]:
                best, floor = min(times[name]), min(times["min_max (dsp_reduce.hip)"])
                rec.update({"launches_per_window": steps[name], "ms_each_round": [round(t * 1e3, 4) for t in times[name]], "ms_best": round(best * 1e3, 4),
                            "waveforms_per_s": round(rows / best), "row_GBps_one_pass": round(rows * n * np.dtype(dt).itemsize / best / 1e9, 1),
                            "ratio_to_min_max": round(best / floor, 3)})
            if name == "psd":
                rec["sum_abs_error_over_sum_of_the_float64_psd_first_rows"] = check
            results.append(rec)
        for d in bufs.values():
            d.free()
        bl.free()
        tp.free()
for rec in results:
    print(json.dumps(rec))
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump({"tool": "tools/spectrum_rate.py", "device": device, "results": results}, f, indent=1)

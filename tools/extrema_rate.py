#!/usr/bin/env python3
"""Rate of the peak finder (dsp_extrema.hip) on a device-resident batch of float32 and int16 rows, search directions 0 and 3, for a
delta above the noise (a handful of extrema per row: the stream) and one inside it (hundreds: the transitions); beside it min_max of the
same rows through dsp_reduce.hip, the streaming rate this access pattern reaches here.  Device events around `steps` launches after
two warm-up launches; the forms alternate over `repeats` rounds, every round's figure is kept.
python tools/extrema_rate.py [rows] [samples] [steps] [repeats] [json file]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain, Program, Scalar  # noqa: E402
from dspeed_amd.device import DeviceArray, Event, Stream, sync  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_file = sys.argv[5] if len(sys.argv) > 5 else None


def extrema_program(dtype, direction, delta, M):
    p = Program()
    p.slots = [n, M, M]
    p.n_sregs = 2
    wf = p.add_io("wf", _lib.IO_WF_IN, dtype, n, 0, n)
    p.add_op(_lib.OP_LOAD, dst=0, io=wf)
    p.add_op(_lib.OP_MULTI_EXTREMA, dst=1, src=0, ip=(direction, 2, 0),
             sp=(Scalar.const(delta), Scalar.const(delta), Scalar.const(-np.inf), Scalar.const(np.inf)))
    p.add_op(_lib.OP_STORE, src=1, io=p.add_io("vt_max", _lib.IO_WF_OUT, np.float32, M, 0, 2048))
    p.add_op(_lib.OP_STORE, src=2, io=p.add_io("vt_min", _lib.IO_WF_OUT, np.float32, M, 0, 2048))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_max", _lib.IO_SCALAR_OUT, np.uint32), ip=(0,))
    p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_min", _lib.IO_SCALAR_OUT, np.uint32), ip=(1,))
    return p


def min_max_program(dtype):
    p = Program()
    p.slots = [n]
    p.n_sregs = 4
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io("wf", _lib.IO_WF_IN, dtype, n, 0, n))
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
    for r in range(4):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(f"o{r}", _lib.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p


st = Stream()
results = []
for dtype, code in ((np.float32, _lib.F32), (np.int16, _lib.I16)):
    wf = DeviceArray((rows, n), dtype)
    bl, tp = DeviceArray((rows,), np.float32), DeviceArray((rows,), np.float32)
    _lib.check(_lib.lib().dsp_synth_waveforms(wf.ptr, code, rows, n, n, bl.ptr, tp.ptr, 0xD5BEED, 0, 1716.28, 5.0, 625 + 0.8 * 188,
                                              -30.0, 30.0, 500.0, 15000.0, st.ptr), what="synth")
    sync()
    M_MOST = 2048  # (the lists' buffers: rows of the longest m, every form writes the first m of each)
    bufs = {"wf": wf, "vt_max": DeviceArray((rows, M_MOST), np.float32), "vt_min": DeviceArray((rows, M_MOST), np.float32),
            "n_max": DeviceArray((rows,), np.uint32), "n_min": DeviceArray((rows,), np.uint32)}
    bufs.update({f"o{r}": DeviceArray((rows,), np.float32) for r in range(4)})
    forms = [("min_max (dsp_reduce.hip)", min_max_program(dtype))]
    # delta 100: the pulse and little else, lists of 20; delta 20 (four sigma of the noise): hundreds of extrema, lists long enough to hold them
    for delta, direction, m in ((100.0, 0, 20), (100.0, 3, 20), (20.0, 0, 2048), (20.0, 3, 64)):
        forms.append((f"extrema direction {direction} delta {delta:g} m {m}", extrema_program(dtype, direction, delta, m)))
    chains = [(name, Chain(prog, name, np.float32), prog) for name, prog in forms]
    for name, ch, prog in chains:
        for _ in range(2):
            ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
        sync()
        ch.check(st)
    times = {name: [] for name, _, _ in chains}
    for _ in range(repeats):
        for name, ch, prog in chains:
            e0, e1 = Event(), Event()
            e0.record(st)
            for _ in range(steps):
                ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
            e1.record(st)
            sync()
            ch.check(st)
            times[name].append(e0.elapsed_ms(e1) * 1e-3 / steps)
    found = {}
    for name, ch, prog in chains:
        if "extrema" in name:
            ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
            sync()
            found[name] = float(bufs["n_max"].to_numpy()[:4096].mean())
    for name, ch, prog in chains:
        best = min(times[name])
        byts = rows * n * np.dtype(dtype).itemsize
        rec = {"form": name, "rows_dtype": np.dtype(dtype).name, "kernel": ch.kernel_name, "rows": rows, "samples": n,
               "ms_each_round": [round(t * 1e3, 4) for t in times[name]], "ms_best": round(best * 1e3, 4), "waveforms_per_s": round(rows / best),
               "row_GBps": round(byts / best / 1e9, 1), "frac_of_8TBps": round(byts / best / 8e12, 3)}
        if name in found:
            rec["mean_maxima_found_of_m"] = round(found[name], 2)
        results.append(rec)
        print(json.dumps(rec))
    del chains, bufs, wf
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump({"tool": "tools/extrema_rate.py", "device": "MI355X", "results": results}, f, indent=1)

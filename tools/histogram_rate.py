#!/usr/bin/env python3
"""Rate of the histogram kernel (dsp_hist.hip) on a device-resident batch of float32 rows, 100 bins: rows spread over the bins, noise rows
concentrated in a few bins (same-address LDS increments), and the fused launch with histogram_stats that stores no weights or borders;
beside each, min_max of the same rows through dsp_reduce.hip -- one streaming pass, the natural floor for two.  Device events around
`steps` launches after two warm-up launches; the forms alternate over `repeats` rounds, every round's figure is kept.
The kernel's two choices against their alternatives: name libraries built with -DDSP_HIST_KEEP (rows of at most 1024 float32 samples stay
in registers between the passes instead of being read twice) and -DDSP_HIST_NO_COMBINE (every lane adds for itself) as the sixth argument
(python -m dspeed_amd.build --variant keep --define DSP_HIST_KEEP; ... --variant nocombine --define DSP_HIST_NO_COMBINE).  Every library
(the product's first, then the ones named, comma-separated) is measured in a process of its own and the figures stand side by side.
python tools/histogram_rate.py [rows] [samples] [steps] [repeats] [json file] [further libraries]"""
import json
import os
import subprocess
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
out_file = sys.argv[5] if len(sys.argv) > 5 and sys.argv[5] != "-" else None
M = 100
CHILD = "--measure" in sys.argv

if not CHILD:  # a fresh process per library: a library is loaded once per process
    libs = [None] + [os.path.abspath(x) for x in (sys.argv[6].split(",") if len(sys.argv) > 6 else []) if x]
    results, device = [], None
    for lib in libs:
        env = dict(os.environ)
        env.pop("DSPEED_HIP_LIB", None)
        if lib:
            env["DSPEED_HIP_LIB"] = lib
        done = subprocess.run([sys.executable, os.path.abspath(__file__), str(rows), str(n), str(steps), str(repeats), "-", "--measure"], env=env,
                              stdout=subprocess.PIPE, text=True, check=True)
        for line in done.stdout.splitlines():
            rec = json.loads(line)
            if "device" in rec and "form" not in rec:
                device = rec["device"]
                continue
            results.append(rec)
            print(json.dumps(rec))
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as f:
            json.dump({"tool": "tools/histogram_rate.py", "device": device, "results": results}, f, indent=1)
    sys.exit(0)

from dspeed_amd.device import device_info  # noqa: E402

print(json.dumps({"device": device_info(0).get("name")}))


def hist_program(wf, stats, stores):
    p = Program()
    p.slots = [n, M, M + 1]
    p.n_sregs = 3 if stats else 0
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io(wf, _lib.IO_WF_IN, np.float32, n, 0, n))
    p.add_op(_lib.OP_HISTOGRAM, dst=1, src=0, ip=(2,))
    if stats:
        p.add_op(_lib.OP_HISTOGRAM_STATS, src=1, ip=(2, 0), sp=(Scalar.const(np.nan),))
    if stores:
        p.add_op(_lib.OP_STORE, src=1, io=p.add_io("weights", _lib.IO_WF_OUT, np.float32, M))
        p.add_op(_lib.OP_STORE, src=2, io=p.add_io("borders", _lib.IO_WF_OUT, np.float32, M + 1))
    if stats:
        for k in range(3):
            p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(f"o{k}", _lib.IO_SCALAR_OUT, np.float32), ip=(k,))
    return p


def min_max_program(wf):
    p = Program()
    p.slots = [n]
    p.n_sregs = 4
    p.add_op(_lib.OP_LOAD, dst=0, io=p.add_io(wf, _lib.IO_WF_IN, np.float32, n, 0, n))
    p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
    for r in range(4):
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(f"o{r}", _lib.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p


st = Stream()
# (a) pure noise, no pulse: a bell over the bins, the fullest holding a few per cent of the row;  (b) a pulse on a quiet baseline, as a
#     SiPM or Ge trace has it: the range is the pulse's, the samples ahead of it -- half the row -- fall into one or two bins
bl, tp = DeviceArray((rows,), np.float32), DeviceArray((rows,), np.float32)
spread, noise = DeviceArray((rows, n), np.float32), DeviceArray((rows, n), np.float32)
for wf, sigma, amp in ((spread, 50.0, (0.0, 0.0)), (noise, 5.0, (5000.0, 15000.0))):
    _lib.check(_lib.lib().dsp_synth_waveforms(wf.ptr, _lib.F32, rows, n, n, bl.ptr, tp.ptr, 0xD5BEED, 0, 1716.28, sigma, 625 + 0.8 * 188,
                                              -30.0, 30.0, amp[0], amp[1], st.ptr), what="synth")
sync()
bufs = {"spread": spread, "noise": noise, "weights": DeviceArray((rows, M), np.float32), "borders": DeviceArray((rows, M + 1), np.float32)}
bufs.update({f"o{r}": DeviceArray((rows,), np.float32) for r in range(4)})
forms = []
for wf in ("spread", "noise"):
    forms += [(f"min_max of the {wf} rows (dsp_reduce.hip)", min_max_program(wf)), (f"histogram, {wf} rows", hist_program(wf, False, True)),
              (f"histogram + histogram_stats in one launch, weights and borders stored, {wf} rows", hist_program(wf, True, True)),
              (f"histogram + histogram_stats in one launch, three values per row stored, {wf} rows", hist_program(wf, True, False))]
chains = [(name, Chain(prog, name, np.float32)) for name, prog in forms]
for name, ch in chains:
    for _ in range(2):
        ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
    sync()
    ch.check(st)
times = {name: [] for name, _ in chains}
for _ in range(repeats):
    for name, ch in chains:
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(steps):
            ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
        e1.record(st)
        sync()
        ch.check(st)
        times[name].append(e0.elapsed_ms(e1) * 1e-3 / steps)
results = []
filled = {}
for wf in ("spread", "noise"):  # how concentrated: the share of a row's samples in its fullest bin
    name = f"histogram, {wf} rows"
    ch = dict(chains)[name]
    ch.execute({k: bufs[k] for k in ch.io_names}, rows, st)
    sync()
    w = bufs["weights"].to_numpy()[:1024]
    filled[wf] = float((w.max(axis=1) / np.maximum(w.sum(axis=1), 1)).mean())
for name, ch in chains:
    best = min(times[name])
    byts = rows * n * 4
    rec = {"form": name, "kernel": ch.kernel_name, "rows": rows, "samples": n, "bins": M, "library": os.path.basename(os.environ.get("DSPEED_HIP_LIB", "")) or "product",
           "ms_each_round": [round(t * 1e3, 4) for t in times[name]], "ms_best": round(best * 1e3, 4), "waveforms_per_s": round(rows / best),
           "row_GBps_one_pass": round(byts / best / 1e9, 1)}
    for wf in filled:
        if name.endswith(f"{wf} rows") and "histogram" in name:
            rec["mean_share_of_fullest_bin"] = round(filled[wf], 3)
    results.append(rec)
    print(json.dumps(rec))

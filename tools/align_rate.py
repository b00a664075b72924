#!/usr/bin/env python3
"""Rate of the waveform aligner (dsp_align.hip) on device-resident rows of 1024 and 8192 samples (a step pulse on a baseline with noise):
  * ``dsp_inl_correction_rows`` alone (uint16 rows read, a 65536-entry float32 table gathered, float32 rows written),
  * ``dsp_wf_centroid_rows`` alone, on the float32 rows filtered with the step kernel,
  * ``dsp_wf_alignment_rows`` alone on float32 rows (the whole row read for its NaN rule) and on uint16 rows (the window alone), size = n / 8,
  * ``dsp_wf_correction_rows`` alone on the aligned rows,
  * alignment and correction apart -- two launches with the aligned rows in memory between them -- and in one launch,
  * a device copy of the float32 rows (``x2.copy_(x)``: every row read, every row written -- the yardstick).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of
`seconds` each, every round's figure is kept, and the spread of the rounds stands beside the best.
python tools/align_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import align_cases as ac  # noqa: E402
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain  # noqa: E402
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.gufunc import run  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r23_align_rate.json")
lengths = [int(v) for v in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1024, 8192]
SHIFT = 8.0

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("align_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
L = _lib.lib()
F32 = _lib.F32
results = []
for n in lengths:
    size = n // 8
    gen = torch.Generator(device="cuda").manual_seed(0xA119 + n)
    t0 = torch.randint(n // 4, 3 * n // 4, (rows, 1), device="cuda", generator=gen)
    raw = (1000 + 2000 * (torch.arange(n, device="cuda")[None, :] >= t0) + torch.randint(0, 8, (rows, n), device="cuda", generator=gen)).to(torch.int16)  # (below 2**15: the bits of the uint16 rows they are read as)
    table = torch.from_numpy(ac.inl_table("f32", 65536)).cuda()
    tpl = torch.from_numpy(ac.template("f32", size)).cuda()
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda")  # inl-corrected rows
    x2 = torch.empty_like(x)
    centroid = torch.empty(rows, dtype=torch.float32, device="cuda")
    aligned = [torch.empty((rows, size), dtype=torch.float32, device="cuda") for _ in range(2)]
    corrected = [torch.empty((rows, size), dtype=torch.float32, device="cuda") for _ in range(2)]
    raw_args = (raw.data_ptr(), _lib.U16, rows, n, n, F32)
    x_args = (x.data_ptr(), F32, rows, n, n, F32)
    run(L.dsp_inl_correction_rows, "inl_correction", *raw_args, table.data_ptr(), 65536, x.data_ptr(), n)
    # the filtered rows the centroid is read off: the step kernel's convolution, made once with torch (not measured)
    kern = torch.from_numpy(ac.emulate_step(16)).cuda()
    step = torch.nn.functional.conv1d(x[:, None, :], kern.flip(0)[None, None, :], padding=8)[:, 0, :n].contiguous()
    step_args = (step.data_ptr(), F32, rows, n, n, F32)
    run(L.dsp_wf_centroid_rows, "get_wf_centroid", *step_args, SHIFT, centroid.data_ptr())
    assert bool(torch.isfinite(centroid).all()), "a row without a centroid"
    d = lambda t, shape: DeviceArray.from_ptr(t.data_ptr(), shape, np.float32)  # noqa: E731
    fused_chain = Chain(ac.program(n, "fused", rows=np.float32, size=size, centroid="column", shift=SHIFT, start=0, stop=size, table_len=size, store_aligned=False),
                        "align_rate fused", np.float32)
    assert fused_chain.kernel_name == ac.KERNEL
    fused_bufs = {"w": d(x, (rows, n)), "c": d(centroid, (rows,)), "w_corr": d(tpl, (size,)), "out": d(corrected[1], (rows, size))}
    torch.cuda.synchronize()

    def inl_alone():
        run(L.dsp_inl_correction_rows, "inl_correction", *raw_args, table.data_ptr(), 65536, x2.data_ptr(), n)  # (ends in the chain's check: the device is idle when it returns)

    def centroid_alone():
        run(L.dsp_wf_centroid_rows, "get_wf_centroid", *step_args, SHIFT, centroid.data_ptr())

    def align_f32():
        run(L.dsp_wf_alignment_rows, "wf_alignment", *x_args, centroid.data_ptr(), 0.0, SHIFT, float(size), aligned[0].data_ptr(), size, size)

    def align_u16():
        run(L.dsp_wf_alignment_rows, "wf_alignment", *raw_args, centroid.data_ptr(), 0.0, SHIFT, float(size), aligned[1].data_ptr(), size, size)

    def correct_alone():
        run(L.dsp_wf_correction_rows, "wf_correction", aligned[0].data_ptr(), F32, rows, size, size, F32, tpl.data_ptr(), size, 0, size, corrected[0].data_ptr(), size)

    def apart():
        align_f32()
        correct_alone()

    def fused():
        fused_chain.execute(fused_bufs, rows)
        fused_chain.check()

    def copy():
        x2.copy_(x)
        torch.cuda.synchronize()

    forms = [("inl_correction, uint16 rows, 65536 entries", inl_alone), ("get_wf_centroid of the step-filtered rows", centroid_alone),
             ("wf_alignment of float32 rows, size n/8", align_f32), ("wf_alignment of uint16 rows, size n/8", align_u16), ("wf_correction of the aligned rows", correct_alone),
             ("wf_alignment, wf_correction: two launches", apart), ("wf_alignment + wf_correction in one launch", fused), ("device copy of the float32 rows (x2.copy_(x))", copy)]
    steps = {}
    for form, fn in forms:
        fn(), fn()
        sync()
        t_start = time.perf_counter()
        for _ in range(3):
            fn()
        steps[form] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t_start) / 3, 1e-6))))
    # what is measured: the same rows, the same results
    assert torch.equal(corrected[0], corrected[1]), "the fused launch and the calls apart disagree"
    assert bool(torch.isfinite(corrected[0]).all()) and torch.equal(x, x2)
    times = {form: [] for form, _ in forms}
    for _ in range(repeats):
        for form, fn in forms:
            sync()
            t_start = time.perf_counter()
            for _ in range(steps[form]):
                fn()
            times[form].append((time.perf_counter() - t_start) / steps[form])
    t_copy, t_apart, t_f32 = min(times[forms[7][0]]), min(times[forms[5][0]]), min(times[forms[2][0]])
    for form, _ in forms:
        best, t = min(times[form]), times[form]
        results.append({"form": form, "rows": rows, "samples": n, "size": size, "calls_per_window": steps[form], "ms_each_round": [round(v * 1e3, 4) for v in t],
                        "ms_best": round(best * 1e3, 4), "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                        "ratio_to_the_copy": round(best / t_copy, 3), "ratio_to_the_two_calls_apart": round(best / t_apart, 3),
                        "ratio_to_the_float32_alignment": round(best / t_f32, 3)})
    fused_chain.close()
    del raw, x, x2, step, aligned, corrected
    torch.cuda.empty_cache()

for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/align_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

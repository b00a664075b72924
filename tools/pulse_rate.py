#!/usr/bin/env python3
"""Rate of the pulse picker (dsp_pulses.hip) on device-resident float32 rows of 1024 and 8192 samples (a pulse train on noise), lists of
20 candidates at the pulses' places, width 10 and ratio 0.8 -- the SiPM config's values:
  * ``processors.peak_snr_threshold`` alone (m windows of 2 width samples a row read, the packed list and the count written),
  * ``processors.multi_a_filter`` alone, on the packed lists (the row streamed for "a NaN", m samples picked),
  * the two calls apart (the packed list through memory),
  * LOAD, LOAD, PEAK_SNR_THRESHOLD, MULTI_A_FILTER in one launch (the packed list stays in registers), and
  * a device copy of the rows (``y.copy_(x)``: the yardstick of the streaming pass -- it writes what it reads, the pick-off only reads).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of
`seconds` each, every round's figure is kept, and the spread of the rounds stands beside the best.
python tools/pulse_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pulse_cases as pc  # noqa: E402
from dspeed_amd.chain import Chain  # noqa: E402
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import multi_a_filter, peak_snr_threshold  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r21_pulse_rate.json")
lengths = [int(v) for v in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1024, 8192]
M, WIDTH, RATIO = 20, 10, 0.8

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("pulse_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
results = []
for n in lengths:
    gen = torch.Generator(device="cuda").manual_seed(0x5199 + n)
    x = 20 + torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
    # 20 candidates a row, n / 21 apart and a few samples off per row; a pulse with an undershoot at every other one
    places = (torch.arange(1, M + 1, device="cuda")[None, :] * (n // (M + 1)) + torch.randint(-3, 4, (rows, M), device="cuda", generator=gen)).to(torch.int64)
    r = torch.arange(rows, device="cuda")[:, None]
    x[r, places[:, ::2]] += 200.0
    x[r, places[:, ::2] + 4] -= 60.0
    cands = places.to(torch.float32)
    cands[:, M - 2:] = float("nan")  # (the peak finder pads its lists)
    y = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    lists = [torch.empty((rows, M), dtype=torch.float32, device="cuda") for _ in range(4)]
    counts = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_in, d_c = DeviceArray.from_ptr(x.data_ptr(), (rows, n), np.float32), DeviceArray.from_ptr(cands.data_ptr(), (rows, M), np.float32)
    d_l = [DeviceArray.from_ptr(t.data_ptr(), (rows, M), np.float32) for t in lists]
    d_n = [DeviceArray.from_ptr(t.data_ptr(), (rows,), np.uint32) for t in counts]
    fused_chain = Chain(pc.program(n, M, np.float32, np.float32, amp=True, store_list=False, ratio=RATIO, width=float(WIDTH)), "pulse_rate fused", np.float32)
    assert fused_chain.kernel_name == pc.KERNEL
    fused_bufs = {"w": d_in, "list": d_c, "va_max": d_l[2], "count": d_n[1]}
    torch.cuda.synchronize()

    def picker_alone():
        peak_snr_threshold(d_in, d_c, RATIO, WIDTH, d_l[0], d_n[0])  # (ends in the chain's check: the device is idle when it returns)

    def pickoff_alone():
        multi_a_filter(d_in, d_l[0], d_l[1])

    def apart():
        picker_alone()
        pickoff_alone()

    def fused():
        fused_chain.execute(fused_bufs, rows)
        fused_chain.check()

    def copy():
        y.copy_(x)
        torch.cuda.synchronize()

    forms = [("peak_snr_threshold (dsp_pulses.hip)", picker_alone), ("multi_a_filter of the packed lists", pickoff_alone),
             ("peak_snr_threshold, then multi_a_filter: two launches", apart), ("peak_snr_threshold + multi_a_filter in one launch", fused),
             ("device copy of the rows (y.copy_(x))", copy)]
    steps = {}
    for form, fn in forms:
        fn(), fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        steps[form] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    # what is measured: the same rows, the same results
    assert torch.equal(counts[0], counts[1]) and torch.equal(lists[1].nan_to_num(-1), lists[2].nan_to_num(-1)), "the fused launch and the two calls apart disagree"
    kept = float(counts[0].to(torch.float32).mean())
    times = {form: [] for form, _ in forms}
    for _ in range(repeats):
        for form, fn in forms:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[form]):
                fn()
            times[form].append((time.perf_counter() - t0) / steps[form])
    t_copy, t_apart = min(times[forms[4][0]]), min(times[forms[2][0]])
    for form, _ in forms:
        best, t = min(times[form]), times[form]
        results.append({"form": form, "rows": rows, "row_type": "float32", "samples": n, "list_entries": M, "width": WIDTH, "ratio": RATIO,
                        "kept_per_row": round(kept, 2), "calls_per_window": steps[form], "ms_each_round": [round(v * 1e3, 4) for v in t],
                        "ms_best": round(best * 1e3, 4), "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                        "ratio_to_the_copy": round(best / t_copy, 3), "ratio_to_the_two_calls_apart": round(best / t_apart, 3)})
    fused_chain.close()
    del x, y, lists, counts, cands
    torch.cuda.empty_cache()

for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/pulse_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

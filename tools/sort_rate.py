#!/usr/bin/env python3
"""Rate of the sorting kernel (dsp_sort.hip): ``processors.sort`` on device-resident float32 rows of 1024 samples (a wavefront per row) and
8192 (a workgroup per row), beside ``torch.sort(x, dim=1)`` on the same tensor -- the library's segmented sort, the yardstick from outside
this code (it also returns the indices, which nobody asked it for here: the figure is what a user of it pays).  A host clock around calls
that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of `seconds` each, every
round's figure is kept.
python tools/sort_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import sort  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r15_sort_rate.json")
lengths = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1024, 8192]

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("sort_rate.py measures on the device: no GPU here, no figure")


def lds_passes(n, tile=512):
    """dsp_sort::lds_passes of dsp_kernels.h, for the record: passes over a row's keys in LDS behind the staging"""
    p = 8
    while p < n:
        p *= 2
    passes, k = 1, 2 * tile
    while k <= p:
        passes += (k // tile).bit_length()  # log2(k / tile) LDS steps and a tile pass
        k *= 2
    return passes


device = device_info(0).get("name")
results = []
for n in lengths:
    gen = torch.Generator(device="cuda").manual_seed(0xD5BEED + n)
    x = torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
    y = torch.empty_like(x)
    d_in, d_out = DeviceArray.from_ptr(x.data_ptr(), (rows, n), np.float32), DeviceArray.from_ptr(y.data_ptr(), (rows, n), np.float32)
    torch.cuda.synchronize()

    def ours():
        sort(d_in, d_out)  # (ends in the chain's check: the device is idle when it returns)

    def library():
        torch.sort(x, dim=1)
        torch.cuda.synchronize()

    forms = [("processors.sort (dsp_sort.hip)", ours), ("torch.sort(x, dim=1)", library)]
    steps = {}
    for name, fn in forms:
        fn(), fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        steps[name] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    # what is measured: the same rows, the same result
    want, _ = torch.sort(x[:64], dim=1)
    assert torch.equal(y[:64], want), "processors.sort and torch.sort disagree"
    times = {name: [] for name, _ in forms}
    for _ in range(repeats):
        for name, fn in forms:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[name]):
                fn()
            times[name].append((time.perf_counter() - t0) / steps[name])
    for name, _ in forms:
        best, t = min(times[name]), times[name]
        results.append({"form": name, "rows": rows, "samples": n, "calls_per_window": steps[name], "ms_each_round": [round(v * 1e3, 4) for v in t],
                        "ms_best": round(best * 1e3, 4), "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                        "keys_GBps_in": round(rows * n * 4 / best / 1e9, 1), "lds_passes_per_row_from_the_schedule": lds_passes(n) if "dsp_sort" in name else None,
                        "ratio_to_torch_sort": round(best / min(times["torch.sort(x, dim=1)"]), 3)})
    del x, y
    torch.cuda.empty_cache()
for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/sort_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

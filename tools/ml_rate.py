#!/usr/bin/env python3
"""Rate of the dense-layer kernel (dsp_dense.hip): ``processors.dense_layer_with_bias`` / ``classification_layer_with_bias`` with 'r' on
device-resident float32 rows -- n = 1024 -> m = 1 (the classification layer), 16, 64, 256, and n = 256 -> 64 -- beside, on the same tensors:
  * a device copy of the input bytes (``x2.copy_(x)``): a pass that reads the rows once and writes as much;
  * ``torch.nn.functional.linear`` (+ relu) on the same rows and weights.
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats`
rounds of `seconds` each, every round's figure is kept.  What is measured is checked first, against torch's product.
python tools/ml_rate.py [rows] [seconds] [repeats] [json file]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import classification_layer_with_bias, dense_layer_with_bias  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r18_ml_rate.json")
SHAPES = [(1024, 1), (1024, 16), (1024, 64), (1024, 256), (256, 64)]

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("ml_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
results = []
for n, m in SHAPES:
    gen = torch.Generator(device="cuda").manual_seed(0xD5BEED + n + m)
    x = torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
    x2 = torch.empty_like(x)
    w = torch.randn((n, m), dtype=torch.float32, device="cuda", generator=gen) / n ** 0.5
    wt = w.t().contiguous()  # (torch's linear takes (m, n))
    b = torch.randn(m, dtype=torch.float32, device="cuda", generator=gen)
    y = torch.empty((rows, m) if m > 1 else (rows,), dtype=torch.float32, device="cuda")
    d_in = DeviceArray.from_ptr(x.data_ptr(), (rows, n), np.float32)
    d_w = DeviceArray.from_ptr(w.data_ptr(), (n, m) if m > 1 else (n,), np.float32)
    d_b = DeviceArray.from_ptr(b.data_ptr(), (m,), np.float32)
    d_out = DeviceArray.from_ptr(y.data_ptr(), tuple(y.shape), np.float32)
    torch.cuda.synchronize()

    def ours():
        if m > 1:
            dense_layer_with_bias(d_in, d_w, d_b, "r", d_out)  # (ends in the chain's check: the device is idle when it returns)
        else:
            classification_layer_with_bias(d_in, d_w, d_b, "r", d_out)

    def copy():
        x2.copy_(x)
        torch.cuda.synchronize()

    def library():
        torch.relu(torch.nn.functional.linear(x, wt, b))
        torch.cuda.synchronize()

    ours()
    ref = torch.relu(torch.nn.functional.linear(x[:256].double(), wt.double(), b.double()))
    err = (y[:256].reshape(256, m).double() - ref).abs().max().item()
    assert err < 1e-3, f"the layer is not the product: {err}"
    forms = [("dense_layer_with_bias 'r' (dsp_dense.hip)" if m > 1 else "classification_layer_with_bias 'r' (dsp_dense.hip)", ours),
             ("x2.copy_(x) of the input bytes", copy), ("torch.relu(torch.nn.functional.linear)", library)]
    steps = {}
    for name, fn in forms:
        fn(), fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        steps[name] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    times = {name: [] for name, _ in forms}
    for _ in range(repeats):
        for name, fn in forms:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[name]):
                fn()
            times[name].append((time.perf_counter() - t0) / steps[name])
    t_copy = min(times["x2.copy_(x) of the input bytes"])
    for name, _ in forms:
        best, t = min(times[name]), times[name]
        results.append({"form": name, "rows": rows, "inputs": n, "outputs": m, "calls_per_window": steps[name],
                        "ms_each_round": [round(v * 1e3, 4) for v in t], "ms_best": round(best * 1e3, 4),
                        "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                        "read_GBps": round(rows * n * 4 / best / 1e9, 1), "TFLOPs": round(2.0 * rows * n * m / best / 1e12, 2),
                        "time_over_copy": round(best / t_copy, 3)})
    del x, x2, y
    torch.cuda.empty_cache()
for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/ml_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

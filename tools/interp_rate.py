#!/usr/bin/env python3
"""Rate of the resampling kernel (dsp_interp.hip): ``processors.interpolating_upsampler`` in each of its seven modes on device-resident
float32 and int16 rows -- 1024 -> 16384 samples, 512 -> 5120, and 1024 -> 3000 (a ratio that is no integer; mode 'i' does not apply) --
beside, on the same tensors:
  * a device fill and a device copy of the output bytes (``y.fill_``, ``y2.copy_(y)``): the store bound, and a pass that also reads them;
  * the existing ``processors.upsampler`` (sample repetition, the integer ratios);
  * ``torch.nn.functional.interpolate(mode="linear")`` for mode 'l' (float32 rows).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats`
rounds of `seconds` each, every round's figure is kept.  What is measured is checked first: 'f' at an integer ratio is np.repeat.
python tools/interp_rate.py [rows] [seconds] [repeats] [json file]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import interpolating_upsampler, upsampler  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r17_interp_rate.json")
SHAPES = [(1024, 16384), (512, 5120), (1024, 3000)]

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("interp_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
results = []
for n, m in SHAPES:
    for rows_type, tdt in (("float32", torch.float32), ("int16", torch.int16)):
        gen = torch.Generator(device="cuda").manual_seed(0xD5BEED + n)
        xf = 1000.0 + 50.0 * torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
        x = xf if tdt is torch.float32 else xf.round().to(torch.int16)
        y, y2 = torch.empty((rows, m), dtype=torch.float32, device="cuda"), torch.empty((rows, m), dtype=torch.float32, device="cuda")
        d_in = DeviceArray.from_ptr(x.data_ptr(), (rows, n), np.float32 if tdt is torch.float32 else np.int16)
        d_out = DeviceArray.from_ptr(y.data_ptr(), (rows, m), np.float32)
        torch.cuda.synchronize()

        def ours(mode):
            return lambda: interpolating_upsampler(d_in, mode, d_out)  # (ends in the chain's check: the device is idle when it returns)

        def fill():
            y.fill_(1.0)
            torch.cuda.synchronize()

        def copy():
            y2.copy_(y)
            torch.cuda.synchronize()

        def repetition():
            upsampler(d_in, float(m // n), d_out)

        def library():
            torch.nn.functional.interpolate(x[:, None, :], size=m, mode="linear")
            torch.cuda.synchronize()

        forms = [(f"interpolating_upsampler '{c}' (dsp_interp.hip)", ours(c)) for c in "infclhs" if not (c == "i" and m % n)]
        forms += [("y.fill_ of the output bytes", fill), ("y2.copy_(y) of the output bytes", copy)]
        if m % n == 0:
            forms.append(("processors.upsampler (sample repetition)", repetition))
        if tdt is torch.float32:
            forms.append(("torch.nn.functional.interpolate(mode='linear')", library))
        if m % n == 0:  # what is measured: 'f' at an integer ratio repeats every sample
            interpolating_upsampler(d_in, "f", d_out)
            assert torch.equal(y[:64], x[:64].to(torch.float32).repeat_interleave(m // n, dim=1)), "mode 'f' is not the repetition"
        steps = {}
        for name, fn in list(forms):
            try:
                fn(), fn()
            except (NotImplementedError, ValueError) as e:  # a form that does not take the shape: recorded, not timed
                results.append({"form": name, "rows": rows, "rows_type": rows_type, "samples_in": n, "samples_out": m, "refused": str(e)})
                forms.remove((name, fn))
                continue
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
        t_fill, t_copy = min(times["y.fill_ of the output bytes"]), min(times["y2.copy_(y) of the output bytes"])
        for name, _ in forms:
            best, t = min(times[name]), times[name]
            results.append({"form": name, "rows": rows, "rows_type": rows_type, "samples_in": n, "samples_out": m, "calls_per_window": steps[name],
                            "ms_each_round": [round(v * 1e3, 4) for v in t], "ms_best": round(best * 1e3, 4),
                            "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                            "stored_GBps": round(rows * m * 4 / best / 1e9, 1), "time_over_fill": round(best / t_fill, 3),
                            "time_over_copy": round(best / t_copy, 3)})
        del x, xf, y, y2
        torch.cuda.empty_cache()
for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/interp_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

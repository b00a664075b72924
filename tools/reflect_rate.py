#!/usr/bin/env python3
"""Rate of the mirrored-edge FIR kernel (dsp_reflect.hip): ``processors.reflected_convolve_wf`` on device-resident float32 and int16 rows of
1024 samples with 9 taps (the SiPM recipes' case: a wavefront per row) and of 8192 samples with 9, 65 and 257 taps (a workgroup per row),
plain and with ``avg_current(5)`` in the same launch, beside
  * a device copy of the same bytes (``y2.copy_(x)``: the rows read, float32 rows written -- the memory bound),
  * the two launches apart (``reflected_convolve_wf`` to memory, then ``avg_current`` from it: what the fusion saves), and
  * ``torch.nn.functional.conv1d`` over ``F.pad(mode="reflect")`` on the same tensors, the yardstick from outside this code (float32
    accumulation there; int16 rows are converted first, which is part of what a user of it pays).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of
`seconds` each, every round's figure is kept.  For information, the distance of the device's float32 loop from the reference's float64 body
on the fixture's pedestal rows, beside the reference's own float32 ``np.convolve`` (tests/golden/reflected_convolve.npz).
python tools/reflect_rate.py [rows] [seconds] [repeats] [json file] [cases n:m, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain, Program, Scalar  # noqa: E402
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import avg_current, gaussian_filter1d, reflected_convolve_wf  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r19_reflect_rate.json")
cases = [tuple(int(v) for v in x.split(":")) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [(1024, 9), (8192, 9), (8192, 65), (8192, 257)]
LAG = 5

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("reflect_rate.py measures on the device: no GPU here, no figure")


def fused_program(n, m, rows_dtype):
    """LOAD, REFLECTED_CONVOLVE, AVG_CURRENT, STORE of the current: the filtered row never goes to memory"""
    p = Program()
    s_in, s_out, s_cur = p.add_slot(n), p.add_slot(n), p.add_slot(n - LAG)
    p.add_op(_lib.OP_LOAD, dst=s_in, io=p.add_io("w", _lib.IO_WF_IN, rows_dtype, n, 0, None))
    p.add_op(_lib.OP_REFLECTED_CONVOLVE, dst=s_out, src=s_in, io=p.add_io("taps:k", _lib.IO_TAPS, np.float32, m, 0, 0))
    p.add_op(_lib.OP_AVG_CURRENT, dst=s_cur, src=s_out, sp=(Scalar.const(float(LAG)),))
    p.add_op(_lib.OP_STORE, src=s_cur, io=p.add_io("curr", _lib.IO_WF_OUT, np.float32, n - LAG, 0, None))
    return p


device = device_info(0).get("name")
results = []
for n, m in cases:
    k = gaussian_filter1d(np.float32((m - 1) // 2 / 4), np.float32(4), np.empty(m, np.float32))
    kd = DeviceArray.from_numpy(k)
    kt = torch.from_numpy(k[::-1].copy()).cuda().reshape(1, 1, m)  # conv1d correlates: the kernel flipped
    for name, tdt, ndt in (("float32", torch.float32, np.float32), ("int16", torch.int16, np.int16)):
        gen = torch.Generator(device="cuda").manual_seed(0xEF1EC7 + n + m)
        x = (2000 + 4 * torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)).round().to(tdt)  # noise on a pedestal of 2000
        y, y2, g, c, c2 = (torch.empty((rows, w), dtype=torch.float32, device="cuda") for w in (n, n, n, n - LAG, n - LAG))
        d_in = DeviceArray.from_ptr(x.data_ptr(), (rows, n), ndt)
        d_y, d_g = (DeviceArray.from_ptr(t.data_ptr(), (rows, n), np.float32) for t in (y, g))
        d_c, d_c2 = (DeviceArray.from_ptr(t.data_ptr(), (rows, n - LAG), np.float32) for t in (c, c2))
        chain = Chain(fused_program(n, m, ndt), "reflect_rate fused", np.float32)
        assert chain.kernel_name == "dsp_reflect_kernel"
        bufs = {"w": d_in, "taps:k": kd, "curr": d_c}
        torch.cuda.synchronize()

        def plain():
            reflected_convolve_wf(d_in, kd, d_y)  # (ends in the chain's check: the device is idle when it returns)

        def fused():
            chain.execute(bufs, rows)
            chain.check()

        def apart():
            reflected_convolve_wf(d_in, kd, d_g)
            avg_current(d_g, LAG, d_c2)

        def copy():
            y2.copy_(x)
            torch.cuda.synchronize()

        def library():
            out = F.conv1d(F.pad(x.to(torch.float32).unsqueeze(1), (m // 2, (m - 1) // 2), mode="reflect"), kt)
            torch.cuda.synchronize()
            return out

        forms = [("reflected_convolve_wf (dsp_reflect.hip)", plain), (f"reflected_convolve_wf + avg_current({LAG}) in one launch", fused),
                 (f"reflected_convolve_wf, then avg_current({LAG}): two launches", apart), ("device copy of the same bytes (y2.copy_(x))", copy),
                 ("torch conv1d over F.pad(mode='reflect')", library)]
        steps = {}
        for form, fn in forms:
            fn(), fn()
            sync()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            steps[form] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
        # what is measured: the same rows, the same results
        want = library()[:64, 0]
        assert torch.allclose(y[:64], want, rtol=1e-5, atol=1e-2), "reflected_convolve_wf and conv1d over a reflect pad disagree"
        assert torch.equal(c, c2), "the fused current and the two launches apart disagree"
        del want
        times = {form: [] for form, _ in forms}
        for _ in range(repeats):
            for form, fn in forms:
                sync()
                t0 = time.perf_counter()
                for _ in range(steps[form]):
                    fn()
                times[form].append((time.perf_counter() - t0) / steps[form])
        t_copy, t_plain = min(times[forms[3][0]]), min(times[forms[0][0]])
        for form, _ in forms:
            best, t = min(times[form]), times[form]
            results.append({"form": form, "rows": rows, "row_type": name, "samples": n, "taps": m, "geometry": "workgroup per row" if n + m - 1 > 2048 else "wavefront per row",
                            "calls_per_window": steps[form], "ms_each_round": [round(v * 1e3, 4) for v in t], "ms_best": round(best * 1e3, 4),
                            "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best),
                            "GBps_rows_in_plus_rows_out": round(rows * n * (np.dtype(ndt).itemsize + 4) / best / 1e9, 1),
                            "float64_multiply_adds_per_s": round(rows * n * m / best) if "dsp_reflect" in form or "one launch" in form else None,
                            "ratio_to_the_copy": round(best / t_copy, 3), "ratio_to_the_plain_launch": round(best / t_plain, 3)})
        chain.close()
        del x, y, y2, g, c, c2
        torch.cuda.empty_cache()
    kd.free()

# for information: the float32 loop's distance from the reference's float64 body on the fixture's pedestal rows, beside the reference's own
# float32 np.convolve (the device equals the emulation bit for bit: tests/test_gpu_reflect.py)
accuracy = []
try:
    import reflect_cases as rc

    book = np.load(os.path.join(ROOT, "tests", "golden", f"{rc.BOOK}.npz"))
    ped = rc.families("f32").index("pedestal")
    for key, n, m, kname, k in rc.fixture_cases("f32"):
        if kname != "gauss" or n < 63:
            continue
        taps = book[f"{key}/kernel"]
        got = reflected_convolve_wf(rc.rows_of("f32", n), taps)[ped].astype(np.float64)
        f64, f32 = book[f"{key}/f64_of_f32"][ped], book[f"{key}/f32"][ped].astype(np.float64)
        peak = np.abs(f64).max()
        accuracy.append({"samples": n, "taps": m, "device_vs_float64_body_over_peak": float(np.abs(got - f64).max() / peak),
                         "reference_float32_vs_float64_body_over_peak": float(np.abs(f32 - f64).max() / peak)})
except Exception as e:  # (information only: the rates above stand without it)
    accuracy.append({"skipped": repr(e)})

for rec in results + accuracy:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/reflect_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results,
               "pedestal_rows_accuracy_information_only": accuracy}, f, indent=1)

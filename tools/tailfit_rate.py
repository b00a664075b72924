#!/usr/bin/env python3
"""Rate of the decay-tail fitter (dsp_tailfit.hip) on device-resident float32 rows of 1024 and 8192 samples (a decaying tail with noise), on
the tail slice of the reference's docstring example, wf_blsub[2100:] of 8192 samples, scaled to each length:
  * ``dsp_log_check_rows`` alone (the slice read, float32 rows written),
  * ``dsp_poly_fit_rows`` alone, on the logged rows (4 coefficients),
  * ``dsp_poly_residual_rows`` alone: poly_diff of the logged rows, poly_exp_rms of the slice,
  * the chain apart: log_check, poly_fit, poly_exp_rms, three launches with the logged rows in memory between them,
  * LOAD, LOG_CHECK, POLY_FIT in one launch and LOAD, LOG_CHECK, POLY_FIT, POLY_EXP_RMS in one launch (the logged row never goes to memory),
  * a device copy of the same bytes (``y2.copy_(x[:, start:])``: the slice read, float32 rows written -- the yardstick).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of
`seconds` each, every round's figure is kept, and the spread of the rounds stands beside the best.
python tools/tailfit_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import tailfit_cases as tc  # noqa: E402
from dspeed_amd import _lib  # noqa: E402
from dspeed_amd.chain import Chain  # noqa: E402
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.gufunc import run  # noqa: E402
from dspeed_amd.processors import poly_fit_inverse  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r22_tailfit_rate.json")
lengths = [int(v) for v in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1024, 8192]
M = 4

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("tailfit_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
L = _lib.lib()
results = []
for total in lengths:
    start = 2100 * total // 8192
    n = total - start
    gen = torch.Generator(device="cuda").manual_seed(0x7A11 + total)
    x = 3000 * torch.exp(-torch.arange(total, dtype=torch.float32, device="cuda") / (4 * total)) + 8 * torch.randn((rows, total), dtype=torch.float32, device="cuda", generator=gen)
    y, y2 = (torch.empty((rows, n), dtype=torch.float32, device="cuda") for _ in range(2))
    pars = [torch.empty((rows, M), dtype=torch.float32, device="cuda") for _ in range(3)]
    outs = [torch.empty(rows, dtype=torch.float32, device="cuda") for _ in range(6)]
    inv = torch.from_numpy(np.ascontiguousarray(poly_fit_inverse(n, M - 1))).cuda()
    d_x = DeviceArray.from_ptr(x.data_ptr(), (rows, total), np.float32)
    d_inv = DeviceArray.from_ptr(inv.data_ptr(), (M * M,), np.float64)
    d_pars = [DeviceArray.from_ptr(t.data_ptr(), (rows, M), np.float32) for t in pars]
    d_outs = [DeviceArray.from_ptr(t.data_ptr(), (rows,), np.float32) for t in outs]
    slice_args = (x.data_ptr() + 4 * start, _lib.F32, rows, n, total, _lib.F32)
    logged_args = (y.data_ptr(), _lib.F32, rows, n, n, _lib.F32)
    kw = dict(offset=start, row_stride=total, log=True, fit=True, m=M, store_log=False)
    fit_chain = Chain(tc.program(n, np.float32, np.float32, **kw), "tailfit_rate log_check + poly_fit", np.float32)
    fused_chain = Chain(tc.program(n, np.float32, np.float32, resid="exp", **kw), "tailfit_rate fused", np.float32)
    assert fit_chain.kernel_name == fused_chain.kernel_name == tc.KERNEL
    fit_bufs = {"w": d_x, "inv": d_inv, "pars_out": d_pars[1]}
    fused_bufs = {"w": d_x, "inv": d_inv, "pars_out": d_pars[2], "mean": d_outs[4], "rms": d_outs[5]}
    torch.cuda.synchronize()

    def log_alone():
        run(L.dsp_log_check_rows, "log_check", *slice_args, y.data_ptr(), n)  # (ends in the chain's check: the device is idle when it returns)

    def fit_alone():
        run(L.dsp_poly_fit_rows, "poly_fit", *logged_args, inv.data_ptr(), M, pars[0].data_ptr(), M)

    def diff_alone():
        run(L.dsp_poly_residual_rows, "poly_diff", *logged_args, 0, pars[0].data_ptr(), M, M, outs[0].data_ptr(), outs[1].data_ptr())

    def exp_alone():
        run(L.dsp_poly_residual_rows, "poly_exp_rms", *slice_args, 1, pars[0].data_ptr(), M, M, outs[2].data_ptr(), outs[3].data_ptr())

    def apart():
        log_alone()
        fit_alone()
        exp_alone()

    def log_fit():
        fit_chain.execute(fit_bufs, rows)
        fit_chain.check()

    def fused():
        fused_chain.execute(fused_bufs, rows)
        fused_chain.check()

    def copy():
        y2.copy_(x[:, start:])
        torch.cuda.synchronize()

    forms = [("log_check (dsp_tailfit.hip)", log_alone), ("poly_fit of the logged rows", fit_alone), ("poly_diff of the logged rows", diff_alone),
             ("poly_exp_rms of the slice", exp_alone), ("log_check, poly_fit, poly_exp_rms: three launches", apart), ("log_check + poly_fit in one launch", log_fit),
             ("log_check + poly_fit + poly_exp_rms in one launch", fused), ("device copy of the same bytes (y2.copy_(x[:, start:]))", copy)]
    steps = {}
    for form, fn in forms:
        fn(), fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        steps[form] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    # what is measured: the same rows, the same results
    assert torch.equal(pars[0], pars[1]) and torch.equal(pars[0], pars[2]) and torch.equal(outs[2], outs[4]) and torch.equal(outs[3], outs[5]), "the fused launches and the calls apart disagree"
    assert bool(torch.isfinite(pars[0]).all()) and bool(torch.isfinite(outs[3]).all())
    tail_rms = float(outs[3].mean())
    times = {form: [] for form, _ in forms}
    for _ in range(repeats):
        for form, fn in forms:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[form]):
                fn()
            times[form].append((time.perf_counter() - t0) / steps[form])
    t_copy, t_apart = min(times[forms[7][0]]), min(times[forms[4][0]])
    for form, _ in forms:
        best, t = min(times[form]), times[form]
        results.append({"form": form, "rows": rows, "row_type": "float32", "samples": total, "slice_start": start, "slice_samples": n, "coefficients": M,
                        "mean_tail_rms": round(tail_rms, 3), "calls_per_window": steps[form], "ms_each_round": [round(v * 1e3, 4) for v in t], "ms_best": round(best * 1e3, 4),
                        "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best), "samples_per_s": round(rows * n / best),
                        "ratio_to_the_copy": round(best / t_copy, 3), "ratio_to_the_three_calls_apart": round(best / t_apart, 3)})
    fit_chain.close(), fused_chain.close()
    del x, y, y2, pars, outs
    torch.cuda.empty_cache()

for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/tailfit_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

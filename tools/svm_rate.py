#!/usr/bin/env python3
"""Rate of the support-vector kernel (dsp_svm.hip): ``processors.svm_predict`` on device-resident float32 rows, for
(n, n_sv, classes) = (256, 512, 2), (256, 2048, 8), (1024, 2048, 16), rbf -- beside, on the same tensor:
  * a device copy of the input bytes (``x2.copy_(x)``): a pass that reads the rows once and writes as much;
  * torch doing the same float64 arithmetic: the rows cast up, the expansion |x|^2 + |sv|^2 - 2 x.sv^T by ``matmul``, ``exp``, ``matmul`` with
    D, the intercepts (no vote).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds
of `seconds` each, every round's figure is kept.  What is measured is checked first, against torch's decisions' signs for two classes.
python tools/svm_rate.py [rows] [seconds] [repeats] [json file]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import svm_device_arrays, svm_predict  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r19_svm_rate.json")
SHAPES = [(256, 512, 2), (256, 2048, 8), (1024, 2048, 16)]

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("svm_rate.py measures on the device: no GPU here, no figure")


def model_of(n, n_sv, k, seed):
    rng = np.random.default_rng(seed)
    n_support = np.full(k, n_sv // k, dtype=np.int32)
    n_support[-1] += n_sv - int(n_support.sum())
    return {"kernel": "rbf", "gamma": 1.0 / n, "support_vectors": rng.standard_normal((n_sv, n)), "n_support": n_support,
            "dual_coef": rng.standard_normal((k - 1, n_sv)), "intercept": rng.standard_normal(k * (k - 1) // 2), "classes": np.arange(k, dtype=np.float64)}


device = device_info(0).get("name")
results = []
for n, n_sv, k in SHAPES:
    model = model_of(n, n_sv, k, 0xD5BEED + n + n_sv + k)
    g = svm_predict(model)
    sv_h, norm_h, D_h, icpt_h, _cls = svm_device_arrays(g.model)
    gen = torch.Generator(device="cuda").manual_seed(0xD5BEED + n)
    x = torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
    x2 = torch.empty_like(x)
    sv_t, norm_t, D_t, icpt_t = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sv_h.T, norm_h, D_h, icpt_h))
    y = torch.empty(rows, dtype=torch.float32, device="cuda")
    d_in = DeviceArray.from_ptr(x.data_ptr(), (rows, n), np.float32)
    d_out = DeviceArray.from_ptr(y.data_ptr(), (rows,), np.float32)
    gamma = float(model["gamma"])
    torch.cuda.synchronize()

    def ours():
        g(d_in, d_out)  # (ends in the chain's check: the device is idle when it returns)

    def copy():
        x2.copy_(x)
        torch.cuda.synchronize()

    def decisions(xs):
        xd = xs.double()
        d2 = ((xd * xd).sum(dim=1, keepdim=True) + norm_t[None, :] - 2.0 * torch.matmul(xd, sv_t)).clamp_(min=0.0)
        return torch.matmul(torch.exp(-gamma * d2), D_t) + icpt_t

    def library():
        for at in range(0, rows, 16384):  # (the float64 kernel matrix of all rows at once is rows * n_sv * 8 bytes: in slabs)
            decisions(x[at:at + 16384])
        torch.cuda.synchronize()

    ours()
    ref = decisions(x[:512])
    if k == 2:
        want = torch.where(ref[:, 0] > 0, 0.0, 1.0).float()
        assert torch.equal(y[:512], want), "the labels are not the decisions' signs"
    forms = [("svm_predict (dsp_svm.hip)", ours), ("x2.copy_(x) of the input bytes", copy), ("torch float64: expansion, exp, matmul", library)]
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
            times[name].append((time.perf_counter() - t0) / steps[name] * 1e3)
    flop = 2.0 * rows * n_sv * (n + k * (k - 1) // 2)
    entry = {"n": n, "n_sv": n_sv, "classes": k, "rows": rows, "ms_per_call": {name: [round(t, 4) for t in ts] for name, ts in times.items()},
             "calls_per_round": steps, "float64_tflops_of_ours": round(flop / (min(times["svm_predict (dsp_svm.hip)"]) * 1e-3) / 1e12, 2),
             "rows_per_s_of_ours": round(rows / (min(times["svm_predict (dsp_svm.hip)"]) * 1e-3))}
    print(json.dumps(entry), flush=True)
    results.append(entry)
    for d in g.device_arrays:
        d.free()

record = {"device": device, "rows": rows, "seconds_per_round": seconds, "rounds": repeats, "clock": "host perf_counter around calls that end in a synchronise",
          "results": results}
if out_file:
    os.makedirs(os.path.dirname(out_file), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")

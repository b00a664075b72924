#!/usr/bin/env python3
"""Rate of the pile-up kernel (dsp_pileup.hip) on device-resident int16 rows of 1024 and 8192 samples (a step on noise on a pedestal):
  * ``processors.rc_cr2`` alone (rows read, float32 rows written),
  * ``processors.bi_level_zero_crossing_time_points`` alone, on the filtered rows,
  * the two calls apart (the filter to memory, then the walk from it),
  * LOAD, RC_CR2, BI_LEVEL_ZERO_CROSSING in one launch (the filtered row never goes to memory),
  * the same with a bl_subtract by a per-event baseline folded into the load, and
  * a device copy of the same bytes (``y2.copy_(x)``: the rows read, float32 rows written -- the yardstick).
A host clock around calls that end in a device synchronise, after two warm-up calls of each form; the forms alternate over `repeats` rounds of
`seconds` each, every round's figure is kept, and the spread of the rounds stands beside the best.
python tools/pileup_rate.py [rows] [seconds] [repeats] [json file] [lengths, comma separated]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pileup_cases as pc  # noqa: E402
from dspeed_amd.chain import Chain  # noqa: E402
from dspeed_amd.device import DeviceArray, device_info, sync  # noqa: E402
from dspeed_amd.processors import bi_level_zero_crossing_time_points, rc_cr2  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out_file = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else os.path.join(ROOT, "profiles", "r20_pileup_rate.json")
lengths = [int(v) for v in sys.argv[5].split(",")] if len(sys.argv) > 5 else [1024, 8192]
TAU, POS, NEG, GATE, M = 20.0, 40.0, -40.0, 200.0, 20

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("pileup_rate.py measures on the device: no GPU here, no figure")

device = device_info(0).get("name")
results = []
for n in lengths:
    gen = torch.Generator(device="cuda").manual_seed(0x9113 + n)
    x = 2000 + 8 * torch.randn((rows, n), dtype=torch.float32, device="cuda", generator=gen)
    x[:, n // 3:] += 600
    x = x.round().to(torch.int16)
    ndt = np.int16
    y, y2 = (torch.empty((rows, n), dtype=torch.float32, device="cuda") for _ in range(2))
    lists = [torch.empty((rows, M), dtype=torch.float32, device="cuda") for _ in range(6)]
    counts = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(3)]
    bl = torch.full((rows,), 2000.0, dtype=torch.float32, device="cuda")
    d_in, d_y = DeviceArray.from_ptr(x.data_ptr(), (rows, n), ndt), DeviceArray.from_ptr(y.data_ptr(), (rows, n), np.float32)
    d_l = [DeviceArray.from_ptr(t.data_ptr(), (rows, M), np.float32) for t in lists]
    d_n = [DeviceArray.from_ptr(t.data_ptr(), (rows,), np.uint32) for t in counts]
    d_bl = DeviceArray.from_ptr(bl.data_ptr(), (rows,), np.float32)
    kw = dict(walk=True, m=M, store_row=False, tau=TAU, operands=(POS, NEG, GATE, 0.0))
    fused_chain = Chain(pc.program(n, ndt, np.float32, **kw), "pileup_rate fused", np.float32)
    folded_chain = Chain(pc.program(n, ndt, np.float32, subtract="column", **kw), "pileup_rate fused + bl_subtract", np.float32)
    assert fused_chain.kernel_name == folded_chain.kernel_name == pc.KERNEL
    fused_bufs = {"w": d_in, "polarity": d_l[2], "times": d_l[3], "count": d_n[1]}
    folded_bufs = {"w": d_in, "bl": d_bl, "polarity": d_l[4], "times": d_l[5], "count": d_n[2]}
    torch.cuda.synchronize()

    def filter_alone():
        rc_cr2(d_in, TAU, d_y)  # (ends in the chain's check: the device is idle when it returns)

    def walk_alone():
        bi_level_zero_crossing_time_points(d_y, POS, NEG, GATE, 0, d_n[0], d_l[0], d_l[1])

    def apart():
        filter_alone()
        walk_alone()

    def fused():
        fused_chain.execute(fused_bufs, rows)
        fused_chain.check()

    def folded():
        folded_chain.execute(folded_bufs, rows)
        folded_chain.check()

    def copy():
        y2.copy_(x)
        torch.cuda.synchronize()

    forms = [("rc_cr2 (dsp_pileup.hip)", filter_alone), ("bi_level_zero_crossing_time_points of the filtered rows", walk_alone),
             ("rc_cr2, then the walk: two launches", apart), ("rc_cr2 + the walk in one launch", fused),
             ("bl_subtract + rc_cr2 + the walk in one launch", folded), ("device copy of the same bytes (y2.copy_(x))", copy)]
    steps = {}
    for form, fn in forms:
        fn(), fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        steps[form] = max(3, int(np.ceil(seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    # what is measured: the same rows, the same results
    assert torch.equal(counts[0], counts[1]) and torch.equal(lists[1].nan_to_num(-1), lists[3].nan_to_num(-1)), "the fused launch and the two calls apart disagree"
    found = float(counts[0].to(torch.float32).mean())
    times = {form: [] for form, _ in forms}
    for _ in range(repeats):
        for form, fn in forms:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps[form]):
                fn()
            times[form].append((time.perf_counter() - t0) / steps[form])
    t_copy, t_apart = min(times[forms[5][0]]), min(times[forms[2][0]])
    for form, _ in forms:
        best, t = min(times[form]), times[form]
        results.append({"form": form, "rows": rows, "row_type": np.dtype(ndt).name, "samples": n, "tau": TAU, "list_entries": M, "crossings_per_row": round(found, 2),
                        "calls_per_window": steps[form], "ms_each_round": [round(v * 1e3, 4) for v in t], "ms_best": round(best * 1e3, 4),
                        "spread_max_over_min": round(max(t) / min(t), 4), "rows_per_s": round(rows / best), "samples_per_s": round(rows * n / best),
                        "ratio_to_the_copy": round(best / t_copy, 3), "ratio_to_the_two_calls_apart": round(best / t_apart, 3)})
    fused_chain.close(), folded_chain.close()
    del x, y, y2, lists, counts
    torch.cuda.empty_cache()

for rec in results:
    print(json.dumps(rec))
os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
with open(out_file, "w") as f:
    json.dump({"tool": "tools/pileup_rate.py", "device": device, "timing": "host clock around calls that end in a device synchronise", "results": results}, f, indent=1)

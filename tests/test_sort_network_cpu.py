"""The schedule of dsp_sort.hip and the planner's part of DSP_OP_SORT on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: two
stand-alone programs with a ``main`` of their own, plain g++, no HIP, no LD_PRELOAD.

``tests/sort_network.cpp`` includes ``dsp_kernels.h`` and runs the ``dsp_sort`` namespace -- the key map, the padding, every step's partner,
direction and kind -- for every length from 1 to 300 and every edge length of the case book, over the key map of the families: the result
must equal ``std::sort`` of the keys, in the schedule's order and in the order the kernel's passes run the steps; every step is exactly one
of register, cross-lane or LDS; no partner leaves [0, P).

``tests/sort_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild lengths, slots, offsets and strides: each is
planned -- on dsp_sort_kernel, with an argument block that fits its LDS -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


def test_the_network_sorts_every_length_and_family(tmp_path):
    exe = build(tmp_path, "sort_network", with_planner=False)
    rep = run([exe])
    # 12 padded lengths from 8 to 16384: 6 + 10 + .. + 105 steps; (300 + 16 lengths) x 9 families in float32, those up to 8192 in float64
    assert rep == {"steps": sum(k * (k + 1) // 2 for k in range(3, 15)), "rows": (316 + 314) * 9, "failures": 0}


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("sort_plan_fuzz"), "sort_plan_fuzz")


@pytest.mark.parametrize("seed", [0x50F7, 2])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # both geometries were planned, and refusals by name were reached: the shape's and the limit's
    assert rep["narrow"] > 1000 and rep["wide"] > 1000 and rep["accepted"] == rep["narrow"] + rep["wide"] and rep["refused_by_name"] > 500, rep

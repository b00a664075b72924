"""The index rules of dsp_interp.hip and the planner's part of DSP_OP_INTERP_UPSAMPLE on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: two stand-alone programs with a ``main`` of their own, plain g++, no HIP, no LD_PRELOAD.

``tests/interp_index.cpp`` includes ``dsp_kernels.h`` and runs the ``dsp_interp`` namespace -- for an output, its input segment and whether
it is one of 'i''s zeros or a tail sample -- for every n <= 130, m <= 400 and mode against the reference's loops run forward, restated
there as loops: the float64 bound expressions, one multiply with one rounding, not the rational quotient; and the geometry for every
length up to the limits.

``tests/interp_plan_fuzz.cpp`` feeds ``dsp_plan_build`` programs that hold the op with wild modes, lengths, slots, offsets and strides:
each is planned -- on dsp_interp_kernel, with an argument block that fits its LDS -- or refused with a reason."""
import pytest

from plan_fuzz_util import build, run


def test_the_index_map_is_the_references_loops_run_forward(tmp_path):
    exe = build(tmp_path, "interp_index", with_planner=False)
    rep = run([exe])
    # 130 x 400 pairs; per pair m outputs in each of the six modes that always apply ('h' from n = 2 on) and in 'i' where n divides m
    outputs = sum(m * (5 + (n >= 2) + (m % n == 0)) for n in range(1, 131) for m in range(1, 401))
    assert rep["pairs"] == 130 * 400 and rep["outputs"] == outputs and rep["failures"] == 0
    assert rep["float_bound_pairs"] > 500  # pairs where some ceil(u i), i < n, is not the rational ceil(m i / n)


@pytest.fixture(scope="module")
def fuzzer(tmp_path_factory):
    return build(tmp_path_factory.mktemp("interp_plan_fuzz"), "interp_plan_fuzz")


@pytest.mark.parametrize("seed", [0x17E, 2])
def test_programs_with_the_op_plan_clean_under_asan_and_ubsan(fuzzer, seed):
    rep = run([fuzzer, "20000", str(seed)])
    assert rep["programs"] == 20000
    # both geometries and all seven modes were planned, and refusals by name were reached: the shape's, the mode's and the limits'
    assert rep["narrow"] > 500 and rep["wide"] > 1000 and rep["accepted"] == rep["narrow"] + rep["wide"] and rep["refused_by_name"] > 500, rep
    assert rep["modes"] == 127

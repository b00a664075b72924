"""The stage lists of recipes that chain the row kernels (tests/stage_composition_cases.py), without a device: every case is built with
``build_processing_chain`` and its stage programs handed to the planner.  One launch per processor that owns a kernel, in the order the data
flows: no stage writes what another one wrote, no "-> HBM" program holds a row kernel's op, and every reader stands behind the one stage that
writes what it reads -- in the list and in ``_stage_plan()``, which the side streams follow."""
import re

import numpy as np
import pytest

import stage_composition_cases as sc
from dspeed_amd import _lib
from dspeed_amd.chain import plan
from dspeed_amd.errors import DSPFatal
from dspeed_amd.processing_chain import build_processing_chain

CASES = sc.cases()
ROW_OPS = {_lib.OP_MULTI_EXTREMA, _lib.OP_HISTOGRAM, _lib.OP_HISTOGRAM_STATS, _lib.OP_MULTI_TIME_POINT_THRESH, _lib.OP_TIME_OVER_THRESHOLD, _lib.OP_PSD,
           _lib.OP_FFT, _lib.OP_SORT, _lib.OP_INTERP_UPSAMPLE, _lib.OP_NORMALISE, _lib.OP_DENSE, _lib.OP_REFLECTED_CONVOLVE}


@pytest.fixture(scope="module")
def inputs():
    return sc.table(), sc.constants()


def test_the_book_is_what_it_claims():
    from dspeed_amd.compiler import STAGE_MIN_TAPS

    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    pairs = [c for c in CASES if c.group == "pair"]
    assert len(pairs) == len(sc.PRODUCERS) * len(sc.CONSUMERS) * len(sc.VARIANTS) == 9 * 8 * 3
    assert {c.group for c in CASES} == {"pair", "between", "deep", "fan-out", "long-fir"}
    assert sc.LONG_TAPS >= STAGE_MIN_TAPS and len(sc.constants()["long_kernel"]) == sc.LONG_TAPS
    # refusals are limits of the consumer's shapes, never of a composition: no plain pair on 1000 samples is refused, and nothing deeper
    assert all(c.refusal is None for c in CASES if c.group != "pair")
    refused = {c.name.split("/")[0] for c in pairs if c.refusal}
    assert all(name.split("->")[1] in ("reflect", "extrema", "ml") for name in refused), refused
    w, f, bl = sc.rows()
    assert w.shape == f.shape == (sc.ROWS, sc.N) and w.dtype == np.uint16 and f.dtype == bl.dtype == np.float32 and sc.ROWS % 4 == 1
    bad = ~np.isfinite(f)
    assert bad.sum() == 2 and np.isnan(f[sc.NAN_ROW, sc.NAN_AT]) and f[sc.INF_ROW, sc.INF_AT] == np.inf
    assert np.array_equal(f[~bad], w.astype(np.float32)[~bad]) and (w[sc.CONSTANT_ROW] == w[sc.CONSTANT_ROW, 0]).all()
    x = np.float32([[0.0, -0.0, np.inf, -1.0, -0.0, 2.0], [1.0, np.nan, 0.0, 0.0, 0.0, 0.0]])
    s = sc.total_order_sort(x)
    assert np.array_equal(s[0], [-1.0, -0.0, -0.0, 0.0, 2.0, np.inf]) and np.array_equal(np.signbit(s[0]), [1, 1, 1, 0, 0, 0]) and np.isnan(s[1]).all()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_one_launch_per_processor_in_the_order_the_data_flows(case, inputs):
    tb, db = inputs
    if case.refusal and case.refused_at == "build":
        with pytest.raises(Exception, match=case.refusal):
            build_processing_chain(case.recipe(), tb, db_dict=db)
        return
    chain, _, out = build_processing_chain(case.recipe(), tb, db_dict=db)
    assert set(out) >= set(case.outputs)
    stages = chain._stages
    if case.refusal:  # (a check of the reference's body on the row's length, made where the reference makes it: when the stage first runs)
        with pytest.raises(DSPFatal, match=case.refusal):
            for st in stages:
                plan(st["program"])
        return
    # every stage's program is one the planner takes, and the kernels are the case's: one launch per processor that owns one
    kernels = [plan(st["program"])["kernel"] for st in stages]
    whats = [st["what"] for st in stages]
    assert sorted(k for k in kernels if k in sc.OWN_KERNELS) == sorted(case.kernels), list(zip(whats, kernels))
    for st, kernel in zip(stages, kernels):
        ops = {op[0] for op in st["program"].ops}
        if "-> HBM" in st["what"] or kernel not in sc.OWN_KERNELS:
            assert not ops & ROW_OPS, (st["what"], kernel, sorted(ops))
        else:
            assert ops & (ROW_OPS | {_lib.OP_CONVOLVE}), (st["what"], kernel)
    assert not {op[0] for op in chain._program.ops} & ROW_OPS
    # no two stages write the same key
    written = [key for st in stages for _o, key, _n in st["outs"]]
    assert len(set(written)) == len(written), written
    # what a stage or the program reads of a stage's was written by exactly one earlier stage, and the plan of the streams knows it
    deps = chain._stage_plan()["deps"]
    assert chain._chain is None and chain._lanes == []  # (nothing was created on a device)
    assert all(i < j for j, d in enumerate(deps) for i in d)
    writers = lambda key, before: [i for i in range(before) if key in {k for _o, k, _n in stages[i]["outs"]}]
    for j, st in enumerate(stages):
        for key in st["alias"].values():
            if str(key).startswith("in:"):
                by = writers(key, j)
                assert len(by) == 1 and by[0] in deps[j], (st["what"], key, by, deps[j])
    for key in chain._ext_alias.values():
        if str(key).startswith("in:"):
            assert len(writers(key, len(stages))) == 1, ("program", key)


def test_the_fusions_survive_a_reader_staged_first():
    """a fused pair is the one launch it was, with its rows written only where someone reads them"""
    tb, db = sc.table(), sc.constants()
    by_name = {c.name: c for c in CASES}

    def stores(name, what):
        chain, _, _ = build_processing_chain(by_name[name].recipe(), tb, db_dict=db)
        st = next(st for st in chain._stages if what in st["what"])
        return [key for _o, key, _n in st["outs"]]

    # the current's histogram reads wf_cur: the filtered row itself never reaches memory
    assert stores("current->histogram/direct", "+ avg_current") == ["in:wf_cur"]
    # histogram_stats joins its histogram, whose rows the recipe asks for here
    assert stores("sort->histogram/direct", "+ histogram_stats") == ["in:wf_c_hw", "in:wf_c_hb", "in:c_mode", "in:c_max", "in:c_fwhm"]
    assert stores("histogram+sort(interp)", "+ histogram_stats") == ["in:h_mode", "in:h_max", "in:h_fwhm"]  # ... and here it does not
    # a normalisation only a layer reads is folded into it -- also where the layer is staged ahead of its family's turn, for a reader
    r = sc.Recipe("sort(dense(normalise))", "deep")
    r.out(r.sort(r.dense(r.normalise("waveform", launch=False))))
    chain, _, _ = build_processing_chain(r.recipe(), tb, db_dict=db)
    assert [st["what"] for st in chain._stages] == ["normalisation_layer wf_norm + dense_layer_with_bias wf_y in one launch on rows", "sort wf_sorted on rows"]
    assert [plan(st["program"])["kernel"] for st in chain._stages] == r.kernels == [sc.K_DENSE, sc.K_SORT]


def test_a_per_event_operand_off_a_row_kernel_s_result_waits_for_it():
    """time_over_threshold above half the maximum of the sorted, baseline-subtracted row: the sort is staged once, ahead of the small program
    that writes the maximum to memory"""
    M = sc.M
    procs = {"wf_blsub": {"function": "bl_subtract", "module": M, "args": ["waveform", "bl", "wf_blsub"]},
             "wf_sorted": {"function": "sort", "module": M, "args": ["wf_blsub", "wf_sorted"]},
             "wf_shift": {"function": "bl_subtract", "module": M, "args": ["wf_sorted", "bl", "wf_shift"]},
             "tp_min, tp_max, wf_min, wf_max": {"function": "min_max", "module": M, "args": ["wf_shift", "tp_min", "tp_max", "wf_min", "wf_max"]},
             "n_over": {"function": "time_over_threshold", "module": M, "args": ["waveform", "0.5*wf_max", "n_over"]}}
    chain, _, _ = build_processing_chain({"outputs": ["n_over"], "processors": procs}, sc.table())
    kernels = [plan(st["program"])["kernel"] for st in chain._stages]
    assert kernels.count(sc.K_SORT) == 1 and kernels.count(sc.K_THRESH) == 1 and kernels.index(sc.K_SORT) < kernels.index(sc.K_THRESH)
    written = [key for st in chain._stages for _o, key, _n in st["outs"]]
    assert len(set(written)) == len(written)

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
           _lib.OP_FFT, _lib.OP_SORT, _lib.OP_INTERP_UPSAMPLE, _lib.OP_NORMALISE, _lib.OP_DENSE, _lib.OP_REFLECTED_CONVOLVE,
           _lib.OP_RC_CR2, _lib.OP_BI_LEVEL_ZERO_CROSSING, _lib.OP_PEAK_SNR_THRESHOLD, _lib.OP_MULTI_A_FILTER, _lib.OP_LOG_CHECK, _lib.OP_POLY_FIT,
           _lib.OP_POLY_DIFF, _lib.OP_POLY_EXP_RMS, _lib.OP_INL_CORRECTION, _lib.OP_WF_CENTROID, _lib.OP_WF_ALIGNMENT, _lib.OP_WF_CORRECTION}


@pytest.fixture(scope="module")
def inputs():
    return sc.table(), sc.constants()


def test_the_book_is_what_it_claims():
    from dspeed_amd.compiler import STAGE_MIN_TAPS

    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    pairs = [c for c in CASES if c.group == "pair"]
    assert len(pairs) == len(sc.PRODUCERS) * len(sc.CONSUMERS) * len(sc.VARIANTS) == 17 * 12 * 3
    assert len(sc.OLD_PRODUCERS) == 9 and len(sc.NEW_CONSUMERS) == 4 and len(sc.OWN_KERNELS) == 13
    by_group = {g: sum(c.group == g for c in CASES) for g in {c.group for c in CASES}}
    assert by_group == {"pair": 612, "between": 3, "deep": 23, "fan-out": 8, "long-fir": 6, "fatal": 6}
    assert sc.LONG_TAPS >= STAGE_MIN_TAPS and len(sc.constants()["long_kernel"]) == sc.LONG_TAPS
    # refusals are limits of the consumer's shapes, never of a composition: no plain pair on 1000 samples is refused, and nothing deeper --
    # but inl_correction, which reads the ADC codes of an integer column and nothing else
    assert all(c.refusal is None for c in CASES if c.group != "pair")
    refused = {c.name.split("/")[0] for c in pairs if c.refusal}
    assert all(name.split("->")[1] in ("reflect", "extrema", "ml", "pileup", "pulses", "align") or name.startswith("inl->") for name in refused), refused
    assert all(bool(c.refusal) == (not c.name.endswith("/direct")) for c in pairs if c.name.startswith("inl->"))
    assert not any(c.refusal for c in pairs if c.len_of(c.read) == sc.N and not c.name.startswith("inl->"))
    # a row a model calls fatal is a case of its own: every pair runs to values in at least one variant (all three, in fact: where the
    # infinity of waveform_f would be fatal, the slice variant reads waveform_n).  The one exception is the old book's: a consumer that
    # refuses the producer's result for its shape in all three variants -- a layer of 1000 inputs on anything else (psd->ml was one
    # already), the peak finder on a walk's six times, the aligner on four energies -- never runs on it; a refusal of a producer's source
    # (inl_correction's) does not count
    assert all(c.fatal is None for c in CASES if c.group != "fatal") and all(c.fatal and not c.refusal for c in CASES if c.group == "fatal")
    for name in {c.name.split("/")[0] for c in pairs}:
        variants = [c for c in pairs if c.name.split("/")[0] == name]
        assert len(variants) == 3 and (any(c.refusal is None and c.fatal is None for c in variants)
                                       or all(c.refused_for == "the consumer's shapes" for c in variants)), name
    tb = sc.table()
    assert set(tb) == {"waveform", "waveform_f", "waveform_n", "bl", "cands", "cands_half"}
    n, cands, half = tb["waveform_n"], tb["cands"], tb["cands_half"]
    assert np.isnan(n[sc.NAN_ROW, sc.NAN_AT]) and np.isfinite(np.delete(n, sc.NAN_ROW, axis=0)).all() and np.array_equal(np.isnan(n), np.isnan(tb["waveform_f"]))
    whole = cands[np.isfinite(cands)]
    assert cands.shape == (sc.ROWS, sc.CANDS) and np.array_equal(whole, np.floor(whole)) and np.isnan(cands).sum() == 1
    shortest = min(c.len_of(c.read) for c in pairs if "->pulses/" in c.name and c.refusal is None)  # (the deeper cases' pickers read 1000 samples)
    assert shortest == 5 and ((whole >= 0) & (whole < shortest)).sum() == whole.size - 1 and (whole > sc.N).sum() == 1
    differ = np.argwhere(~((cands == half) | (np.isnan(cands) & np.isnan(half))))
    assert differ.tolist() == [[sc.FRACTION_ROW, 2]] and half[sc.FRACTION_ROW, 2] == 2.5
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
    # the decay-tail group is one launch that writes tm and tr alone, also where a reader of either is staged ahead of the group's turn: a
    # family asked for a group's head stages the launch the head would have joined
    tail = "log_check wf_log + poly_fit wf_pars + poly_exp_rms tm, tr in one launch on rows"

    def stages_of(r):
        chain, _, _ = build_processing_chain(r.recipe(), tb, db_dict=db)
        assert sorted(k for k in (plan(st["program"])["kernel"] for st in chain._stages) if k in sc.OWN_KERNELS) == sorted(r.kernels), r.name
        return {st["what"]: [key for _o, key, _n in st["outs"]] for st in chain._stages}

    def tail_group(r, rows="waveform"):
        return r.residual(rows, r.poly_fit(r.log_check(rows, launch=False), launch=False))

    for reader in ("time_over_threshold", "peak finder", "picker"):
        r = sc.Recipe(f"{reader} of the tail's residual", "deep")
        tm, tr = tail_group(r)
        if reader == "time_over_threshold":
            r.out(r.time_over("waveform", over=sc._value(tm)))
        elif reader == "peak finder":
            r.out(*r.extrema("waveform", a_abs_max=sc._times(3, tr)))
        else:
            r.out(*r.picker("waveform", ratio=sc._times(0.001, tr)))
        got = stages_of(r)
        assert got[tail] == ["in:tm", "in:tr"] and list(got)[0] == tail, (reader, got)
        assert not any("in:wf_log" in keys or "in:wf_pars" in keys for keys in got.values()), (reader, got)
    assert stores("extrema@3*tr+picker@tr(tailfit)", "poly_exp_rms") == ["in:tm", "in:tr"]
    assert stores("extrema@3*tr+picker@tr(tailfit)+rows", "poly_exp_rms") == ["in:wf_log", "in:wf_pars", "in:tm", "in:tr"]  # (the recipe asks for them)
    r = sc.Recipe("sort of the coefficients", "deep")  # something outside the group reads them: written, the logged row still not
    tail_group(r)
    r.out("tr", r.sort("wf_pars"))
    assert stages_of(r)[tail] == ["in:wf_pars", "in:tm", "in:tr"]
    r = sc.Recipe("a fit without its logarithm", "deep")  # the head is the fit: its residual takes it along all the same
    tm, tr = r.residual("waveform", r.poly_fit("waveform", launch=False), exp=False)
    r.out(r.time_over("waveform", over=sc._value(tr)))
    assert stages_of(r)["poly_fit wf_pars + poly_diff tm, tr in one launch on rows"] == ["in:tm", "in:tr"]
    # the pile-up pair is one launch where a histogram -- a family ahead of it in the order -- reads its times, or the filtered row, which
    # is then among the launch's outputs
    pair = "rc_cr2 wf_rc + bi_level_zero_crossing_time_points w_n, wf_w_pol, wf_w_tt in one launch on rows"
    assert stores("walk->histogram/direct", "rc_cr2 wf_rc +") == ["in:wf_w_pol", "in:wf_w_tt", "in:w_n"]  # (the filtered row stays in the launch)
    r = sc.Recipe("histogram of the filtered row", "fan-out")
    flt = r.rc_cr2("waveform", launch=False)
    r.histogram(flt)
    r.out(*r.walk(flt), "wf_hw")
    got = stages_of(r)
    assert got[pair] == ["in:wf_rc", "in:wf_w_pol", "in:wf_w_tt", "in:w_n"] and list(got) == [pair, "histogram wf_hw, wf_hb on rows"], got
    # a walk whose thresholds come from the filtered row cannot take the filter along: the filter first, alone
    got = stages_of(by_name["walk(rc_cr2)@3*fwhm(histogram(rc_cr2))"])
    assert got["rc_cr2 wf_rc on rows"] == ["in:wf_rc"] and list(got)[-1] == "bi_level_zero_crossing_time_points w_n, wf_w_pol, wf_w_tt on rows", got
    # the picker and the aligner kept their partners before: the head's own loop looks for it
    assert stores("energies->histogram/direct", "+ multi_a_filter") == ["in:wf_k_en", "in:k_n"]  # (the list of positions is nobody's)
    assert stores("corrected->thresholds/direct", "+ wf_correction") == ["in:wf_corr"]


def test_the_rows_the_models_call_fatal():
    """every fatal case whose links all have CPU models: the models name the one row the case expects, at the link it expects; and the
    producers listed as carrying the infinity to rc_cr2 are those whose model-made slice holds an infinity, no NaN, ahead of its last sample
    (of the producers with CPU models; that ``normalise`` and ``logged`` carry it, and ``psd``, ``dense`` and ``pars`` do not, is for the device
    to say: their fatal cases and their slice variants on ``waveform_f`` in test_gpu_stage_composition.py)"""
    link_of = {sc.FATAL_FILTER: "rc_cr2", sc.FATAL_CENTROID: "align", sc.FATAL_FRACTION: "pickoff"}
    checked = 0
    for c in CASES:
        if c.group == "fatal" and not c.name.startswith(("normalise", "logged")):  # (those two links' models are the device's: the GPU test holds them)
            assert c.fatal_rows() == [(link_of[c.fatal[0]], c.fatal[1])], c.name
            checked += 1
    assert checked == 4
    by_name = {c.name: c for c in CASES}
    for producer in ("reflect", "current", "histogram", "multi_thresh", "sort", "interp", "aligned", "corrected", "energies"):
        r = sc.Recipe(producer, "pair")
        add, cut = sc.PRODUCERS[producer]
        made = add(r, "waveform_f") + cut
        row = r.take(r._run(), made)[sc.INF_ROW]
        carries = bool(np.isinf(row[:-1]).any() and not np.isnan(row).any() and len(row) > 3)
        assert carries == (producer in sc.INF_TO_FILTER), (producer, row)
        assert by_name[f"{producer}->pileup/slice"].made["waveform_n" if carries else "waveform_f"]


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

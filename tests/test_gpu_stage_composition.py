"""Recipes that chain the row kernels, on the device: every case of tests/stage_composition_cases.py through
``build_processing_chain(...).execute()`` on the book's 13 rows.  Each owning kernel is launched as often as the case says, and every output
equals, bit for bit, the chain of the CPU models applied link by link (``psd`` and the layers: the device gufunc on the model-made rows; a
``psd`` also within the spectrum's bound of NumPy's float64 transform; a long FIR within its suite's bound of the float64 convolution; the
decay-tail fitter's links the device gufuncs too, and within that family's bounds of its long-double sums).  The same bits on a second
``execute``, with the host rows passing in several pieces, and with the stages on side streams and on one.  A case whose models call a row
fatal raises the DSPFatal at ``execute``, naming that row."""
import numpy as np
import pytest

import spectrum_cases as spc
import stage_composition_cases as sc
import tailfit_cases as fc

pytestmark = pytest.mark.gpu

CASES = sc.cases()
RUN = [c for c in CASES if c.refusal is None and c.fatal is None]
BEYOND_PAIRS = [c for c in RUN if c.group != "pair"]
IN_PIECES = BEYOND_PAIRS + [c for c in RUN if c.group == "pair" and c.name.endswith("/slice")]  # (the slice variants hold the non-finite rows)
PIECE_ROWS = 4  # the 13 host rows pass in pieces of 1, 2, 4, 4 and 2 (processing_chain._piece_sizes)


@pytest.fixture(scope="module")
def inputs():
    return sc.table(), sc.constants()


def _same(got, want, tell):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (tell, got.dtype, got.shape, want.dtype, want.shape)
    differ = ~((got == want) | (np.isnan(got) & np.isnan(want))) if got.dtype.kind == "f" else got != want
    assert not differ.any(), (tell, np.argwhere(differ)[:5].tolist(), got[differ][:5], want[differ][:5])
    if got.dtype.kind == "f":
        assert np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)])), (tell, "the sign of a zero")


#: the links whose model-made values were held to their bounds, by their description.  The values of a link are the same memoised arrays
#: in every case that has it (stage_composition_cases._MEMO, under the same description), so they are held once, in whichever case comes
#: first -- also alone under ``-k`` --, and a value out of bounds fails that case, not every case with the link
_BOUNDS_HELD = set()


def _check_bounds(case, env, tell):
    """the links whose expected values the device made, on the model-made source rows, within the bounds their own suites derive"""
    for src, name in case.psd_links:  # within the spectrum's bound of the float64 truth, on the finite rows (spectrum_cases.check_psd)
        if case.made[name] in _BOUNDS_HELD:
            continue
        x = case.take(env, src).astype(np.float64)
        n, P = x.shape[1], env[name].astype(np.float64)
        c = spc.cap(n, np.float32)
        for r in np.flatnonzero(np.isfinite(x).all(axis=1)):
            X64 = np.fft.rfft(x[r])
            P64 = (X64.real ** 2 + X64.imag ** 2) / n
            assert np.abs(P[r] - P64).sum() <= (2 * c + c * c) * P64.sum(), (tell, name, r, np.abs(P[r] - P64).sum() / P64.sum(), c)
        _BOUNDS_HELD.add(case.made[name])
    T = np.float32
    for fn, src, pars, outs, deg in case.tail_links:  # tailfit_cases' bounds, as test_gpu_tailfit.py holds the gufuncs to them
        if case.made[outs[0]] in _BOUNDS_HELD:
            continue
        x = case.take(env, src)
        if fn == "log_check":
            want = fc.emulate_log_check(x, T)
            assert np.array_equal(np.isnan(env[outs[0]]), np.isnan(want)), (tell, outs)
            held = [(env[outs[0]], *fc.log_bound(x, T), want)]
        elif fn == "poly_fit":
            inv = fc.inverse(x.shape[1], deg)
            held = [(env[outs[0]], *fc.fit_bound(x, inv, T), fc.emulate_poly_fit(x, inv, T))]
        else:
            p, exp = case.take(env, pars), fn == "poly_exp_rms"
            want = fc.emulate_residual(x, p, T, exp)
            x_mean, x_rms, b_mean, b_rms = fc.residual_bound(x, p, T, exp)
            held = [(env[outs[0]], x_mean, b_mean, want[0]), (env[outs[1]], x_rms, b_rms, want[1])]
        for name, (got, exact, bound, finite_of) in zip(outs, held):
            ok, ratio = fc.within(got, exact, bound, finite_of)
            assert ok, (tell, fn, name, ratio)
        _BOUNDS_HELD.add(case.made[outs[0]])


def _check(case, out, want, env, tell):
    behind_fir = case.of_device_rows[1] if case.of_device_rows else []
    for name in case.outputs:
        if name in case.fir_links:
            got, w64 = np.asarray(out[name]), want[name]
            assert got.dtype == np.float32 and got.shape == w64.shape, (tell, name)
            err, peak = np.abs(got - w64).max(axis=1), np.abs(w64).max(axis=1)
            # the bar of the filter's own suite on every row; on the rows the book marks as cancelling, that suite's rule for them
            # (test_gpu_fir_mfma.py's pedestal test): within 8 times the error of the reference's own arithmetic, NumPy's float32
            # convolution.  The premise is asserted, not assumed: on such a row the products are so many times the peak they leave that
            # one float32 rounding of a partial sum, 2**-24 of the products, is already beyond the bar
            x32, k32 = case.take(env, case.fir_sources[name]).astype(np.float32), env["db"]["long_kernel"].astype(np.float32)
            bar = sc.FIR_TOL * peak
            for r in case.fir_cancelling.get(name, ()):
                products = np.convolve(np.abs(x32[r]).astype(np.float64), np.abs(k32).astype(np.float64), "valid").max()
                assert 2.0**-24 * products > sc.FIR_TOL * peak[r], (tell, name, r, products / peak[r])
                numpy_err = np.abs(np.convolve(x32[r], k32, "valid") - w64[r]).max()
                print(f"{case.name} {name} row {r}: products / peak {products / peak[r]:.3g}, error / peak {err[r] / peak[r]:.3g}, of NumPy's float32 convolution {numpy_err / peak[r]:.3g}")
                bar[r] = 8 * numpy_err
            print(f"{case.name} {name}: error / filtered peak {np.max(err / peak):.3g}")
            assert (err <= bar).all(), (tell, name, (err / peak).tolist())
        elif name not in behind_fir:
            _same(out[name], want[name], (tell, name))
    if case.of_device_rows:  # what follows a long FIR: the models of the row the device made, bit for bit -- or, where that row is not
        fir, names = case.of_device_rows  # among the outputs, what the chain that has it there gave, itself held to those models
        models = sc.after_long_fir(np.asarray(out[fir])) if fir else [_with_rows(case.same_as)[name] for name in names]
        for name, model in zip(names, models):
            _same(out[name], model, (tell, name, "of the device's FIR"))
    _check_bounds(case, env, tell)
    # a row with a NaN stays a row of NaNs through every link -- but a histogram's: its weights of such a row are zeros, the reference's rule;
    # a walk's and a picker's count of such a row is 0; its centroid and the mean and rms of its residuals are NaN
    if ("waveform_f" in str(case.procs) or "waveform_n" in str(case.procs)) and not case.name.startswith("histogram->"):
        for name in case.outputs:
            got = np.asarray(out[name])
            if name in case.near_candidates and not np.isnan(case.take(env, case.near_candidates[name])[sc.NAN_ROW]).all():
                continue  # (a picker of a row with a lone NaN, far from its candidates: the models' word stands)
            if got.ndim == 2 and got.dtype.kind == "f" and name not in ("wf_hw", "wf_c_hw"):
                assert np.isnan(got[sc.NAN_ROW]).all(), (tell, name)
            if name in case.nan_counts:
                assert got[sc.NAN_ROW] == 0, (tell, name)
            if name in case.nan_values:
                assert np.isnan(got[sc.NAN_ROW]), (tell, name)


_WITH_ROWS = {}  # the checked outputs of a case that others are ``same_as``, by its name


def _with_rows(case):
    """the outputs of ``case`` -- the chain with the intermediate rows among its outputs --, run here and held to its own models first"""
    from dspeed_amd.processing_chain import build_processing_chain

    if case.name not in _WITH_ROWS:
        chain, _, out = build_processing_chain(case.recipe(), sc.table(), db_dict=sc.constants())
        chain.execute()
        _launches(case, chain, case.name)
        _check(case, out, *case.expected(), (case.name, "for the case without the rows"))
        _WITH_ROWS[case.name] = {k: np.array(out[k]) for k in case.outputs}
    return _WITH_ROWS[case.name]


def _launches(case, chain, tell):
    kernels = [k for _what, k in chain.kernels()]
    for own in sc.OWN_KERNELS:
        assert kernels.count(own) == case.kernels.count(own), (tell, own, chain.kernels())


def _poison(out):
    for a in out.values():
        np.asarray(a).fill(7)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_case_bit_for_bit_twice(case, inputs):
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    tb, db = inputs
    if case.refused_at == "build":
        with pytest.raises(Exception, match=case.refusal):
            build_processing_chain(case.recipe(), tb, db_dict=db)
        return
    chain, _, out = build_processing_chain(case.recipe(), tb, db_dict=db)
    if case.refused_at == "execute":
        with pytest.raises(DSPFatal, match=case.refusal):
            chain.execute()
        return
    if case.fatal:  # the models call one row fatal, and the device names it
        text, row = case.fatal
        assert [r for _link, r in case.fatal_rows()] == [row], case.fatal_rows()
        with pytest.raises(DSPFatal, match=text) as e:
            chain.execute()
        assert e.value.wf_range == range(row, row + 1)
        return
    want, env = case.expected()
    for turn in ("first", "second"):
        _poison(out)
        chain.execute()
        _launches(case, chain, turn)
        _check(case, out, want, env, (case.name, turn))


@pytest.mark.parametrize("case", IN_PIECES, ids=[c.name for c in IN_PIECES])
def test_the_host_rows_in_several_pieces(case, inputs):
    from dspeed_amd.processing_chain import _piece_sizes, build_processing_chain

    tb, db = inputs
    chain, _, out = build_processing_chain(case.recipe(), tb, db_dict=db)
    chain._ensure()
    row_bytes = chain._sort_columns().row_bytes()
    chain.pipeline_bytes = PIECE_ROWS * row_bytes
    assert row_bytes > 0 and _piece_sizes(sc.ROWS, row_bytes, chain.pipeline_bytes)[1] == [1, 2, 4, 4, 2]
    _poison(out)
    chain.execute()
    want, env = case.expected()
    _launches(case, chain, "pieces")
    _check(case, out, want, env, (case.name, "in pieces"))


@pytest.mark.parametrize("concurrent", [True, False], ids=["side-streams", "one-stream"])
@pytest.mark.parametrize("case", BEYOND_PAIRS, ids=[c.name for c in BEYOND_PAIRS])
def test_the_stages_on_side_streams_and_on_one(case, concurrent, inputs):
    from dspeed_amd.processing_chain import build_processing_chain

    tb, db = inputs
    chain, _, out = build_processing_chain(case.recipe(), tb, db_dict=db)
    chain.concurrent_stages = concurrent
    want, env = case.expected()
    for turn in ("first", "second"):
        _poison(out)
        chain.execute()
        _check(case, out, want, env, (case.name, concurrent, turn))
    _launches(case, chain, concurrent)


def test_the_non_finite_rows_through_sort_and_behind_it(inputs):
    """one sorted row read by a spectrum and a histogram: the NaN row is NaNs everywhere; the +inf row is a value through sort alone (its
    last sample) and a NaN row behind psd and in the histogram's borders; the clean rows beside them are finite and the models'"""
    from dspeed_amd.processing_chain import build_processing_chain

    tb, db = inputs
    r = sc.Recipe("psd+histogram(sort)", "fan-out")
    s = r.sort("waveform_f")
    r.histogram(s)
    r.out(s, r.psd(s), "wf_hw", "wf_hb")
    chain, _, out = build_processing_chain(r.recipe(), tb, db_dict=db)
    chain.execute()
    _launches(r, chain, r.name)
    want, env = r.expected()
    _check(r, out, want, env, r.name)
    srt, psd, hw, hb = (np.asarray(out[k]) for k in ("wf_sorted", "wf_psd", "wf_hw", "wf_hb"))
    assert np.isnan(srt[sc.NAN_ROW]).all() and np.isnan(psd[sc.NAN_ROW]).all() and np.isnan(hb[sc.NAN_ROW]).all() and not hw[sc.NAN_ROW].any()
    assert not np.isnan(srt[sc.INF_ROW]).any() and srt[sc.INF_ROW, -1] == np.inf and np.isfinite(srt[sc.INF_ROW, :-1]).all()
    assert np.isnan(psd[sc.INF_ROW]).all() and np.isnan(hb[sc.INF_ROW]).all() and not hw[sc.INF_ROW].any()
    clean = [sc.NAN_ROW - 1, sc.NAN_ROW + 1, sc.INF_ROW - 1, sc.INF_ROW + 1]
    for a in (srt, psd, hw, hb):
        assert np.isfinite(a[clean]).all()
    assert np.array_equal(hw[clean].sum(axis=1), (srt[clean] != srt[clean][:, -1:]).sum(axis=1))  # (every sample but the maxima: the reference's rule)


def test_the_non_finite_rows_through_the_filter_and_the_fit(inputs):
    """one filtered row read by a walk (in the filter's launch), a histogram and get_wf_centroid, and the decay-tail fit of the same rows: the
    NaN row is NaN or a count of zero everywhere, the clean rows beside it are the models'; with the +inf row among them the filter's DSPFatal
    names that row, and nothing else is raised"""
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    tb, db = inputs

    def recipe(rows):
        r = sc.Recipe(f"walk+histogram+centroid(rc_cr2)+tailfit({rows})", "fan-out")
        flt = r.rc_cr2(rows, launch=False)
        r.histogram(flt)
        r.out(flt, *r.walk(flt), "wf_hw", "wf_hb", r.centroid(flt))
        return r.out(*r.residual(rows, r.poly_fit(r.log_check(rows, launch=False), launch=False)))

    r = recipe("waveform_n")
    chain, _, out = build_processing_chain(r.recipe(), tb, db_dict=db)
    chain.execute()
    _launches(r, chain, r.name)
    assert [k for _what, k in chain.kernels()].count(sc.K_PILEUP) == 1 and [k for _what, k in chain.kernels()].count(sc.K_TAILFIT) == 1
    want, env = r.expected()
    _check(r, out, want, env, r.name)
    got = {k: np.asarray(out[k]) for k in r.outputs}
    bad = sc.NAN_ROW
    assert np.isnan(got["wf_rc"][bad]).all() and got["w_n"][bad] == 0 and np.isnan(got["wf_w_pol"][bad]).all() and np.isnan(got["wf_w_tt"][bad]).all()
    assert not got["wf_hw"][bad].any() and np.isnan(got["wf_hb"][bad]).all() and np.isnan(got["cen"][bad]) and np.isnan(got["tm"][bad]) and np.isnan(got["tr"][bad])
    clean = [bad - 1, bad + 1]
    for k in r.outputs:  # (``_check`` held every row to the models; the clean rows hold values)
        _same(got[k][clean], want[k][clean], (r.name, k))
        assert np.isfinite(got[k][clean]).all() or k in ("cen", "wf_w_pol", "wf_w_tt"), k  # (a centroid the reference leaves undefined, lists that end)
    assert (got["w_n"][clean] > 0).all() and np.isfinite(got["wf_w_tt"][clean, 0]).all()
    r = recipe("waveform_f")
    chain, _, out = build_processing_chain(r.recipe(), tb, db_dict=db)
    with pytest.raises(DSPFatal, match=sc.FATAL_FILTER) as e:
        chain.execute()
    assert e.value.wf_range == range(sc.INF_ROW, sc.INF_ROW + 1)
    assert [row for _link, row in r.fatal_rows()] == [sc.INF_ROW]

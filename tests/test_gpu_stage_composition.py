"""Recipes that chain the row kernels, on the device: every case of tests/stage_composition_cases.py through
``build_processing_chain(...).execute()`` on the book's 13 rows.  Each owning kernel is launched as often as the case says, and every output
equals, bit for bit, the chain of the CPU models applied link by link (``psd`` and the layers: the device gufunc on the model-made rows; a
``psd`` also within the spectrum's bound of NumPy's float64 transform; a long FIR within its suite's bound of the float64 convolution).  The
same bits on a second ``execute``, with the host rows passing in several pieces, and with the stages on side streams and on one."""
import numpy as np
import pytest

import spectrum_cases as spc
import stage_composition_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()
RUN = [c for c in CASES if c.refusal is None]
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


def _check(case, out, want, env, tell):
    for name in case.outputs:
        if name in case.fir_links:
            got, w64 = np.asarray(out[name]), want[name]
            assert got.dtype == np.float32 and got.shape == w64.shape, (tell, name)
            err, peak = np.abs(got - w64).max(axis=1), np.abs(w64).max(axis=1)
            print(f"{case.name} {name}: error / filtered peak {np.max(err / peak):.3g}")
            assert (err <= sc.FIR_TOL * peak).all(), (tell, name, np.max(err / peak))
        else:
            _same(out[name], want[name], (tell, name))
    for src, name in case.psd_links:  # within the spectrum's bound of the float64 truth, on the finite rows (spectrum_cases.check_psd)
        x = case.take(env, src).astype(np.float64)
        n, P = x.shape[1], env[name].astype(np.float64)
        c = spc.cap(n, np.float32)
        for r in np.flatnonzero(np.isfinite(x).all(axis=1)):
            X64 = np.fft.rfft(x[r])
            P64 = (X64.real ** 2 + X64.imag ** 2) / n
            assert np.abs(P[r] - P64).sum() <= (2 * c + c * c) * P64.sum(), (tell, name, r, np.abs(P[r] - P64).sum() / P64.sum(), c)
    # a row with a NaN stays a row of NaNs through every link -- but a histogram's: its weights of such a row are zeros, the reference's rule
    if "waveform_f" in str(case.procs) and not case.name.startswith("histogram->"):
        for name in case.outputs:
            got = np.asarray(out[name])
            if got.ndim == 2 and got.dtype.kind == "f" and name not in ("wf_hw", "wf_c_hw"):
                assert np.isnan(got[sc.NAN_ROW]).all(), (tell, name)


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

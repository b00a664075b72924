"""The matrix-core FIR kernels at every tile and alignment edge (tests/fir_tile_cases.py): all eight alignments ``e`` of a kept output's
window with resident and with streamed taps, every width of the last column tile, every stage count, slices that are no multiple of 8
samples, 1 .. 577 rows, three row types and three baselines -- and the amax form at every ``p``, stage count and number of kernels.

One test per case and form of the kernels (the float16 matrix instructions, and the float32 ones under DSPEED_HIP_FIR_F32=1).  It runs the
case's recipe -- and, where the slice is the whole row, the processor call, which must agree bit for bit -- on two families of rows and taps:

  exact     integer taps and rows whose every partial sum is an integer below 2^24: the int64 convolution, ``np.array_equal``;
  fraction  taps and rows that fill the ``lo`` planes of the float16 split: the float64 convolution at TOL of the row's filtered peak.

Rows with a NaN or an infinity follow ``oracle.convolve_wf``: NaN positions and the infinities' signs equal, the finite outputs of the
exact family equal.  profiles/r12_fir_tiles.md holds what the module measured on an MI355X."""
import numpy as np
import pytest

import fir_tile_cases as K

pytestmark = pytest.mark.gpu
CASES = K.cases()


@pytest.fixture(autouse=True, params=["f16", "f32"])
def fir_kind(request, monkeypatch):
    """every case on both forms (as in test_gpu_fir_mfma.py): the float16 matrix instructions on two-way split operands, the default, and
    the float32 ones (DSPEED_HIP_FIR_F32=1)"""
    if request.param == "f32":
        monkeypatch.setenv("DSPEED_HIP_FIR_F32", "1")
    else:
        monkeypatch.delenv("DSPEED_HIP_FIR_F32", raising=False)
    return request.param


@pytest.fixture(scope="module")
def P():
    from dspeed_amd import processors

    return processors


def _same(a, b):
    """bit for bit, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def run_recipe(c, family):
    from dspeed_amd.processing_chain import build_processing_chain

    recipe, names = K.recipe(c, family)
    try:
        chain, _, out = build_processing_chain(recipe, dict(K.table(c.id, family)))
        chain._ensure()
        chain._chain.set_fused(1)
        chain.execute()
    except RuntimeError as e:  # (the runtime's own error: nothing more is started on a device that may have faulted)
        pytest.exit(f"{c.id} {family}: {e}", returncode=3)
    return chain._chain.kernel_name, [np.array(out[k]) for k in names]


def hold(c, family, q, got, found, what):
    """the output of kernel ``q`` -- a waveform per row, or its maximum -- against the case's expectation"""
    want, peak, conv = K.expect(c.id, family)[q]
    fin = K.finite_rows(c.id, family)
    if c.form == "amax":
        want = want.max(axis=1)
        conv_max = K.amax_of(conv)
        conv_max[np.isnan(conv).any(axis=1)] = np.nan  # (numpy.amax: a NaN wins)
        conv = conv_max
    if got.shape != want.shape or got.dtype != np.float32:
        found.append(f"{what}: shape / type {got.shape} {got.dtype}, expected {want.shape} float32")
        return
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    if family == "exact":
        dev = np.abs(g - w)
        print(f"FIGURE {what}: finite rows, largest |device - int64| {dev.max() if dev.size else 0.0:.6g}")
        if not np.array_equal(g, w):
            rows = np.flatnonzero(fin)[np.unique(np.nonzero(dev)[0])][:8].tolist()
            cols = np.unique(np.nonzero(dev.reshape(len(dev), -1))[1])[:12].tolist()
            found.append(f"{what}: not equal to the int64 convolution in rows {rows}, columns {cols}, largest difference {dev.max():g}")
    else:
        scale = np.where(peak[fin] > 0, peak[fin], 1.0).reshape((-1,) + (1,) * (g.ndim - 1))
        err = np.abs(g - w) / scale
        print(f"FIGURE {what}: finite rows, largest |device - float64| / peak {err.max() if err.size else 0.0:.3e}")
        if not (err <= K.TOL).all():
            row = int(np.flatnonzero(fin)[np.argmax(err.reshape(len(err), -1).max(axis=1))])
            found.append(f"{what}: {err.max():.3e} of the filtered peak from the float64 convolution in row {row}")
    if not fin.all():
        g, w = got[~fin], conv[~fin]
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            found.append(f"{what}: NaN positions differ from the oracle's in the rows with a NaN / an infinity")
        elif not np.array_equal(np.isinf(g), np.isinf(w)) or not np.array_equal(np.sign(g[np.isinf(g)]), np.sign(w[np.isinf(w)])):
            found.append(f"{what}: infinities differ from the oracle's")
        elif family == "exact" and not np.array_equal(g[np.isfinite(w)], w[np.isfinite(w)]):
            found.append(f"{what}: finite outputs of a row with an infinity differ from the oracle's")


@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_fir_tile_case(case_id, fir_kind, P):
    c = K.by_id(case_id)
    found = []
    for family in ("exact", "fraction"):
        kernel, outs = run_recipe(c, family)
        assert kernel == c.kernel(fir_kind == "f32"), (case_id, family, kernel)
        for q, got in enumerate(outs):
            hold(c, family, q, got, found, f"{case_id} {fir_kind} {family} recipe kernel {q}")
        if K.has_call(c):
            try:
                called = K.call(P, c, family)
            except RuntimeError as e:
                pytest.exit(f"{case_id} {family} processor call: {e}", returncode=3)
            hold(c, family, 0, called, found, f"{case_id} {fir_kind} {family} call")
            if not _same(called, outs[0]):
                found.append(f"{case_id} {fir_kind} {family}: processor call and recipe differ")
    for f in found:
        print("DIFFERS", f)
    assert not found, found[:8]


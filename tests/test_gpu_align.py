"""inl_correction, get_wf_centroid, wf_alignment and wf_correction on the device (dsp_align.hip): the whole book of tests/align_cases.py against its
emulation, bit for bit in both loops, through every door -- the gufuncs with host arrays and with DeviceArrays, the C entries (for the layouts
a gufunc call cannot make: padded strides, a start that breaks the 16-byte alignment, a sentinel behind every output row), a recipe's stages,
and the alignment with the correction in one launch against the two apart.  None of these inputs faults a kernel: the refusals happen on the
host, the error-word cases are ordinary data-dependent DSPFatals."""
import numpy as np
import pytest

import align_cases as ac

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
CODES = {np.dtype(np.float32): "F32", np.dtype(np.int16): "I16", np.dtype(np.uint16): "U16", np.dtype(np.float64): "F64", np.dtype(np.int32): "I32", np.dtype(np.uint32): "U32"}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _diff(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return int(bad.sum()), [i[:6].tolist() for i in np.nonzero(bad)], got[bad][:4], want[bad][:4]


def _count(index):
    return ac.ROW_COUNTS[index % len(ac.ROW_COUNTS)]


# ---------------------------------------------------------------------------------------------------------------- 1. get_wf_centroid
@pytest.mark.parametrize("loop", list(ac.LOOPS))
def test_get_wf_centroid_the_whole_book(loop):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import get_wf_centroid

    T = ac.LOOPS[loop]
    for index, n in enumerate(ac.LENGTHS):
        names, rows = ac.centroid_rows(loop, n)
        for k, shift in enumerate(ac.centroid_shifts(n)):
            R = max(_count(index + k), len(rows)) if k == 0 else _count(index + k)  # (every row of the book once, then the partial workgroups)
            w = ac.tile_rows(rows, R)
            before = w.copy()
            out = np.full(R, SENTINEL, T)
            assert get_wf_centroid(w, shift, out) is out
            want, defined = ac.emulate_centroid(w, shift, T)
            assert same(out, want), (n, shift, R, [names[i % len(names)] for i in np.flatnonzero(~((out == want) | (np.isnan(out) & np.isnan(want))))])
            assert np.isnan(out[~defined]).all() and w.tobytes() == before.tobytes()
        d, o = DeviceArray.from_numpy(rows), DeviceArray.from_numpy(np.full(len(rows), SENTINEL, T))  # on the device: nothing copied
        assert get_wf_centroid(d, 0.0, o) is o
        assert same(o.to_numpy(), ac.emulate_centroid(rows, 0.0, T)[0]), n
        d.free(), o.free()
    row = ac.centroid_rows(loop, 65)[1][ac.centroid_rows(loop, 65)[0].index("measured")]
    assert [float(get_wf_centroid(row, s)) for s in (0, 3, 2.5)] == [19, 22, 22]  # a 1-D call; the issue's measurement
    # int16 rows in the float32 loop
    if loop == "f32":
        names, rows = ac.centroid_rows(loop, 129)
        keep = np.isfinite(rows).all(axis=1) & (rows == np.rint(rows)).all(axis=1)
        assert same(get_wf_centroid(rows[keep].astype(np.int16), 2.5), ac.emulate_centroid(rows[keep], 2.5, T)[0]) and keep.sum() > 10


def test_get_wf_centroid_on_the_longest_row_and_one_past_it():
    from dspeed_amd.processors import get_wf_centroid

    n = 1 << 20  # (two passes over memory: no row is staged, the planner's bound on a waveform variable is the only one)
    with pytest.raises(ValueError, match="get_wf_centroid: slot 0: 1048577 samples; a waveform variable lives in LDS \\(at most 2\\^20 samples are addressable\\)"):
        get_wf_centroid(np.zeros((1, n + 1), np.float32), 1.0)
    w = np.zeros((2, n), np.float32)
    w[0, 700000:800000], w[0, 800010:900000], w[0, 700001], w[0, 899999] = -1, 1, -5, 5
    w[1] = w[0]
    w[1, n - 1] = np.nan
    assert same(get_wf_centroid(w, 1.0), ac.emulate_centroid(w, 1.0, np.float32)[0]) and ac.emulate_centroid(w, 1.0, np.float32)[0][0] == 800006


# ---------------------------------------------------------------------------------------------------------------- 2. wf_alignment
def _batch(rows, params):
    """every row of ``rows`` with every centroid of ``params`` (one shift, one size): (rows, a centroid per row)"""
    cs = np.repeat([p[0] for p in params], len(rows))
    return np.tile(rows, (len(params), 1)), cs


@pytest.mark.parametrize("loop", list(ac.LOOPS))
def test_wf_alignment_the_whole_book(loop):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processors import wf_alignment

    T = ac.LOOPS[loop]
    branches, undefined = set(), 0
    for index, n in enumerate(ac.LENGTHS):
        _, rows = ac.align_rows(loop, n)
        groups = {}
        for c, sh, s in ac.align_params(n):
            groups.setdefault((sh, s), []).append((c, sh, s))
        for k, ((sh, s), params) in enumerate(sorted(groups.items())):
            w, cs = _batch(rows, params)  # a centroid per event: one launch for the group
            out = np.full((len(w), s), SENTINEL, T)
            assert wf_alignment(w, cs.astype(T), sh, s, out) is out
            want, status = ac.emulate_alignment(w, cs, sh, s, T)
            assert same(out, want), (n, sh, s, _diff(out, want))
            assert np.isnan(out[status == ac.NUMPY_ERROR]).all() and not (status == ac.FATAL).any()
            undefined += int((status == ac.NUMPY_ERROR).sum())
            branches |= {(ac.align_window(T(c), T(sh), s, n) or ("undefined",))[0] for c, _sh, _s in params}
            c = params[(index + k) % len(params)][0]  # one centroid for every row: a constant of the launch
            R = _count(index + k)
            w1 = ac.tile_rows(rows, R)
            out = np.full((R, s), SENTINEL, T)
            wf_alignment(w1, c, float(sh), float(s), out)
            assert same(out, ac.emulate_alignment(w1, c, sh, s, T)[0]), (n, c, sh, s, R)
        (sh, s), params = sorted(groups.items())[index % len(groups)]  # on the device: nothing copied
        w, cs = _batch(rows, params)
        d, dc, o = DeviceArray.from_numpy(w), DeviceArray.from_numpy(cs.astype(T)), DeviceArray.from_numpy(np.full((len(w), s), SENTINEL, T))
        assert wf_alignment(d, dc, sh, s, o) is o
        assert same(o.to_numpy(), ac.emulate_alignment(w, cs, sh, s, T)[0]) and d.to_numpy().tobytes() == w.tobytes()
        d.free(), dc.free(), o.free()
    assert branches == {"window", "pad", "head", "undefined"} and undefined > 0


def test_a_nan_centroid_on_a_clean_row_is_fatal_and_names_the_row():
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import wf_alignment

    for T in (np.float32, np.float64):
        _, rows = ac.align_rows("f32" if T is np.float32 else "f64", 129)
        w = ac.tile_rows(rows, 9)  # rows 2, 3, 4, 7, 8 hold a NaN
        cs = np.full(9, 70.0, T)
        cs[[3, 6]] = np.nan  # row 3 holds a NaN: its rule comes first; row 6 is clean
        out = np.zeros((9, 10), T)
        with pytest.raises(DSPFatal, match="(?m)^centroid is nan$") as e:
            wf_alignment(w, cs, 0.0, 10, out)
        assert e.value.wf_range == range(6, 7)
        cs[6] = 70.0  # (the error word is clean again: the same call goes through)
        wf_alignment(w, cs, 0.0, 10, out)
        assert same(out, ac.emulate_alignment(w, cs, 0.0, 10, T)[0]) and np.isnan(out[3]).all()


# ---------------------------------------------------------------------------------------------------------------- 3. wf_correction
@pytest.mark.parametrize("loop", list(ac.LOOPS))
def test_wf_correction_the_whole_book(loop):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import wf_correction

    T = ac.LOOPS[loop]
    for index, n in enumerate(ac.LENGTHS):
        _, rows = ac.correction_rows(loop, n)
        for k, (m, start, stop, nan_at) in enumerate(ac.correction_params(n)):
            R = _count(index + k)
            w, tpl = ac.tile_rows(rows, R), ac.template(loop, m, nan_at)
            out = np.full((R, n), SENTINEL, T)
            assert wf_correction(w, tpl, start, stop, out) is out
            want = ac.emulate_correction(w, tpl, start, stop, T)
            assert same(out, want), (n, m, start, stop, nan_at, R, _diff(out, want))
        m, start, stop, _ = ac.correction_params(n)[0]
        d, dt = DeviceArray.from_numpy(rows), DeviceArray.from_numpy(ac.template(loop, m))
        got = wf_correction(d, dt, start, stop)
        assert same(np.asarray(got.to_numpy() if isinstance(got, DeviceArray) else got), ac.emulate_correction(rows, ac.template(loop, m), start, stop, T)), n
        d.free(), dt.free()
    for n, m, start, stop, text in ac.CORRECTION_REFUSALS:
        with pytest.raises(DSPFatal, match=f"(?m)^{text}$"):
            wf_correction(np.zeros((2, n), T), np.zeros(m, T), start, stop)
    if loop == "f32":  # uint16 rows in the float32 loop
        w = (1000 + np.arange(5 * 129).reshape(5, 129) % 50).astype(np.uint16)
        assert same(wf_correction(w, ac.template(loop, 40), 50, 90), ac.emulate_correction(w, ac.template(loop, 40), 50, 90, T))


# ---------------------------------------------------------------------------------------------------------------- 4. inl_correction
@pytest.mark.parametrize("loop", list(ac.LOOPS))
def test_inl_correction_the_whole_book(loop):
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processors import inl_correction

    T = ac.LOOPS[loop]
    for name, rows, p, nan_at in ac.inl_cases(loop):
        table = ac.inl_table(loop, p, nan_at)
        want, status, text = ac.emulate_inl(rows, table, T)
        if text is None:
            out = np.full(rows.shape, SENTINEL, T)
            assert inl_correction(rows, table, out) is out
            assert same(out, want), (name, _diff(out, want))
            if p <= 65536:
                d, dt = DeviceArray.from_numpy(rows), DeviceArray.from_numpy(table)
                got = inl_correction(d, dt)
                assert same(got.to_numpy() if isinstance(got, DeviceArray) else got, want), name
                d.free(), dt.free()
        else:
            for w in (rows, None):
                d = None if w is not None else DeviceArray.from_numpy(rows)
                with pytest.raises(DSPFatal, match="(?m)^" + text + "$") as e:
                    inl_correction(rows if d is None else d, table)
                bad = np.flatnonzero(status == ac.FATAL)
                assert e.value.wf_range.start in bad and str(p) in str(e.value)
                if d is not None:
                    d.free()
            clean = rows[status != ac.FATAL]  # (the error word is clean again)
            assert same(inl_correction(clean, table), ac.emulate_inl(clean, table, T)[0])
    rows = ac.inl_cases(loop)[7][1]
    once = inl_correction(rows, ac.inl_table(loop, ac.INL_BIG))
    if loop == "f32":
        assert (once != rows.astype(np.float32) + ac.inl_table(loop, ac.INL_BIG)[rows]).any()  # the float64 sum rounded once is not two float32 roundings


# ---------------------------------------------------------------------------------------------------------------- 5. the C entries
def _blocks(w, in_off, in_stride):
    block = np.full(8 + len(w) * in_stride, 77, dtype=w.dtype)
    block[in_off:in_off + len(w) * in_stride].reshape(len(w), in_stride)[:, :w.shape[1]] = w
    return block


def _rows_out(dev, off, R, stride, width):
    """(the rows written, is everything around them untouched)"""
    got = dev.to_numpy()
    body = got[off:off + R * stride].reshape(R, stride)
    return np.ascontiguousarray(body[:, :width]), bool((got[:off] == SENTINEL).all() and (body[:, width:] == SENTINEL).all() and (got[off + R * stride:] == SENTINEL).all())


@pytest.mark.parametrize("rows_type, loop", [(np.float32, "f32"), (np.int16, "f32"), (np.uint16, "f32"), (np.float64, "f64"), (np.int32, "f64"), (np.int32, "f32"), (np.uint16, "f64")])
def test_layouts_through_the_c_entries_with_sentinels(rows_type, loop):
    """rows n or n + 3 apart, from a 16-byte boundary or from an element 1 .. 3 past one, outputs likewise: 16-byte loads and stores where start
    and stride allow, an element per lane otherwise, and nothing but the outputs written"""
    from dspeed_amd import _lib
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.gufunc import run

    L = _lib.lib()
    T = ac.LOOPS[loop]
    esz, isz = np.dtype(T).itemsize, np.dtype(rows_type).itemsize
    loop_code, code = _lib.F32 if T is np.float32 else _lib.F64, getattr(_lib, CODES[np.dtype(rows_type)])
    integer = np.dtype(rows_type).kind in "iu"
    natural = (rows_type, loop) in ((np.float32, "f32"), (np.int16, "f32"), (np.uint16, "f32"), (np.float64, "f64"))  # the rows every processor's loop takes
    aligns = not (rows_type is np.int32 and loop == "f32")  # (int32 rows feed the float32 loop of inl_correction alone)
    vectors = set()
    for index, n in enumerate(ac.LENGTHS + (512,)):
        R = _count(index)
        for padded in (False, True):
            in_off, in_stride = (1 + index % 3, n + 3) if padded else (0, n)
            off, out_stride = ((index // 2) % 4, n + 3) if padded else (0, n)
            vectors.add((in_off * isz % 16 == 0 and in_stride * isz % 16 == 0 and n * isz % 16 == 0, off * esz % 16 == 0 and out_stride * esz % 16 == 0))

            def rows_on_device(w):
                block = _blocks(w, in_off, in_stride)
                d = DeviceArray.from_numpy(block)
                return d, block, (d.ptr + in_off * isz, code, R, n, in_stride, loop_code)

            def output(width, stride):
                return DeviceArray.from_numpy(np.full(4 + R * stride + 8, SENTINEL, T))

            if aligns:
                # wf_alignment: float rows of the loop, int16 / uint16 in either loop, int32 in the float64 loop
                w = ac.tile_rows(ac.align_rows(loop, n, rows_type if integer else None)[1], R)
                d, block, rows_args = rows_on_device(w)
                params = ac.align_params(n)
                for c, sh, s in (params[(7 * index + j * 13) % len(params)] for j in range(4)):
                    s_stride = s + 3 if padded else s
                    cs = (c + np.arange(R) % 3).astype(T)
                    dc, o = DeviceArray.from_numpy(cs), output(s, s_stride)
                    run(L.dsp_wf_alignment_rows, "wf_alignment", *rows_args, dc.ptr, 0.0, float(sh), float(s), o.ptr + off * esz, s, s_stride)
                    got, clean = _rows_out(o, off, R, s_stride, s)
                    want = ac.emulate_alignment(w, cs, sh, s, T)[0]
                    assert same(got, want) and clean, (rows_type, n, c, sh, s, padded, _diff(got, want))
                    dc.free(), o.free()
                assert d.to_numpy().tobytes() == block.tobytes()  # (the rows are read, never written)
                d.free()
            if integer:  # inl_correction: integer rows, either loop
                p = 256
                w = ac.tile_rows((np.arange(3 * n).reshape(3, n) * 7 % p).astype(rows_type), R)
                table = ac.inl_table(loop, p)
                d, block, rows_args = rows_on_device(w)
                dt, o = DeviceArray.from_numpy(table), output(n, out_stride)
                run(L.dsp_inl_correction_rows, "inl_correction", *rows_args, dt.ptr, p, o.ptr + off * esz, out_stride)
                got, clean = _rows_out(o, off, R, out_stride, n)
                assert same(got, ac.emulate_inl(w, table, T)[0]) and clean, (rows_type, n, padded)
                d.free(), dt.free(), o.free()
            if not natural:
                continue
            # get_wf_centroid
            names, rows = ac.centroid_rows(loop, n)
            if integer:
                rows = rows[np.isfinite(rows).all(axis=1) & (rows == np.rint(rows)).all(axis=1)]
                rows = np.abs(rows) if rows_type is np.uint16 else rows
            w = ac.tile_rows(rows, R).astype(rows_type)
            d, block, rows_args = rows_on_device(w)
            o = DeviceArray.from_numpy(np.full(R + 4, SENTINEL, T))
            shift = ac.centroid_shifts(n)[index % len(ac.centroid_shifts(n))]
            run(L.dsp_wf_centroid_rows, "get_wf_centroid", *rows_args, float(shift), o.ptr)
            got = o.to_numpy()
            assert same(got[:R], ac.emulate_centroid(w.astype(T), shift, T)[0]) and (got[R:] == SENTINEL).all(), (rows_type, n, shift, padded)
            d.free(), o.free()
            # wf_correction
            rows = ac.correction_rows(loop, n)[1]
            if integer:
                rows = np.rint(rows[np.isfinite(rows).all(axis=1)])
            w = ac.tile_rows(rows, R).astype(rows_type)
            d, block, rows_args = rows_on_device(w)
            for m, start, stop, nan_at in ac.correction_params(n)[index % 2::2]:
                tpl = ac.template(loop, m, nan_at)
                dt, o = DeviceArray.from_numpy(tpl), output(n, out_stride)
                run(L.dsp_wf_correction_rows, "wf_correction", *rows_args, dt.ptr, m, start, stop, o.ptr + off * esz, out_stride)
                got, clean = _rows_out(o, off, R, out_stride, n)
                want = ac.emulate_correction(w, tpl, start, stop, T)
                assert same(got, want) and clean, (rows_type, n, m, start, stop, padded, _diff(got, want))
                dt.free(), o.free()
            assert d.to_numpy().tobytes() == block.tobytes()
            d.free()
    assert {v[0] for v in vectors} == {True, False} and {v[1] for v in vectors} == {True, False}


# ---------------------------------------------------------------------------------------------------------------- 6. alignment and correction in one launch
def _launch(prog, T, R, arrays, outs):
    """one launch of a program of ac.program(...): the outputs it stores, by name"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray, sync

    chain = Chain(prog, compute_dtype=T)
    assert chain.kernel_name == ac.KERNEL and chain.geometry(R)["blocks"] == -(-R // 4)
    names = [i[0] for i in prog.io]
    dev = {k: DeviceArray.from_numpy(v) for k, v in arrays.items() if k in names}
    for name, shape in outs.items():
        if name in names:
            dev[name] = DeviceArray.from_numpy(np.full(shape, SENTINEL, T))
    chain.execute(dev, R)
    sync()
    chain.check()
    got = {k: dev[k].to_numpy() for k in outs if k in dev}
    assert dev["w"].to_numpy().tobytes() == arrays["w"].tobytes()
    chain.close()
    for d in dev.values():
        d.free()
    return got


@pytest.mark.parametrize("rows_type, loop", [(np.float32, "f32"), (np.uint16, "f32"), (np.int16, "f32"), (np.float64, "f64"), (np.int32, "f64")])
def test_the_fused_launch_equals_the_two_apart(rows_type, loop):
    from dspeed_amd.processors import wf_alignment, wf_correction

    T = ac.LOOPS[loop]
    integer = np.dtype(rows_type).kind in "iu"
    for index, n in enumerate((3, 65, 129, 1000)):
        rows = ac.align_rows(loop, n, rows_type if integer else None)[1]
        params = ac.align_params(n)
        for j in range(6):
            c, sh, s = params[(11 * index + 17 * j) % len(params)]
            R = _count(index + j)
            w = ac.tile_rows(rows, R)
            cs = (c + np.arange(R) % 4).astype(T)
            start, stop = (0, s) if j % 3 == 0 else ((s // 3, s // 3 + 1) if j % 3 == 1 else (s // 4, max(s // 4 + 1, s - 1)))
            tpl = ac.template(loop, stop - start + j % 2, 0 if j == 5 else None)
            aligned = np.full((R, s), SENTINEL, T)
            wf_alignment(w, cs, sh, s, aligned)
            assert same(aligned, ac.emulate_alignment(w, cs, sh, s, T)[0])
            apart = wf_correction(aligned, tpl, start, stop)
            assert same(apart, ac.emulate_correction(aligned, tpl, start, stop, T))
            for store_aligned in (True, False):
                prog = ac.program(n, "fused", rows=rows_type, loop=T, size=s, centroid="column", shift=sh, start=start, stop=stop, table_len=len(tpl), store_aligned=store_aligned)
                got = _launch(prog, T, R, {"w": w, "c": cs, "w_corr": tpl}, {"aligned": (R, s), "out": (R, s)})
                assert same(got["out"], apart), (rows_type, n, c, sh, s, start, stop, store_aligned, _diff(got["out"], apart))
                assert ("aligned" in got) == store_aligned and (not store_aligned or same(got["aligned"], aligned))  # written only when asked for


# ---------------------------------------------------------------------------------------------------------------- 7. the recipe
M = "dspeed.processors"


def _recipe():
    return {"wf_inl": {"function": "inl_correction", "module": M, "args": ["waveform", "db.inl", "wf_inl"]},
            "kern_step": {"function": "step", "module": M, "args": [16, "kern_step(16, 'f')"]},
            "wf_step": {"function": "convolve_wf", "module": M, "args": ["wf_inl", "kern_step", "'s'", "wf_step(1000, 'f')"]},
            "centroid": {"function": "get_wf_centroid", "module": M, "args": ["wf_step", 8, "centroid"]},
            "wf_align": {"function": "wf_alignment", "module": M, "args": ["wf_inl", "centroid", 8, 200, "wf_align(200)"]},
            "wf_corr": {"function": "wf_correction", "module": M, "args": ["wf_align", "db.tpl", 20, 120, "wf_corr"]}}


def test_the_chain_of_the_issue_from_a_recipe():
    from dspeed_amd.processing_chain import WaveformInput, build_processing_chain

    n_rows, n = 70, 1000
    t0 = np.where(np.arange(n_rows) % 2 == 1, 60 + np.arange(n_rows) // 2, 300 + 7 * np.arange(n_rows))  # most edges mid-row, some near its start
    i = np.arange(n)[None, :]
    w = (1000 + i % 3 + 2000 * ((i >= t0[:, None]) & (i < t0[:, None] + 250))).astype(np.uint16)  # (a box: the row ends on its baseline, the filter's edge effects stay below the pulse's)
    db = {"inl": [0.25 * (i % 5) for i in range(65536)], "tpl": [0.5 * i for i in range(100)]}
    T = np.float32
    for outputs in (["wf_corr"], ["wf_inl", "wf_step", "centroid", "wf_align", "wf_corr"]):
        chain, _, out = build_processing_chain({"outputs": outputs, "processors": _recipe()}, {"waveform": WaveformInput(w, 16.0)}, db_dict=db)
        chain.execute()
        assert [kernel for _what, kernel in chain.kernels()].count(ac.KERNEL) == 3
        fused = next(st for st in chain._stages if st["what"].startswith("wf_alignment wf_align + wf_correction wf_corr in one launch"))
        assert [o[0] for o in fused["outs"]] == (["out:wf_corr"] if len(outputs) == 1 else ["out:wf_align", "out:wf_corr"])  # the aligned row: only when asked for
        corr = np.asarray(out["wf_corr"])
        assert corr.shape == (n_rows, 200) and corr.dtype == T
        if len(outputs) == 1:
            first = corr
            continue
        inl = np.asarray(out["wf_inl"])
        assert same(inl, ac.emulate_inl(w, np.asarray(db["inl"], T), T)[0])
        cen, defined = ac.emulate_centroid(np.asarray(out["wf_step"]), 8, T)  # (of the filtered rows the device wrote: the FIR is not this test's)
        assert defined.all() and same(np.asarray(out["centroid"]), cen)
        aligned, status = ac.emulate_alignment(inl, cen, 8, 200, T)
        assert (status == ac.OK).all() and same(np.asarray(out["wf_align"]), aligned)
        assert {ac.align_window(c, 8.0, 200, n)[0] for c in cen} == {"window", "pad", "head"}
        assert same(corr, ac.emulate_correction(aligned, np.asarray(db["tpl"], T), 20, 120, T)) and same(corr, first)

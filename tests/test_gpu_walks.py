"""The threshold walk of time_point_thresh / interpolated_time_point_thresh on every route, on the rows of walk_cases.py: one feature a row, at
every distance from the start at which a search changes gear -- the two single steps and the rounds of 4 (find_crossing, dsp_vm.hip) and of
8 (reduce_finish, dsp_reduce_tail.h: dsp_reduce_kernel on both load paths, dsp_fir_runs_kernel on the row it filtered), the blocks of 8 of
the streaming walk (rows_consume, dsp_rows.hip) --, at both ends of the row, with every form of a sample that equals the threshold.  The
walks are comparisons on small integers: every output is the oracle's, bit for bit, dtype and shape included; no row is left out of a
comparison; every output buffer starts as a sentinel.  test_walk_cases_cpu.py shows on the oracle alone what the rows tell apart."""
import numpy as np
import pytest

import walk_cases as wc

pytestmark = pytest.mark.gpu


def _launch(program, inputs, outs, rows, kernel, fused=None, T=np.float32, widths=None):
    """one launch over ``rows`` rows: {output: array}.  ``widths``: elements per row of the outputs that are not columns"""
    from dspeed_amd.chain import Chain
    from dspeed_amd.device import DeviceArray

    ch = Chain(program, "walks", T)
    if fused is not None:
        ch.set_fused(fused)
    assert kernel in ch.kernel_name, ch.kernel_name
    bufs = {name: DeviceArray.from_numpy(np.ascontiguousarray(v)) for name, v in inputs.items()}
    for name in outs:
        shape = (rows, widths[name]) if widths and name in widths else (rows,)
        bufs[name] = DeviceArray.from_numpy(np.full(shape, wc.SENTINEL, dtype=T))
    ch.execute(bufs, rows)
    ch.check()
    return {name: bufs[name].to_numpy() for name in outs}


def _check(book, sel, got, want, what):
    """bit for bit, NaN equal to NaN, with the names of the rows that differ"""
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError((what, len(bad), [(book.name(sel[r]), float(got[r]), float(want[r])) for r in bad[:8]]))


def _vm(tag):
    book = wc.steps_book()
    T = wc.loop_of(tag)
    offset, stride = book.layout(tag, "vector")
    everything = np.arange(book.rows)
    inputs = {"wf": book.block(tag, "vector"), "thr": np.full(book.rows, wc.THR, T), "ts": book.ts.astype(T)}
    w = book.samples(tag)
    for fwd in (True, False):
        got = _launch(wc.vm_program(book.n, tag, fwd, offset, stride), inputs, ["out"], book.rows, "dsp_vm_kernel", fused=0, T=T)
        _check(book, everything, got["out"], wc.want_walk(w, wc.THR, book.ts, fwd, T), ("time_point_thresh", fwd))
        outs = [f"out_{m}" for m in wc.MODES]
        got = _launch(wc.interp_program(book.n, tag, fwd, offset, stride), inputs, outs, book.rows, "dsp_vm_kernel", fused=0, T=T)
        for m in wc.MODES:
            _check(book, everything, got[f"out_{m}"], wc.want_interp(w, wc.THR, book.ts, fwd, m, T), ("interpolated_time_point_thresh", fwd, m))


def _reduce(tag, path):
    book = wc.steps_book()
    offset, stride = book.layout(tag, path)
    everything = np.arange(book.rows)
    launches = [("column", everything, wc.COLUMN_WALKS, {}), ("promise", everything, wc.COLUMN_WALKS, dict(promise=True)),
                ("extremes", everything, wc.EXTREME_WALKS, dict(min_max=True)), ("chain", everything, wc.CHAIN_WALKS, {})]
    launches += [(f"constant{ts}", np.flatnonzero(book.ts == ts), wc.constant_walks(ts), {}) for ts in book.starts]
    for what, sel, walks, kw in launches:
        program, outs = wc.reduce_program(book.n, tag, offset, stride, walks, **kw)
        inputs = dict(wc.walk_inputs(len(sel)), wf=book.block(tag, path, sel), ts=book.ts[sel].astype(np.float32))
        got = _launch(program, inputs, outs, len(sel), "dsp_reduce_kernel", fused=1)
        want = wc.want_walks(book.samples(tag)[sel], walks, inputs["ts"])
        assert sorted(want) == sorted(outs)
        for name in outs:
            _check(book, sel, got[name], want[name], (what, name))
        vm = _launch(program, inputs, outs, len(sel), "dsp_vm_kernel", fused=0)  # the interpreter on the same program: the same bits
        for name in outs:
            _check(book, sel, vm[name], got[name], (what, name, "vm"))


def _fir_runs():
    book = wc.steps_book()
    n = book.n
    offset, stride = book.layout("f32", "vector")
    everything = np.arange(book.rows)
    taps = np.zeros(16, np.float32)
    taps[:len(wc.FIR_TAPS)] = wc.FIR_TAPS
    launches = [("column and extremes", everything, wc.FIR_WALKS)]
    launches += [(f"constant{ts}", np.flatnonzero(book.ts == ts), wc.constant_walks(ts)) for ts in book.starts]
    for what, sel, walks in launches:
        inputs = dict(wc.walk_inputs(len(sel)), wf=book.block("f32", "vector", sel), ts=book.ts[sel].astype(np.float32), taps=taps)
        rows = book.samples("f32")[sel]
        program, outs = wc.fir_program(n, offset, stride, walks, keep=True)
        kept = _launch(program, inputs, outs + ["filtered"], len(sel), "dsp_fir_runs_kernel", fused=1, widths={"filtered": n + 8})
        assert np.array_equal(kept["filtered"][:, :n], rows) and np.all(kept["filtered"][:, n:] == wc.SENTINEL)  # the filtered row IS the row
        want = dict(wc.want_min_max(rows), **wc.want_walks(rows, walks, inputs["ts"]))
        assert sorted(want) == sorted(outs)
        for name in outs:
            _check(book, sel, kept[name], want[name], (what, name))
        program, outs2 = wc.fir_program(n, offset, stride, walks, keep=False)  # the row left in the wavefront's scratch row
        scratch = _launch(program, inputs, outs2, len(sel), "dsp_fir_runs_kernel", fused=1)
        assert outs2 == outs
        for name in outs:
            _check(book, sel, scratch[name], kept[name], (what, name, "scratch row"))


def _rows(tag, build):
    for book in (wc.blocks_book(), wc.skip_book()):
        _rows_of(book, tag, build)


def _rows_of(book, tag, build):
    from dspeed_amd.processing_chain import build_processing_chain

    everything = np.arange(book.rows)
    tb, bl = wc.rows_input(book, tag)
    tb.update(thr=np.full(book.rows, wc.THR, np.float32), ts=book.ts.astype(np.float32))
    for start, fwd in wc.rows_launches(build):
        stop = build == "stop"
        chain, _, _ = build_processing_chain(wc.rows_recipe(bl, start, fwd, stop), tb)
        program = wc.lk.set_load_promise(chain.program) if stop else chain.program
        names = [io[0] for io in program.io]
        inputs = {name: tb[name[3:]] for name in names if name.startswith("in:")}
        outs = [name for name in names if name.startswith("out:")]
        assert outs == (["out:tp_0"] if stop else ["out:tp_min", "out:tp_max", "out:wf_min", "out:wf_max", "out:tp_0"])
        got = _launch(program, inputs, outs, book.rows, "dsp_rows_kernel")
        want = wc.rows_want(book, start, fwd)
        for name in outs:
            _check(book, everything, got[name], want[name[4:]], (build, start, fwd, name))


@pytest.mark.parametrize("route,tag,path", wc.families(), ids=lambda v: v)
def test_walks(route, tag, path):
    if route == "vm":
        _vm(tag)
    elif route == "reduce":
        _reduce(tag, path)
    elif route == "fir_runs":
        _fir_runs()
    else:
        _rows(tag, path)

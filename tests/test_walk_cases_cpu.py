"""Do the rows of walk_cases.py say something?  On the oracle and the planner alone: the oracle reports the sample every row was designed
for (NaN where none was), the NumPy model of the stepped search agrees with it on every row and each of its wrong neighbours -- < for <=, a
lost lane, the farthest hit, a bound one sample out, a round without its last step -- disagrees in both directions; the filters that stand
in front of two of the routes give the designed rows back bit for bit; every program is planned onto the kernel its route names.  If a
changed generator breaks a condition here, the generator is what changes."""
import numpy as np
import pytest

import oracle
import row_stream_cases as rs
import walk_cases as wc

BOOKS = {"steps": wc.steps_book, "blocks": wc.blocks_book}
KERNEL_OF = {"vm": "dsp_vm_kernel", "reduce": "dsp_reduce_kernel", "fir_runs": "dsp_fir_runs_kernel", "rows": "dsp_rows_kernel"}


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _oracle_own_direction(book, interp=False):
    """the oracle on every row in the direction the row was made for (both calls return rc == 0: want_walk asserts it)"""
    w = book.samples("f32")
    if interp:
        f, b = (wc.want_interp(w, wc.THR, book.ts, fwd, "i") for fwd in (True, False))
    else:
        f, b = (wc.want_walk(w, wc.THR, book.ts, fwd) for fwd in (True, False))
    return np.where(book.fwd, f, b).astype(np.float64)


@pytest.mark.parametrize("which", list(BOOKS))
def test_the_oracle_reports_the_designed_sample(which):
    book = BOOKS[which]()
    got = _oracle_own_direction(book)
    want = np.where(book.index >= 0, book.index, np.nan)
    bad = np.flatnonzero(~_same(got, want))
    assert not len(bad), [(book.name(r), got[r]) for r in bad[:8]]
    assert np.isnan(got[np.isin(book.kind, wc.NAN_KINDS)]).all() and np.isfinite(got[~np.isin(book.kind, wc.NAN_KINDS)]).all()
    # the same rows in every row type and in the float64 loop: the values are exact everywhere
    for tag in ("i16", "u16", "f64"):
        assert np.array_equal(book.samples(tag).astype(np.int64), book.w)
    f64 = np.where(book.fwd, wc.want_walk(book.w, wc.THR, book.ts, True, np.float64), wc.want_walk(book.w, wc.THR, book.ts, False, np.float64))
    assert np.array_equal(f64, got, equal_nan=True)
    # the interpolated walk backward stops one pair earlier: the rows whose crossing is the pair (0, 1) are NaN there and only there
    gi = _oracle_own_direction(book, interp=True)
    shifted = np.where(book.fwd, want, want - 1)
    lost = ~book.fwd & (book.index == 1)
    assert lost.sum() >= len(book.dists) and np.isnan(gi[lost]).all() and _same(gi[~lost], shifted[~lost]).all()
    assert np.isfinite(gi[~book.fwd & (book.index == 2)]).all() and (~book.fwd & (book.index == 2)).sum() >= len(book.dists)


@pytest.mark.parametrize("which", list(BOOKS))
def test_every_kind_at_every_distance_in_both_directions(which):
    book = BOOKS[which]()
    for fwd in (True, False):
        sel = book.fwd == fwd
        assert np.isfinite(_oracle_own_direction(book)[sel]).sum() * 2 >= sel.sum()
        for kind in wc.D_KINDS:
            for up in (True, False):
                have = set(book.d[sel & (book.kind == kind) & (book.up == up)].tolist())
                assert have == set(book.dists), (fwd, kind, up, sorted(set(book.dists) - have))
        for kind in wc.FLAT_KINDS:
            assert (sel & (book.kind == kind)).sum() >= 2 * len(book.starts) - 2
        # the starts from which no pair exists, and the last pair the walk may look at
        assert (sel & (book.ts == (book.n - 1 if fwd else 0))).sum() >= 2
        last = book.n - 2 if fwd else 1
        assert set(book.d[sel & (book.index == last) & (book.anchor != "cycle")].tolist()) == set(book.dists)
    if which == "blocks":  # the reported sample at every position of the two-block loop turn, at every distance
        for fwd in (True, False):
            for d in book.dists:
                sel = (book.fwd == fwd) & (book.d == d) & (book.kind == "cross")
                assert set((book.index[sel] % 16).tolist()) == set(range(16)), (fwd, d)
    assert 0 < book.touch.sum() and np.all(book.d[book.touch] == 0) and np.all(book.w[book.touch, book.ts[book.touch]] == wc.THR)


@pytest.mark.parametrize("which", list(BOOKS))
def test_the_marked_start_is_the_first_extreme(which):
    book = BOOKS[which]()
    mm = wc.want_min_max(book.samples("f32"))
    up, down = ~book.touch & book.up, ~book.touch & ~book.up
    assert np.array_equal(mm["t_min"][up], book.ts[up]) and np.array_equal(mm["t_max"][down], book.ts[down])
    assert np.all(mm["a_min"][up] == wc.LO - 1) and np.all(mm["a_max"][down] == wc.HI + 1)


def test_the_rows_of_the_block_test_leave_it_alone_to_decide():
    """skip_book: in every group of 64 rows (a wavefront of the rows kernel) no row has a new extreme in the block of the feature or the one
    behind it, and THR is that block's maximum (up) or minimum (down) -- only the equality of "threshold between the block's extremes" makes
    the wavefront look at the block"""
    book = wc.skip_book()
    assert book.rows == 64 * len(wc.SKIP_GROUPS) and np.array_equal(_oracle_own_direction(book), book.index)
    parity = {(fwd, up): set() for fwd in (True, False) for up in (True, False)}
    for g in range(0, book.rows, 64):
        sel = slice(g, g + 64)
        blocks = set((book.index[sel] // 8).tolist())
        assert len(blocks) == 1 and len(set(book.fwd[sel].tolist())) == 1 and len(set(book.up[sel].tolist())) == 1  # (one polarity: one equality)
        b = blocks.pop()
        parity[(bool(book.fwd[g]), bool(book.up[g]))].add(b % 2)
        assert set((book.index[sel] % 8).tolist()) == set(range(8)) and len(set(book.ts[sel].tolist())) == 8 and book.d[sel].min() >= 16
        for r in range(g, g + 64):
            seen, later, blk = book.w[r, :8 * b], book.w[r, 8 * b:8 * b + 16], book.w[r, 8 * b:8 * b + 8]
            assert later.max() <= seen.max() and later.min() >= seen.min()
            assert (blk.max() if book.up[r] else blk.min()) == wc.THR and (blk != wc.THR).sum() == 7
    assert all(v == {0, 1} for v in parity.values())
    mm = wc.want_min_max(book.samples("f32"))  # the mark is still the first extreme: the walks from the running extreme start there
    assert np.array_equal(np.where(book.up, mm["t_min"], mm["t_max"]), book.ts)


def test_the_memory_next_to_a_row_crosses_against_its_edge():
    book = wc.steps_book()
    before, after = book.pads()
    assert np.all((before > wc.THR) != (book.w[:, 0] > wc.THR)) and np.all((after > wc.THR) != (book.w[:, -1] > wc.THR))
    for tag in ("f32", "i16", "u16"):
        for path in rs.PATHS:
            offset, stride = book.layout(tag, path)
            assert rs.whole_vectors(tag, book.n, offset, stride) == (path == "vector"), (tag, path)
            b = book.block(tag, path)
            assert stride > book.n and offset >= 1 and np.array_equal(b[:, offset:offset + book.n], book.samples(tag))
            assert np.array_equal(b[:, offset - 1], before) and np.array_equal(b[:, offset + book.n], after)
    offset, stride = book.layout("f64", "vector")
    assert rs.whole_vectors("f64", book.n, offset, stride)


@pytest.mark.parametrize("per_round", [4, 8])
@pytest.mark.parametrize("which", list(BOOKS))
def test_the_model_is_the_oracle_and_its_wrong_neighbours_are_not(which, per_round):
    book = BOOKS[which]()
    want = _oracle_own_direction(book)
    assert _same(wc.model_rows(book, per_round=per_round), want).all()
    assert _same(wc.model_rows(book, per_round=per_round, interp=True), _oracle_own_direction(book, interp=True)).all()
    # (rows of 264 samples never leave the first two steps and never fill the last lane of one: the comparisons, the nearest hit and the
    # bounds are what they pin)
    variants = wc.WRONG if which == "steps" else ("strict", "farthest", "clamp")
    for variant in variants:
        bad = ~_same(wc.model_rows(book, per_round=per_round, variant=variant), want)
        assert (bad & book.fwd).any() and (bad & ~book.fwd).any(), variant


def test_what_each_family_of_rows_catches():
    """the counts profiles/r13_walks.md quotes: which kinds a wrong search gets wrong"""
    book = wc.steps_book()
    want = _oracle_own_direction(book)
    kinds = {v: set(book.kind[~_same(wc.model_rows(book, variant=v), want)].tolist()) for v in wc.WRONG}
    assert {"eq_near", "eq_far"} <= kinds["strict"] and "cross" not in kinds["strict"]
    assert kinds["farthest"] == {"two"}
    assert {"cross", "two", "eq_near", "eq_far"} <= kinds["lane63"] and {"cross", "eq_near"} <= kinds["skip_last"]
    assert {"none", "behind", "plateau"} <= kinds["clamp"]


def test_the_chain_of_walks_is_what_it_says():
    book = wc.steps_book()
    w, ts = book.samples("f32"), book.ts.astype(np.float32)
    out = wc.want_walks(w, wc.CHAIN_WALKS, ts)
    a, b, c, d = (out[f"walk{k}"] for k in range(4))
    found = np.isfinite(a)
    assert np.isnan(b[~found]).all() and np.isnan(c[~found]).all() and np.isnan(d[~found]).all()
    sel = found & book.fwd & (book.kind == "cross")
    assert sel.sum() > 100 and np.array_equal(b[sel], a[sel])                      # the same pair from a computed start
    far = sel & (book.d >= 1)
    assert np.array_equal(c[far & book.up], ts[far & book.up] + 1) and np.array_equal(d[far & ~book.up], ts[far & ~book.up] + 1)
    assert np.isnan(c[far & ~book.up]).all() and np.isnan(d[far & book.up]).all()  # (the other threshold is never reached)


def test_the_filters_in_front_give_the_rows_back():
    book = wc.steps_book()
    w = book.samples("f32")
    y, rc = oracle.convolve_wf(w, wc.FIR_TAPS, "s", book.n)
    assert rc == 0 and np.array_equal(y, w)
    for book in (wc.blocks_book(), wc.skip_book()):
        x = wc.inverse_trapezoid(book.w)
        assert np.abs(x).max() < wc.U16_UP and x.min() + wc.U16_UP > 0
        for tag in ("f32", "i16", "u16"):
            tb, bl = wc.rows_input(book, tag)
            rows = tb["waveform"].astype(np.float32)
            if bl:
                rows, rc = oracle.bl_subtract(rows, tb[bl])
                assert rc == 0
            y, rc = oracle.trap_filter(rows, *wc.TRAP[1:])
            assert rc == 0 and np.array_equal(y, book.samples("f32")), tag


def _plan(program, T=np.float32):
    from dspeed_amd.chain import plan

    return plan(program, T)["kernel"]


def test_the_interpreter_s_programs():
    book = wc.steps_book()
    for tag in ("f32", "i16", "u16", "f64"):
        offset, stride = book.layout(tag, "vector")
        for fwd in (True, False):
            k = _plan(wc.vm_program(book.n, tag, fwd, offset, stride), wc.loop_of(tag))
            # (LOAD, TIME_POINT_THRESH, STORE_SCALAR of a float32 loop is the reductions kernel's by default: the test switches it off)
            assert (KERNEL_OF["reduce"] if tag != "f64" else KERNEL_OF["vm"]) in k, (tag, k)
            assert KERNEL_OF["vm"] in _plan(wc.interp_program(book.n, tag, fwd, offset, stride), wc.loop_of(tag))


@pytest.mark.parametrize("path", rs.PATHS)
@pytest.mark.parametrize("tag", ["f32", "i16", "u16"])
def test_the_reductions_programs(tag, path):
    book = wc.steps_book()
    offset, stride = book.layout(tag, path)
    programs = [wc.reduce_program(book.n, tag, offset, stride, wc.COLUMN_WALKS), wc.reduce_program(book.n, tag, offset, stride, wc.COLUMN_WALKS, promise=True),
                wc.reduce_program(book.n, tag, offset, stride, wc.EXTREME_WALKS, min_max=True), wc.reduce_program(book.n, tag, offset, stride, wc.CHAIN_WALKS)]
    programs += [wc.reduce_program(book.n, tag, offset, stride, wc.constant_walks(ts)) for ts in book.starts]
    for p, _outs in programs:
        assert KERNEL_OF["reduce"] in _plan(p)


def test_the_run_length_fir_s_programs():
    book = wc.steps_book()
    offset, stride = book.layout("f32", "vector")
    for keep in (True, False):
        for walks in [wc.FIR_WALKS] + [wc.constant_walks(ts) for ts in book.starts]:
            assert KERNEL_OF["fir_runs"] in _plan(wc.fir_program(book.n, offset, stride, walks, keep)[0])


@pytest.mark.parametrize("build", wc.ROWS_BUILDS)
@pytest.mark.parametrize("tag", ["f32", "i16", "u16"])
def test_the_rows_kernel_s_programs(tag, build):
    for book in (wc.blocks_book(), wc.skip_book()):
        _rows_programs(book, tag, build)


def _rows_programs(book, tag, build):
    from dspeed_amd.processing_chain import build_processing_chain

    tb, bl = wc.rows_input(book, tag)
    tb.update(thr=np.full(book.rows, wc.THR, np.float32), ts=book.ts.astype(np.float32))
    for start, fwd in wc.rows_launches(build):
        chain, _, _ = build_processing_chain(wc.rows_recipe(bl, start, fwd, build == "stop"), tb)
        assert not chain._stages and chain._tail is None and chain._walks is None  # (one program, one kernel)
        if build == "stop":
            wc.lk.set_load_promise(chain.program)
        assert _plan(chain.program) == KERNEL_OF["rows"]
        want = wc.rows_want(book, start, fwd)["tp_0"]
        assert np.isfinite(want).sum() * 4 >= book.rows  # (every row walks in this direction, the ones made for the other one too)

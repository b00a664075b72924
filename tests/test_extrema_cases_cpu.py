"""Do the cases of get_multi_local_extrema say something?  On the fixtures alone (tests/golden/get_multi_local_extrema.npz: the rows of
extrema_cases.py with what the reference's body returned), no GPU: the book holds, for either sweep direction, rows that put a transition on
every boundary the kernel has, and the NumPy model of the kernel's group formulation returns what the reference returned on every case --
for every number of samples per lane the kernels are built with.  A condition that fails means the generator's rows change, not the condition."""
import os

import numpy as np
import pytest

import extrema_cases as xc
import golden_util

@pytest.fixture(scope="module")
def book():
    return golden_util.cases(xc.BOOK, kernel=xc.KERNEL)


def _sweeps(book, direction, tag="f32"):
    """(case, row, m, x in sweep order, par, vt_max, vt_min, n_max, n_min) of every row and m the reference swept in ``direction``"""
    for c in book:
        if c.tag != tag:
            continue
        w, par = c["w"].astype(c.dtype), c["par"]
        for d, m in c.params["combos"]:
            if d != direction:
                continue
            out = [c[xc.key(d, m, what)] for what in ("vt_max", "vt_min", "n_max", "n_min")]
            for r in range(len(w)):
                yield c, r, m, w[r], par[:, r], out[0][r], out[1][r], int(out[2][r]), int(out[3][r])


def _events(book, direction):
    """(case, row, m, x in sweep order, [(is_max, extreme, trigger)]) of the rows that got past the NaN rule"""
    for c, r, m, w, par, vt_max, vt_min, n_max, n_min in _sweeps(book, direction):
        if np.isnan(w).any() or np.isnan(par[:2]).any():
            continue
        yield c, r, m, (w if direction == 0 else w[::-1]), xc.sweep_events(w, direction, par[0], par[1], vt_max, vt_min)


def test_the_book_is_what_the_generator_builds(book):
    built = {g.name: g for g in xc.groups()}
    assert sorted(built) == sorted(c.name for c in book)
    for c in book:
        g = built[c.name]
        assert c["w"].dtype == g.w.dtype and np.array_equal(c["w"], g.w, equal_nan=True)
        assert np.array_equal(c["par"], g.par.astype(g.loop), equal_nan=True)
        assert all(np.array_equal(c[k], v) for k, v in g.extra.items())
        assert c.params["rows"] == g.names and [tuple(x) for x in c.params["combos"]] == g.combos and c.params["n"] == g.w.shape[1]
    assert sorted({c.params["n"] for c in book if c.name.startswith("f32")}) == sorted(xc.LENGTHS)
    assert any(n % 4 for n in xc.LENGTHS if n > 64) and 8192 in xc.LENGTHS
    for c in book:  # m = 1, 2, 5, 20, n - 1 wherever the row is long enough
        if c.name.startswith("f32") and c.params["n"] != 8192:
            n = c.params["n"]
            assert {m for d, m in c.params["combos"] if d == 0} == {m for m in (1, 2, 5, 20, n - 1) if m < n}
    assert os.path.getsize(os.path.join(golden_util.GOLDEN_DIR, xc.BOOK + ".npz")) <= 640 * 1024


def test_lists_are_padded_and_counted_as_the_reference_does(book):
    for c in book:
        for d, m in c.params["combos"]:
            vt_max, vt_min, n_max, n_min = (c[xc.key(d, m, what)] for what in ("vt_max", "vt_min", "n_max", "n_min"))
            assert vt_max.dtype == c.dtype and vt_min.dtype == c.dtype and n_max.dtype == np.uint32 and n_min.dtype == np.uint32
            for vt, cnt in ((vt_max, n_max), (vt_min, n_min)):
                assert vt.shape == (len(c["w"]), m)
                assert np.array_equal((~np.isnan(vt)).sum(axis=1), cnt)
                assert all(not np.isnan(row[:k]).any() for row, k in zip(vt, cnt))


@pytest.mark.parametrize("direction", [0, 1])
def test_transitions_fall_on_every_boundary(book, direction):
    trigger_mod = {64: set(), 256: set(), 512: set()}
    most_in_a_group, in_last_partial_group, extreme_groups_ahead = 0, False, False
    for c, r, m, x, events in _events(book, direction):
        n = len(x)
        for is_max, e, t in events:
            for k in trigger_mod:
                trigger_mod[k].add(t % k)
            in_last_partial_group |= n % 64 != 0 and t // 64 == (n - 1) // 64
            extreme_groups_ahead |= e // 64 < t // 64 and e // 512 < t // 512
        per_group = np.bincount([t // 64 for _, _, t in events]) if events else [0]
        most_in_a_group = max(most_in_a_group, int(max(per_group)))
    assert {0, 63} <= trigger_mod[64]
    assert {0, 255} <= trigger_mod[256]
    assert {0, 511} <= trigger_mod[512]  # (eight samples per lane: the int16 / uint16 kernels' groups)
    assert most_in_a_group >= 3
    assert in_last_partial_group
    assert extreme_groups_ahead


@pytest.mark.parametrize("direction", [0, 1])
def test_a_counter_saturates_and_the_machine_goes_on(book, direction):
    """with the smaller m both lists are full -- the minimum behind the last maximum is still found --, with a larger m the same row has more"""
    seen = False
    by_row = {}
    for c, r, m, w, par, vt_max, vt_min, n_max, n_min in _sweeps(book, direction):
        by_row.setdefault((c.name, r), {})[m] = (n_max, n_min)
    for counts in by_row.values():
        for m_small, (n_max, n_min) in counts.items():
            seen |= n_max == m_small and n_min == m_small and any(m > m_small and counts[m][0] > m_small and counts[m][1] > m_small for m in counts)
    assert seen


@pytest.mark.parametrize("direction", [0, 1])
def test_a_tied_extreme_is_tagged_at_its_first_occurrence(book, direction):
    seen, lists = False, {}
    for c, r, m, x, events in _events(book, direction):
        if (c.name, m) not in lists:
            lists[(c.name, m)] = [c[xc.key(d, m, "vt_max")] for d in (0, 1)]
        forward, backward = (a[r] for a in lists[(c.name, m)])
        for is_max, e, t in events:
            tied_behind = is_max and bool((x[e + 1:t] == x[e]).any())
            differs = not np.array_equal(forward, backward, equal_nan=True)
            seen |= tied_behind and differs
    assert seen


@pytest.mark.parametrize("direction", [0, 1])
def test_parameters_at_their_edges(book, direction):
    delta_zero = suppressed = nothing_found = infinite = False
    found = {}
    for c, r, m, w, par, vt_max, vt_min, n_max, n_min in _sweeps(book, direction):
        ok = not (np.isnan(w).any() or np.isnan(par[:2]).any())
        delta_zero |= ok and par[0] == 0 and par[1] == 0 and n_max > 0 and n_min > 0
        nothing_found |= ok and n_max == 0 and n_min == 0
        infinite |= ok and np.isinf(w).any() and n_max > 0 and n_min > 0
        found[(c.name, r, m)] = (w, par, n_max + n_min)
    for (name, r, m), (w, par, total) in found.items():  # the same row and deltas without the thresholds finds more
        if np.isinf(par[2]) and np.isinf(par[3]):
            continue
        for (name2, r2, m2), (w2, par2, total2) in found.items():
            if name2 == name and m2 == m and r2 != r and np.isinf(par2[2]) and np.isinf(par2[3]) and np.array_equal(par[:2], par2[:2]) and np.array_equal(w, w2):
                suppressed |= total < total2
    assert delta_zero and suppressed and nothing_found and infinite


def test_the_nan_rule_and_the_union_have_their_cases(book):
    names = set()
    for c in book:
        vt, cnt = c[xc.key(0, 1, "vt_max")] if [0, 1] in c.params["combos"] else None, None
        for r, name in enumerate(c.params["rows"]):
            if name.startswith("nan_") and not name.startswith("nan_abs") and vt is not None:
                assert np.isnan(vt[r]).all() and c[xc.key(0, 1, "n_max")][r] == 0 and c[xc.key(0, 1, "n_min")][r] == 0
                names.add(name.replace("_rev", ""))
    assert {"nan_first", "nan_last", "nan_delta_max", "nan_delta_min"} <= names
    duplicates = longer = False
    for c in book:
        for d, m in c.params["combos"]:
            if d != 3 or [0, m] not in c.params["combos"]:
                continue
            for r in range(len(c["w"])):
                f, b = (c[xc.key(k, m, "vt_max")][r] for k in (0, 1))
                f, b = set(f[~np.isnan(f)]), set(b[~np.isnan(b)])
                duplicates |= bool(f & b) and bool(f ^ b)
                longer |= len(f | b) > m and c[xc.key(3, m, "n_max")][r] == m
    assert duplicates and longer
    assert {"i16", "u16", "i32", "u32", "f64"} <= {c.name.split("_")[0] for c in book}
    # copies of the same integer-valued rows in four types (the unsigned ones shifted, the 32-bit ones scaled, their thresholds with them): the same lists
    by_name = {c.name: c for c in book}
    for n in (65, 513):
        i16 = by_name[f"i16_n{n}"]
        assert i16["w"].dtype == np.int16 and by_name[f"u16_n{n}"]["w"].dtype == np.uint16
        assert np.array_equal(by_name[f"u16_n{n}"]["w"], i16["w"].astype(np.int32) + 1000)
        for d, m in i16.params["combos"]:
            for what in ("vt_max", "vt_min", "n_max", "n_min"):
                want = i16[xc.key(d, m, what)].astype(np.float64)
                for other in ("u16", "i32", "u32"):
                    assert np.array_equal(by_name[f"{other}_n{n}"][xc.key(d, m, what)].astype(np.float64), want, equal_nan=True), (other, n, d, m, what)


@pytest.mark.parametrize("lane_samples", xc.LANE_SAMPLES)
def test_the_group_formulation_returns_what_the_reference_returns(book, lane_samples):
    """the kernel's algorithm -- groups of 64 x lane_samples samples, a prefix inside the lane and one across the lanes, the first trigger,
    the rest of the group again -- in NumPy, on every row, search direction and m of the book: indices, counts and NaN padding identical"""
    n_checked = 0
    for c in book:
        # the widths the rows' kernels have: one sample per lane, or a 16-byte vector of the rows' type; rows up to 257 samples at every width
        if lane_samples not in (1, 16 // c["w"].dtype.itemsize) and c.params["n"] > 257:
            continue
        w, par = c["w"], c["par"]
        for d, m in c.params["combos"]:
            want = [c[xc.key(d, m, what)] for what in ("vt_max", "vt_min", "n_max", "n_min")]
            for r in range(len(w)):
                got = xc.model(w[r], par[0, r], par[1, r], d, par[2, r], par[3, r], m, c.dtype, lane_samples)
                for k in range(2):
                    assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k][r], equal_nan=True), (c.name, c.params["rows"][r], d, m, k)
                assert (got[2], got[3]) == (want[2][r], want[3][r]), (c.name, c.params["rows"][r], d, m)
                n_checked += 1
    assert n_checked > 2000

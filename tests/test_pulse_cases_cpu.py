"""The case book of the pulse picker (tests/pulse_cases.py) against the reference bodies' recorded results (tests/golden/pulses.npz,
tools/gen_golden_pulses.py): the emulation -- the yardstick of the GPU tests -- equals what peak_snr_threshold and multi_a_filter returned
under CPython exactly, lists, counts and amplitudes, in both loops (nothing here rounds: no tolerance), on every row outside the two
classes the reference defines no result for; and each wrong neighbour of the rule fails on the book."""
import json
import os

import numpy as np
import pytest

import pulse_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{pc.BOOK}.npz")


@pytest.fixture(scope="module")
def book():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def emulated():
    """the emulation of the whole book, computed once: {key: (case, idx_out, count, trace, amplitudes or None, fatal or None)}"""
    out = {}
    for loop, T in pc.LOOPS.items():
        for c in pc.all_cases(loop):
            idx, count, trace = pc.emulate_picker(c["rows"], c["lists"], c["ratio"], c["width"], T)
            amp, fatal = pc.emulate_pickoff(c["rows"], idx, T) if c["m"] < c["n"] else (None, None)
            out[c["key"]] = (c, idx, count, trace, amp, fatal)
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def test_the_fixture_holds_outputs_only_and_every_case(book, emulated):
    keys = {e["case"] for e in json.loads(str(book["__index__"]))}
    assert keys == set(emulated)
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(k == "__index__" or k.split("/")[1] in ("idx_out", "n_idx_out", "va_max_out", "fatal", "va_max_direct", "fatal_direct") for k in book)
    assert max(v.shape[-1] for k, v in book.items() if k != "__index__" and v.ndim == 2) <= 64


def test_the_book_covers_the_shapes_and_names_the_issue_sets():
    for loop in pc.LOOPS:
        sweep = pc.sweep_cases(loop)
        assert {(c["n"], c["m"]) for c in sweep} == {(n, m) for n in pc.LENGTHS for m in pc.LIST_LENGTHS}
        assert {c["width"] for c in sweep if c["n"] == 257} == {0, 1, 10, 64, 262}
        names = [nm for c in pc.named_cases(loop) for nm in c["names"]]
        assert len(names) == len(set(names)) and set(pc.EXEMPT) <= set(names)
        for needed in ("minimum-at-c-plus-width-unseen", "minimum-at-last-sample-unseen-under-the-clamp", "minimum-at-a", "tied-minima", "window-clamped-at-0",
                       "width-0-ratio-above-1", "width-0-ratio-below-1", "negative-minimum-abs-matters", "plus-inf-at-candidate", "minus-inf-in-window",
                       "nan-inside-window", "nan-at-candidate", "nan-outside-every-window", "all-nan", "nans-in-front", "nans-in-the-middle", "nans-trailing",
                       "duplicates", "candidate-0-and-n-1", "half-integer-kept", "fraction-in-minus-1-0", "every-candidate-kept", "none-kept", "nan-ratio",
                       "ratio-equal-to-the-quotient"):
            assert needed in names, needed
        rows = sum(len(c["names"]) for c in pc.all_cases(loop))
        exempt = sum(int(c["exempt"].sum()) for c in pc.all_cases(loop))
        assert exempt == len(pc.EXEMPT) and exempt * 10 < rows  # the only exemptions, under a tenth of the cases
    assert pc.ROW_COUNTS == (1, 3, 4, 5, 9) and pc.LENGTHS == (2, 3, 21, 64, 65, 257, 1003) and pc.LIST_LENGTHS == (1, 2, 20, 63, 64)


@pytest.mark.parametrize("loop", list(pc.LOOPS))
def test_the_emulation_equals_the_reference_exactly(book, emulated, loop):
    kept = dropped = picked = fatal_rows = 0
    middle = False
    for key, (c, idx, count, _trace, amp, fatal) in emulated.items():
        if f"_{loop}_" not in key:
            continue
        held = ~c["exempt"]
        assert count.dtype == np.uint32 and np.array_equal(count[held], book[f"{key}/n_idx_out"][held]), key
        assert _same(idx[held], book[f"{key}/idx_out"][held]), key
        kept += int(count.sum())
        dropped += int((~np.isnan(c["lists"])).sum() - count.sum())
        if amp is None:
            assert f"{key}/va_max_out" not in book
            continue
        assert np.array_equal(fatal[held], book[f"{key}/fatal"][held] != 0), key
        assert _same(amp[held], book[f"{key}/va_max_out"][held]), key
        picked += int((~np.isnan(amp)).sum())
        fatal_rows += int(fatal.sum())
        # the case's own list, NaNs where they stand: the result is per entry, a NaN in the middle stays a NaN in its place
        direct, direct_fatal = pc.emulate_pickoff(c["rows"], c["lists"], pc.LOOPS[loop])
        assert np.array_equal(direct_fatal, book[f"{key}/fatal_direct"] != 0) and _same(direct, book[f"{key}/va_max_direct"]), key
        if "nans-in-the-middle" in c["names"]:
            r = c["names"].index("nans-in-the-middle")
            assert np.isnan(direct[r, 1:3]).all() and direct[r, 0] == 100 and direct[r, 3] == 100
            middle = True
    assert kept > 2000 and dropped > 2000 and picked > 1500 and fatal_rows == 3 and middle  # the book is not trivial; the three fractional candidates that are kept


def test_what_the_named_rows_say(emulated):
    for loop in pc.LOOPS:
        rows = {}
        for key, (c, idx, count, trace, amp, fatal) in emulated.items():
            if key.startswith(f"named_{loop}_"):
                for r, name in enumerate(c["names"]):
                    rows[name] = (c["lists"][r], idx[r], int(count[r]), trace[r], amp[r], bool(fatal[r]))
        assert rows["minimum-at-c-plus-width-unseen"][2] == 0 and rows["minimum-at-c-plus-width-minus-1-seen"][2] == 1
        assert rows["minimum-at-last-sample-unseen-under-the-clamp"][2] == 0 and rows["minimum-at-last-but-one-seen-under-the-clamp"][2] == 1
        assert rows["minimum-at-a"][2] == 1 and rows["minimum-just-below-a-unseen"][2] == 0 and rows["tied-minima"][3][0] == 8
        assert rows["width-0-ratio-above-1"][2] == 2 and rows["width-0-ratio-below-1"][2] == 0 and rows["width-0-ratio-1-strict"][2] == 0
        assert rows["width-0-ratio-above-1"][3][0] == 10  # an empty window leaves min_index = a = c
        assert rows["negative-minimum-abs-matters"][2] == 0 and rows["negative-candidate-sample"][2] == 0 and rows["all-negative-kept"][2] == 1
        assert rows["plus-inf-at-candidate"][2] == 1 and rows["minus-inf-in-window"][2] == 0 and rows["minus-inf-over-plus-inf"][2] == 0
        assert rows["nan-inside-window"][2] == 1 and rows["nan-at-window-start"][2] == 0 and rows["nan-at-candidate"][2] == 0
        # a NaN outside every window: the picker keeps its list, the pick-off of that row is all NaN
        assert rows["nan-outside-every-window"][2] == 1 and np.isnan(rows["nan-outside-every-window"][4]).all()
        assert rows["all-nan"][2] == 0 and rows["nans-in-front"][2] == 2 and list(rows["nans-in-front"][1][:2]) == [10, 10]
        assert rows["nans-in-the-middle"][2] == 2 and list(rows["nans-in-the-middle"][1][:2]) == [10, 3] and np.isnan(rows["nans-in-the-middle"][1][2:]).all()
        assert rows["duplicates"][2] == 4 and list(rows["unsorted"][1][:3]) == [10, 3, 10] and rows["unsorted"][2] == 3
        assert rows["half-integer-kept"][1][0] == 10.5 and rows["half-integer-kept"][5] and rows["fraction-truncated-not-rounded"][1][0] == 10.75
        assert rows["fraction-in-minus-1-0"][2] == 0 and rows["fraction-in-minus-1-0-kept"][2] == 3 and not rows["fraction-in-minus-1-0-kept"][5]
        got = rows["fraction-in-minus-1-0-kept"][4]  # -0.5 and -0.999 are below 0: NaN; -0.0 is not: w[0]
        assert np.isnan(got[0]) and got[1] == 100 and np.isnan(got[2])
        assert rows["every-candidate-kept"][2] == 4 and rows["none-kept"][2] == 0 and list(rows["kept-and-dropped-alternate"][1][:2]) == [10, 16]
        assert list(rows["every-candidate-kept"][4]) == [100, 100, 100, 100]
        assert rows["nan-ratio"][2] == 0 and rows["ratio-equal-to-the-quotient"][2] == 0 and rows["ratio-just-above-the-quotient"][2] == 1
        assert rows["ratio-zero-and-negative"][2] == 0 and rows["ratio-inf"][2] == 3
        # the device's decisions where the reference has none: dropped, and the others of the list kept
        for name in ("outside-below", "outside-fraction-below", "outside-n", "outside-above", "plus-inf", "minus-inf"):
            assert rows[name][2] == 1 and rows[name][1][0] == 10, name
        assert rows["zero-at-candidate"][2] == 0 and rows["zero-at-candidate-and-minimum"][2] == 0


NEIGHBOURS = {"window_includes_b": "picker", "last_tie": "trace", "b_clamped_to_n": "picker", "no_abs": "picker", "less_or_equal": "picker",
              "rounded_index": "picker", "nan_kept_in_place": "picker", "picker_row_nan_check": "picker", "no_pickoff_row_nan_check": "pickoff"}


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_a_wrong_neighbour_of_the_rule_fails_on_the_book(emulated, wrong):
    """each on the named rows and on the sweep: it must change a list or a count (the order of ties: the trace -- equal minima give equal
    quotients, so it shows in no output), or an amplitude for the pick-off's rule"""
    assert set(NEIGHBOURS) == set(pc.WRONG)
    differs = 0
    for key, (c, idx, count, trace, amp, _fatal) in emulated.items():
        if "_f32_" not in key or c["n"] > 65:
            continue
        T = np.float32
        if NEIGHBOURS[wrong] == "pickoff":
            if amp is not None:
                differs += int(not _same(pc.emulate_pickoff(c["rows"], idx, T, wrong=(wrong,))[0], amp))
            continue
        idx2, count2, trace2 = pc.emulate_picker(c["rows"], c["lists"], c["ratio"], c["width"], T, wrong=(wrong,))
        if NEIGHBOURS[wrong] == "trace":
            differs += int(not np.array_equal(trace, trace2))
        else:
            differs += int(not (np.array_equal(count, count2) and _same(idx, idx2)))
    assert differs > 0, wrong

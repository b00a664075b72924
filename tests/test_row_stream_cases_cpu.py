"""The case list of test_gpu_row_stream.py, held to what it promises before anything runs on a GPU: a sample on every boundary of the
load loop for every (kernel, row type, path), the planner's rule sending every launch down the path it is meant for, every model defined
on every row, and no case lost on the way."""
import numpy as np
import pytest

import row_stream_cases as rs

# what the kernels are built with: the samples of 16 bytes of a row, and the groups of loads in flight (vector path, scalar path)
SAMPLES_OF_16_BYTES = {"f32": 4, "i16": 8, "u16": 8, "f64": 2, "i32": 4, "u32": 4}
IN_FLIGHT = {"min_max": (4, 8), "time_over_threshold": (4, 8), "multi_time_point_thresh": (4, 8), "histogram": (4, 4), "extrema_forward": (4, 4),
             "extrema_backward": (4, 4)}
ROW_TYPES = {"min_max": 3, "time_over_threshold": 4, "multi_time_point_thresh": 4, "histogram": 4, "extrema_forward": 6, "extrema_backward": 6}


def test_every_kernel_type_and_path_is_a_family():
    fams = rs.families()
    assert len(fams) == len(set(fams)) == 2 * sum(ROW_TYPES.values())
    for kernel, count in ROW_TYPES.items():
        assert len({tag for k, tag, _p in fams if k == kernel}) == count


@pytest.mark.parametrize("kernel,tag,path", rs.families())
def test_the_cases_of_a_family(kernel, tag, path):
    from dspeed_amd.chain import plan

    N = SAMPLES_OF_16_BYTES[tag] if path == "vector" else 1
    K = IN_FLIGHT[kernel][path == "scalar"]
    every = [N * v for v in (1, 63, 64, 65, 64 * K - 1, 64 * K, 64 * K + 1)] if path == "vector" else [63, 64, 65, 64 * K - 1, 64 * K, 64 * K + 1]
    assert rs.all_lengths(kernel, tag, path) == every
    # what is left out: lists of 4 tags need rows of 5 samples -- one vector of 2 or 4 samples of the peak finder -- and nothing else
    out = rs.left_out(kernel, tag, path)
    assert out == ([N] if kernel.startswith("extrema") and path == "vector" and N <= 4 else [])
    cases = rs.cases(kernel, tag, path)
    assert [c.n for c in cases] == [n for n in every if n not in out] and len(cases) == len(every) - len(out)
    forced = set()
    for c in cases:
        n = c.n
        assert (c.N, c.K) == (N, K) and c.rows.dtype == rs.TYPES[tag] and c.rows.shape[1] == n and len(c.rows) <= 10 and n <= 4104
        # the path: the planner's rule on the binding
        assert rs.whole_vectors(tag, n, c.offset, c.stride) == (path == "vector"), c.name
        assert c.offset + n <= c.stride
        prog, kernel_name = c.program()
        assert plan(prog, c.loop)["kernel"] == kernel_name, c.name
        if path == "scalar":
            forced.add("offset" if c.offset else "stride")
        b = c.block()
        assert np.array_equal(b[:, c.offset:c.offset + n], c.rows, equal_nan=True) and (np.delete(b, np.s_[c.offset:c.offset + n], axis=1) == rs.PAD).all()
        # a row for every boundary position, flat elsewhere
        marks = sorted({p for p in (0, N - 1, N, 64 * N - 1, 64 * N, 64 * N * K - 1, 64 * N * K, n - 1) if 0 <= p < n})
        found = []
        for row in c.rows[:-2]:
            odd = np.flatnonzero(~(row == rs.BASE))
            assert len(odd) == 1
            found.append(int(odd[0]))
        assert found == marks, c.name
        assert (np.diff(c.rows[-2].astype(np.float64)) > 0).all() and (np.diff(c.rows[-1].astype(np.float64)) < 0).all()
        # every model is defined on every row, and sees the one sample
        want = c.expected()
        for name, a in want.items():
            assert len(a) == len(c.rows) and a.dtype in (c.loop, np.uint32), (c.name, name)
        if kernel == "min_max":
            assert list(want["t_max"][:-2]) == marks and not np.isnan(want["a_min"]).any()
        elif kernel == "time_over_threshold":
            assert (want["count"][:-2] == 1).all() and want["count"][-1] == want["count"][-2] == max(0, n - 3)
        elif kernel == "multi_time_point_thresh":
            if c.nan_marks:
                assert np.isnan(want["t_out"][:-2]).all()
            else:  # a step up at p is crossed between p - 1 and p (from sample 0 upwards: not at p = 0)
                for p, t in zip(marks, want["t_out"][:-2]):
                    assert np.isnan(t).all() if p == 0 else np.array_equal(t, (c.loop(p - 1) + (np.array(rs.THRESHOLDS, dtype=c.loop) - c.loop(10)) / c.loop(5)).astype(c.loop))
            if n >= 6:
                assert np.isfinite(want["t_out"][-2]).all()
        elif kernel == "histogram":
            assert (want["weights"][:-2].sum(axis=1) == n - 1).all() and (want["weights"][:-2, 0] == n - 1).all()
            assert (want["weights"][-2:].sum(axis=1) == n - 1).all()
        else:
            forward = kernel == "extrema_forward"
            for p, tags, count in zip(marks, want["vt_max"][:-2], want["n_max"][:-2]):
                seen = p < n - 1 if forward else p > 0  # (a sample behind the peak, in sweep order, triggers it)
                assert count == (1 if seen else 0) and (tags[0] == p if seen else np.isnan(tags[0]))
            # the rising row and the falling one: whichever falls in sweep order has its first sample tagged, three samples on
            assert (want["n_min"] == 0).all() and list(want["n_max"][-2:]) == ([0, 1] if forward else [1, 0])
            assert want["vt_max"][-1 if forward else -2][0] == (0 if forward else n - 1)
    if path == "scalar":
        assert forced == {"offset", "stride"}

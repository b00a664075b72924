"""Cases for the load loops of the row-streaming kernels (one layout, dsp_row_stream.h: dsp_reduce.hip, dsp_thresh.hip, dsp_hist.hip,
dsp_extrema.hip): a wavefront reads samples [g 64 N + lane N, + N) of group g, K groups in flight, N the samples of a 16-byte vector or 1.
Every length puts a group boundary somewhere else; every row is flat but for one sample that sits on a boundary of the loop, so a sample
that is dropped, read twice or taken for its neighbour changes a t_max, a count, a crossing time, a bin or a tag.  Expected values come
from NumPy (min_max) and from the case books' models of the other kernels, which the CPU tests pin to the reference's fixtures.
Nothing here needs a GPU."""
import numpy as np

import extrema_cases as xc
import histogram_cases as hc
import threshold_cases as tc

TYPES = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64, "i32": np.int32, "u32": np.uint32}
LANE_SAMPLES = {"f32": 4, "i16": 8, "u16": 8, "f64": 2, "i32": 4, "u32": 4}  # RowVec<IN>::N: the samples of 16 bytes
_F32_LOOP, _F64 = ("f32", "i16", "u16"), ("f64",)
EXTREMA_M, HIST_BINS = 4, 4
THRESHOLDS = (11.0, 12.5, 14.0)
# kernel -> (row types, groups in flight on the vector path, on the scalar path, the shortest row the processor takes)
KERNELS = {
    "min_max": (_F32_LOOP, 4, 8, 1),
    "time_over_threshold": (_F32_LOOP + _F64, 4, 8, 1),
    "multi_time_point_thresh": (_F32_LOOP + _F64, 4, 8, 2),  # (the walks compare neighbours)
    "histogram": (_F32_LOOP + _F64, 4, 4, 1),
    "extrema_forward": (_F32_LOOP + _F64 + ("i32", "u32"), 4, 4, EXTREMA_M + 1),  # (a list is shorter than its row)
    "extrema_backward": (_F32_LOOP + _F64 + ("i32", "u32"), 4, 4, EXTREMA_M + 1),
}
PATHS = ("vector", "scalar")
BASE, SPIKE, PAD = 10, 15, 99  # a flat row, its one sample, and what lies between the rows in memory


def loop_of(tag):
    return np.float32 if tag in _F32_LOOP else np.float64


def geometry(kernel, tag, path):
    """(N, K) of the loop for rows of this type on this path"""
    _types, k_vec, k_scalar, _shortest = KERNELS[kernel]
    return (LANE_SAMPLES[tag], k_vec) if path == "vector" else (1, k_scalar)


def all_lengths(kernel, tag, path):
    N, K = geometry(kernel, tag, path)
    if path == "vector":
        return [N * v for v in (1, 63, 64, 65, 64 * K - 1, 64 * K, 64 * K + 1)]
    return [63, 64, 65, 64 * K - 1, 64 * K, 64 * K + 1]


def lengths(kernel, tag, path):
    """the lengths a launch is made for: all of them but those the processor itself refuses (extrema: one vector of float64, int32, uint32
    or float32 is no longer than the lists; every other length, v = 1 of multi_time_point_thresh on float64 included, stays)"""
    return [n for n in all_lengths(kernel, tag, path) if n >= KERNELS[kernel][3]]


def left_out(kernel, tag, path):
    return [n for n in all_lengths(kernel, tag, path) if n < KERNELS[kernel][3]]


def boundaries(n, N, K):
    return sorted({p for p in (0, N - 1, N, 64 * N - 1, 64 * N, 64 * N * K - 1, 64 * N * K, n - 1) if 0 <= p < n})


def layout(tag, path, n, k):
    """(offset, stride) of the rows in memory, in elements.  Vector path: a whole vector in front of every row and two behind it.  Scalar
    path: an odd stride (even k) or rows that start one element behind a 16-byte boundary (odd k)."""
    N = LANE_SAMPLES[tag]
    if path == "vector":
        return N, n + 3 * N
    if k % 2 == 0:
        return 0, n + 1 + (n % 2)
    return 1, -(-(n + 1) // N) * N


def whole_vectors(tag, n, offset, stride):
    """the planner's rule for 16-byte loads"""
    es = np.dtype(TYPES[tag]).itemsize
    return (stride * es) % 16 == 0 and (offset * es) % 16 == 0 and (n * es) % 16 == 0


class Case:
    """one launch: rows of one length and type through one kernel"""

    def __init__(self, kernel, tag, path, n, k):
        self.kernel, self.tag, self.path, self.n = kernel, tag, path, n
        self.N, self.K = geometry(kernel, tag, path)
        self.offset, self.stride = layout(tag, path, n, k)
        self.loop = loop_of(tag)
        self.marks = boundaries(n, self.N, self.K)
        # multi_time_point_thresh streams the row for its NaN rule alone and walks it with plain reads: the one sample of a float row is a
        # NaN (every time NaN when it is seen), that of an integer row a step the walk has to find
        self.nan_marks = kernel == "multi_time_point_thresh" and tag in ("f32", "f64")
        dt = TYPES[tag]
        rows = np.full((len(self.marks) + 2, n), BASE, dtype=dt)
        for r, p in enumerate(self.marks):
            rows[r, p] = np.nan if self.nan_marks else SPIKE
        rows[-2] = BASE + np.arange(n)
        rows[-1] = BASE + np.arange(n)[::-1]
        self.rows = rows

    @property
    def name(self):
        return f"{self.kernel}:{self.tag}:{self.path}:n{self.n}"

    def block(self):
        """the rows as they lie in memory: ``stride`` apart from element ``offset`` on, PAD everywhere else"""
        b = np.full((len(self.rows), self.stride), PAD, dtype=self.rows.dtype)
        b[:, self.offset:self.offset + self.n] = self.rows
        return b

    def expected(self):
        """name of the output binding -> (rows, ...) array"""
        T, w = self.loop, self.rows
        if self.kernel == "min_max":
            f = w.astype(T)
            return {"t_min": np.argmin(f, axis=1).astype(T), "t_max": np.argmax(f, axis=1).astype(T), "a_min": f.min(axis=1), "a_max": f.max(axis=1)}
        if self.kernel == "time_over_threshold":
            return {"count": np.array([tc.model_time_over_threshold(r, 12.0, T) for r in w], dtype=T)}
        if self.kernel == "multi_time_point_thresh":
            return {"t_out": np.stack([tc.model(r.astype(T), np.array(THRESHOLDS, dtype=T), 0.0, 1.0, "l", T) for r in w])}
        if self.kernel == "histogram":
            got = [hc.model_histogram(r, HIST_BINS, T, self.N) for r in w]
            return {"weights": np.stack([g[0] for g in got]), "borders": np.stack([g[1] for g in got])}
        direction = 0 if self.kernel == "extrema_forward" else 1
        got = [xc.model(r, 2.0, 2.0, direction, 0.0, 1000.0, EXTREMA_M, T, self.N) for r in w]
        return {"vt_max": np.stack([g[0] for g in got]), "vt_min": np.stack([g[1] for g in got]),
                "n_max": np.array([g[2] for g in got], dtype=np.uint32), "n_min": np.array([g[3] for g in got], dtype=np.uint32)}

    def program(self):
        """(the program, name of its kernel); the row binding is "wf", the outputs those of ``expected``"""
        from dspeed_amd import _lib
        from dspeed_amd.chain import Program, Scalar

        dt, T, n = TYPES[self.tag], self.loop, self.n
        if self.kernel == "multi_time_point_thresh":
            return tc.multi_program(n, len(THRESHOLDS), dt, T, offset=self.offset, row_stride=self.stride), "dsp_thresh_kernel"
        if self.kernel == "histogram":
            return hc.hist_program(n, HIST_BINS, dt, T, offset=self.offset, row_stride=self.stride), "dsp_hist_kernel"
        p = Program()
        wf = p.add_io("wf", _lib.IO_WF_IN, dt, n, self.offset, self.stride)
        if self.kernel == "min_max":
            p.slots, p.n_sregs = [n], 4
            p.add_op(_lib.OP_LOAD, dst=0, io=wf)
            p.add_op(_lib.OP_MIN_MAX, dst=0, src=0)
            for r, name in enumerate(("t_min", "t_max", "a_min", "a_max")):
                p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io(name, _lib.IO_SCALAR_OUT, T), ip=(r,))
            return p, "dsp_reduce_kernel"
        if self.kernel == "time_over_threshold":
            p.slots, p.n_sregs = [n], 1
            p.add_op(_lib.OP_LOAD, dst=0, io=wf)
            p.add_op(_lib.OP_TIME_OVER_THRESHOLD, dst=0, src=0, sp=(Scalar.const(12.0),))
            p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("count", _lib.IO_SCALAR_OUT, T), ip=(0,))
            return p, "dsp_thresh_kernel"
        p.slots, p.n_sregs = [n, EXTREMA_M, EXTREMA_M], 2
        p.add_op(_lib.OP_LOAD, dst=0, io=wf)
        p.add_op(_lib.OP_MULTI_EXTREMA, dst=1, src=0, ip=(0 if self.kernel == "extrema_forward" else 1, 2, 0),
                 sp=(Scalar.const(2.0), Scalar.const(2.0), Scalar.const(0.0), Scalar.const(1000.0)))
        p.add_op(_lib.OP_STORE, src=1, io=p.add_io("vt_max", _lib.IO_WF_OUT, T, EXTREMA_M))
        p.add_op(_lib.OP_STORE, src=2, io=p.add_io("vt_min", _lib.IO_WF_OUT, T, EXTREMA_M))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_max", _lib.IO_SCALAR_OUT, np.uint32), ip=(0,))
        p.add_op(_lib.OP_STORE_SCALAR, io=p.add_io("n_min", _lib.IO_SCALAR_OUT, np.uint32), ip=(1,))
        return p, "dsp_extrema_kernel"

    def inputs(self):
        """bindings other than the rows"""
        return {"thr": np.array(THRESHOLDS, dtype=self.loop)} if self.kernel == "multi_time_point_thresh" else {}


def families():
    """every (kernel, row type, path): a test case each"""
    return [(kernel, tag, path) for kernel, spec in KERNELS.items() for tag in spec[0] for path in PATHS]


def cases(kernel, tag, path):
    return [Case(kernel, tag, path, n, k) for k, n in enumerate(lengths(kernel, tag, path))]

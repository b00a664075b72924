"""Cases of the single threshold walk -- time_point_thresh and interpolated_time_point_thresh (reference processors/time_point_thresh.py:12-92
and :95-222) -- for the four places the device searches for the crossing: find_crossing of the waveform VM (dsp_vm.hip: two single steps of
64 samples, then rounds of 4), reduce_finish of the kernels that read per-event values off rows (dsp_reduce_tail.h: two single steps, then
rounds of 8; run by dsp_reduce_kernel and by dsp_fir_runs_kernel on the row it just filtered) and the streaming rewrite of the
lane-per-waveform kernel (dsp_rows.hip: blocks of 8 samples, two a loop turn).

Every row is flat but for ONE feature whose index lies at a chosen distance d from the start of the walk, and d takes every value at which
one of the searches changes gear.  The values are small integers -- exact in int16, uint16, float32 and float64, through a one-tap FIR and
through a trapezoid -- so every route sees the same rows and every comparison is one of bits.

The rows in outward coordinates: u = 0 is the start, u grows away from it in the direction of the walk, s(u) is the sample.  The walk's
test at u is  (s(u) <= thr < s(u+1)) or (s(u) >= thr > s(u+1))  in either direction, and it reports the index of s(u).  An "up" row is
flat at LO and rises to HI, a "down" row is flat at HI and falls to LO (24 - v); THR lies half way.  The start sample is one count beyond the
flat level on the side away from THR (MARK: 9 or 15): the row's unique first extreme, so the same rows serve a constant start, a column,
t_min / t_max and the running extreme of the rows kernel.  Kinds:
    cross    s = flat up to d, the other level behind it: the strict crossing ("rise" on an up row, "fall" on a down row)
    eq_near  s(d) = THR, the other level behind it: the near sample equals the threshold, a hit by the <= (up) / >= (down) half
    eq_far   s(d) = THR alone, flat again behind it: the pair (d-1, d) has THR as its FAR sample and is no hit; the next pair outward,
             (d, d+1), is one by the other half of the test (>= on an up row)
    plateau  s = THR from d to the end of the row: both samples equal from d on, no hit anywhere, the walk runs to the end
    two      the other level at d+1 .. d+3 only: a second crossing three samples further out; the nearer one is reported
    behind   the other level everywhere behind the start: the only crossing is the pair just behind it, (ts-1, ts) forward and
             (ts, ts+1) backward, which is not the walk's -- NaN
    none     flat -- NaN
    shadowed (skip_book only) an eq_far row whose other level was seen before the feature: what the rows kernel's block test needs
A feature at d = 0 that needs s(0) = THR (eq_near, eq_far, plateau) takes the mark's place: those rows ("touch") have no unique extreme at
the start and the programs that start from an extreme are not pinned to the mark there.

Expected values come from the oracle alone.  The NumPy model of the stepped search below exists to show, on the oracle and without a GPU,
that the rows tell a correct search from its plausible wrong neighbours (WRONG).  Nothing here needs a GPU."""
import numpy as np

import lane_kernel_cases as lk
import oracle
import row_stream_cases as rs

LO, THR, HI = 10, 12, 14
PAD_HIGH, PAD_LOW = 20, 4  # what lies in front of / behind a row in memory: across THR from the row's edge sample
SENTINEL = -7777.0
D_KINDS = ("cross", "eq_near", "eq_far", "plateau", "two")  # kinds with a distance
FLAT_KINDS = ("behind", "none")
NAN_KINDS = ("plateau", "behind", "none")
MODES = "ibcafrnl"
TYPES = {"f32": np.float32, "i16": np.int16, "u16": np.uint16, "f64": np.float64}


def step_distances(rounds=(4, 8)):
    """every boundary of "two single steps of 64, then rounds of R steps", for both values of R in use"""
    d = {0, 1, 62, 63, 64, 65, 126, 127, 128, 129}
    for R in rounds:
        d |= {128 + 64 * R - 1, 128 + 64 * R, 128 + 64 * R + 1, 128 + 128 * R - 1, 128 + 128 * R}
    return tuple(sorted(d))


BLOCK_DISTANCES = (0, 1, 6, 7, 8, 9, 15, 16, 17)  # the rows kernel: blocks of 8, two a loop turn


def loop_of(tag):
    return np.float64 if tag == "f64" else np.float32


def _row(n, ts, fwd, kind, d, up, shadow=False):
    """(samples, touch) or None where the row has no room for the feature.  ``shadow``: the other level everywhere behind the start and in
    the first 8 samples as well, so that the feature is no new extreme of the row, from whichever end the row is read"""
    sg = 1 if fwd else -1
    umax = (n - 1 - ts) if fwd else ts
    flat, other, mark = (LO, HI, LO - 1) if up else (HI, LO, HI + 1)
    w = np.full(n, flat, dtype=np.int64)

    def fill(u0, u1, v):
        a, b = ts + sg * u0, ts + sg * u1
        w[min(a, b):max(a, b) + 1] = v

    touch = False
    if kind == "cross":
        if d + 1 > umax:
            return None
        fill(d + 1, umax, other)
    elif kind == "eq_near":
        if d + 1 > umax:
            return None
        fill(d + 1, umax, other)
        w[ts + sg * d], touch = THR, d == 0
    elif kind == "eq_far":
        if d + 1 > umax:
            return None
        w[ts + sg * d], touch = THR, d == 0
    elif kind == "plateau":
        if d > umax:
            return None
        fill(d, umax, THR)
        touch = d == 0
    elif kind == "two":
        if d + 4 > umax:
            return None
        fill(d + 1, d + 3, other)
    elif kind == "behind":
        if (ts - 1 < 0) if fwd else (ts + 1 > n - 1):
            return None
        if fwd:
            w[:ts] = other
        else:
            w[ts + 1:] = other
    else:
        assert kind == "none"
    if shadow:  # (the kernels that stream a row meet its first block first: the other level stands there in either direction)
        w[:8] = other
        if fwd:
            w[:ts] = other
        else:
            w[ts + 1:] = other
    if not touch:
        w[ts] = mark
    return w, touch


class Book:
    """The rows of one length: ``w`` (rows, n) int64, ``ts`` the start, ``fwd`` the direction the row was made for, ``kind`` / ``up`` / ``d``
    (-1: the kind has none) / ``anchor`` ("start", "end", "cycle") / ``touch``, and ``index``: the sample the walk has to report (-1: NaN)."""

    def __init__(self, n, dists, starts, cycle=None, made=None):
        self.n, self.dists, self.starts = n, tuple(dists), tuple(starts)
        W, meta = made if made else ([], [])
        for fwd in (True, False) if not made else ():
            where = [("start", ts, d) for ts in starts for d in dists]
            # the crossing at the last pair the walk may look at: i = n - 2 forward, i = 1 backward (i = 2: the interpolated walk's last)
            for last in ((n - 2,) if fwd else (1, 2)):
                where += [("end", last - d if fwd else last + d, d) for d in dists]
            if cycle:
                where += [("cycle", ts, d) for ts in cycle[fwd] for d in dists]
            seen = set()
            for anchor, ts, d in where:
                if not 0 <= ts < n or (ts, d) in seen:
                    continue
                seen.add((ts, d))
                for kind in D_KINDS:
                    for up in (True, False):
                        r = _row(n, ts, fwd, kind, d, up)
                        if r is not None:
                            W.append(r[0])
                            meta.append((ts, fwd, kind, up, d, anchor, r[1]))
            for ts in sorted({ts for ts, _d in seen}):
                for kind in FLAT_KINDS:
                    for up in (True, False):
                        r = _row(n, ts, fwd, kind, -1, up)
                        if r is not None:
                            W.append(r[0])
                            meta.append((ts, fwd, kind, up, -1, "start" if ts in starts else "end", False))
        self.w = np.array(W)
        self.ts = np.array([m[0] for m in meta])
        self.fwd = np.array([m[1] for m in meta])
        self.kind = np.array([m[2] for m in meta])
        self.up = np.array([m[3] for m in meta])
        self.d = np.array([m[4] for m in meta])
        self.anchor = np.array([m[5] for m in meta])
        self.touch = np.array([m[6] for m in meta])
        self.index = np.where(np.isin(self.kind, NAN_KINDS), -1, self.ts + np.where(self.fwd, 1, -1) * self.d)
        self.rows = len(self.w)

    def name(self, r):
        kind = self.kind[r] if self.kind[r] != "cross" else ("rise" if self.up[r] else "fall")
        return f"{kind}{'+' if self.up[r] else '-'}:{'fwd' if self.fwd[r] else 'bwd'}:ts{self.ts[r]}:d{self.d[r]}:{self.anchor[r]}"

    def samples(self, tag):
        """the rows in a row type (exact: small non-negative integers)"""
        return self.w.astype(TYPES[tag])

    def pads(self):
        """per row, what lies in front of and behind it in memory: across THR from its first / last sample, so that a read one element
        outside the row is a crossing the row does not have"""
        return np.where(self.w[:, 0] <= THR, PAD_HIGH, PAD_LOW), np.where(self.w[:, -1] <= THR, PAD_HIGH, PAD_LOW)

    def layout(self, tag, path):
        """(offset, stride) in elements.  vector: a whole 16-byte vector in front of every row and two behind it, as
        row_stream_cases.Case.block() has them; scalar: rows that start one element behind a 16-byte boundary"""
        N = rs.LANE_SAMPLES[tag]
        return (N, self.n + 3 * N) if path == "vector" else (1, -(-(self.n + 1) // N) * N)

    def block(self, tag, path, rows=None):
        """the rows (all, or those of the index array ``rows``) as they lie in memory"""
        offset, stride = self.layout(tag, path)
        sel = np.arange(self.rows) if rows is None else rows
        before, after = self.pads()
        b = np.empty((len(sel), stride), dtype=TYPES[tag])
        b[:, :offset] = before[sel, None]
        b[:, offset + self.n:] = after[sel, None]
        b[:, offset:offset + self.n] = self.w[sel]
        return b


_BOOKS = {}


def steps_book():
    """n = 1200: two rounds of 8 steps behind the two single ones, whole 16-byte vectors in every row type (VM, reductions, run-length FIR)"""
    if "steps" not in _BOOKS:
        n = 1200
        _BOOKS["steps"] = Book(n, step_distances(), (0, 1, 5, n // 2, n - 2, n - 1))
    return _BOOKS["steps"]


def blocks_book():
    """n = 264: 33 blocks of 8 (an odd number for the two-block loop); the "cycle" starts put the reported sample at every i mod 16"""
    if "blocks" not in _BOOKS:
        n = 264
        _BOOKS["blocks"] = Book(n, BLOCK_DISTANCES, (0, 1, 5, n // 2, n - 2, n - 1), cycle={True: range(96, 112), False: range(150, 166)})
    return _BOOKS["blocks"]


#: (direction, polarity, latest / earliest start, first sample of the feature's block): an even and an odd block each
SKIP_GROUPS = tuple((fwd, up, ts, first) for fwd, ts, firsts in ((True, 40, (56, 64)), (False, 223, (200, 192))) for first in firsts for up in (True, False))


def skip_book():
    """Rows for the block test of rows_consume alone.  A group of 64 rows shares a wavefront, and a block is looked at when ANY of them has a
    new extreme in it or its threshold between the block's extremes -- in the other books some neighbour always has.  Here a launch is whole
    groups of 64 "shadowed" rows of ONE polarity: eq_far rows (THR touched once, 16 samples and more from the start) with the other level
    everywhere behind the start and in the row's first block, so that both extremes of the row are known before the feature's block and THR
    EQUALS the block's maximum (up) or minimum (down): one equality of the block test decides alone, in an even and in an odd block of the
    two-block loop turn, with the touching sample at each of the 8 positions of its block (position 7 forward / 0 backward: the pair lies
    across two blocks) and 8 starts."""
    if "skip" not in _BOOKS:
        n, W, meta = 264, [], []
        for fwd, up, ts0, first in SKIP_GROUPS:
            for j in range(64):
                i, ts = first + j % 8, (ts0 - j // 8 if fwd else ts0 + j // 8)
                d = i - ts if fwd else ts - i
                w, touch = _row(n, ts, fwd, "eq_far", d, up, shadow=True)
                W.append(w)
                meta.append((ts, fwd, "shadowed", up, d, "start", touch))
        _BOOKS["skip"] = Book(n, sorted({m[4] for m in meta}), sorted({m[0] for m in meta}), made=(W, meta))
    return _BOOKS["skip"]


# ------------------------------------------------------------------------------------------------------------------------------------
# expected values: the oracle, processor by processor
# ------------------------------------------------------------------------------------------------------------------------------------
def _col(v, rows, T):
    return np.full(rows, v, dtype=T) if np.ndim(v) == 0 else np.asarray(v, dtype=T)


def want_walk(w, thr, ts, fwd, T=np.float32):
    """oracle.time_point_thresh on rows ``w`` (any row type: converted to the loop's type as the LOAD does)"""
    w = np.ascontiguousarray(w, dtype=T)
    out, rc = oracle.time_point_thresh(w, _col(thr, len(w), T), _col(ts, len(w), T), 1.0 if fwd else 0.0)
    assert rc == 0, rc
    return out


def want_interp(w, thr, ts, fwd, mode, T=np.float32):
    w = np.ascontiguousarray(w, dtype=T)
    out, rc = oracle.interpolated_time_point_thresh(w, _col(thr, len(w), T), _col(ts, len(w), T), 1 if fwd else 0, mode)
    assert rc == 0, rc
    return out


def want_min_max(w, T=np.float32):
    *mm, rc = oracle.min_max(np.ascontiguousarray(w, dtype=T))
    assert rc == 0, rc
    return dict(zip(("t_min", "t_max", "a_min", "a_max"), mm))


# ------------------------------------------------------------------------------------------------------------------------------------
# the stepped search, and its wrong neighbours
# ------------------------------------------------------------------------------------------------------------------------------------
WRONG = ("strict", "lane63", "farthest", "clamp", "skip_last")


def model(w, thr, ts, fwd, singles=2, per_round=8, back_lo=1, variant=None, before=None, after=None):
    """The index find_crossing / reduce_finish report on one row, or -1: ``singles`` steps of 64 lanes one at a time, then rounds of
    ``per_round`` steps whose reads are clamped into [.., n - 2] or [back_lo, ..] and whose clamped lanes do not count; the first step with a
    hit ends the walk and its lane nearest to the start wins.  ``before`` / ``after``: the elements next to the row in memory (only a wrong
    search reads them).  ``variant``, one of WRONG:
        strict     < for <= (and > for >=) on the near sample
        lane63     the ballot loses its last lane
        farthest   the farthest hit of a step instead of the nearest
        clamp      the bound of the reads and of the live lanes one sample too far out (n - 1 forward, back_lo - 1 backward)
        skip_last  a round does not look at its last step"""
    assert variant is None or variant in WRONG
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    ext = np.concatenate([[w[0] if before is None else before], w, [w[-1] if after is None else after]])
    near, far = ext[1:n + 1], (ext[2:n + 2] if fwd else ext[0:n])
    if variant == "strict":
        hit = ((near < thr) & (thr < far)) | ((near > thr) & (thr > far))
    else:
        hit = ((near <= thr) & (thr < far)) | ((near >= thr) & (thr > far))
    off = 1 if variant == "clamp" else 0
    lo, hi = (ts, n - 2 + off) if fwd else (back_lo - off, ts)
    i = np.arange(n)
    hit = hit & (i >= lo) & (i <= hi)
    sg = 1 if fwd else -1

    def step(b):
        if b < 0 or b >= n:
            return -1
        seg = hit[b:b + 64] if fwd else hit[max(b - 63, 0):b + 1][::-1]
        if variant == "lane63":
            seg = seg[:63]
        k = np.flatnonzero(seg)
        if not len(k):
            return -1
        return b + sg * int(k[-1] if variant == "farthest" else k[0])

    def inside(b):
        return b <= hi if fwd else b >= lo

    b = ts
    for _s in range(singles):
        if not inside(b):
            return -1
        f = step(b)
        if f >= 0:
            return f
        b += 64 * sg
    while inside(b):
        for q in range(per_round):
            if variant == "skip_last" and q == per_round - 1:
                continue
            f = step(b + 64 * q * sg)
            if f >= 0:
                return f
        b += 64 * per_round * sg
    return -1


def model_rows(book, fwd_of_walk=None, interp=False, **kw):
    """the model on every row of a book in the direction it was made for (or ``fwd_of_walk``), as the float64 the processors return:
    the index, one less for the interpolated walk backward (mode 'i'), NaN for -1"""
    before, after = book.pads()
    out = np.full(book.rows, np.nan)
    for r in range(book.rows):
        fwd = bool(book.fwd[r]) if fwd_of_walk is None else fwd_of_walk
        f = model(book.w[r], THR, int(book.ts[r]), fwd, back_lo=2 if interp else 1, before=before[r], after=after[r], **kw)
        if f >= 0:
            out[r] = f - (1 if interp and not fwd else 0)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# programs
# ------------------------------------------------------------------------------------------------------------------------------------
def vm_program(n, tag, fwd, offset, stride):
    """LOAD, TIME_POINT_THRESH, STORE_SCALAR: threshold and start are columns "thr" and "ts" of the loop's type; the output is "out"."""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program, Scalar

    T = loop_of(tag)
    p = Program()
    p.slots, p.n_sregs = [n], 1
    p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, TYPES[tag], n, offset, stride))
    thr, ts = Scalar.input(p.add_io("thr", L.IO_SCALAR_IN, T)), Scalar.input(p.add_io("ts", L.IO_SCALAR_IN, T))
    p.add_op(L.OP_TIME_POINT_THRESH, dst=0, src=0, sp=(thr, ts, Scalar.const(1.0 if fwd else 0.0)))
    p.add_op(L.OP_STORE_SCALAR, io=p.add_io("out", L.IO_SCALAR_OUT, T), ip=(0,))
    return p


def interp_program(n, tag, fwd, offset, stride):
    """LOAD, INTERP_TIME_POINT_THRESH in each of the eight modes, a STORE_SCALAR each: outputs "out_<mode>" """
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program, Scalar

    T = loop_of(tag)
    p = Program()
    p.slots, p.n_sregs = [n], len(MODES)
    p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, TYPES[tag], n, offset, stride))
    thr, ts = Scalar.input(p.add_io("thr", L.IO_SCALAR_IN, T)), Scalar.input(p.add_io("ts", L.IO_SCALAR_IN, T))
    for k, mode in enumerate(MODES):
        p.add_op(L.OP_INTERP_TIME_POINT_THRESH, dst=k, src=0, ip=(ord(mode),), sp=(thr, ts, Scalar.const(1.0 if fwd else 0.0)))
    for k, mode in enumerate(MODES):
        p.add_op(L.OP_STORE_SCALAR, io=p.add_io(f"out_{mode}", L.IO_SCALAR_OUT, T), ip=(k,))
    return p


def _add_walks(p, slot, walks, mm_reg):
    """TIME_POINT_THRESH ops on ``slot`` and their stores ("walk<k>").  A walk is (threshold, start, forward):
    threshold  a number | "thr" (the column) | ("thr2", factor): the column "thr2" times a constant, a SCALAR_AFFINE in front of the walk
    start      a number | "ts" (the column) | "t_min" | "t_max" (registers mm_reg, mm_reg + 1) | ("walk", j): where walk j ended"""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Scalar

    cols, regs = {}, []

    def col(name):
        if name not in cols:
            cols[name] = p.add_io(name, L.IO_SCALAR_IN, np.float32)
        return Scalar.input(cols[name])

    for thr, start, fwd in walks:
        if isinstance(thr, tuple):
            r = p.add_sregs(1)
            p.add_op(L.OP_SCALAR_AFFINE, dst=r, sp=(col(thr[0]), Scalar.const(thr[1]), Scalar.const(0.0)))
            t = Scalar.reg(r)
        else:
            t = col(thr) if isinstance(thr, str) else Scalar.const(float(thr))
        if isinstance(start, tuple):
            s = Scalar.reg(regs[start[1]])
        elif start in ("t_min", "t_max"):
            s = Scalar.reg(mm_reg + (start == "t_max"))
        else:
            s = col(start) if isinstance(start, str) else Scalar.const(float(start))
        regs.append(p.add_sregs(1))
        p.add_op(L.OP_TIME_POINT_THRESH, dst=regs[-1], src=slot, sp=(t, s, Scalar.const(1.0 if fwd else 0.0)))
    return regs


def reduce_program(n, tag, offset, stride, walks, min_max=False, promise=False):
    """LOAD, [MIN_MAX,] the walks, STORE_SCALARs: (program, names of its outputs).  ``promise``: the LOAD says every row is free of NaN or NaN
    throughout (ip[2] = 1), and with walks alone nothing streams the row"""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program

    p = Program()
    p.slots = [n]
    p.add_op(L.OP_LOAD, dst=0, io=p.add_io("wf", L.IO_WF_IN, TYPES[tag], n, offset, stride), ip=(0, 0, 1 if promise else 0))
    outs = []
    if min_max:
        p.add_sregs(4)
        p.add_op(L.OP_MIN_MAX, dst=0, src=0)
        outs += [("t_min", 0), ("t_max", 1), ("a_min", 2), ("a_max", 3)]
    outs += [(f"walk{k}", r) for k, r in enumerate(_add_walks(p, 0, walks, 0))]
    for name, r in outs:
        p.add_op(L.OP_STORE_SCALAR, io=p.add_io(name, L.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p, [name for name, _r in outs]


FIR_TAPS = np.array([1.0], np.float32)  # convolve_wf with it, mode 's': the filtered row is the row


def fir_program(n, offset, stride, walks, keep):
    """LOAD, CONVOLVE with the one-tap kernel (mode 's', the caller's word that it is piecewise constant), [STORE "filtered",] MIN_MAX, the
    walks on the FILTERED row, STORE_SCALARs: (program, names of the scalar outputs)"""
    from dspeed_amd import _lib as L
    from dspeed_amd.chain import Program

    p = Program()
    p.slots = [n, n]
    wf = p.add_io("wf", L.IO_WF_IN, np.float32, n, offset, stride)
    taps = p.add_io("taps", L.IO_TAPS, np.float32, 16, 0, 0)
    p.add_op(L.OP_LOAD, dst=0, io=wf)
    p.add_op(L.OP_CONVOLVE, dst=1, src=0, io=taps, ip=(ord("s"), 0, 1, len(FIR_TAPS)))
    if keep:
        p.add_op(L.OP_STORE, src=1, io=p.add_io("filtered", L.IO_WF_OUT, np.float32, n, 0, n + 8))
    p.add_sregs(4)
    p.add_op(L.OP_MIN_MAX, dst=0, src=1)
    outs = [("t_min", 0), ("t_max", 1), ("a_min", 2), ("a_max", 3)]
    outs += [(f"walk{k}", r) for k, r in enumerate(_add_walks(p, 1, walks, 0))]
    for name, r in outs:
        p.add_op(L.OP_STORE_SCALAR, io=p.add_io(name, L.IO_SCALAR_OUT, np.float32), ip=(r,))
    return p, [name for name, _r in outs]


# the walks of each family of reductions programs
COLUMN_WALKS = [(float(THR), "ts", True), (float(THR), "ts", False), ("thr", "ts", True), ("thr", "ts", False),
                (("thr2", 0.5), "ts", True), (("thr2", 0.5), "ts", False)]  # (the column thr2 holds 2 THR: the product is exact)
EXTREME_WALKS = [(float(THR), "t_min", True), (float(THR), "t_min", False), (float(THR), "t_max", True), (float(THR), "t_max", False)]
#: A forward from the column at THR; B forward from A's end at 13: the same pair, at distance 0 from a start computed on the device; C and D
#: backward from A's end at 9.5 and 14.5: the pair at the marked start of an up / a down row, d - 1 from a computed start.  NaN where A is
CHAIN_WALKS = [(float(THR), "ts", True), (13.0, ("walk", 0), True), (9.5, ("walk", 0), False), (14.5, ("walk", 0), False)]
FIR_WALKS = [("thr", "ts", True), ("thr", "ts", False)] + EXTREME_WALKS


def constant_walks(ts):
    return [(float(THR), float(ts), True), (float(THR), float(ts), False)]


def want_walks(w, walks, ts):
    """{"walk<k>": column} of the oracle, walk by walk, on float32 rows ``w`` with the start column ``ts``; with an extreme among the
    starts also the four values of min_max"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = {}
    if any(isinstance(s, str) and s.startswith("t_m") for _t, s, _f in walks):
        out.update(want_min_max(w))
    for k, (thr, start, fwd) in enumerate(walks):
        t = np.float32(THR) if isinstance(thr, (str, tuple)) else np.float32(thr)  # (the columns hold THR, or 2 THR times 0.5)
        if isinstance(start, tuple):
            s = out[f"walk{start[1]}"]
        elif isinstance(start, str):
            s = ts if start == "ts" else out[start]
        else:
            s = np.float32(start)
        out[f"walk{k}"] = want_walk(w, t, s, fwd)
    return out


def walk_inputs(rows):
    """the columns the walks' programs may bind"""
    return {"thr": np.full(rows, THR, np.float32), "thr2": np.full(rows, 2 * THR, np.float32)}


# ------------------------------------------------------------------------------------------------------------------------------------
# the rows kernel: trap_filter(8, 8) of the inverse trapezoid of the designed rows
# ------------------------------------------------------------------------------------------------------------------------------------
TRAP = ("trap_filter", 8, 8)
U16_UP = 1000  # uint16 rows sit this far up; bl_subtract takes it off again
ROWS_BUILDS = ("tpt1", "tpt2", "tpt3", "tpt4", "stop")  # rows_consume<.., TPT, STOP>


def inverse_trapezoid(y):
    """x with trap_filter(x, 8, 8) == y:  y[i] = y[i-1] + x[i] - x[i-8] - x[i-16] + x[i-24], everything before the row zero"""
    y = np.asarray(y, dtype=np.int64)
    dy = np.diff(y, axis=1, prepend=0)
    x = np.zeros((len(y), y.shape[1] + 24), dtype=np.int64)
    for i in range(y.shape[1]):
        x[:, 24 + i] = dy[:, i] + x[:, 16 + i] + x[:, 8 + i] - x[:, i]
    return x[:, 24:]


def rows_input(book, tag):
    """(table entries of the recipe, name of the baseline column or None) for rows of type ``tag``"""
    x = inverse_trapezoid(book.w)
    if tag == "u16":
        return {"waveform": (x + U16_UP).astype(np.uint16), "bl": np.full(book.rows, U16_UP, np.float32)}, "bl"
    return {"waveform": x.astype(TYPES[tag])}, None


def rows_launches(build):
    """the launches of a build: (start as the recipe spells it, forward).  TPT 1 / 3: backward / forward from the column; TPT 2 / 4: backward /
    forward from the running extreme -- the minimum (the mark of an up row) and the maximum (of a down row); the STOP build: TPT 1"""
    return {"tpt1": [("ts", 0)], "tpt3": [("ts", 1)], "tpt2": [("tp_min", 0), ("tp_max", 0)], "tpt4": [("tp_min", 1), ("tp_max", 1)],
            "stop": [("ts", 0)]}[build]


def rows_recipe(bl, start, fwd, stop):
    return lk.rows_recipe(None, TRAP, bl=bl, tpt=("thr", start, fwd), mm=not stop)


def rows_want(book, start, fwd):
    """the oracle on the DESIGNED rows (test_walk_cases_cpu shows its trap_filter gives them back bit for bit)"""
    w = book.w.astype(np.float32)
    out = want_min_max(w)
    s = book.ts.astype(np.float32) if start == "ts" else out[{"tp_min": "t_min", "tp_max": "t_max"}[start]]
    out = {"tp_min": out["t_min"], "tp_max": out["t_max"], "wf_min": out["a_min"], "wf_max": out["a_max"]}
    out["tp_0"] = want_walk(w, THR, s, bool(fwd))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the tests of test_gpu_walks.py: a route, a row type, a path
# ------------------------------------------------------------------------------------------------------------------------------------
def families():
    out = [("vm", tag, "lds") for tag in ("f32", "i16", "u16", "f64")]
    out += [("reduce", tag, path) for tag in ("f32", "i16", "u16") for path in rs.PATHS]
    out += [("fir_runs", "f32", "vector")]
    out += [("rows", tag, build) for tag in ("f32", "i16", "u16") for build in ROWS_BUILDS]
    return out

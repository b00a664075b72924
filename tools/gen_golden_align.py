"""Writes tests/golden/align.npz: what the REFERENCE's own bodies of inl_correction (processors/inl_correction.py), get_wf_centroid
(processors/get_wf_centroid.py), wf_alignment (processors/wf_alignment.py), wf_correction (processors/wf_correction.py) and step
(processors/kernels.py) return for tests/align_cases.py -- nothing of the product, nothing of the emulation.

    python tools/gen_golden_align.py

Runs only where the reference checkout is (oracle/gen_golden.py knows where: its numba stub and importer are used as they are).  The bodies
run under CPython.  Where CPython with NumPy and numba type an expression differently the body is handed numba's types: the scalars of the
float32 loop (shift, centroid) and the table of inl_correction arrive as float64 values holding the float32 ones, so that every sum is the
float64 sum numba forms; the outputs stay arrays of the loop's type.  ``size`` of wf_alignment arrives as a Python int: numba truncates a float
slice bound, CPython refuses one.
A row on which the body raises is recorded as such, not as an output: ``status`` holds 0 (returned), 1 (an IndexError or ValueError out of
NumPy: the reference defines nothing there) or 2 (DSPFatal, its text in the entry's note); the row's output is then NaN in the file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import align_cases as ac  # noqa: E402
from oracle import gen_golden  # noqa: E402

ALIGN_LENGTHS = (2, 3, 40, 129)  # (the windows are recorded whole: the short rows, which hold every branch and edge)
CORRECTION_LENGTHS = (3, 65, 129)


def run_rows(body, rows, out, args_of):
    """the body on every row; -> status per row, the texts of the DSPFatals"""
    from dspeed.errors import DSPFatal

    status, texts = np.zeros(len(rows), np.int8), []
    for r in range(len(rows)):
        try:
            body(*args_of(r))
        except DSPFatal as e:
            status[r], out[r] = ac.FATAL, np.nan
            texts.append(str(e))
        except (IndexError, ValueError):
            status[r], out[r] = ac.NUMPY_ERROR, np.nan
    return status, texts


def main():
    gen_golden._install_stubs()
    inl_correction = gen_golden._ref("inl_correction").inl_correction
    get_wf_centroid = gen_golden._ref("get_wf_centroid").get_wf_centroid
    wf_alignment = gen_golden._ref("wf_alignment").wf_alignment
    wf_correction = gen_golden._ref("wf_correction").wf_correction
    step = gen_golden._ref("kernels").step
    book = gen_golden.Book(ac.BOOK)
    with np.errstate(all="ignore"):
        for loop, T in ac.LOOPS.items():
            for n in ac.LENGTHS:
                _, rows = ac.centroid_rows(loop, n)
                shifts = ac.centroid_shifts(n)
                outs, stats = np.empty((len(shifts), len(rows)), T), np.empty((len(shifts), len(rows)), np.int8)
                for k, shift in enumerate(shifts):  # (a row of the arrays per shift)
                    out = outs[k]
                    stats[k], _ = run_rows(get_wf_centroid, rows, out, lambda r: (rows[r], np.float64(T(shift)), out[r:r + 1]))
                book.add(f"centroid_{loop}_n{n}", ac.KERNEL, loop, {"out": outs, "status": stats}, params={"n": n, "shifts": list(shifts)})
            for n in ALIGN_LENGTHS:
                _, rows = ac.align_rows(loop, n)
                rows = np.concatenate([rows, rows[:1]])  # (the last row meets a NaN centroid)
                for s in sorted({p[2] for p in ac.align_params(n)}):
                    params = [p for p in ac.align_params(n) if p[2] == s]  # (a plane of the arrays per (centroid, shift) of this size, in the book's order)
                    outs, stats, texts = np.empty((len(params), len(rows), s), T), np.empty((len(params), len(rows)), np.int8), set()
                    for k, (c, sh, _s) in enumerate(params):
                        out = outs[k]
                        cs = np.full(len(rows), np.float64(T(c)))
                        cs[-1] = np.nan
                        stats[k], t = run_rows(wf_alignment, rows, out, lambda r: (rows[r], cs[r], np.float64(T(sh)), int(s), out[r]))
                        texts |= set(t)
                    book.add(f"align_{loop}_n{n}_size{s}", ac.KERNEL, loop, {"out": outs, "status": stats}, params={"n": n, "size": s}, note="; ".join(sorted(texts)))
            for n in CORRECTION_LENGTHS:
                _, rows = ac.correction_rows(loop, n)
                for k, (m, start, stop, nan_at) in enumerate(ac.correction_params(n)):
                    out = np.empty(rows.shape, T)
                    tpl = ac.template(loop, m, nan_at)
                    status, _ = run_rows(wf_correction, rows, out, lambda r: (rows[r], tpl, start, stop, out[r]))
                    book.add(f"correct_{loop}_n{n}_p{k}", ac.KERNEL, loop, {"out": out, "status": status}, params={"n": n, "m": m, "start": start, "stop": stop})
            _, rows = ac.correction_rows(loop, 129)
            for k, (n, m, start, stop, _text) in enumerate(ac.CORRECTION_REFUSALS):
                out = np.empty(rows[:1].shape, T)
                status, texts = run_rows(wf_correction, rows[:1], out, lambda r: (rows[r], ac.template(loop, m), start, stop, out[r]))
                book.add(f"correct_refused_{loop}_{k}", ac.KERNEL, loop, {"status": status}, params={"n": n, "m": m, "start": start, "stop": stop}, fatal=True, note="; ".join(texts))
            for name, rows, p, nan_at in ac.inl_cases(loop):
                table = ac.inl_table(loop, p, nan_at).astype(np.float64)  # (numba's int32 + float32 is a float64 sum)
                out = np.empty(rows.shape, T)
                status, texts = run_rows(inl_correction, rows, out, lambda r: (rows[r].astype(np.int32), table, out[r]))
                book.add(f"inl_{loop}_{name}", ac.KERNEL, loop, {"out": out, "status": status}, params={"p": p}, note="; ".join(texts))
            for n in (1, 2, 3, 4, 10, 16, 17):
                kernel = np.zeros(n, T)
                step(T(16), kernel)
                book.add(f"step_{loop}_n{n}", "host", loop, {"out": kernel}, params={"n": n})
    book.save()


if __name__ == "__main__":
    main()

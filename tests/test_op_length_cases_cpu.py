"""Do the cases of op_length_cases.py say something?  On the oracle and the planner alone (no device): every op has a case at every
length in every row type, with an error expected exactly below the op's minimum length; the expectations are not vacuous (half of the rows
give finite results, the walks cross in a quarter of the rows and miss in a quarter); a zero pad taken for a sample would change the
result on the one-signed rows at every length that has a pad; the recipes of forms B and C plan onto the interpreter with the chunk the
module computes; and the kernel that form A's program plans onto is recorded per op, length and type (profiles/r10_op_lengths.md holds
the table, and a route whose admission flips inside the sweep has both sides of a flip among LENGTHS).  If a changed rule breaks a
condition here, the rule is what changes."""
import os

import numpy as np
import pytest

import op_length_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
NOTE = os.path.join(HERE, "..", "profiles", "r10_op_lengths.md")
OPS = list(K.OPS)
SEEDS_PER_SIGN = K.SEEDS


def _rows_with_results(out):
    """rows in which at least half of the values of every output are finite (a window partly outside the row and the last sample of an
    upsampled row are NaN by the processors' definition)"""
    ok = np.ones(K.ROWS, dtype=bool)
    for o in out:
        o = np.asarray(o, dtype=np.float64).reshape(K.ROWS, -1)
        ok &= 2 * np.isfinite(o).sum(axis=1) >= o.shape[1]
    return ok


# ------------------------------------------------------------------------------------------------------------------------------------
# lengths and rows
# ------------------------------------------------------------------------------------------------------------------------------------
def test_every_length_has_a_class_and_every_class_a_length():
    assert K.LAYOUT_LENGTHS == (1, 2, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 1009, 1023, 1024, 1025, 2047, 2049, 3073)
    assert set(K.LAYOUT_LENGTHS) < set(K.LENGTHS) and len(K.LENGTHS) == len(K.LAYOUT_LENGTHS) + len(K.ROUTE_LENGTHS)
    by_class = {c: [n for n in K.LENGTHS if c in K.classes(n)] for c in K.CLASSES}
    assert all(K.classes(n) for n in K.LENGTHS), [n for n in K.LENGTHS if not K.classes(n)]
    assert all(by_class.values()), by_class
    assert by_class["len == 64 * C"] == [1024] and by_class["C just grown"] == [1025, 2049, 3073]
    assert [K.chunk(n) for n in (1, 1024, 1025, 2048, 2049, 3072, 3073)] == [16, 16, 32, 32, 48, 48, 64]
    # half of the lanes own nothing just past 1024, a single sample sits alone in its chunk at 17, 33, 65, 1009, 1025 and 3073
    assert (1025 - 1) // K.chunk(1025) + 1 == 33
    assert all(n - K.last_chunk_start(n) == 1 for n in by_class["one sample into the next chunk"])


@pytest.mark.parametrize("n", K.LENGTHS)
def test_the_rows_are_what_their_kinds_say(n):
    f32, f64, i16 = (K.batch(n, t) for t in K.TAGS)
    assert f32.shape == f64.shape == i16.shape == (K.ROWS, n) and K.ROWS == 70 and (f32.dtype, f64.dtype, i16.dtype) == (np.float32, np.float64, np.int16)
    assert np.array_equal(f32, f64.astype(np.float32), equal_nan=True)
    nan = np.isnan(f64)
    assert np.array_equal(i16[~nan], np.rint(f64[~nan]).astype(np.int16))
    last, first = K.is_kind("nan-last"), K.is_kind("nan-first")
    want = np.zeros_like(nan)
    want[last, n - 1] = True
    want[first, 0] = True
    assert np.array_equal(nan, want)  # (NaN in that one sample and nowhere else)
    assert (i16[last, n - 1] == 32767).all() and (i16[first, 0] == -32768).all()
    for w in (f32, f64, i16):
        x = w.astype(np.float64)
        assert (x[K.is_kind("negative")] < -2900).all() and (x[K.is_kind("positive")] > 2900).all()
        assert (x[K.is_kind("constant")] == x[K.is_kind("constant"), :1]).all() and (x[K.is_kind("constant")] != 0).all()
        if n >= 2:
            a, b = x[K.is_kind("max-first-min-last")], x[K.is_kind("min-first-max-last")]
            assert (a.argmax(axis=1) == 0).all() and (a.argmin(axis=1) == n - 1).all() and (b.argmin(axis=1) == 0).all() and (b.argmax(axis=1) == n - 1).all()
        step = x[K.is_kind("step-in-last-chunk")]
        onset = (step > 300).argmax(axis=1)
        assert (step > 300).any(axis=1).all() and (onset >= K.last_chunk_start(n)).all()
        assert len(np.unique(x[~np.isnan(x).any(axis=1)], axis=0)) >= (K.ROWS - 14 if n > 1 else 20)  # (distinct rows)


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage, minimum lengths, vacuity
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_coverage_and_minimum_lengths(op):
    """a case at every length in all three row types; an error exactly below the minimum length, which is the oracle's: the table of the
    module is held against the return codes at every length from 1 to 40, not only at LENGTHS"""
    for tag in K.TAGS:
        for n in sorted(set(K.LENGTHS) | set(range(1, 41))):
            cs = K.cases(op, n, tag)
            assert cs, (op, n, tag)
            assert all(c.op == op and c.n == n and c.tag == tag and len(c.bars) == len(c.outs) for c in cs)
            for c in cs:
                out, err = c.expect()
                assert (err is None) == (n >= K.min_length(c)), (c.id, err, K.min_length(c))
                if err is None:
                    assert len(out) == len(c.outs) and all(o.dtype == c.ft for o in out), c.id
                    assert all(o.shape == ((K.ROWS, length) if length else (K.ROWS,)) for o, (_k, length) in zip(out, c.outs)), c.id
        names = {n: sorted(c.name for c in K.cases(op, n, tag)) for n in K.LENGTHS}
        if op == "upsampler":
            assert all(("upsampler-x16" in names[n]) == (n <= K.UPSAMPLE_16_MAX) and "upsampler-x2" in names[n] for n in K.LENGTHS)
        elif op == "convolve_wf":
            assert all(len(names[n]) == 3 * len(K.fir_lengths(n)) for n in K.LENGTHS) and K.fir_lengths(3073) == [1, 2, 16, 17, 133]
        elif op == "slice":
            assert all(len(names[n]) == (5 if n > 1 else 3) for n in K.LENGTHS)
        else:
            assert all(names[n] == names[1] for n in K.LENGTHS), op  # (every variant at every length)
    assert set(K.MIN_LENGTH) == set(K.OPS)


def test_the_largest_upsampled_row_is_the_planner_s():
    """x16 where the output fits: the planner takes 16 x 1025 samples beside the row in both loops and refuses 16 x 2047"""
    from dspeed_amd.chain import plan

    for tag in ("f32", "f64"):
        fits = next(c for c in K.cases("upsampler", K.UPSAMPLE_16_MAX, tag) if c.name == "upsampler-x16")
        assert plan(K.processor_program(fits), fits.ft)["kernel"].startswith("dsp_vm_kernel")
    c = next(c for c in K.cases("upsampler", 2047, "f64") if c.name == "upsampler-x2")
    c16 = K.Case(c.op, "upsampler-x16", 2047, "f64", {}, [("o", 16 * 2047)], None, c.call, None, c.bars)
    with pytest.raises(ValueError, match="LDS"):
        plan(K.processor_program(c16), c16.ft)


@pytest.mark.parametrize("op", OPS)
def test_the_expectations_are_not_vacuous(op):
    for tag in K.TAGS:
        finite_in = K.finite_rows(K.in_loop(K.batch(5, tag), tag))
        for n in K.LENGTHS:
            for c in K.cases(op, n, tag):
                out, err = c.expect()
                if err is not None:
                    continue
                got = _rows_with_results(out)
                if c.walk:
                    first = K.WALK_CAN_CROSS[c.name.rsplit("-", 1)[0] if c.op.startswith("interp") else c.name]
                    if n < first:
                        assert not got.any(), c.id  # (no pair of samples to cross between: every row misses)
                        continue
                    assert not got[~finite_in].any()
                    crossed, missed = got[finite_in].mean(), 1 - got[finite_in].mean()
                    assert crossed >= 0.25 and missed >= 0.25, (c.id, crossed, missed)
                    assert not got[K.is_kind(*K.ONE_SIGNED)].any(), c.id  # (no sample of a one-signed row crosses its threshold)
                else:
                    assert got.mean() >= 0.5, (c.id, got.mean())


# ------------------------------------------------------------------------------------------------------------------------------------
# discrimination
# ------------------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    return ~((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1)


@pytest.mark.parametrize("op", K.PAD_SENSITIVE)
def test_a_pad_read_as_a_sample_would_show(op):
    """the oracle on the one-signed rows extended with zeros to 64 * C samples -- what a kernel would compute that let the pads take part --
    against the oracle on the rows themselves: different wherever the slot has a pad, for at least the rows of one sign (a maximum
    cannot see a zero beside an all-positive row), for every other op on all 14 rows"""
    signed = K.is_kind(*K.ONE_SIGNED)
    for tag in K.TAGS:
        for n in K.LENGTHS:
            if n == 64 * K.chunk(n) or n < K.MIN_LENGTH[op]:
                continue
            assert n % K.chunk(n) != 0 or n < 64 * K.chunk(n)
            sensitive = [c for c in K.cases(op, n, tag) if c.pad_oracle is not None]
            assert sensitive, (op, n, tag)
            for c in sensitive:
                out, err = c.expect()
                assert err is None
                w = K.in_loop(c.rows, tag)
                cols = {k: v[signed] for k, v in c.cols.items()}
                *padded, rc = c.pad_oracle(K.padded(w[signed], n), cols)
                assert rc == 0
                changed = np.zeros(int(signed.sum()), dtype=bool)
                for o, p in zip(out, padded):
                    changed |= _differs(o[signed], p)
                assert changed.sum() >= SEEDS_PER_SIGN if op == "amax" else changed.all(), (c.id, int(changed.sum()))


# ------------------------------------------------------------------------------------------------------------------------------------
# the planner
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_forms_b_and_c_plan_onto_the_interpreter(op):
    """one program, one launch, the interpreter's; every slot with the chunk of its length at a pitch of chunk + 1 -- but the input of a FIR
    that nothing else touches (form B), which lies linear --; form C keeps wf_c beside the amax; below the minimum length the build raises
    the oracle's error"""
    from dspeed_amd import _lib
    from dspeed_amd.chain import plan
    from dspeed_amd.errors import DSPFatal
    from dspeed_amd.processing_chain import build_processing_chain

    raised = {K.FATAL: DSPFatal, K.ZERODIV: ZeroDivisionError}
    for tag in K.TAGS:
        for n in K.LENGTHS:
            for c in K.cases(op, n, tag):
                out, err = c.expect()
                for form in "BC":
                    recipe, table, names, extra = c.recipe(form)
                    with K.switches():
                        if err is not None:
                            with pytest.raises(raised[err]):  # (when the recipe is translated, or when its chain is created)
                                plan(build_processing_chain(recipe, table)[0].program, c.ft)
                            continue
                        chain, _, bufs = build_processing_chain(recipe, table)
                        info = plan(chain.program, c.ft)
                    assert not chain._stages and not chain._aux and chain._tail is None and chain._walks is None, (c.id, form)
                    assert info["kernel"].startswith("dsp_vm_kernel") and info["team"] == 1, (c.id, form, info["kernel"])
                    assert info["lds_bytes_per_wave"] == c.ft.itemsize * info["lds_elems_per_wave"], (c.id, form)
                    codes = [o[0] for o in chain.program.ops]
                    assert codes[0] == _lib.OP_LOAD
                    for i, (s, length) in enumerate(zip(info["slots"], chain.program.slots)):
                        linear = c.op == "convolve_wf" and form == "B" and i == chain.program.ops[0][1]
                        assert s["chunk"] == K.chunk(length) and s["pitch"] == s["chunk"] + (0 if linear else 1), (c.id, form, s, length)
                    if form == "C":
                        assert _lib.OP_AMAX in codes and _lib.OP_ELEMENTWISE in codes and (not c.outs[0][1] or (_lib.OP_MIN_MAX in codes and _lib.OP_STORE in codes))
                    for k, want in zip(names, out):
                        assert bufs[k].shape == want.shape and (bufs[k].dtype == want.dtype or c.op == "slice"), (c.id, form, k, bufs[k].dtype)


def _short(kernel):
    return "vm" if kernel.startswith("dsp_vm_kernel") else kernel.replace("dsp_", "").replace("_kernel", "")


def _variant_over_lengths(op, name, tag, n):
    """the case of the variant ``name`` at length n (the longest FIR's name carries its number of taps, min(n, 133))"""
    for c in K.cases(op, n, tag):
        if c.name == name or (name.endswith("-longest") and c.name == f"{name[:-8]}-{min(n, 133)}taps"):
            return c
    return None


def _variants(op, tag):
    names = [c.name for c in K.cases(op, 1, tag)]
    if op == "convolve_wf":
        names = [f"convolve_wf-{mode}-{m}taps" for m in (1, 2, 16, 17) for mode in "fvs"] + [f"convolve_wf-{mode}-longest" for mode in "fvs"]
    if op == "slice":
        names += ["slice-tail", "slice-head"]
    return names


def route_table():
    """{(variant, tag): [route at every length]}: the kernel form A plans onto, '!' behind it where the expectation is an error, '-' where
    the variant has no case"""
    table = {}
    for op in OPS:
        for tag in K.TAGS:
            for name in _variants(op, tag):
                row = []
                for n in K.LENGTHS:
                    c = _variant_over_lengths(op, name, tag, n)
                    if c is None:
                        row.append("-")
                    elif c.expect()[1] is not None:
                        row.append(c.expect()[1] + "!")
                    else:
                        row.append(_short(K.route_a(c)))
                table[(name, tag)] = row
    return table


def route_table_text(table):
    """the table as the profile note holds it: one line per run of variants and row types of an op that share their routes"""
    lines = ["lengths: " + " ".join(map(str, K.LENGTHS))]
    groups = {}
    for (name, tag), row in table.items():
        op = next(o for o in sorted(K.OPS, key=len, reverse=True) if name.startswith(o))
        groups.setdefault((op, tuple(row)), []).append((name[len(op) + 1:], tag))
    for (op, row), who in groups.items():
        variants, tags = list(dict.fromkeys(v for v, _ in who)), list(dict.fromkeys(t for _, t in who))
        if len(who) == len(variants) * len(tags):
            label = op + (" [" + " ".join(variants) + "]" if variants != [""] else "") + " (" + " ".join(tags) + ")"
        else:
            label = op + " " + " ".join(f"{v}/{t}" for v, t in who)
        lines.append(f"{label}: " + " ".join(row))
    return "\n".join(lines)


@pytest.fixture(scope="module")
def routes():
    return route_table()


def test_form_a_routes_are_the_recorded_ones(routes):
    """where the planner puts the single-processor programs, per op, length and type: the table of the profile note, line by line"""
    with open(NOTE) as f:
        note = f.read()
    text = route_table_text(routes)
    missing = [line for line in text.splitlines() if line not in note]
    assert not missing, "profiles/r10_op_lengths.md does not hold these lines of the route table:\n" + "\n".join(missing)
    # an error expected is an error planned: the planner refuses what the oracle refuses, before anything runs
    assert all(r.endswith("!") or r in ("-", "vm", "reduce", "pz_rows", "fir_f16", "fir_store") for row in routes.values() for r in row)


def test_both_sides_of_every_admission_flip_are_among_the_lengths(routes):
    """a route that changes inside the sweep: every length from 1 to 3073 is planned for that variant, and every kind of flip found (the
    specialised kernel below, the interpreter above, or the reverse) happens between two neighbouring LENGTHS as well"""
    lengths = set(K.LENGTHS)
    checked = 0
    for (name, tag), row in routes.items():
        kernels = {r for r in row if not r.endswith("!") and r != "-"}
        if len(kernels) < 2:
            continue
        op = name.split("-")[0]
        seen = {}
        for n in range(K.MIN_LENGTH[op], K.LENGTHS[-1] + 1):
            c = _variant_over_lengths(op, name, tag, n)
            seen[n] = _short(K.route_a(c)) if c is not None else None
        flips = {(seen[n - 1], seen[n]) for n in seen if n - 1 in seen and seen[n - 1] != seen[n] and None not in (seen[n - 1], seen[n])}
        among = {(seen[n - 1], seen[n]) for n in seen if n in lengths and n - 1 in lengths and n - 1 in seen}
        assert flips and flips <= among, (name, tag, flips - among)
        checked += 1
    assert checked >= 2  # (pole_zero and the longest FIR: the rows kernel and the two matrix-core FIR kernels take some lengths)

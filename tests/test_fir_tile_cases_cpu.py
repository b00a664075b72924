"""Is the case list of fir_tile_cases.py what it claims?  On the planner, the oracle and NumPy alone (no device): every class of tile
geometry is hit by a case that names it; what test_gpu_fir_mfma.py's own shapes reach is the incomplete set the list was made for; every
case plans onto the intended kernel under both settings of DSPEED_HIP_FIR_F32; the exact family's expectation is an integer below 2^24
that the float16 form's arithmetic reproduces bit for bit in any summation order; the fraction family's inputs leave that arithmetic
half of the bar; and a shifted, a dropped tap or a skipped column-tile group changes the exact expectation of every case.  If a changed
rule breaks a condition here, the rule (or the input) is what changes, never the bar."""
import os
import re

import numpy as np
import pytest

import fir_tile_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "dspeed_amd", "csrc")
CASES = K.cases()
IDS = [c.id for c in CASES]
FAMILIES = ("exact", "fraction")


def _sample_rows(c, family, count=6):
    """finite rows for the emulation: the special ones and the first seeded ones"""
    return np.flatnonzero(K.finite_rows(c.id, family))[:count]


# ------------------------------------------------------------------------------------------------------------------------------------
# the geometry and the classes
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_kernels():
    with open(os.path.join(CSRC, "dsp_kernels.h")) as f:
        h = f.read()
    with open(os.path.join(CSRC, "dsp_fir_f16.hip")) as f:
        k = f.read()
    with open(os.path.join(CSRC, "dsp_fir_mfma.hip")) as f:
        k32 = f.read()
    assert f"#define F16_BK {K.BK}" in h and f"#define F16_BM {K.BM}" in h and f"constexpr int TB = {K.TB};" in h
    assert "constexpr int TPITCH = ((TWIN + 8 + 15 * 8 + 127) / 128) * 128;" in h and K.TPITCH == 640
    assert f"constexpr int BN = {K.BN}, MT = 2, NT = 5;" in k and "constexpr int RES_HALFS = 2 * 16 * TPITCH;" in k
    assert "return ((kt + TB + 8 + 15 * 8 + 127) / 128) * 128;" in k and f"#define F16_KFLUSH {K.KFLUSH}" in k
    assert f"constexpr int KFLUSH_STORE = {K.KFLUSH_STORE};" in k
    assert f"constexpr int BK = {K.F32_BK}, KCHUNK = {K.KCHUNK};" in k32 and f"constexpr int SCHUNK = {K.SCHUNK};" in k32
    assert len(re.findall(r"\{(?:\d+, ){7}\d+\}", k[k.index("tap_slot[8][8]"):k.index("F16_PIPE 0")])) == 8  # (a tap_slot row per e)
    # resident taps end where the issue says: a full tile from 443 taps on fetches them stage by stage
    assert K.resident(442, 320) and not K.resident(443, 320) and K.amax_n_pipe(383, (64,)) == 4 and K.amax_kend(383, (64,)) == 384


def test_every_class_is_hit_by_a_case_that_names_it():
    hit = {}
    for c in CASES:
        cl = K.classes(c)
        assert c.why in cl, (c.id, c.why, cl)
        for name in cl:
            hit.setdefault(name, []).append(c)
    wanted = K.STORE_CLASSES + K.AMAX_CLASSES
    assert not [name for name in wanted if name not in hit]
    # a case of its own for every class but those that follow from the rotation of types and baselines and the amax form's p / m / slice classes,
    # which ride on the cases made for its stage counts
    derived = ("type ", "baseline ", "e32=", "amax p=", "amax m=", "amax longest", "amax slice", "amax 1 ", "amax 2 ")
    assert not [n for n in wanted if not n.startswith(derived) and n not in {c.why for c in CASES}]
    # a NaN in the last sample and +inf in the first in every class (one row cannot hold both)
    assert [n for n in wanted if not any(c.nonfinite for c in hit[n])] == ["rows 1"]
    store = [c for c in K.store_cases() if "unaligned offset" not in K.classes(c)]
    assert {(c.e, c.res) for c in store} == {(e, r) for e in range(8) for r in (True, False)}
    assert {K.align_e32(c.mode, c.m) for c in K.store_cases()} == {0, 1, 2, 3}
    assert {c.mode for c in store if c.res} == {c.mode for c in store if not c.res} == set("vsf")
    assert len(IDS) == len(set(IDS))
    # the sizes stay small: a few hundred samples by at most 577 rows
    assert max(c.row_len for c in CASES) <= 784 and max(c.rows for c in CASES) == 577


def test_the_existing_store_shapes_reach_an_incomplete_set():
    """the premise: test_gpu_fir_mfma.py feeds the float16 store form e in {0, 1, 4, 5, 6} with resident taps and {0, 2, 5} without --
    never e = 3 or 7, never a slice that is no multiple of 8 samples, never more than 131 rows"""
    import test_gpu_fir_mfma as T

    marks = {m.args[0]: m.args[1] for m in T.test_stored_output_all_modes.pytestmark if m.name == "parametrize"}
    assert tuple(marks["m,n,n_wf"]) == K.EXISTING_ALL_MODES and marks["mode"] == ["s", "v", "f"]
    pairs = K.e_res_pairs(K.EXISTING_STORE_SHAPES)
    assert {e for e, res in pairs if not res} == {0, 2, 5}
    assert {e for e, res in pairs if res} == {0, 1, 4, 5, 6}
    assert not {3, 7} & {e for e, _ in pairs}
    assert all(n % 8 == 0 for _, n, _ in K.EXISTING_STORE_SHAPES) and max(r for _, _, r in K.EXISTING_ALL_MODES) == 131


def test_the_case_with_the_alignment_only_stage_and_why_no_full_tile_is_one():
    c = next(c for c in CASES if c.why == "last stage from the alignment alone")
    assert (c.m, c.mode, c.e, K.tile_cols(c.P, 1)) == (126, "f", 3, 3)
    assert K.store_kt("f", 126, c.P, 1) == 192 and K.store_kt("f", 126, c.P, 1, e=0) == 128
    assert K.store_kt("f", 126, c.P, 0) == 448 == 320 + 125 + 3  # (the issue's example: the full tile's window ends on the stage's edge)
    for mode in "vsf":
        for m in range(64, 1200):
            assert K.store_kt(mode, m, 320, 0) == K.store_kt(mode, m, 320, 0, e=0), (mode, m)


def test_the_skip_test_is_mixed_and_the_grid_decode_covers_every_tile_once():
    c = next(c for c in CASES if c.why == "m=64 full tile: skip test mixed")
    assert K.skip_is_mixed(c) and c.m == 64 and K.tile_cols(c.P, 0) == 320
    # every column of a tile that a group is skipped for has no tap there
    for st in range(c.n_stages[0]):
        for g in range(2):
            kb = st * K.BK + 32 * g
            for wn in range(4):
                for tn in range(5):
                    if K.tile_skipped(c.m, c.e, wn, tn, kb):
                        cl = 16 * (wn + 4 * tn) + np.arange(16)[:, None]
                        t = kb + np.arange(32)[None, :] - cl - c.e
                        assert not ((t >= 0) & (t < c.m)).any()
    big = next(c for c in CASES if c.rows == 577)
    n_parts = K.parts(big.P)
    seen = [K.grid_decode(b, n_parts) for b in range(K.grid_blocks(big.rows, n_parts))]
    live = [(p, rb) for p, rb in seen if rb * K.BM < big.rows]
    assert n_parts == 2 and sorted(live) == [(p, rb) for p in range(2) for rb in range(10)] and len(seen) == 32
    # (577 rows are ten row blocks: the second group of eight has two live XCD slots, each with both parts, the last holding one row)
    assert len(seen) == len(set(seen)) and [rb for _, rb in seen[16:] if rb * K.BM < big.rows] == [8, 9, 8, 9]


# ------------------------------------------------------------------------------------------------------------------------------------
# the planner
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32_form", [False, True])
def test_every_case_plans_onto_the_intended_kernel(f32_form, monkeypatch):
    from dspeed_amd.chain import plan
    from dspeed_amd.processing_chain import build_processing_chain

    if f32_form:
        monkeypatch.setenv("DSPEED_HIP_FIR_F32", "1")
    else:
        monkeypatch.delenv("DSPEED_HIP_FIR_F32", raising=False)
    kinds = set()
    for c in CASES:
        want = c.kernel(f32_form)
        kinds.add(want)
        for family in FAMILIES:
            recipe, names = K.recipe(c, family)
            chain, _, out = build_processing_chain(recipe, dict(K.table(c.id, family)))
            assert not chain._stages, c.id
            assert plan(chain.program, np.float32)["kernel"] == want, (c.id, family)
            assert [out[k].shape for k in names] == [(c.rows, K.out_len(c.mode, m, c.n)) if c.form == "store" else (c.rows,) for m in c.ms]
            if K.has_call(c):
                assert plan(K.call_program(c, family), np.float32)["kernel"] == want, (c.id, family)
        if "unaligned offset" in K.classes(c):
            assert want == "dsp_fir_store_kernel" and K.takes_matrix_core(c.tag, c.lo, c.row_len) and (c.lo * 2) % 16 == 8
    assert kinds == ({"dsp_fir_store_kernel", "dsp_fir_mfma_kernel"} if f32_form else {"dsp_fir_f16_kernel", "dsp_fir_store_kernel"})
    assert sum(K.has_call(c) for c in K.store_cases()) >= 30


# ------------------------------------------------------------------------------------------------------------------------------------
# the two families
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_taps_are_what_the_families_say():
    for m in sorted({m for c in CASES for m in c.ms}):
        k = K.taps("exact", m).astype(np.int64)
        assert np.array_equal(k, K.taps("exact", m)) and len(set(np.abs(k))) == m and np.abs(k).max() == 1023
        assert (np.sign(k[:-1]) == (-1) ** np.arange(m - 1)).all() and (k[0], k[-1]) == (1023, -1022) and sorted(np.abs(k))[-2:] == [1022, 1023]
        f = K.taps("fraction", m)
        assert f.dtype == np.float32 and (np.abs(f) >= 0.5).all() and (np.abs(f) <= 1).all() and 0.3 < (f > 0).mean() < 0.7
        hi, lo = K.split16(k[None, :], K.pow2_scale(k[None, :]))
        assert not lo.any()
        hi, lo = K.split16(f[None, :], K.pow2_scale(f[None, :]))
        assert (lo != 0).mean() > 0.9


@pytest.mark.parametrize("case_id", IDS)
def test_the_rows_are_what_the_families_say(case_id):
    c = K.by_id(case_id)
    for family in FAMILIES:
        t = K.table(case_id, family)
        wf, x = t["waveform"], K.filtered_input(case_id, family)
        assert wf.shape == (c.rows, c.row_len) and wf.dtype == K.ROW_TYPES[c.tag] and x.shape == (c.rows, c.n) and x.dtype == np.float32
        assert ("baseline" in t) == (c.bl == "col")
        fin = K.finite_rows(case_id, family)
        if c.nonfinite:
            assert not fin[4] and not fin[5] and fin.sum() == c.rows - 2
            if c.tag == "f32":
                assert np.isnan(x[4]).all() if c.bl != "none" else (np.isnan(x[4, -1]) and np.isfinite(x[4, :-1]).all())
                assert x[5, 0] == np.inf and np.isfinite(x[5, 1:]).all()
        else:
            assert fin.all()
        hi, lo = K.split16(x[fin], K.pow2_scale(x[fin]))
        if family == "exact":
            assert np.array_equal(x[fin], np.rint(x[fin])) and np.abs(x[fin]).max() <= 4 and not lo.any()
            if c.bl != "none" and c.tag != "f32":
                assert (np.abs(wf.astype(np.int64) - K.PEDESTAL) <= 10).all()  # (the pedestal the baseline takes off)
            if c.bl == "none":
                assert np.abs(wf[fin].astype(np.float64)).max() <= 4
        else:
            assert (lo != 0).mean() > 0.5  # (the rows' lo plane takes part)
        if c.rows >= 8 and family == "exact":
            assert np.count_nonzero(x[0]) == 1 and x[0, 0] != 0 and np.count_nonzero(x[1]) == 1 and x[1, -1] != 0
            assert (x[3] == x[3, 0]).all() and x[3, 0] != 0 and not x[2].any()
        if family == "fraction":  # spread over [-1, 1] times the type's amplitude, about zero
            amp = {"f32": 1.0, "i16": 30000.0, "u16": 29450.0}[c.tag]
            assert 0.9 * amp < np.abs(x[fin]).max() <= amp + 101 and abs(x[fin].mean()) < 0.1 * amp


@pytest.mark.parametrize("case_id", IDS)
def test_exact_family_is_an_integer_below_2_24_in_any_order(case_id):
    c = K.by_id(case_id)
    fin = K.finite_rows(case_id, "exact")
    x = K.filtered_input(case_id, "exact")
    for m, (want, peak, conv) in zip(c.ms, K.expect(case_id, "exact")):
        assert want.dtype == np.int64 and np.abs(want).max() < 2 ** 24 and 4 * 1023 * max(c.ms) < 2 ** 24
        assert np.abs(x[fin]).astype(np.float64).max() * np.abs(K.taps("exact", m)).astype(np.float64).sum() < 2 ** 24  # (every partial sum, any order)
        assert np.array_equal(conv[fin].astype(np.int64), want[fin]) and np.array_equal(conv[fin], conv[fin].astype(np.int64))
        assert (peak[fin] > 0).sum() >= fin.sum() - 1  # (all but the row of zeros)
        if c.nonfinite:  # the oracle's rows with a NaN are NaN throughout; an infinity leaves the outputs it does not meet finite
            assert np.isnan(conv[4]).all() and not np.isfinite(conv[5]).all()
            d = K.dshift(c.mode, m)  # (the slice's first sample meets the outputs max(0, d - m + 1) .. d; a baseline of +inf every output)
            meets = np.zeros(conv.shape[1], dtype=bool)
            meets[max(0, d - m + 1):d + 1] = True
            assert np.array_equal(np.isfinite(conv[5]), ~meets if c.tag == "f32" else np.zeros_like(meets))


SAMPLE = [c.id for c in CASES if c.why in ("e=3 resident", "e=7 non-resident", "mode s e=7", "store slice n%8=7", "last tile 1 columns",
                                            "amax 3 kernels", "amax kend = n rounded up to 32")]


@pytest.mark.parametrize("case_id", SAMPLE)
def test_float16_form_reproduces_the_exact_family_bit_for_bit(case_id):
    c = K.by_id(case_id)
    rows = _sample_rows(c, "exact")
    x = K.filtered_input(case_id, "exact")[rows]
    for m, (want, _, _) in zip(c.ms, K.expect(case_id, "exact")):
        k = K.taps("exact", m)
        for seed, chunk in ((None, 128), (1, 256), (2, m)):
            order = None if seed is None else np.random.default_rng(seed).permutation(m)
            got = K.emulate_f16(x, k, c.mode, chunk, order)
            assert np.array_equal(got, want[rows].astype(np.float64)), (m, seed, chunk)


@pytest.mark.parametrize("case_id", IDS)
def test_fraction_family_leaves_the_float16_form_half_of_the_bar(case_id):
    """the float16 form as the kernels run it -- lo.lo dropped, a rounding per matrix instruction of 32 samples, float32 partial sums of
    128 (kept output) and 256 (amax) samples, float64 totals -- against the float64 convolution, on every finite row: at most TOL / 2 of
    the row's filtered peak.  A condition on the inputs"""
    c = K.by_id(case_id)
    rows = np.flatnonzero(K.finite_rows(case_id, "fraction"))
    x = K.filtered_input(case_id, "fraction")[rows]
    for m, (want, peak, _) in zip(c.ms, K.expect(case_id, "fraction")):
        assert want.dtype == np.float64 and (peak[rows] > 0).all()
        scale = peak[rows, None]
        for chunk in (128, 256):
            got = K.emulate_f16_mfma(x, K.taps("fraction", m), c.mode, chunk)
            worst = np.max(np.abs(got - want[rows]) / scale)
            assert worst <= 0.5 * K.TOL, (m, chunk, worst)
        # a misplaced lo operand would show: without the lo planes the same product misses the bar by far
        xs = K.pow2_scale(x)
        hi_only = (K.split16(x, xs)[0] / xs).astype(np.float32)
        coarse = K.convolve_rows(hi_only, K.taps("fraction", m), c.mode, np.float64)
        assert np.max(np.abs(coarse - want[rows]) / scale) > 5 * K.TOL


@pytest.mark.parametrize("case_id", IDS)
def test_fraction_family_leaves_the_float32_forms_room_too(case_id):
    """The float32 forms round once per fused multiply-add at most (the model here: once per sample) into partial sums of 64 (kept output)
    and 128 (amax) samples; the float32 result adds 2^-24 of the value.  Where the model stays below 0.75 TOL the device has a quarter of
    the bar to spare.  A condition on the inputs as well"""
    c = K.by_id(case_id)
    rows = np.flatnonzero(K.finite_rows(case_id, "fraction"))
    x = K.filtered_input(case_id, "fraction")[rows]
    for m, (want, peak, _) in zip(c.ms, K.expect(case_id, "fraction")):
        got = K.emulate_f32_chain(x, K.taps("fraction", m), c.mode, K.SCHUNK if c.form == "store" else K.KCHUNK)
        worst = np.max(np.abs(got - want[rows]) / peak[rows, None])
        assert worst <= 0.75 * K.TOL, (m, worst)


def test_the_processors_cache_keys_on_every_switch_the_planner_reads():
    """a processor call keeps its planned chain by the program (dsp_gufuncs.cpp); the plan depends on the environment switches read while
    planning as well (DSPEED_HIP_FIR_F32 decides between the two forms here): dsp_plan_switches names every one of them"""
    with open(os.path.join(CSRC, "dsp_plan.cpp")) as f:
        src = f.read()
    body = src[src.index("uint64_t dsp_plan_switches()"):]
    listed = set(re.findall(r'"(DSPEED_HIP_\w+)"', body[:body.index("}")]))
    read = set(re.findall(r'getenv\("(DSPEED_HIP_\w+)"\)', src))
    assert read and read == listed, read ^ listed
    with open(os.path.join(CSRC, "dsp_gufuncs.cpp")) as f:
        assert "key.v.push_back((int64_t)dsp_plan_switches());" in f.read()


# ------------------------------------------------------------------------------------------------------------------------------------
# non-vacuity
# ------------------------------------------------------------------------------------------------------------------------------------
def _group_delta(x, kr, d, cols, samples):
    """what the samples ``samples`` contribute to the output columns ``cols``: column c multiplies sample i by reversed tap i - c + d"""
    out = np.zeros((len(x), len(cols)), dtype=np.int64)
    for a, cl in enumerate(cols):
        for i in samples:
            if 0 <= i < x.shape[1] and 0 <= i - cl + d < len(kr):
                out[:, a] += x[:, i] * kr[i - cl + d]
    return out


@pytest.mark.parametrize("case_id", IDS)
def test_a_wrong_tap_or_a_skipped_group_changes_the_exact_expectation(case_id):
    c = K.by_id(case_id)
    fin = K.finite_rows(case_id, "exact")
    x = K.filtered_input(case_id, "exact")[fin].astype(np.int64)
    for m, (want, _, _) in zip(c.ms, K.expect(case_id, "exact")):
        k = K.taps("exact", m).astype(np.int64)
        want = want[fin]
        final = (lambda a: a.max(axis=1)) if c.form == "amax" else (lambda a: a)
        shifted, no_first, no_last = np.concatenate([[0], k[:-1]]), k.copy(), k.copy()
        no_first[0] = no_last[-1] = 0
        for name, wrong in (("shifted", shifted), ("k[0] dropped", no_first), ("k[m-1] dropped", no_last)):
            assert not np.array_equal(final(K.convolve_rows(x, wrong, c.mode, np.int64)), final(want)), (m, name)
        # one (column tile, 32-sample group) pair of the first tile left out
        d = K.dshift(c.mode, m)
        e = K.align_e(c.mode, m) if c.form == "store" else 0
        ks = -d - e if c.form == "store" else 0
        P = want.shape[1]
        if c.form == "store":
            tile, kb = 0, (max(0, -ks) // 32) * 32  # the first tile's first columns; the group that holds the rows' first sample
        else:
            col = int(want[min(6, len(want) - 1)].argmax())  # the tile that holds the maximum of the first seeded row; its first group
            tile, kb = col // 16, (col // 32) * 32
        assert not K.tile_skipped(m, e, tile % 4, tile // 4, kb)
        cols = [cl for cl in range(16 * tile, 16 * tile + 16) if cl < min(P, K.BN)]
        holed = want.copy()
        holed[:, cols] -= _group_delta(x, k[::-1], d, cols, range(ks + kb, ks + kb + 32))
        assert not np.array_equal(final(holed), final(want)), (m, "group", tile, kb)

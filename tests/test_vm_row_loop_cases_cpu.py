"""Do the cases of vm_row_loop_cases.py say something?  On the planner (which needs no device) and the oracle alone: every program is
the interpreter's, with the team intended; the programs whose slots are meant to take over each other's LDS do; between them the
programs hold every opcode of the interpreter's switch; the probes give finite, varied outputs and every poison kind shows in its own
row.  If a changed generator breaks a condition here, the generator is what changes."""
import os
import re

import numpy as np
import pytest

import vm_row_loop_cases as V
from dspeed_amd import _lib
from dspeed_amd.chain import plan

CASES = V.cases()
IDS = [c.name for c in CASES]
HERE = os.path.dirname(os.path.abspath(__file__))


def _planned(case):
    with V.switches(case.env):
        chain, _out = case.build()
        return chain.program, plan(chain.program, case.ft)


def _finite_rows(v):
    v = np.asarray(v)
    return np.isfinite(v.reshape(len(v), -1)).all(axis=1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_program_is_the_interpreter_s(case):
    program, info = _planned(case)
    assert info["kernel"].startswith("dsp_vm_kernel"), info["kernel"]
    assert info["lds_bytes_per_wave"] == case.ft.itemsize * info["lds_elems_per_wave"], info  # (the float64 loop's build for program 6)
    assert info["team"] == case.team, info
    if case.name == "p5-team3-wpb4-8192":
        assert info["waves_per_block"] == 4, info  # (row slots per workgroup: twelve wavefronts)
    if case.program == 3:
        assert _lib.OP_CONVOLVE in [o[0] for o in program.ops]  # (the build with the FIR op)


def test_the_switches_leave_the_environment_as_it_was(monkeypatch):
    monkeypatch.setenv("DSPEED_HIP_TEAM_MAX", "3")
    monkeypatch.delenv("DSPEED_HIP_NO_FUSED", raising=False)
    with V.switches({"DSPEED_HIP_NO_TEAMS": "1"}):
        assert os.environ["DSPEED_HIP_NO_FUSED"] == "1" and os.environ["DSPEED_HIP_NO_TEAMS"] == "1" and "DSPEED_HIP_TEAM_MAX" not in os.environ
    assert os.environ["DSPEED_HIP_TEAM_MAX"] == "3" and "DSPEED_HIP_NO_FUSED" not in os.environ and "DSPEED_HIP_NO_TEAMS" not in os.environ


@pytest.mark.parametrize("case", [c for c in CASES if c.program in (1, 2, 3)], ids=[c.name for c in CASES if c.program in (1, 2, 3)])
def test_slots_take_over_each_other_s_regions(case):
    """two slots whose [base, base + elems) overlap: the later one finds what the earlier one's last row left (DSP_OP_INTERNAL_ZERO); the
    planner adds one device op per slot that shares"""
    program, info = _planned(case)
    slots = info["slots"]
    pairs = [(a, b) for i, a in enumerate(slots) for b in slots[i + 1:] if a["base"] < b["base"] + b["elems"] and b["base"] < a["base"] + a["elems"]]
    assert pairs, slots
    for a, b in pairs:
        assert a["last_op"] < b["first_op"] or b["last_op"] < a["first_op"], (a, b)  # (never at the same time)
    if case.program == 2:
        assert any(a["chunk"] != b["chunk"] for a, b in pairs), pairs


def test_the_programs_hold_every_opcode_of_the_interpreter():
    held = set()
    for case in CASES:
        held |= {o[0] for o in _planned(case)[0].ops}
    names = {getattr(_lib, k): k for k in dir(_lib) if k.startswith("OP_")}
    assert sorted(held) == V.INTERPRETER_OPCODES, sorted(names[o] for o in held ^ set(V.INTERPRETER_OPCODES))
    # the list is the switch's: every `case DSP_OP_X` of dsp_vm.hip that is not host-made (DSP_OP_INTERNAL_*) is an opcode of the C header
    with open(os.path.join(HERE, "..", "dspeed_amd", "csrc", "dsp_vm.hip")) as f:
        labels = set(re.findall(r"case DSP_OP_([A-Z_]+):", f.read()))
    with open(os.path.join(HERE, "..", "include", "dspeed_hip.h")) as f:
        header = dict(re.findall(r"#define DSP_OP_([A-Z_]+) +(\d+)", f.read()))
    public = {k for k in labels if not k.startswith("INTERNAL_")}
    assert labels - public == {"INTERNAL_ZERO", "INTERNAL_STORES", "INTERNAL_NOP"}
    assert sorted(int(header[k]) for k in public) == V.INTERPRETER_OPCODES, sorted(public)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probes_are_finite_and_poison_rows_show(case):
    want = case.want()
    table = case.table()
    assert all(len(v) == V.N_PROBES + len(V.POISON) for v in table.values())
    # every probe row has every output finite, but for the walks of the designated probes
    never = set(range(V.N_PROBES))
    for k, (v, _bar) in want.items():
        bad = set(np.flatnonzero(~_finite_rows(v)[:V.N_PROBES]).tolist())
        assert bad <= set(V.NO_CROSSING), (k, sorted(bad))
        never -= bad
    assert len(V.NO_CROSSING) <= 4 and never == set(range(V.N_PROBES)) - set(V.NO_CROSSING)  # (the designated ones do miss)
    # the probes are distinct rows
    wf = next(v for v in table.values() if v.ndim == 2)
    assert len(np.unique(wf[:V.N_PROBES], axis=0)) == V.N_PROBES
    # every poison kind changes an output of its own row (a copy of probe 0 but for the poison) to NaN, an infinity or 0 -- or, the row of
    # denormals, to a denormal: the value that arithmetic which flushes to zero would lose
    tiny = np.finfo(case.ft).tiny
    for j, kind in enumerate(V.POISON):
        if not case.float_rows and kind in V.FLOAT_ONLY:
            continue  # (an integer row holds the extremes it can in their place: rows that differ from every probe)
        r = V.N_PROBES + j
        shown = [k for k, (v, _bar) in want.items()
                 if ((~np.isfinite(np.asarray(v)[r])) | (np.abs(np.asarray(v)[r]) < (tiny if kind == "denormal" else 0) ) | (np.asarray(v)[r] == 0)).any()
                 and not ((~np.isfinite(np.asarray(v)[0])) | (np.asarray(v)[0] == 0)).any()]
        assert shown, (case.name, kind)
    # walks and pick-offs land on at least 8 different samples across the probes
    landed = {k: np.asarray(v)[:V.N_PROBES] for k, (v, bar) in want.items()
              if bar == "exact" and np.asarray(v).ndim == 1 and (k.startswith("tp") or k.startswith("t_"))}
    landed.update({k: np.floor(v[:V.N_PROBES]) for k, v in table.items() if k in ("t_pick", "t_int")})
    assert landed, list(want)
    for k, v in landed.items():
        assert len(np.unique(v[np.isfinite(v)])) >= 8, (k, np.unique(v))


def test_the_layout_is_the_one_the_gpu_test_reads():
    for S in (64, 999, 3072):
        idx = V.layout(S)
        assert len(idx) == 3 * S + S // 2
        assert np.array_equal(idx[:S], np.arange(S) % V.N_PROBES) and np.array_equal(idx[2 * S:3 * S], idx[:S])
        assert np.array_equal(idx[S:2 * S], V.N_PROBES + np.arange(S) % len(V.POISON))
        assert (idx[3 * S:] < V.N_PROBES).all() and (idx[3 * S:] != idx[:S // 2]).all()
        pairs = set(zip(idx[:S].tolist(), idx[S:2 * S].tolist()))
        if S >= V.N_PROBES * len(V.POISON):
            assert len(pairs) == V.N_PROBES * len(V.POISON)  # (every probe is followed by every kind of poison somewhere)
    assert V.rows_per_round({"blocks": 256, "waves_per_block": 12}, 3) == 1024

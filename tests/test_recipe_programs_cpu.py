"""Translation of recipes, pinned: every case of ``tests/recipe_program_cases.py`` is built again on the CPU (``build_processing_chain`` needs
the library for the planner and nothing of a device) and what it gives -- the device programs of the chain, of its stages, tail, head and walks,
with every operand; the fit descriptors; bindings, constants, output buffers -- or the error it raises is compared with
``tests/golden/recipe_programs.json.gz``, EXACTLY.  The fixture was recorded once (``tools/record_recipe_programs.py``) from the code as it stood
before ``dspeed_amd/language.py`` got typed operands and one evaluator method per syntax node (profiles/r14_language.md names the commit): a
slip in the order in which sub-expressions are evaluated, slots and registers are handed out or operands are converted shows here as the first
op that differs, not as a wrong number on the device.  It is recorded again only when a recipe is meant to translate differently."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import recipe_program_cases as book

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "recipe_programs.json.gz")


def make_table(spec):
    """the table of a case: zeros of the recorded shapes and types; an integer column holds its first value and its maximum (what translation
    reads of a ``len(...)`` column or of a grouped integer parameter)"""
    from dspeed_amd.device import DeviceArray
    from dspeed_amd.processing_chain import WaveformInput

    if spec is None:
        return None
    tb = {}
    for name, col in spec.items():
        kind = col[0]
        if kind == "W":
            _k, shape, dtype, dt, t0 = col
            t0 = np.zeros(shape[0], dtype=t0[0]) if isinstance(t0, tuple) else t0
            tb[name] = WaveformInput(np.zeros(shape, dtype=dtype), dt, t0)
        elif kind == "D":  # (a column on the device: only its shape and type are looked at)
            tb[name] = DeviceArray.from_ptr(64, col[1], col[2])
        else:
            a = np.zeros(col[1], dtype=col[2])
            if len(col) > 3 and a.size:
                a[...] = col[3]
                a[-1] = col[4]
            tb[name] = a
    return tb


def _array(a):
    a = np.ascontiguousarray(a)
    return [a.dtype.str, list(a.shape), hashlib.sha1(a.tobytes()).hexdigest()]


def _program(p):
    if p is None:
        return None
    return {"ops": [[opcode, dst, src, io, list(ip), [[s.kind, s.index, float(s.value).hex()] for s in sp]] for opcode, dst, src, io, ip, sp in p.ops],
            "io": [list(x) for x in p.io], "slots": list(p.slots), "n_sregs": p.n_sregs}


def _split(record):
    return None if record is None else {"program": _program(record["program"]), "handover": list(record["handover"])}


def _plain(x):
    """JSON's view of a descriptor: tuples as lists, NumPy numbers as Python's, types by name"""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.dtype) or isinstance(x, type):
        return str(np.dtype(x))
    if isinstance(x, np.generic):
        return x.item()
    return x


def describe(chain, mask, tb_out):
    out_vars = {nm: [v.name, str(np.dtype(v.dtype)), length, str(getattr(v, "table_dtype", None))] for nm, (v, length) in chain._out_vars.items()}
    stages = [{"what": st["what"], "program": _program(st["program"]), "outs": _plain(st["outs"]), "alias": _plain(st["alias"]),
               "consts": {k: _array(v) for k, v in st["consts"].items()}, "in_vars": {k: v.source for k, v in st["in_vars"].items()},
               "out_dtypes": _plain(st.get("out_dtypes", {})), "compute": _plain(st.get("compute"))} for st in chain._stages]
    return {"class": type(chain).__name__, "group_columns": list(getattr(chain, "group_columns", [])), "mask": list(mask),
            "loop_dtype": str(chain.loop_dtype), "program": _program(chain._program), "stages": stages, "tail": _split(chain._tail),
            "walks": _split(chain._walks), "fits": _plain(chain._aux), "in_vars": {k: v.source for k, v in chain._in_vars.items()},
            "out_vars": out_vars, "ext_alias": _plain(chain._ext_alias), "vector_lens": _plain(chain.vector_lens),
            "hidden_outputs": list(chain.hidden_outputs), "output_attrs": _plain(chain.output_attrs), "copy_pars": list(chain._copy_pars),
            "consts": {k: _array(v) for k, v in chain._consts.items()},
            "tb_out": {k: [str(v.dtype), list(v.shape)] for k, v in tb_out.items()}, "proc_strings": list(chain.proc_strings)}


def build_case(case):
    """what the case translates to (``describe``), or {"raises": class, "message": text}"""
    from dspeed_amd import build_processing_chain

    _name, recipe, outputs, table, db_dict, switches = case
    if isinstance(recipe, str) and recipe.startswith("@"):  # "@NAME" / "@name()": of tests/recipes.py
        recipe = getattr(book.recipes, recipe[1:-2])() if recipe.endswith("()") else getattr(book.recipes, recipe[1:])
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        chain, mask, tb_out = build_processing_chain(recipe, make_table(table), db_dict, outputs)
        return describe(chain, mask, tb_out)
    except Exception as e:  # noqa: BLE001  (which one, and what it says, is the recording)
        return {"raises": type(e).__name__, "message": str(e)}
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def record_all():
    names = [c[0] for c in book.CASES]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {c[0]: json.loads(json.dumps(build_case(c))) for c in book.CASES}


def _first_difference(want, got, path=""):
    """where two recordings first differ, as a path into them (an op of a program by its number)"""
    if type(want) is not type(got):
        return f"{path}: recorded {want!r}, now {got!r}"
    if isinstance(want, dict):
        for k in list(want) + [k for k in got if k not in want]:
            if k not in want or k not in got:
                return f"{path}/{k}: {'not recorded' if k not in want else 'missing now'}"
            d = _first_difference(want[k], got[k], f"{path}/{k}")
            if d:
                return d
        return None
    if isinstance(want, list):
        for i, (w, g) in enumerate(zip(want, got)):
            d = _first_difference(w, g, f"{path}[{i}]")
            if d:
                return d
        return None if len(want) == len(got) else f"{path}: {len(want)} entries recorded, {len(got)} now"
    return None if want == got else f"{path}: recorded {want!r}, now {got!r}"


def test_every_recipe_translates_to_the_recorded_programs():
    with gzip.open(GOLDEN, "rt") as f:
        golden = json.load(f)
    got = record_all()
    assert list(got) == list(golden), sorted(set(got) ^ set(golden))
    compared, differ = 0, []
    for name, want in golden.items():
        compared += 1
        if got[name] != want:
            differ.append(f"{name}: {_first_difference(want, got[name])}")
    assert not differ, "\n".join([f"{len(differ)} cases differ from tests/golden/recipe_programs.json.gz:"] + differ[:20])
    assert compared == len(golden) == len(book.CASES)


def test_the_corpus_holds_every_recipe_and_every_switch():
    """every recipe of tests/recipes.py, the Ge recipes once more under each switch; cases that build and cases that raise"""
    names = [c[0] for c in book.CASES]
    for r in ("C1", "C2", "C2_UNITS", "C3", "c3_small", "C5", "ICPC", "ICPC_REF"):
        assert f"recipes.{r}" in names, r
    for r in ("ICPC", "ICPC_REF"):
        for switch in book.SWITCHES:
            assert f"recipes.{r} {switch}=1" in names
    with gzip.open(GOLDEN, "rt") as f:
        golden = json.load(f)
    raising = sum(1 for v in golden.values() if "raises" in v)
    assert 0 < raising < len(golden), raising


@pytest.mark.parametrize("arg", ["not 1", "~1", "np.sin(1)", "lambda: 1"])
def test_syntax_that_no_method_of_the_evaluator_takes_is_refused(arg):
    """(the two ``return self._no_parse(...)`` that no recipe of the corpus reaches, profiles/r14_language.md: an operator ``_eval_unary`` does not
    know, a call of something that is not a name -- refused with the text of the one final ``raise`` they came from)"""
    from dspeed_amd.errors import ProcessingChainError
    from dspeed_amd.processing_chain import _Builder

    with pytest.raises(ProcessingChainError, match="could not parse argument"):
        _Builder({}, None).eval_arg(arg)

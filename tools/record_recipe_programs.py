"""Records tests/golden/recipe_programs.json.gz: what every case of tests/recipe_program_cases.py translates to -- the device programs with every
operand, the stages, tail, head and walks, the fit descriptors, bindings, constants and output buffers (tests/test_recipe_programs_cpu.py,
``describe``) -- or the error it raises.  On the CPU; the library must be built (the translation asks the planner).

    python tools/record_recipe_programs.py [OUT.json.gz]           (zcat shows it)
    python tools/record_recipe_programs.py --trace                  lines of the evaluator and of compiler._add_step that no case runs

tests/test_recipe_programs_cpu.py compares a fresh translation with this file EXACTLY.  It was recorded from ``dspeed_amd/language.py`` and
``compiler.py`` as they stood before operands got types (profiles/r14_language.md names the commit) and is recorded again only when a recipe
is meant to translate differently -- never to make a failing comparison pass.

``--trace`` runs the corpus under the standard library's ``trace`` module and prints every executable line of ``language.py`` from
``class _Builder`` to the end of the file, and of ``compiler._add_step``, that did not run."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_recipe_programs_cpu as T  # noqa: E402


def _traced_ranges():
    """{file: (first line, last line)} of what the corpus has to cover"""
    import dspeed_amd.compiler as compiler
    import dspeed_amd.language as language

    lang = open(language.__file__).read().splitlines()
    comp = open(compiler.__file__).read().splitlines()
    first = next(i for i, s in enumerate(comp, 1) if s.startswith("def _add_step("))
    last = next(i for i, s in enumerate(comp, 1) if i > first and s and not s[0].isspace() and not s.startswith("def _add_step(")) - 1
    return {language.__file__: (next(i for i, s in enumerate(lang, 1) if s.startswith("class _Builder")), len(lang)),
            compiler.__file__: (first, last)}


def trace_corpus():
    import trace

    tracer = trace.Trace(count=1, trace=0)
    tracer.runfunc(T.record_all)
    counts = tracer.results().counts
    missed = 0
    for path, (lo, hi) in _traced_ranges().items():
        executable = {n for n in trace._find_executable_linenos(path) if lo <= n <= hi}
        lines = open(path).read().splitlines()
        for n in sorted(executable):
            if (path, n) not in counts and not lines[n - 1].lstrip().startswith(('"""', "def ", "class ", "@")):
                missed += 1
                print(f"{os.path.relpath(path, ROOT)}:{n}: {lines[n - 1].strip()[:150]}")
        print(f"-- {os.path.relpath(path, ROOT)}:{lo}-{hi}: {len(executable)} executable lines")
    print(f"{missed} lines did not run")


def main():
    if "--trace" in sys.argv[1:]:
        trace_corpus()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    text = json.dumps(T.record_all(), indent=0, separators=(",", ":"))
    with open(out, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:  # (no name, no time: the same bytes every time)
        z.write(text.encode())
    n_raise = text.count('"raises":')
    print(f"{len(T.book.CASES)} cases ({n_raise} raise) -> {out} ({len(text)} bytes, {os.path.getsize(out)} compressed)")


if __name__ == "__main__":
    main()

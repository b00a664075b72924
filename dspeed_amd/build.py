"""Builds libdspeed_hip.so (the HIP kernels + C ABI) in-tree for gfx950.

    python -m dspeed_amd.build [--force]

hipcc cross-compiles without a GPU; the resulting .so is git-ignored but travels with the tree.

    python -m dspeed_amd.build --diag

builds libdspeed_hip_diag.so beside it: the same sources with -DDSPEED_HIP_DIAG, which compiles the kernels' diagnostic switches
in (DSPEED_HIP_ABLATE: skip passes / per-phase cycle stamps).  The product library does not contain them; tools select the
diagnostic one with DSPEED_HIP_LIB=.../libdspeed_hip_diag.so.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdspeed_hip.so")
LIB_DIAG = os.path.join(HERE, "libdspeed_hip_diag.so")
SOURCES = ["dsp_vm.hip", "dsp_energy.hip", "dsp_energy_h.hip", "dsp_fit.hip", "dsp_rows.hip", "dsp_current.hip", "dsp_scalar.hip", "dsp_reduce.hip", "dsp_extrema.hip", "dsp_hist.hip", "dsp_thresh.hip", "dsp_spectrum.hip", "dsp_sort.hip", "dsp_interp.hip", "dsp_dense.hip", "dsp_reflect.hip", "dsp_pileup.hip", "dsp_tailfit.hip", "dsp_align.hip", "dsp_pulses.hip", "dsp_svm.hip", "dsp_pz.hip", "dsp_fir_mfma.hip", "dsp_fir_f16.hip", "dsp_fir_runs.hip", "dsp_plan.cpp", "dsp_host.cpp", "dsp_gufuncs.cpp"]
DEPS = SOURCES + ["dsp_program.h", "dsp_kernels.h", "dsp_launch.h", "dsp_plan.h", "dsp_gufuncs.h", "dsp_wave.h", "dsp_reduce_tail.h", "dsp_row_stream.h", "dsp_lane_tiles.h", "dsp_spectrum_tables.h", os.path.join("..", "..", "include", "dspeed_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall",
         "-Wno-unused-function"]


#: kernels that must not use scratch memory: name fragment -> why.  The waveform VM keeps its interpreter state (Ctx) in registers; it
#: lands in scratch memory -- and every op of every chain pays -- as soon as a helper that takes the state by reference is not inlined
#: (the compiler decides by size: one more branch in op_pickoff did it once, C2 on the VM 129 -> 113 M waveforms/s) or an indexed local
#: array appears.  The build fails rather than ship that.
NO_SCRATCH = {"dsp_vm.hip": "dsp_vm_kernel"}


def _check_scratch(src: str, remarks: str) -> None:
    frag, name, bad = NO_SCRATCH[src], None, []
    for line in remarks.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif "ScratchSize [bytes/lane]:" in line and name and frag in name:
            n = int(line.split("ScratchSize [bytes/lane]:")[1].split()[0])
            if n:
                bad.append((name, n))
    skip = 0
    for line in remarks.splitlines():  # (the compiler's other diagnostics stay visible; a remark is followed by its source excerpt)
        if "remark:" in line:
            skip = 2
        elif skip and (line.lstrip()[:1].isdigit() or line.lstrip().startswith("|")):
            skip -= 1
        else:
            skip = 0
            sys.stderr.write(line + "\n")
    if bad:
        raise RuntimeError(f"{src}: scratch memory in " + ", ".join(f"{n} ({b} B/lane)" for n, b in bad) +
                           " -- a helper taking Ctx& was outlined, or a local array is indexed at run time (see NO_SCRATCH in build.py)")


#: kernels whose code must hold none of the listed instructions: source -> (name fragment, mnemonics, why).  The register-resident
#: energy kernel reads and writes LDS 8 bytes a lane because ds_read_b64 costs the LDS array 2 cycles; hipcc fuses two neighbouring ones
#: into ds_read2_b64 / ds_write2_b64, which the array serves at the 4-byte rate (8 cycles for 16 bytes), and only RR_NO_MERGE in
#: dsp_energy.hip keeps it from doing so.  Every test passes either way and the kernel is 2 % slower: the build fails rather than ship that.
#: (dsp_energy_h.hip is dsp_energy.hip's second translation unit: the same kernel built for the 4-point pick-off mode)
RR_NO_FUSED_LDS = {src: ("dsp_energy_rr_kernel", ("ds_read2_b64", "ds_write2_b64"),
                         "RR_NO_MERGE no longer keeps neighbouring 8-byte LDS accesses apart (see dsp_energy.hip)")
                   for src in ("dsp_energy.hip", "dsp_energy_h.hip")}


def _llvm_tool(name: str) -> str | None:
    """a tool of the LLVM that hipcc drives (beside its clang), or None"""
    roots = [os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "llvm", "bin"),
             os.path.join(os.path.dirname(os.path.realpath(_hipcc())), "..", "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"]
    for r in roots:
        if os.path.exists(os.path.join(r, name)):
            return os.path.join(r, name)
    return shutil.which(name)


def _check_instructions(src: str, obj: str) -> None:
    """disassembles the gfx950 code of `obj` and counts the mnemonics RR_NO_FUSED_LDS bars in the kernels it names"""
    import re
    import tempfile

    frag, barred, why = RR_NO_FUSED_LDS[src]
    tools = [_llvm_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if os.environ.get("DSPEED_HIP_NO_ISA_CHECK") == "1":  # the explicit way round it, for a host whose ROCm lacks the LLVM tools
        sys.stderr.write(f"{src}: instruction check skipped (DSPEED_HIP_NO_ISA_CHECK=1)\n")
        return
    if None in tools:
        raise RuntimeError(f"{src}: cannot check the kernels' instructions: llvm-objcopy / clang-offload-bundler / llvm-objdump not found beside "
                           "hipcc's clang or on PATH (they ship with ROCm's LLVM; DSPEED_HIP_NO_ISA_CHECK=1 builds without the check)")
    objcopy, bundler, objdump = tools
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        subprocess.check_call([objcopy, f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
        subprocess.check_call([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
        asm = subprocess.run([objdump, "-d", co], check=True, stdout=subprocess.PIPE, text=True).stdout
    name, seen, bad = None, 0, {}
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1) if frag in m.group(1) else None
            seen += name is not None
        elif name:
            for op in barred:
                if re.search(rf"\b{op}\b", line):
                    bad[name] = bad.get(name, 0) + 1
    if not seen:
        raise RuntimeError(f"{src}: no {frag} in the disassembly -- the instruction check looks at nothing (RR_NO_FUSED_LDS in build.py)")
    if bad:
        raise RuntimeError(f"{src}: {' / '.join(barred)} in " + ", ".join(f"{n} ({c})" for n, c in sorted(bad.items())) + f" -- {why}")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm)")


def _stamp(diag: bool) -> str:
    """what a library was built from: the compiler flags, the scratch guard and the content of every source and header"""
    import hashlib

    h = hashlib.sha256(repr((FLAGS, sorted(NO_SCRATCH.items()), sorted(RR_NO_FUSED_LDS.items()), diag)).encode())
    for d in DEPS:
        with open(os.path.join(CSRC, d), "rb") as f:
            h.update(d.encode() + b"\0" + f.read())
    return h.hexdigest()


def _stamp_file(lib: str) -> str:
    return lib + ".stamp"


def needs_build(lib: str = LIB) -> bool:
    """True unless `lib` exists and was built from exactly these sources with exactly these flags (a stamp file beside it says so)"""
    if not os.path.exists(lib) or not os.path.exists(_stamp_file(lib)):
        return True
    with open(_stamp_file(lib)) as f:
        return f.read().strip() != _stamp(lib == LIB_DIAG)


def build(force: bool = False, verbose: bool = False, diag: bool = False, variant: str | None = None, defines=(), extra_flags=()) -> str:
    """``variant`` / ``defines``: an experiment library libdspeed_hip_<variant>.so compiled with -D<define>... beside the product one
    (A/B runs of kernel variants in one GPU session: tools select it with DSPEED_HIP_LIB); always rebuilt."""
    lib = LIB_DIAG if diag else LIB
    if variant:
        lib = os.path.join(HERE, f"libdspeed_hip_{variant}.so")
        force = True
    if not force and not needs_build(lib):
        return lib
    # one hipcc process per source (they are independent translation units), then a link: the wall time of the longest file
    objs, procs = [], []
    for src in SOURCES:
        obj = os.path.join(CSRC, "." + src + (f".{variant}.o" if variant else (".diag.o" if diag else ".o")))
        cmd = [_hipcc(), *[f for f in FLAGS if f != "-shared"], *(["-DDSPEED_HIP_DIAG"] if diag else []), *[f"-D{d}" for d in defines], *extra_flags, "-x", "hip", "-c",
               os.path.join(CSRC, src), "-o", obj]
        guard = src in NO_SCRATCH
        if guard:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE if guard else None, text=True if guard else None), src))
        objs.append(obj)
    failed = None
    try:
        for cmd, p, src in procs:
            err = p.communicate()[1] if src in NO_SCRATCH else None
            if p.wait() != 0:
                if err:
                    sys.stderr.write(err)
                raise subprocess.CalledProcessError(p.returncode, cmd)
            if err is not None:
                _check_scratch(src, err)
            if src in RR_NO_FUSED_LDS:
                _check_instructions(src, objs[SOURCES.index(src)])
    except BaseException as e:
        failed = e
    if failed is not None:  # stop the compiles still running and leave no object behind for a later link to pick up
        for _cmd, p, _src in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for obj in objs:
            if os.path.exists(obj):
                os.remove(obj)
        raise failed
    link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", lib]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    if variant:
        for obj in objs:
            os.remove(obj)
        return lib
    with open(_stamp_file(lib), "w") as f:
        f.write(_stamp(diag) + "\n")
    return lib


if __name__ == "__main__":
    _variant = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    _defines = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--define"]
    _flags = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--flag"]  # raw compiler flags of an experiment library
    print(build(force="--force" in sys.argv, verbose=True, diag="--diag" in sys.argv, variant=_variant, defines=_defines, extra_flags=_flags))

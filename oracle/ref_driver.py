"""TEST INFRASTRUCTURE ONLY -- the one recipe by which a tests/golden/ref_*_driver.c (calls into the reference, no reference code) becomes a
library: compiled against the reference's headers where they lie and linked with the reference objects that oracle/build_ref.sh leaves in
oracle/_ref/obj_all.  The fixture generators (tests/golden/make_golden_*.py), tests/rate_util.py and through them the live *_vs_ref tests
and the CPU yardsticks of tools/*_probe.py build their drivers here.  Importing this module does nothing: where the reference is absent (the
GPU box) reference_available() is false and nobody calls build_driver."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get("SVT_REFERENCE_ROOT", "/root/reference")
OBJ_ALL = os.path.join(ROOT, "oracle", "_ref", "obj_all")
INCLUDE_DIRS = [os.path.join(REF_ROOT, "Source", d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1",
                                                              "Lib/ASM_AVX2")]


def reference_available():
    return os.path.isdir(os.path.join(REF_ROOT, "Source", "Lib", "Codec")) and os.path.isdir(OBJ_ALL) and bool(os.listdir(OBJ_ALL))


def build_driver(source, out_dir, *, leave_out=(), weaken=None, include=()):
    """Compile `source` and link it with the reference objects into out_dir/lib<source's base name>.so; returns the ctypes.CDLL.
    The roots are the exported drv_* functions and --gc-sections drops what they do not reach.  The driver defines the RTCD pointers
    itself, so the encoder's EbEncHandle.o is always left out; `leave_out` names further objects (a driver that includes a reference
    source to reach its statics stands in for that object).  `weaken` maps an object to symbols made weak in a copy of it under out_dir,
    linked in its place, so that the driver's definitions of them win.  What stays undefined after a first link -- functions that exist
    only in the reference's NASM sources, whose addresses setup_rtcd_internal stores and nothing here calls -- is made a weak reference
    in the driver object, which resolves to NULL, and the library is linked again and loaded with lazy binding.  `include`: further -I."""
    at = lambda name: os.path.join(out_dir, name)  # noqa: E731
    obj, wobj, vmap, weak = at("drv.o"), at("drv_weak.o"), at("drv.map"), at("weak.txt")
    so = at(f"lib{os.path.splitext(os.path.basename(source))[0]}.so")
    inc = [f"-I{d}" for d in (*INCLUDE_DIRS, *include)]
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-w", "-mavx2", "-fPIC", "-ffunction-sections", "-fdata-sections", *inc, "-c", source, "-o", obj])
    with open(vmap, "w") as f:
        f.write("{ global: drv_*; local: *; };\n")
    objs = {o: os.path.join(OBJ_ALL, o) for o in sorted(os.listdir(OBJ_ALL)) if o.endswith(".o") and o not in ("EbEncHandle.o", *leave_out)}
    for o, symbols in (weaken or {}).items():
        objs[o] = at(o[:-2] + "_weak.o")
        subprocess.check_call(["objcopy", *[f"--weaken-symbol={s}" for s in symbols], os.path.join(OBJ_ALL, o), objs[o]])

    def link(driver):   # plain objects under --gc-sections: their order does not decide which definition is taken
        subprocess.check_call(["gcc", "-shared", "-o", so, driver, *objs.values(), "-Wl,--gc-sections", f"-Wl,--version-script={vmap}", "-lm", "-lpthread"])

    link(obj)
    und = subprocess.check_output(["nm", "-D", "--undefined-only", so], text=True).split("\n")
    with open(weak, "w") as f:
        f.write("\n".join(ln.split()[-1] for ln in und if ln.strip() and "@" not in ln.split()[-1]) + "\n")
    subprocess.check_call(["objcopy", f"--weaken-symbols={weak}", obj, wobj])
    link(wobj)
    return ctypes.CDLL(so, mode=os.RTLD_LAZY)

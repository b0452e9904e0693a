"""Builds the reference's own core and oracle/ref_driver.cpp into oracle/_ref/ref_driver (TEST
INFRASTRUCTURE ONLY; oracle/_ref/ is not committed and no test needs it).

The reference tree is read where MRT_REFERENCE_DIR says, by default a checkout named ``reference``
beside this repository.  Its third-party libraries are not needed: oracle/refshim/ holds stand-ins
for the little the core uses of them ("What is pinned to the reference itself").  The
flags are oracle/Makefile's, so the reference and the oracle are compiled alike.

    python oracle/ref_build.py          # build (does nothing, and says so, without a reference tree)
"""
import concurrent.futures
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
DRIVER = os.path.join(OUT_DIR, "ref_driver")
SHIM = os.path.join(HERE, "refshim")
CXX = os.environ.get("CXX", "g++")
FLAGS = ["-std=c++17", "-O3", "-DNDEBUG", "-ffp-contract=off", "-include", "cstring", "-pthread"]
QUIET = ["-w"]  # for the reference's own sources only; the driver is compiled with -Wall
# the samplers that draw from PCG are left out (the stand-in for it only has to compile)
SKIP = ("ObjectLoader.cpp", "PCG.cpp", "StaticPCG.cpp")


def reference_dir():
    return os.environ.get("MRT_REFERENCE_DIR") or os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference")


def sources(app):
    pats = ["MobileRT/*.cpp", "MobileRT/*/*.cpp", "Components/Cameras/*.cpp", "Components/Lights/*.cpp",
            "Components/Shaders/*.cpp", "Components/Samplers/*.cpp", "Scenes/Scenes.cpp",
            "System_dependent/Native/Utils_dependent.cpp"]
    out = []
    for p in pats:
        out += [s for s in sorted(glob.glob(os.path.join(app, p))) if os.path.basename(s) not in SKIP]
    return out


def compiler_version():
    return subprocess.run([CXX, "--version"], capture_output=True, text=True).stdout.splitlines()[0].strip()


def _newer(target, inputs):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(i) for i in inputs)


def build(verbose=True):
    """True if oracle/_ref/ref_driver is there afterwards.  Never raises for a missing or broken
    reference: the product and its tests do not depend on it."""
    app = os.path.join(reference_dir(), "app")
    if not os.path.isdir(os.path.join(app, "MobileRT")):
        if verbose:
            print("ref_build: no reference tree at %s, nothing to build" % reference_dir())
        return False
    srcs = sources(app)
    shim = [os.path.join(d, f) for d, _, fs in os.walk(SHIM) for f in fs]
    driver_src = os.path.join(HERE, "ref_driver.cpp")
    if _newer(DRIVER, srcs + shim + [driver_src, os.path.abspath(__file__)]):
        return True
    obj_dir = os.path.join(OUT_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    inc = ["-I" + SHIM, "-I" + app, "-I" + os.path.join(app, "System_dependent", "Native")]

    def compile_one(src):
        obj = os.path.join(obj_dir, os.path.relpath(src, app).replace(os.sep, "_")[:-4] + ".o") if src != driver_src \
            else os.path.join(obj_dir, "ref_driver.o")
        r = subprocess.run([CXX] + FLAGS + (QUIET if src != driver_src else ["-Wall"]) + inc + ["-c", src, "-o", obj],
                           capture_output=True, text=True)
        if src == driver_src and r.returncode == 0 and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return obj, r

    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            done = list(pool.map(compile_one, srcs + [driver_src]))
        for obj, r in done:
            if r.returncode != 0:
                raise RuntimeError("%s:\n%s" % (obj, r.stderr[-4000:]))
        r = subprocess.run([CXX, "-pthread", "-o", DRIVER] + [o for o, _ in done], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-4000:])
    except (RuntimeError, OSError) as e:
        print("ref_build: WARNING: the reference did not build, oracle/_ref/ref_driver is missing:\n%s" % e,
              file=sys.stderr)
        return False
    if verbose:
        print("ref_build: built %s from %d reference sources" % (os.path.relpath(DRIVER, os.path.dirname(HERE)), len(srcs)))
    return True


if __name__ == "__main__":
    build()

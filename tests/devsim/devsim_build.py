"""Build the device twins of hostsim (tests/devsim/devsim_gl.hip, devsim_bls.hip) for gfx950 with the flags the product library
is built with, so the primitives under test are the code the library gets. Two translation units, compiled in parallel, one
shared object each; rebuilt when a source or a header of csrc/ is newer. Cross-compiles without a GPU."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
from cityprover.build import FLAGS  # noqa: E402  (the product's own: no -ffast-math, no GL_PORTABLE)

CSRC = os.path.join(ROOT, "city-rollup_amd", "csrc")
SIM = os.path.join(HERE, "..", "hostsim")
UNITS = {"gl": ["sim_gl.h"], "bls": ["sim_bls.h"]}


def so(unit):
    return os.path.join(HERE, "libdevsim_%s.so" % unit)


def _stale(unit):
    out = so(unit)
    if not os.path.exists(out):
        return True
    deps = [os.path.join(HERE, "devsim_%s.hip" % unit), os.path.join(HERE, "devsim.h")] + [os.path.join(SIM, f) for f in UNITS[unit]]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _compile(unit):
    out = so(unit)
    if _stale(unit):
        tmp = "%s.%d.tmp" % (out, os.getpid())
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-shared", "-o", tmp, os.path.join(HERE, "devsim_%s.hip" % unit)], check=True)
        os.replace(tmp, out)
    return out


def build():
    """unit name -> path of its shared object"""
    if not os.path.exists(os.path.join(CSRC, "poseidon_tables.h")):
        subprocess.run([sys.executable, os.path.join(CSRC, "gen_tables.py")], check=True)
    with ThreadPoolExecutor(len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(_compile, UNITS)))


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(build(), "%.1f s" % (time.time() - t0))

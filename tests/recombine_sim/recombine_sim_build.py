"""Build the test-only libraries of tests/recombine_sim: the host instantiation as the product compiles it ("host"), the same with the
forms kept for the A/B ("host_v1": -DPOSEIDON_RECOMBINE_V1 -DPOSEIDON_BBLOCK_DENSE), and the device entry with the product's flags
("device"). Each is rebuilt when a source or a header it includes is newer. Cross-compiles without a GPU."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
from cityprover.build import FLAGS  # noqa: E402  (the product's own: no -ffast-math, no GL_PORTABLE)

CSRC = os.path.join(ROOT, "city-rollup_amd", "csrc")
HOST_FLAGS = ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-function"]
KINDS = {
    "host": ("recombine_hostsim.hip", HOST_FLAGS),
    "host_v1": ("recombine_hostsim.hip", HOST_FLAGS + ["-DPOSEIDON_RECOMBINE_V1", "-DPOSEIDON_BBLOCK_DENSE"]),
    "device": ("recombine_devsim.hip", FLAGS),
}


def so(kind):
    return os.path.join(HERE, "librecombine_%s.so" % kind)


def build(kind):
    src, flags = KINDS[kind]
    out = so(kind)
    deps = [os.path.join(HERE, src), os.path.join(HERE, "recombine_sim.h")] + [os.path.join(CSRC, f) for f in ("poseidon.h", "poseidon_tables.h", "gl.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    if not os.path.exists(os.path.join(CSRC, "poseidon_tables.h")):
        subprocess.run([sys.executable, os.path.join(CSRC, "gen_tables.py")], check=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-shared", "-o", tmp, os.path.join(HERE, src)], check=True)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    for k in KINDS:
        print(build(k))

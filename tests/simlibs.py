"""The test-only shared objects ("twins": instantiations of the kernels' code for the host or the device, one per tests/*sim*
directory), in one table: name -> (source, flags, output), paths relative to tests/. build(name) compiles one if it is out of date
(cityprover.build.compile_if_needed: the compiler's own dependency list, content hashes) and returns its path. Cross-compiles
without a GPU."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "city-rollup_amd"))
from cityprover.build import FLAGS, compile_if_needed  # noqa: E402  (FLAGS: the product's own, no -ffast-math, no GL_PORTABLE)

HOST = ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-Wno-unused-value"]
RECOMBINE_HOST = HOST + ["-Wno-unused-function"]
TWINS = {name: ("%s/%s.hip" % (name, name), HOST, "%s/lib%s.so" % (name, name)) for name in (
    "hostsim", "renorm_hostsim", "pairingsim", "pointsim", "setupsim", "srsphase1sim", "keyfilesim", "sqrtsim", "r1cs_hostsim",
    "pairs_hostsim", "ntt_pairs_hostsim", "sponge_hostsim")}
TWINS.update({
    "verify_hostsim": ("verify_hostsim/verify_hostsim.hip", ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-pthread", "-Wno-unused-value"],
                       "verify_hostsim/libverify_hostsim.so"),
    "gatesim": ("gatesim/gatesim.hip", ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-function"],
                "gatesim/libgatesim.so"),
    # the device twins of hostsim, and the device entry of recombine_sim: the flags the library is built with
    "devsim_gl": ("devsim/devsim_gl.hip", FLAGS, "devsim/libdevsim_gl.so"),
    "devsim_bls": ("devsim/devsim_bls.hip", FLAGS, "devsim/libdevsim_bls.so"),
    "recombine_device": ("recombine_sim/recombine_devsim.hip", FLAGS, "recombine_sim/librecombine_device.so"),
    # the host instantiation as the product compiles it, and the same with the forms kept for the A/B
    "recombine_host": ("recombine_sim/recombine_hostsim.hip", RECOMBINE_HOST, "recombine_sim/librecombine_host.so"),
    "recombine_host_v1": ("recombine_sim/recombine_hostsim.hip", RECOMBINE_HOST + ["-DPOSEIDON_RECOMBINE_V1", "-DPOSEIDON_BBLOCK_DENSE"],
                          "recombine_sim/librecombine_host_v1.so"),
})


def build(name, force=False, verbose=False):
    src, flags, out = TWINS[name]
    return compile_if_needed(os.path.join(HERE, src), os.path.join(HERE, out), flags, "-shared", force, verbose)


def build_all(names=TWINS, **kw):
    """name -> path, compiled in parallel"""
    with ThreadPoolExecutor(4) as ex:
        return dict(zip(names, ex.map(lambda n: build(n, **kw), names)))


if __name__ == "__main__":
    print(build_all(sys.argv[1:] or TWINS, verbose=True))

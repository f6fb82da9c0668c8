"""Every arithmetic wrapper of the host instantiations (`hs_*` in tests/hostsim/hostsim.hip and tests/renorm_hostsim/renorm_hostsim.hip)
has a device twin (`ds_*` in tests/devsim) or is excluded here by name with its reason — and only host logic may be excluded. The
twins are built with the product's flags. CPU only: sources are parsed, nothing is compiled."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SOURCES = ("hostsim/hostsim.hip", "renorm_hostsim/renorm_hostsim.hip")
DEVICE_SOURCES = ("devsim/devsim_gl.hip", "devsim/devsim_bls.hip")
# name -> why it has no twin. Host logic only: threads, allocators, the AIR analyser / compiler, a compile-time flag
EXCLUDED = {
    "hs_parallel_for": "worker threads of host_util.h: no device code",
    "hs_parallel_for_throw": "worker threads of host_util.h: no device code",
    "hs_pool_script": "dev_pool.h over a counting allocator: host bookkeeping",
    "hs_mem_script": "dev_mem.h over a counting allocator: host bookkeeping",
    "hs_air_point": "air.h analyse + compile run on the host; the interpreter has its own GPU tests (tests/test_gpu_air.py)",
    "hs_air_map_self_read": "air.h map_self_read: a host check of a map program's loads against its stores; the refusals have their own GPU tests (tests/test_gpu_air_semantics.py)",
    "hs_rn_units32": "reports a compile-time constant",
}
HOST_LOGIC = re.compile(r"^hs_(parallel_for|pool_|mem_|air_|rn_units32)")


def exported(path, prefix):
    src = open(os.path.join(HERE, path)).read()
    return set(re.findall(r"^(?:int|long|void|uint64_t|uint32_t)\s+(%s_\w+)\s*\(" % prefix, src, re.M))


def test_names_parse():
    hs = set().union(*(exported(p, "hs") for p in HOST_SOURCES))
    ds = set().union(*(exported(p, "ds") for p in DEVICE_SOURCES))
    assert {"hs_mul", "hs_bls_fp_op", "hs_rn_permute", "hs_cubic", "hs_pool_script", "hs_r1cs_mul_small"} <= hs and len(hs) >= 45
    assert {"ds_mul", "ds_permute", "ds_gl_chain", "ds_bls_g2_loose_step"} <= ds
    # every `hs_` / `ds_` definition is one the pattern sees
    for paths, prefix, names in ((HOST_SOURCES, "hs", hs), (DEVICE_SOURCES, "ds", ds)):
        for p in paths:
            src = open(os.path.join(HERE, p)).read()
            defined = set(re.findall(r"\b(%s_\w+)\s*\([^;{]*\)\s*\{" % prefix, src))
            assert defined <= names, (p, defined - names)


def test_every_host_wrapper_has_a_device_twin_or_a_named_exclusion():
    hs = set().union(*(exported(p, "hs") for p in HOST_SOURCES))
    ds = set().union(*(exported(p, "ds") for p in DEVICE_SOURCES))
    assert set(EXCLUDED) <= hs, "an exclusion names a wrapper that does not exist"
    for name in sorted(hs):
        twin = "ds_" + name[3:]
        if name in EXCLUDED:
            assert HOST_LOGIC.match(name), "%s is arithmetic: it may not be excluded" % name
            assert twin not in ds
        else:
            assert twin in ds, "%s has no device twin (%s) and no exclusion" % (name, twin)
    # the entries the device library adds on top: the whole permutation without a mask
    assert ds - {"ds_" + n[3:] for n in hs} == {"ds_permute"}


def test_twins_share_the_element_bodies_and_the_products_flags():
    import cityprover.build
    import simlibs
    for p in DEVICE_SOURCES:
        (flags,) = [f for src, f, _ in simlibs.TWINS.values() if src == p]
        assert flags is cityprover.build.FLAGS, "%s is not compiled with the product's flags" % p
        assert not re.search(r"ffast-math|GL_PORTABLE", " ".join(flags))   # the entry is the product's list: no flag, no -O of its own
    for p in HOST_SOURCES + DEVICE_SOURCES:
        assert re.search(r'#include "(\.\./hostsim/)?sim_(gl|bls)\.h"', open(os.path.join(HERE, p)).read()), p

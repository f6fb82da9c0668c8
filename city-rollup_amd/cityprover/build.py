"""Build libcityprover_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU). The library is several
translation units (csrc/*.hip) compiled in parallel and linked into one shared object.

compile_if_needed() is the one place that runs hipcc, for the library, the test twins (tests/simlibs.py) and tools/witgen. It
asks the compiler what an output depends on (-MD) and keeps, beside the output, <out>.deps.json: the argv and the sha256 of
the source and of every header in the tree it read. An output is up to date when that manifest still describes the tree;
modification times play no part."""
import glob
import hashlib
import json
import os
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
SO = os.path.join(PKG, "libcityprover_hip.so")
OBJ = os.path.join(PKG, "build")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-function"]


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _key(argv):
    """argv as the manifest keeps it: the tree's own location taken out, so a copy of the tree stays up to date"""
    return [a.replace(ROOT + os.sep, "") for a in argv]


def _argv(src, out, flags, mode):
    return [_hipcc()] + flags + [mode, "-o", out, src]


def _fresh(out, argv):
    """the manifest of `out` if it still describes the tree, else None"""
    try:
        with open(out + ".deps.json") as f:
            m = json.load(f)
        if os.path.exists(out) and m["argv"] == _key(argv) and all(_sha(os.path.join(os.path.dirname(out), p)) == h for p, h in m["files"].items()):
            return m
    except (OSError, ValueError, KeyError):
        pass
    return None


def _write_manifest(out, argv, files):
    tmp = "%s.deps.json.%d.tmp" % (out, os.getpid())
    with open(tmp, "w") as f:
        json.dump({"argv": _key(argv), "files": files}, f, indent=1, sort_keys=True)
    os.replace(tmp, out + ".deps.json")


def compile_if_needed(src, out, flags, mode, force=False, verbose=False):
    """hipcc `flags` `mode` (-c or -shared) `src` -o `out`, unless `out` is up to date. Several processes may build the same
    output at once: private temporary names, the output renamed into place before its manifest. Returns `out`."""
    if not os.path.exists(os.path.join(CSRC, "poseidon_tables.h")):
        subprocess.run([sys.executable, os.path.join(CSRC, "gen_tables.py")], check=True)
    argv = _argv(src, out, flags, mode)
    if not force and _fresh(out, argv):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    cmd = argv[:-3] + ["-MD", "-MF", tmp + ".d", "-o", tmp, src]
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.run(cmd, check=True)
        with open(tmp + ".d") as f:
            deps = shlex.split(f.read().replace("\\\n", " "))[1:]   # make syntax: "target: dep dep \"
        # the source and the headers of this tree (or beside the source); system and ROCm headers are left out
        roots = (os.path.realpath(ROOT) + os.sep, os.path.dirname(os.path.realpath(src)) + os.sep)
        here = os.path.dirname(out)
        files = {os.path.relpath(d, here): _sha(d) for d in sorted({os.path.realpath(d) for d in deps}) if d.startswith(roots)}
        os.replace(tmp, out)
        _write_manifest(out, argv, files)
    finally:
        for t in (tmp, tmp + ".d"):
            if os.path.exists(t):
                os.remove(t)
    return out


def units():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))


def _obj(unit):
    return os.path.join(OBJ, unit + ".o")


def _link_argv():
    return [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + [_obj(u) for u in units()]


def _so_argv():
    # the library's manifest: every unit's command, then the link's; its files are the units' (objects need not be kept)
    return sum((_argv(os.path.join(CSRC, u), _obj(u), FLAGS, "-c") for u in units()), []) + _link_argv()


def stale():
    return _fresh(SO, _so_argv()) is None


def build(force=False, verbose=False):
    if not force and not stale():
        return SO
    with ThreadPoolExecutor(len(units())) as ex:
        objs = list(ex.map(lambda u: compile_if_needed(os.path.join(CSRC, u), _obj(u), FLAGS, "-c", force, verbose), units()))
    tmp = "%s.%d.tmp" % (SO, os.getpid())   # several ranks may build at once: private names, atomic renames
    cmd = _link_argv()
    cmd[cmd.index(SO)] = tmp
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.run(cmd, check=True)
        files = {}
        for o in objs:
            with open(o + ".deps.json") as f:
                files.update({os.path.relpath(os.path.join(OBJ, p), PKG): h for p, h in json.load(f)["files"].items()})
        os.replace(tmp, SO)
        _write_manifest(SO, _so_argv(), files)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

"""cityprover.build.compile_if_needed, the one routine that runs the HIP compiler: an output is rebuilt exactly when its argv, its
source or a header the compiler read has changed in content, whatever the modification times say; a failed or a concurrent build
leaves a loadable output and a readable manifest. Then the two tables it serves: the library's units and tests/simlibs.py. Every
compile here is a source of a few lines in tmp_path, except the library's own build() (up to date in a built tree). No GPU."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest

import cityprover.build as B
import simlibs

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-O1", "-fPIC"]
DRIVER = "import sys; sys.path.insert(0, sys.argv[1])\nfrom cityprover.build import compile_if_needed\ncompile_if_needed(sys.argv[2], sys.argv[3], sys.argv[4:], '-shared')\n"


class Tree:
    """t.hip -> b.inc -> a.h in a directory of its own; build() counts the compiler processes it starts"""

    def __init__(self, path, monkeypatch):
        self.dir, self.src, self.out = str(path), str(path / "t.hip"), str(path / "libt.so")
        self.write("a.h", "__host__ __device__ inline int a_value() { return 1; }\n")
        self.write("b.inc", '#include "a.h"\n')
        self.write("t.hip", '#include <hip/hip_runtime.h>\n#include "b.inc"\nextern "C" int t_value() { return a_value(); }\n')
        self.compiles, run = 0, subprocess.run

        def counting(cmd, *a, **k):
            self.compiles += 1
            return run(cmd, *a, **k)
        monkeypatch.setattr(B.subprocess, "run", counting)

    def write(self, name, text):
        with open(os.path.join(self.dir, name), "w") as f:
            f.write(text)

    def build(self, flags=FLAGS, **kw):
        """-> how many compiler processes this call started"""
        before = self.compiles
        assert B.compile_if_needed(self.src, self.out, flags, "-shared", **kw) == self.out
        return self.compiles - before

    def manifest(self):
        with open(self.out + ".deps.json") as f:
            return json.load(f)

    def value(self):
        return ctypes.CDLL(self.out).t_value()   # once per tree: dlopen would hand back the first build of a path


@pytest.fixture
def tree(tmp_path, monkeypatch):
    t = Tree(tmp_path, monkeypatch)
    assert t.build() == 1 and t.build() == 0
    return t


def test_a_header_edit_behind_an_inc_rebuilds_and_the_manifest_names_it(tree):
    assert sorted(tree.manifest()["files"]) == ["a.h", "b.inc", "t.hip"]       # nothing of the system or of ROCm
    tree.write("a.h", "__host__ __device__ inline int a_value() { return 2; }\n")
    assert tree.build() == 1 and tree.build() == 0
    assert "a.h" in tree.manifest()["files"]


def test_a_newer_mtime_with_the_same_bytes_rebuilds_nothing(tree):
    before = os.stat(tree.out)
    for name in ("a.h", "b.inc", "t.hip"):
        os.utime(os.path.join(tree.dir, name), (before.st_atime + 1000, before.st_mtime + 1000))
    assert tree.build() == 0
    after = os.stat(tree.out)
    assert (after.st_ino, after.st_mtime_ns) == (before.st_ino, before.st_mtime_ns)


def test_an_edit_with_an_older_mtime_than_the_output_rebuilds(tree):
    before = os.stat(tree.out)
    tree.write("a.h", "__host__ __device__ inline int a_value() { return 3; }\n")
    os.utime(os.path.join(tree.dir, "a.h"), (before.st_atime - 1000, before.st_mtime - 1000))
    assert os.path.getmtime(os.path.join(tree.dir, "a.h")) < os.path.getmtime(tree.out)
    assert tree.build() == 1 and tree.build() == 0
    assert os.stat(tree.out).st_ino != before.st_ino


def test_a_flag_change_rebuilds_both_ways(tree):
    assert tree.build(FLAGS + ["-DT_EXTRA"]) == 1 and tree.build(FLAGS + ["-DT_EXTRA"]) == 0
    assert "-DT_EXTRA" in tree.manifest()["argv"]
    assert tree.build() == 1 and tree.build() == 0
    assert "-DT_EXTRA" not in tree.manifest()["argv"]


def test_a_missing_manifest_or_output_rebuilds_and_force_always_does(tree):
    os.remove(tree.out + ".deps.json")
    assert tree.build() == 1 and tree.build() == 0
    os.remove(tree.out)
    assert tree.build() == 1 and tree.build() == 0
    with open(tree.out + ".deps.json", "w") as f:
        f.write("{")
    assert tree.build() == 1 and tree.build() == 0
    assert tree.build(force=True) == 1


def test_a_failed_compile_raises_and_leaves_the_old_pair_and_no_temporaries(tree):
    def pair():
        return [open(p, "rb").read() for p in (tree.out, tree.out + ".deps.json")]
    before = pair()
    tree.write("t.hip", '#include "b.inc"\nextern "C" int t_value() { return a_value() }\n')
    with pytest.raises(subprocess.CalledProcessError):
        tree.build()
    assert pair() == before
    assert sorted(os.listdir(tree.dir)) == ["a.h", "b.inc", "libt.so", "libt.so.deps.json", "t.hip"]


def test_two_processes_building_the_same_output(tmp_path, monkeypatch):
    t = Tree(tmp_path, monkeypatch)
    cmd = [sys.executable, "-c", DRIVER, os.path.dirname(os.path.dirname(B.__file__)), t.src, t.out] + FLAGS
    procs = [subprocess.Popen(cmd) for _ in range(2)]
    assert [p.wait() for p in procs] == [0, 0]
    assert t.value() == 1
    assert sorted(t.manifest()["files"]) == ["a.h", "b.inc", "t.hip"]
    assert t.build() == 0 and not glob.glob(os.path.join(t.dir, "*.tmp*"))


def test_the_librarys_units_and_what_their_manifests_list(monkeypatch):
    assert [os.path.join(B.CSRC, u) for u in B.units()] == sorted(glob.glob(os.path.join(B.CSRC, "*.hip"))) and len(B.units()) >= 4
    assert B.build() == B.SO and not B.stale()
    started = []
    monkeypatch.setattr(B.subprocess, "run", lambda *a, **k: started.append(a))
    assert B.build() == B.SO and started == []          # up to date: no process at all

    def listed(unit):
        with open(os.path.join(B.OBJ, unit + ".o.deps.json")) as f:
            return {os.path.basename(p) for p in json.load(f)["files"]}
    assert {"keyfile.hip", "groth16_keyfile.h", "groth16_key.h"} <= listed("keyfile.hip")
    with open(os.path.join(B.CSRC, "cityprover.hip")) as f:
        incs = set(re.findall(r'^\s*#include "([^"]+\.inc)"', f.read(), re.M))
    assert len(incs) >= 8 and incs <= listed("cityprover.hip")
    with open(B.SO + ".deps.json") as f:
        assert {"groth16_keyfile.h", "cityprover.h"} | incs <= {os.path.basename(p) for p in json.load(f)["files"]}


def test_every_twin_entry_and_no_other_compile_line_under_tests():
    outs = [out for _, _, out in simlibs.TWINS.values()]
    assert len(set(outs)) == len(outs) == len(simlibs.TWINS) >= 18
    for name, (src, flags, out) in simlibs.TWINS.items():
        assert os.path.isfile(os.path.join(HERE, src)), name
        assert os.path.dirname(src) == os.path.dirname(out) and flags[0] == "--offload-arch=gfx950", name
    assert not glob.glob(os.path.join(HERE, "*", "*build.py"))
    names = set()
    for path in glob.glob(os.path.join(HERE, "**", "*.py"), recursive=True):
        with open(path) as f:
            if path != os.path.abspath(__file__) and "hipcc" in f.read():
                names.add(os.path.relpath(path, HERE))
    assert names <= {"simlibs.py", "test_qbench_harness.py", "test_batcher_sim.py"}, names

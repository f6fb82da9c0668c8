#!/usr/bin/env python3
"""Timing of cp_groth16_key_save_file / cp_groth16_key_load_file on the keys of tools/bench_groth16_setup.py (the same generator,
seeds and n_public: tests/r1cs_cases.satisfied_system at 2^k constraints). Correctness is tests/test_gpu_groth16_keyfile.py; this
only measures. Per size and per form of the file (compressed, raw):
  save_ms, load_ms, load_torsion_ms   host clock around the whole call, which ends in a stream synchronisation: one warm-up call,
                                      then median / min / max of --reps. load_torsion is CP_GROTH16_KEY_LOAD_CHECK_TORSION.
  file_bytes                          what the header determines
  kernels                             one further save and one further load (with the torsion check) under cp_profile_begin /
                                      cp_profile_end: device-event time of the keyfile_* launches by name, and their share of
                                      that call's wall time. The rest of a call is the host: reading or writing the file, the
                                      checksum, the copies into and out of the page-locked buffers.
  setup_wall_ms                       the median wall time of the setup of the same system, from profiles/groth16_setup.json as
                                      the parent commit recorded it (what a key file replaces), and one setup timed in this run
The files are written to a temporary directory and read back at once: THEY COME FROM THE PAGE CACHE, not from a disk. A cold read
adds the disk's time for file_bytes. Prints one JSON line and writes profiles/groth16_keyfile.json.

usage: bench_groth16_keyfile.py [log sizes, comma separated: default 16,20] [--reps N] [--n-public N] [--chunk-points N] [--dir DIR]"""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cityprover as cp  # noqa: E402
import groth16_setup_cases as GC  # noqa: E402
import r1cs_cases as RC  # noqa: E402

KERNELS = ("keyfile_pack_g1", "keyfile_pack_g2", "keyfile_unpack_g1", "keyfile_unpack_g2", "keyfile_torsion_g1", "keyfile_torsion_g2")


def stats(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3), "max": round(ms[-1], 3)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def setup_reference(log_n):
    """the setup's wall time for this size as profiles/groth16_setup.json holds it, or None"""
    try:
        for s in json.load(open(os.path.join(ROOT, "profiles", "groth16_setup.json")))["sizes"]:
            if s["log_n"] == log_n:
                return {"wall_ms": s["wall_ms"], "n_wires": s["n_wires"], "n_public": s["n_public"]}
    except (OSError, KeyError, ValueError):
        pass
    return None


def run(prover, log_n, workdir, reps=5, n_public=16, chunk_points=0):
    s = RC.satisfied_system(1 << log_n, 7000 + log_n)
    td = GC.trapdoor(log_n)
    coeffs = RC.limbs4(s["coeffs"])

    def setup():
        key = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], coeffs, s["mats"], n_public, **td)
        prover.sync()
        return key
    setup().free()                                   # warm-up, as tools/bench_groth16_setup.py
    setup_ms, key = timed(setup)
    pk = key.pk()
    out = {"log_n": log_n, "n_constraints": s["n"], "n_wires": pk.n_wires, "n_public": n_public, "reps": reps, "chunk_points": chunk_points or "default (2^16)",
           "points": {"g1": 2 * pk.n_wires + pk.n_private + (1 << pk.log_domain) - 1, "g2": pk.n_wires},
           "setup_wall_ms": {"recorded": setup_reference(log_n), "this_run_one_call": round(setup_ms, 3)}, "forms": {}}
    try:
        for form, raw in (("compressed", False), ("raw", True)):
            path = os.path.join(workdir, "key_%d_%s.cpg16" % (log_n, form))

            def save():
                key.save(path, raw=raw, chunk_points=chunk_points)

            def load(torsion):
                k = cp.Groth16Key.load(prover, path, check_torsion=torsion, chunk_points=chunk_points)
                k.free()
            save()                                   # warm-up: code objects, and the file the loads read
            load(False)
            load(True)
            r = {"save_ms": stats([timed(save)[0] for _ in range(reps)]),
                 "load_ms": stats([timed(lambda: load(False))[0] for _ in range(reps)]),
                 "load_torsion_ms": stats([timed(lambda: load(True))[0] for _ in range(reps)])}
            info = cp.groth16_key_file_info(path, verify_checksum=False)
            r["file_bytes"] = info["file_bytes"]
            assert info["file_bytes"] == os.path.getsize(path) and info["n_wires"] == pk.n_wires
            r["file_info_ms"] = {"with_checksum": round(timed(lambda: cp.groth16_key_file_info(path, True))[0], 3),
                                 "without": round(timed(lambda: cp.groth16_key_file_info(path, False))[0], 3)}
            kern = {}
            for what, call in (("save", save), ("load_torsion", lambda: load(True))):
                prover.profile_begin()
                wall, _ = timed(call)
                prof = prover.profile_end()
                dev = {k: round(prof[k]["total_ms"], 3) for k in KERNELS if k in prof}
                kern[what] = {"wall_ms": round(wall, 3), "kernel_ms": dev, "launches": {k: prof[k]["launches"] for k in dev},
                              "kernels_share_of_wall": round(sum(dev.values()) / wall, 4)}
            # the load without the torsion check runs the unpack kernels alone: their share of its median
            unpack = sum(v for k, v in kern["load_torsion"]["kernel_ms"].items() if "unpack" in k)
            kern["load"] = {"unpack_kernel_ms": round(unpack, 3), "unpack_share_of_median_wall": round(unpack / r["load_ms"]["median"], 4)}
            r["kernels"] = kern
            if out["setup_wall_ms"]["recorded"]:
                ref = out["setup_wall_ms"]["recorded"]["wall_ms"]["median"]
                r["load_over_recorded_setup"] = round(r["load_ms"]["median"] / ref, 3)
                r["load_torsion_over_recorded_setup"] = round(r["load_torsion_ms"]["median"] / ref, 3)
            out["forms"][form] = r
            os.remove(path)
    finally:
        key.free()
    return out


if __name__ == "__main__":
    args, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a.startswith("--"):
            skip = True
        else:
            args.append(a)
    sizes = [int(x) for x in (args[0] if args else "16,20").split(",")]
    opt = lambda name, default, conv=int: conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    p = cp.Prover(0)
    out = {"tool": "tools/bench_groth16_keyfile.py",
           "method": "one warm-up call of each kind; wall = host clock around the call (it ends in a stream synchronisation), median of reps; kernels = "
                     "device events of one further profiled call. Files are read back from the page cache, not from a disk.",
           "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels() if "keyfile::" in r["name"]]
    except Exception as e:   # the LLVM tools are a convenience here, not a dependency of the measurement
        out["kernel_registers"] = "unavailable: %s" % e
    workdir = tempfile.mkdtemp(prefix="cpg16_", dir=opt("--dir", None, str))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    try:
        for k in sizes:
            out["sizes"].append(run(p, k, workdir, reps=opt("--reps", 5), n_public=opt("--n-public", 16), chunk_points=opt("--chunk-points", 0)))
            with open(os.path.join(ROOT, "profiles", "groth16_keyfile.json"), "w") as f:   # after every size: a later size that fails keeps the earlier ones
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
        p.close()
    print(json.dumps(out))

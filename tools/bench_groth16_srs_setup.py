#!/usr/bin/env python3
"""Timing of the Groth16 setup from a powers-of-tau SRS (cp_groth16_setup_srs_bls12381), of a delta contribution and of its check,
beside the trapdoor setup at the same size, on tests/r1cs_cases.satisfied_system at 2^k constraints. Correctness is
tests/test_gpu_groth16_srs_setup.py and tests/test_gpu_groth16_contribute.py; this measures - but at every size the bytes of the
SRS key are compared with the trapdoor key's (gamma = delta = 1) before anything is reported. The issue that asked for this path
sets no time bound: the figures are a record, not a check. In one process, per size:
  srs_build_s            the SRS of a known (tau, alpha, beta) made on the device: cp_groth16_srs_unit_bls12381, then
                         cp_groth16_srs_contribute_bls12381 (tests/test_gpu_groth16_srs_phase1.py holds that pair, word for word,
                         against the fixed-base multiples this tool used to read back through Python integers)
  srs_setup              wall_ms: host clock around one call after one warm-up call. phases_ms: one further call under
                         cp_profile_begin / cp_profile_end, the host clock of each phase (a phase ends with a stream
                         synchronisation, so its clock holds its kernels): point_ntts (the four inverse transforms), columns (the
                         four column products and their normalisation), z, rest (validation, transposition, single points).
                         shares: each phase over their sum. kernels_ms: device-event time of every launch by name.
  trapdoor_setup_wall_ms the same system through cp_groth16_setup_bls12381, one warm-up call, then one timed call
  contribute_ms, check_ms  one call each on the SRS key (the check's verdict must be 0)
Prints one JSON line and writes profiles/groth16_srs_setup.json.

usage: bench_groth16_srs_setup.py [log sizes, comma separated: default 12,16,20] [--n-public N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cityprover as cp  # noqa: E402
import groth16_setup_cases as GC  # noqa: E402
import groth16_srs_cases as SC  # noqa: E402
import r1cs_cases as RC  # noqa: E402

PHASES = {"point_ntts": ("srs_setup_lagrange",), "columns": ("srs_setup_columns",), "z": ("srs_setup_z",),
          "rest": ("srs_setup_validate", "srs_setup_transpose", "srs_setup_rest")}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def run(prover, log_n, n_public=16):
    s = RC.satisfied_system(1 << log_n, 7000 + log_n)
    td = GC.trapdoor(log_n)
    coeffs = RC.limbs4(s["coeffs"])
    L = GC.log_domain(s["n"])
    t0 = time.perf_counter()
    unit = cp.Groth16Srs.unit(prover, L)
    try:
        srs = unit.contribute(td["tau"], td["alpha"], td["beta"])
    finally:
        unit.free()
    srs_build_s = time.perf_counter() - t0

    def from_srs():
        key = cp.Groth16Key.setup_srs(prover, s["n"], s["n_wires"], coeffs, s["mats"], n_public, srs)
        prover.sync()
        return key

    def from_trapdoor():
        key = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], coeffs, s["mats"], n_public, **dict(td, gamma=1, delta=1))
        prover.sync()
        return key

    try:
        from_trapdoor().free()                                    # warm-up: window tables, twiddles, work arrays
        ref, trapdoor_ms = clock(from_trapdoor)
        want = SC.key_bytes(ref)
        ref.free()
        key, first_ms = clock(from_srs)                            # the warm-up call is the one whose bytes are compared
        if SC.key_bytes(key) != want:
            raise SystemExit("2^%d: the SRS key differs from the trapdoor key: nothing is reported" % log_n)
        key.free()
        key, wall_ms = clock(from_srs)
        key.free()
        prover.profile_begin()
        key, profiled_ms = clock(from_srs)
        prof = prover.profile_end()
        ms = lambda name: prof.get(name, {}).get("total_ms", 0.0)
        phases = {k: sum(ms("host:" + p) for p in names) for k, names in PHASES.items()}
        total = sum(phases.values())
        d = int.from_bytes(np.random.default_rng(log_n).bytes(31), "little") | 1
        after, contribute_ms = clock(lambda: key.contribute(d))
        pk = key.pk()
        count = pk.n_private + (1 << pk.log_domain) - 1
        weights = np.frombuffer(np.random.default_rng(log_n + 1).bytes(16 * count), np.uint64).reshape(count, 2) | np.uint64(1)
        (verdict, why), check_ms = clock(lambda: cp.Groth16Key.check_contribution(prover, key, after, np.ascontiguousarray(weights)))
        if verdict != 0:
            raise SystemExit("2^%d: the contribution check says %d (%s)" % (log_n, verdict, why))
        n_wires, n_private = pk.n_wires, pk.n_private
        after.free()
        key.free()
    finally:
        srs.free()
    return {"log_n": log_n, "n_constraints": s["n"], "n_wires": n_wires, "n_private": n_private, "n_public": n_public,
            "terms": [int(m[0][-1]) for m in s["mats"]], "srs_build_s": round(srs_build_s, 2), "keys_equal": True,
            "srs_setup": {"first_call_ms": round(first_ms, 3), "wall_ms": round(wall_ms, 3), "profiled_call_ms": round(profiled_ms, 3),
                          "phases_ms": {k: round(v, 3) for k, v in phases.items()},
                          "shares": {k: round(v / total, 4) if total else None for k, v in phases.items()},
                          "kernels_ms": {k: round(v["total_ms"], 3) for k, v in sorted(prof.items()) if not k.startswith(("host:", "wait:"))}},
            "trapdoor_setup_wall_ms": round(trapdoor_ms, 3), "srs_over_trapdoor": round(wall_ms / trapdoor_ms, 1),
            "contribute_ms": round(contribute_ms, 3), "check_ms": round(check_ms, 3)}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sizes = [int(x) for x in (args[0] if args else "12,16,20").split(",")]
    opt = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    p = cp.Prover(0)
    out = {"tool": "tools/bench_groth16_srs_setup.py", "method": "per size, one process: trapdoor setup (warm-up + one timed call), SRS setup "
           "(first call compared byte for byte with the trapdoor key, one timed call, one profiled call), one contribution, one check",
           "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels()
                                   if "pointntt" in r["name"] or "g16srs" in r["name"]]
    except Exception as e:   # the LLVM tools are a convenience here, not a dependency of the measurement
        out["kernel_registers"] = "unavailable: %s" % e
    for k in sizes:
        out["sizes"].append(run(p, k, n_public=opt("--n-public", 16)))
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "groth16_srs_setup.json"), "w") as f:   # after every size: a long run leaves what it has
            json.dump(out, f, indent=1)
            f.write("\n")
    p.close()
    print(json.dumps(out))

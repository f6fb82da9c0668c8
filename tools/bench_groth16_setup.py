#!/usr/bin/env python3
"""Timing of cp_groth16_setup_bls12381 on tests/r1cs_cases.satisfied_system at 2^k constraints. Correctness is
tests/test_gpu_groth16_setup.py; this only measures. Per size:
  wall_ms        host clock around the whole call (system already in host arrays): one warm-up call, median / min / max of --reps
  profile        one further call under cp_profile_begin / cp_profile_end: device-event time of every launch by name
                 (fixed_base_mul_g1 = the five G1 sets + IC, fixed_base_mul_g2 = the B query in G2, r1cs_eval_* = the transposed
                 products, fr_* = the Lagrange transform) and host-clock time of the host phases (host:setup_transpose = the
                 counting sort of the three matrices, host:setup_columns = transposed system built and staged + the columns,
                 host:setup_points = point sets + the six single points); the event brackets serialise nothing that was parallel
                 (one stream), but they add a few microseconds per launch
  shares         of the profiled call
Prints one JSON line and writes profiles/groth16_setup.json.

usage: bench_groth16_setup.py [log sizes, comma separated: default 16,20] [--reps N] [--n-public N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cityprover as cp  # noqa: E402
import groth16_setup_cases as GC  # noqa: E402
import r1cs_cases as RC  # noqa: E402


def run(prover, log_n, reps=5, n_public=16):
    t0 = time.perf_counter()
    s = RC.satisfied_system(1 << log_n, 7000 + log_n)
    gen_s = time.perf_counter() - t0
    td = GC.trapdoor(log_n)
    coeffs = RC.limbs4(s["coeffs"])

    def call():
        key = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], coeffs, s["mats"], n_public, **td)
        prover.sync()
        return key

    call().free()                                   # warm-up: both window tables, twiddles, work arrays
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        key = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        key.free()
    prover.profile_begin()
    t0 = time.perf_counter()
    key = call()
    profiled_ms = (time.perf_counter() - t0) * 1e3
    prof = prover.profile_end()
    pk = key.pk()
    n_wires, n_private, n_z = pk.n_wires, pk.n_private, (1 << pk.log_domain) - 1
    key.free()
    ms = lambda name: prof.get(name, {}).get("total_ms", 0.0)
    g1_points = 2 * n_wires + n_private + n_z + n_public
    groups = {"fixed_base_g1_ms": ms("fixed_base_mul_g1"), "fixed_base_g2_ms": ms("fixed_base_mul_g2"),
              "transposed_products_ms": ms("r1cs_eval_short") + ms("r1cs_eval_long"),
              "lagrange_ms": sum(v["total_ms"] for k, v in prof.items() if k.startswith("fr_")) + ms("setup_tau_powers"),
              "host_transpose_ms": ms("host:setup_transpose"), "host_validate_ms": ms("host:setup_validate"),
              "host_columns_ms": ms("host:setup_columns"), "host_points_ms": ms("host:setup_points")}
    wall.sort()
    return {"log_n": log_n, "n_constraints": s["n"], "n_wires": n_wires, "n_public": n_public, "terms": [int(m[0][-1]) for m in s["mats"]],
            "generate_system_s": round(gen_s, 2), "reps": reps,
            "wall_ms": {"median": round(wall[len(wall) // 2], 3), "min": round(wall[0], 3), "max": round(wall[-1], 3)},
            "profiled_call_ms": round(profiled_ms, 3), **{k: round(v, 3) for k, v in groups.items()},
            "g1_points": g1_points, "g2_points": n_wires,
            "g1_ns_per_point": round(groups["fixed_base_g1_ms"] * 1e6 / g1_points, 2), "g2_ns_per_point": round(groups["fixed_base_g2_ms"] * 1e6 / n_wires, 2),
            "shares_of_profiled_call": {k[:-3]: round(v / profiled_ms, 4) for k, v in groups.items()},
            "profile": prof}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sizes = [int(x) for x in (args[0] if args else "16,20").split(",")]
    opt = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    p = cp.Prover(0)
    out = {"tool": "tools/bench_groth16_setup.py", "method": "one warm-up call; wall = host clock around the call, median of reps; "
           "kernels = device events of one further profiled call", "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels()
                                   if "fixedbase" in r["name"] or "g16setup" in r["name"]]
    except Exception as e:   # the LLVM tools are a convenience here, not a dependency of the measurement
        out["kernel_registers"] = "unavailable: %s" % e
    for k in sizes:
        out["sizes"].append(run(p, k, reps=opt("--reps", 5), n_public=opt("--n-public", 16)))
    p.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "groth16_setup.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))

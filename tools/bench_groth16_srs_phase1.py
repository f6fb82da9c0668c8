#!/usr/bin/env python3
"""Timing of phase 1 on the device - cp_groth16_srs_unit / _contribute / _points / _check - at SRS sizes 2^L, beside the
one-scalar-per-launch multiplication (pointntt::k_scale) over arrays of the same sizes. Correctness is
tests/test_gpu_groth16_srs_phase1.py; this measures - but at every size the contributed SRS must pass check() with verdict 0
before anything is reported. No bound is set: the figures are a record, not a check. In one process, per size:
  unit_ms, contribute_ms, points_ms, check_ms   host clock around a call that ends on a stream synchronisation: one warm-up call,
                         then the median of 5. contribute runs on the unit SRS with seeded (t, a, b); points and check on its result.
  kernels_ms             one further call of each under cp_profile_begin / cp_profile_end: device-event time of every launch by
                         name. shares: each kernel over the sum of its call.
  k_scale                the uniform-control-flow cost a per-lane scalar can at best reach: the `point_scale_g1` / `point_scale_g2`
                         launches of inverse point transforms (whose last step multiplies every point by the one scalar 1/n) over
                         2^(L+1) points of G1 (tau_g1 has one point fewer), 2^L of G1 twice (alpha_tau_g1, beta_tau_g1) and 2^L of
                         G2 (tau_g2), under the profile; their sum against the sum of the `srs_scale_each_*` launches of contribute.
Prints one JSON line and writes profiles/groth16_srs_phase1.json.

usage: bench_groth16_srs_phase1.py [log sizes, comma separated: default 12,16,20]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cityprover as cp  # noqa: E402
import groth16_setup_cases as GC  # noqa: E402
import oracle_lib as O  # noqa: E402

REPEATS = 5


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def median_ms(prover, fn, drop=lambda out: None):
    """one warm-up call, then the median of REPEATS; every call ends on a stream synchronisation"""
    def once():
        out = fn()
        prover.sync()
        return out
    drop(once())
    times = []
    for _ in range(REPEATS):
        out, ms = clock(once)
        drop(out)
        times.append(ms)
    return statistics.median(times), times


def profiled(prover, fn, drop=lambda out: None):
    prover.profile_begin()
    out = fn()
    prover.sync()
    prof = prover.profile_end()
    drop(out)
    kernels = {k: v["total_ms"] for k, v in sorted(prof.items()) if not k.startswith(("host:", "wait:"))}
    total = sum(kernels.values())
    return {"kernels_ms": {k: round(v, 3) for k, v in kernels.items()}, "shares": {k: round(v / total, 4) if total else None for k, v in kernels.items()}}


def k_scale_ms(prover, log_size, seed):
    """the point_scale_* launches of inverse transforms over arrays of the SRS's sizes, by device events"""
    out = {}
    rng = np.random.default_rng(seed)
    for name, group, log_n in (("tau_g1", 1, log_size + 1), ("alpha_tau_g1", 1, log_size), ("beta_tau_g1", 1, log_size), ("tau_g2", 2, log_size)):
        n = 1 << log_n
        scalars = np.frombuffer(rng.bytes(32 * n), np.uint64).reshape(n, 4).copy()
        scalars[:, 3] &= np.uint64((1 << 62) - 1)                   # below r
        d = prover.to_device(scalars)
        cls, gen, ntt, kernel = ((cp.G1Points, O.bls_constants()[2], cp.point_ntt_g1_dev, "point_scale_g1") if group == 1 else
                                 (cp.G2Points, O.bls_g2_generator(), cp.point_ntt_g2_dev, "point_scale_g2"))
        pts, flags = cls.fixed_base(prover, gen, d.ptr, n)
        try:
            prover.profile_begin()
            ntt(prover, pts, flags, log_n, inverse=True)
            prover.sync()
            prof = prover.profile_end()
            out[name] = round(prof[kernel]["total_ms"], 3)
        finally:
            pts.free()
            flags.free()
            d.free()
    return out


def run(prover, log_size):
    td = GC.trapdoor(500 + log_size)
    t, a, b = td["tau"], td["alpha"], td["beta"]
    n = 1 << log_size
    free = lambda s: s.free()
    unit_ms, unit_all = median_ms(prover, lambda: cp.Groth16Srs.unit(prover, log_size), free)
    unit = cp.Groth16Srs.unit(prover, log_size)
    try:
        srs = unit.contribute(t, a, b)
        try:
            weights = np.frombuffer(np.random.default_rng(log_size).bytes(16 * (5 * n - 5)), np.uint64).reshape(-1, 2) | np.uint64(1)
            weights = np.ascontiguousarray(weights)
            verdict, why = srs.check(weights)
            if verdict != 0:
                raise SystemExit("2^%d: the contributed SRS does not pass its check: verdict %d (%s): nothing is reported" % (log_size, verdict, why))
            contribute_ms, contribute_all = median_ms(prover, lambda: unit.contribute(t, a, b), free)
            points_ms, points_all = median_ms(prover, srs.points)
            check_ms, check_all = median_ms(prover, lambda: srs.check(weights))
            prof = {"unit": profiled(prover, lambda: cp.Groth16Srs.unit(prover, log_size), free),
                    "contribute": profiled(prover, lambda: unit.contribute(t, a, b), free),
                    "points": profiled(prover, srs.points), "check": profiled(prover, lambda: srs.check(weights))}
        finally:
            srs.free()
    finally:
        unit.free()
    uniform = k_scale_ms(prover, log_size, log_size)
    each = {k: v for k, v in prof["contribute"]["kernels_ms"].items() if k.startswith("srs_scale_each")}
    return {"log_size": log_size, "points": {"tau_g1": 2 * n - 1, "tau_g2": n, "alpha_tau_g1": n, "beta_tau_g1": n}, "check_verdict": 0,
            "unit_ms": round(unit_ms, 3), "contribute_ms": round(contribute_ms, 3), "points_ms": round(points_ms, 3), "check_ms": round(check_ms, 3),
            "all_ms": {"unit": [round(x, 3) for x in unit_all], "contribute": [round(x, 3) for x in contribute_all],
                       "points": [round(x, 3) for x in points_all], "check": [round(x, 3) for x in check_all]},
            "profiles": prof,
            "k_scale": {"point_scale_ms": uniform, "point_scale_sum_ms": round(sum(uniform.values()), 3), "scale_each_ms": each,
                        "scale_each_sum_ms": round(sum(each.values()), 3),
                        "scale_each_over_k_scale": round(sum(each.values()) / sum(uniform.values()), 3)}}


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    sizes = [int(x) for x in (args[0] if args else "12,16,20").split(",")]
    p = cp.Prover(0)
    out = {"tool": "tools/bench_groth16_srs_phase1.py", "method": "per size, one process: the contributed SRS passes check() with verdict 0, then for each "
           "of unit / contribute / points / check one warm-up call and the median of %d host-clocked calls, one profiled call, and the point_scale_* "
           "launches of inverse point transforms over arrays of the same sizes" % REPEATS, "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels()
                                   if any(s in r["name"] for s in ("g16srs::k_scale_each", "g16srs::k_fill", "g16srs::k_canonical", "pointntt::k_scale"))]
    except Exception as e:   # the LLVM tools are a convenience here, not a dependency of the measurement
        out["kernel_registers"] = "unavailable: %s" % e
    for k in sizes:
        out["sizes"].append(run(p, k))
        print("2^%d: contribute %.1f ms, check %.1f ms" % (k, out["sizes"][-1]["contribute_ms"], out["sizes"][-1]["check_ms"]), file=sys.stderr, flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "groth16_srs_phase1.json"), "w") as f:   # after every size: a long run leaves what it has
            json.dump(out, f, indent=1)
            f.write("\n")
    p.close()
    print(json.dumps(out))

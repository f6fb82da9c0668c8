#!/usr/bin/env python3
"""One cp_stark_prove_batch call of B traces against B cp_stark_prove calls (include/cityprover.h), at the shape of city-rollup's
SHA-256 `ByteStark` (tools/bench_stark_air.py: 418 + 912 columns, the seeded 10^4-op constraint program, a 912-store map, 304
cubic inversions, 912 prefix sums; rate_bits 1, 84 queries, 16-bit PoW) - the three STARKs of a block are three traces of one
AIR (city_rollup_circuit/src/sighash_circuits/sighash.rs:132-146).

Per (log_rows, B): both forms on the same build, the same context and the same host traces (the upload is inside the timed
window of both); a warm-up pair, then `reps` alternating pairs timed by the host clock around the calls (every call ends in a
stream synchronisation); medians, and the spread (min / max) of both; then one profiled run of each form for the per-kernel
split (cp_profile_begin / cp_profile_end: HIP events around every launch - a run of its own, its wall time is not reported). The
proofs of the two forms are compared byte for byte. A library without the batched entry point (an older build) is measured
in its single form alone. Writes profiles/stark_batch.json (or --out) and prints it.

usage: bench_stark_batch.py [--rows 10 11] [--batches 1 3 8] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import cityprover as cp  # noqa: E402
import air_programs as A  # noqa: E402
from bench_stark_air import K0, K1, programs  # noqa: E402
from bench_stark_fri import arity_for  # noqa: E402

HAS_BATCH = hasattr(cp, "stark_prove_batch")


def kernel_split(prof):
    return {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 4)} for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])
            if not k.startswith(("host:", "wait:"))}


def stats(ts):
    v = sorted(ts)
    return {"median_ms": v[len(v) // 2] * 1e3, "min_ms": v[0] * 1e3, "max_ms": v[-1] * 1e3}


def run(prover, log_rows, B, reps=10, seed=1):
    rb, ch, pow_bits, nq, q, na = 1, 4, 16, 84, 1, 2
    n = 1 << log_rows
    rng = np.random.default_rng(seed)
    cons_b, map_b = programs()
    cons, mp = cons_b.gpu(prover), map_b.gpu(prover)
    try:
        fri = cp.fri_params(log_rows, rb, ch, pow_bits, nq, arity_for(log_rows, rb, ch))
        desc, keep = cp.stark_desc(log_rows, q, na, fri, K0, cons, K1, 6, n_public=4,
                                   steps=[("map", mp), ("cubic_inverse", 0, K1 // 3, A.CUBIC_MODULUS), ("prefix_sum", 0, K1, False)])
        traces = [rng.integers(0, cp.P, size=(K0, n), dtype=np.uint64) for _ in range(B)]
        pubs = rng.integers(0, cp.P, (B, 4), dtype=np.uint64)
        challengers = lambda: [cp.ChallengerState().observe([i + 1]) for i in range(B)]

        def singles():
            chs = challengers()
            prover.sync()
            t0 = time.perf_counter()
            out = [cp.stark_prove(prover, desc, traces[i], chs[i], publics=pubs[i]) for i in range(B)]
            return time.perf_counter() - t0, out

        def batch():
            chs = challengers()
            prover.sync()
            t0 = time.perf_counter()
            out = cp.stark_prove_batch(prover, desc, traces, chs, publics=pubs)
            return time.perf_counter() - t0, out

        forms = [("singles", singles)] + ([("batch", batch)] if HAS_BATCH else [])
        proofs = {name: fn()[1] for name, fn in forms}                 # the warm-up pair
        times = {name: [] for name, _ in forms}
        for _ in range(reps):                                           # alternating: both forms see the same neighbours
            for name, fn in forms:
                times[name].append(fn()[0])
        split = {}
        for name, fn in forms:                                          # per-kernel time: a run of its own
            prover.profile_begin()
            try:
                fn()
            finally:
                split[name] = kernel_split(prover.profile_end())
        r = {"log_rows": log_rows, "B": B, "reps": reps, "proof_bytes": [len(x) for x in proofs["singles"]]}
        for name, _ in forms:
            r[name] = dict(stats(times[name]), kernels=split[name], kernel_ms=round(sum(v["total_ms"] for v in split[name].values()), 4))
        if HAS_BATCH:
            r["same_bytes"] = proofs["batch"] == proofs["singles"]
            r["batch_over_singles"] = r["batch"]["median_ms"] / r["singles"]["median_ms"]
            r["singles_spread"] = (r["singles"]["max_ms"] - r["singles"]["min_ms"]) / r["singles"]["median_ms"]
        return r
    finally:
        cons.close()
        mp.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10, 11])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_batch.json"))
    a = ap.parse_args()
    p = cp.Prover(0)
    try:
        res = {"what": "one cp_stark_prove_batch of B traces against B cp_stark_prove calls: SHA-256-STARK shape (418 + 912 columns), host traces, "
                       "same context; wall clock around the calls (upload included), median of `reps` alternating pairs after a warm-up pair; "
                       "kernels = HIP-event time per kernel name from one profiled run of each form",
               "has_batch_entry_point": HAS_BATCH,
               "cases": [run(p, k, B, a.reps) for k in a.rows for B in a.batches]}
    finally:
        p.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))

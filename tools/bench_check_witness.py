#!/usr/bin/env python3
"""What the witness checks cost beside the proving calls they sit in front of (include/cityprover.h "Does the witness satisfy the
circuit, and where not?"), in ONE process, device events around the calls, median of `reps` after a warm-up:
  * cp_circuit_check_witness_dev of B = 1 / 32 / 256 witnesses at the product shape (2^12 rows, 135 wires, 80 routed, the recursion
    gate mix of tools/bench_prove.py: the q-bench circuits' shape) beside cp_prove_batch of the same batch, with the quotient stage
    of that batch (the quotient_* kernels of the per-kernel profile) - the check evaluates each gate on n rows where the quotient
    evaluates 8 n points;
  * cp_air_check_rows_dev at 418 + 912 columns (the program of tools/bench_stark_air.py), 2^10 and 2^14 rows, beside cp_stark_prove
    of the same shape and its air_quotient kernel.
One JSON object on stdout; --out PATH also writes it there (profiles/check_witness.json is such a file)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("city-rollup_amd", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, d))
import numpy as np  # noqa: E402
import cityprover as cp  # noqa: E402
import air_programs as A  # noqa: E402
import bench_prove  # noqa: E402
import bench_stark_air  # noqa: E402
from bench_stark_fri import arity_for  # noqa: E402


def timed(prover, fn, reps):
    """median / min / max ms of fn() between two events on the context's stream, after one warm-up call"""
    fn()
    e0, e1 = prover.event(), prover.event()
    ms = []
    for _ in range(reps):
        prover.record(e0)
        fn()
        prover.record(e1)
        ms.append(prover.elapsed_ms(e0, e1))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": reps}


def kernels(prover, fn, prefix):
    prover.profile_begin()
    fn()
    prof = prover.profile_end()
    return {k: round(v["total_ms"], 4) for k, v in prof.items() if k.startswith(prefix)}


def plonky2(prover, batches, reps):
    n_circuits = 4
    cases = bench_prove.cases_for(prover, n_circuits, bench_prove.POSEIDON_FRACTION, "city_common")
    sh = cp.standard_recursion_shape(num_constants=cases[0]["num_constants"], num_public_inputs=len(cases[0]["public_inputs"]))
    circs = []
    for i, c in enumerate(cases):
        circ = cp.Circuit(prover, sh, [i, 1, 2, 3], c["cs_values"])
        cp.set_gates(circ, c["gate_list"], c["num_selectors"])
        circs.append(circ)
    out = []
    try:
        for B in batches:
            pick = [i % n_circuits for i in range(B)]
            wires = np.stack([cases[i]["wires"] for i in pick])
            wires[B // 2, 3, 1000] ^= 1       # one witness of the batch is broken: the reports are read, not only timed
            dw = prover.to_device(wires)
            try:
                args = ([circs[i] for i in pick], [cases[i]["public_inputs"] for i in pick], dw.ptr)
                reports = cp.check_witness_batch_dev(prover, *args)
                clean = [r["n_gate_violations"] + r["n_copy_violations"] + r["n_sigma_undecodable"] + r["n_noncanonical"] == 0 for r in reports]
                check = timed(prover, lambda: cp.check_witness_batch_dev(prover, *args), reps)
                prove = timed(prover, lambda: cp.prove_batch_dev(prover, *args), max(3, reps // 4))
                quot = kernels(prover, lambda: cp.prove_batch_dev(prover, *args), "quotient_")
                chk = kernels(prover, lambda: cp.check_witness_batch_dev(prover, *args), "check_")
                out.append({"B": B, "check_witness": check, "prove_batch": prove, "check_kernels_ms": chk, "check_kernels_total_ms": round(sum(chk.values()), 4),
                            "quotient_kernels_total_ms": round(sum(quot.values()), 4),
                            "check_over_prove": round(check["median_ms"] / prove["median_ms"], 4),
                            "check_kernels_over_quotient_kernels": round(sum(chk.values()) / sum(quot.values()), 4),
                            "witnesses_without_a_violation": sum(clean), "broken_witness_reported": not clean[B // 2]})
            finally:
                dw.free()
    finally:
        for c in circs:
            c.close()
    return {"shape": {"degree_bits": 12, "num_wires": 135, "num_routed_wires": 80, "gates": len(cases[0]["gate_list"]), "gate_mix": "recursion (tools/bench_prove.py)"},
            "cases": out}


def stark(prover, sizes, reps):
    K0, K1 = bench_stark_air.K0, bench_stark_air.K1
    rb, ch, pow_bits, nq, q, na = 1, 4, 16, 84, 1, 2
    cons_b, map_b = bench_stark_air.programs()
    cons, mp = cons_b.gpu(prover), map_b.gpu(prover)
    out = []
    try:
        for log_rows in sizes:
            n = 1 << log_rows
            rng = np.random.default_rng(log_rows)
            pub = rng.integers(0, cp.P, 4, dtype=np.uint64)
            cha = rng.integers(0, cp.P, 6, dtype=np.uint64)
            t0v = rng.integers(0, cp.P, size=(K0, n), dtype=np.uint64)
            cols = prover.to_device(rng.integers(0, cp.P, size=(K0 + K1, n), dtype=np.uint64))
            fri = cp.fri_params(log_rows, rb, ch, pow_bits, nq, arity_for(log_rows, rb, ch))
            desc, keep = cp.stark_desc(log_rows, q, na, fri, K0, cons, K1, 6, n_public=4,
                                       steps=[("map", mp), ("cubic_inverse", 0, K1 // 3, A.CUBIC_MODULUS), ("prefix_sum", 0, K1, False)])
            try:
                rows = lambda: cons.check_rows_dev(cols.ptr, n, pub, None, cha)
                trace = lambda: cp.stark_check_trace(prover, desc, t0v, pub, None, cha)
                prove = lambda: cp.stark_prove(prover, desc, t0v, cp.ChallengerState(), publics=pub)
                rep = rows()
                quot = kernels(prover, prove, "air_quotient")
                chk = kernels(prover, rows, "air_check")
                out.append({"log_rows": log_rows, "columns": [K0, K1], "sinks": len(rep["per_sink"]), "violations_of_a_random_trace": rep["n_violations"],
                            "air_check_rows_dev": timed(prover, rows, reps), "stark_check_trace_host_trace": timed(prover, trace, max(3, reps // 2)),
                            "stark_prove_host_trace": timed(prover, prove, max(3, reps // 4)), "air_check_kernels_ms": chk, "air_quotient_kernel_ms": quot})
            finally:
                cols.free()
    finally:
        cons.close()
        mp.close()
    return {"program": "tests/air_programs.py gadget_program(77, 418 + 912 columns, 10500 ops): the program of tools/bench_stark_air.py", "cases": out}


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = argv[argv.index("--out") + 1] if "--out" in argv else None
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 20
    p = cp.Prover(0)
    try:
        res = {"what": "witness checks beside the proving calls, one process, device events around the calls (tools/bench_check_witness.py)",
               "plonky2": plonky2(p, [1, 32, 256], reps), "stark": stark(p, [10, 14], reps)}
    finally:
        p.close()
    line = json.dumps(res)
    if path:
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)

#!/usr/bin/env python3
"""proofs/s of cp_verify_batch (the query phase on the device) beside n sequential cp_verify calls on the same proofs, in one
process and one run, on a synthetic circuit of the reference's shape (tools/bench_prove.py: standard_recursion_config, n = 2^12,
135 wires / 80 routed, 28 queries, arity 16 + 16, the city-common gate set), and the split of one cp_verify_batch call into its
host phase, staging + upload and the two kernels.

usage: bench_verify.py [--sizes 1,64,1024,4096] [--out profiles/verify_batch.json]

Every proof of a size is the same bytes in a buffer of its own (one witness is proved once): the host phase and the kernels walk n
distinct buffers, which is what a batch costs; the contents do not enter the time. Timed windows end in the call's own
synchronisation (both entry points return with the stream idle). The split comes from one profiled call (cp_profile_begin /
cp_profile_end: device events around each kernel, the host clock around each host phase; the upload is synchronised inside its
phase when profiling, so the split call is a little slower than the timed ones)."""
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
import bench_prove  # noqa: E402


def main():
    sizes = [1, 64, 1024, 4096]
    out_path = None
    argv = sys.argv[1:]
    for i, a in enumerate(argv):
        if a == "--sizes":
            sizes = [int(x) for x in argv[i + 1].split(",")]
        if a == "--out":
            out_path = argv[i + 1]
    prover = cp.Prover(0)
    case = bench_prove.cases_for(prover, 1, bench_prove.POSEIDON_FRACTION)[0]
    sh = cp.standard_recursion_shape(num_constants=case["num_constants"], num_public_inputs=len(case["public_inputs"]))
    circ = cp.Circuit(prover, sh, [7, 1, 2, 3], case["cs_values"])
    cp.set_gates(circ, case["gate_list"], case["num_selectors"])
    proof = cp.prove(circ, case["wires"], case["public_inputs"])
    cp.verify(circ, proof)
    lib = prover.lib
    res = {"shape": "standard_recursion_config, degree 2^12, 28 queries, arity 16 + 16", "proof_bytes": len(proof),
           "proofs": "one proof, n buffers of their own", "host_threads_at_most": 16, "sizes": {}}
    for n in sizes:
        bufs = [bytes(bytearray(proof)) for _ in range(n)]
        keep, ptrs, lens = cp._proof_array(bufs)
        out = np.zeros(n, cp.VERDICT)

        def batch():
            prover._check(lib.cp_verify_batch(circ.handle, ptrs, lens, n, 0, out.ctypes.data))
        batch()                                   # warm-up: code objects, the staging area at its size
        assert (out["status"] == 0).all()
        iters = max(2, min(50, 2048 // n))
        t0 = time.perf_counter()
        for _ in range(iters):
            batch()
        t_batch = (time.perf_counter() - t0) / iters
        prover.profile_begin()
        batch()
        prof = prover.profile_end()
        for b in bufs[:2]:
            cp.verify(circ, b)
        t0 = time.perf_counter()
        for b in bufs:
            prover._check(lib.cp_verify(circ.handle, b, len(b)))
        t_seq = time.perf_counter() - t0
        ms = lambda k: round(prof[k]["total_ms"], 4) if k in prof else None
        res["sizes"][str(n)] = {
            "verify_batch_ms_per_call": round(t_batch * 1e3, 4), "verify_batch_proofs_per_s": round(n / t_batch, 1), "timed_calls": iters,
            "sequential_cp_verify_ms": round(t_seq * 1e3, 4), "sequential_cp_verify_proofs_per_s": round(n / t_seq, 1),
            "split_of_one_profiled_call_ms": {
                "host_phase": ms("host:verify_host"), "staging_and_upload": ms("host:verify_upload"),
                "k_paths": ms("verify_paths"), "k_arith": ms("verify_arith"),
                "device_phase_wall": ms("host:verify_device"), "passes": prof["verify_paths"]["launches"]},
        }
        print(n, json.dumps(res["sizes"][str(n)]), flush=True)
    circ.close()
    prover.close()
    line = json.dumps(res, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

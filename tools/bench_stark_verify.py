#!/usr/bin/env python3
"""cp_stark_verify_batch against B calls of cp_stark_verify (include/cityprover.h), at the shape of city-rollup's SHA-256 `ByteStark`:
418 + 912 trace columns, rate_bits 1, cap height 4, 84 query rounds, 16-bit proof of work (tools/bench_stark_fri.py). A verifier
that meets a broken constraint stops before its query phase, so the AIR here is a SATISFIED one of that shape: trace column 0 a
recurrence, every other trace column a product and a sum of earlier ones, every extended column a trace column times a round
challenge plus another (one map step) - a few thousand recorded ops, one trace for all proofs, told apart by their transcripts.

Per (log_rows, B): B proofs from cp_stark_prove_batch (64 per call), then
  host    B calls of cp_stark_verify, each timed on its own (one thread, no device): what a caller had before
  lane    one cp_stark_verify_batch with CP_PATHS_LANE (one lane per Merkle path)
  coop    ... with CP_PATHS_COOP (twelve lanes per path)
  auto    ... with CP_PATHS_AUTO (the library's choice)
A warm-up round, then `reps` rounds of the three batch forms in turn, host clock around the call (it ends in a stream
synchronisation); median, min and max. The host verifier is repeated `host_reps` times (fewer at the large B, where one round is
already hundreds of calls; the JSON says how many). Then one profiled call per form (cp_profile_begin / cp_profile_end) for the
split into host phase, upload and device phase and the kernels' own time: a run of its own, its wall time is not reported.
Every verdict is checked: all accepted. Writes profiles/stark_verify_batch.json (or --out) and prints it.

--one-pass B ...: those batches once more as ONE device pass each (chunk_proofs = B), at the first of --rows: the default passes of
this shape hold 64 proofs, and the two path kernels cross above that.

usage: bench_stark_verify.py [--rows 10 12] [--batches 1 3 16 64 256] [--one-pass 128 256] [--reps 7] [--out FILE]"""
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
from bench_stark_fri import arity_for  # noqa: E402

K0, K1, N_RCH = 418, 912, 2
P = cp.P
FORMS = (("lane", cp.PATHS_LANE), ("coop", cp.PATHS_COOP), ("auto", cp.PATHS_AUTO))


def satisfied_air(seed=5):
    """-> (constraints builder, map builder, trace(n))"""
    rng = np.random.default_rng(seed)
    r = lambda: int(rng.integers(1, P, dtype=np.uint64))
    a, first = r(), r()
    spec = [(int(rng.integers(0, j)), int(rng.integers(0, j)), int(rng.integers(0, j)), r(), r()) for j in range(1, K0)]
    ext = [(int(rng.integers(0, K0)), int(rng.integers(0, K0)), e % N_RCH) for e in range(K1)]
    c = A.Builder(A.CONSTRAINTS, K0 + K1, n_challenge=N_RCH)
    c0 = c.local(0)
    c.assert_zero(c.sub(c.next(0), c.add(c.mul(c0, c0), c.const(a))), "transition")
    c.assert_zero(c.sub(c.local(0), c.const(first)), "first")
    for j, (x, y, z, m, e) in enumerate(spec, 1):
        c.assert_zero(c.sub(c.local(j), c.add(c.add(c.mul(c.local(x), c.local(y)), c.mul(c.const(m), c.local(z))), c.const(e))), "all")
    mp = A.Builder(A.MAP, K0 + K1, n_challenge=N_RCH, n_out_columns=K1)
    for e, (x, y, ci) in enumerate(ext):
        c.assert_zero(c.sub(c.local(K0 + e), c.add(c.mul(c.local(x), c.challenge(ci)), c.local(y))), "all")
        mp.store(e, mp.add(mp.mul(mp.local(x), mp.challenge(ci)), mp.local(y)))

    def trace(n):
        t = np.zeros((K0, n), dtype=object)
        t[0, 0] = first
        for i in range(1, n):
            t[0, i] = (t[0, i - 1] * t[0, i - 1] + a) % P
        for j, (x, y, z, m, e) in enumerate(spec, 1):
            t[j] = (t[x] * t[y] + m * t[z] + e) % P
        return t.astype(np.uint64)
    return c, mp, trace


def stats(ts):
    v = sorted(ts)
    return {"median_ms": round(v[len(v) // 2] * 1e3, 4), "min_ms": round(v[0] * 1e3, 4), "max_ms": round(v[-1] * 1e3, 4), "n": len(v)}


def split(prof):
    host = {k[5:]: round(v["total_ms"], 4) for k, v in prof.items() if k.startswith("host:")}
    kern = {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 4)} for k, v in prof.items() if not k.startswith(("host:", "wait:"))}
    return {"phases_ms": host, "kernels": kern}


def prove(prover, desc, trace, B):
    proofs = []
    for base in range(0, B, 64):
        m = min(64, B - base)
        chs = [cp.ChallengerState().observe([base + i + 1]) for i in range(m)]
        proofs += cp.stark_prove_batch(prover, desc, [trace] * m, chs)
    return proofs


def run(prover, desc, trace, log_rows, B, reps, one_pass=False):
    """one_pass: chunk_proofs = B, so that the whole batch is one device pass whatever its bytes (the default passes hold 64 MiB:
    64 proofs of this shape) - the sizes that place the library's threshold between the two path kernels; no host verifier"""
    proofs = prove(prover, desc, trace, B)
    chunk = B if one_pass else 0
    challengers = lambda: [cp.ChallengerState().observe([i + 1]) for i in range(B)]
    host_reps = 3 if B <= 16 else 1

    def host():
        chs = challengers()
        per = []
        for i in range(B):
            t0 = time.perf_counter()
            cp.stark_verify(desc, chs[i], proofs[i])
            per.append(time.perf_counter() - t0)
        return per, [c.as_tuple() for c in chs]

    def batch(form):
        chs = challengers()
        prover.sync()
        t0 = time.perf_counter()
        v = cp.stark_verify_batch(prover, desc, chs, proofs, path_form=form, chunk=chunk)
        dt = time.perf_counter() - t0
        assert all(x == (0, -1, -1) for x in v), v
        return dt, [c.as_tuple() for c in chs]

    per, want_ch = host()                                               # warm-up round, also the correctness gate
    for _, form in FORMS:
        assert batch(form)[1] == want_ch, "challengers differ from cp_stark_verify's"
    per_call, totals = (list(per), [sum(per)]) if one_pass else ([], [])   # one pass: the warm-up round is the host verifier's only one
    for _ in range(0 if one_pass else host_reps):
        per = host()[0]
        per_call += per
        totals.append(sum(per))
    times = {name: [] for name, _ in FORMS}
    for _ in range(reps):                                               # in turn: every form sees the same neighbours
        for name, form in FORMS:
            times[name].append(batch(form)[0])
    r = {"log_rows": log_rows, "B": B, "proof_bytes": len(proofs[0]), "paths_per_pass": min(B, B if one_pass else (64 << 20) // len(proofs[0])) * 84,
         "one_pass": one_pass, "host_reps": 1 if one_pass else host_reps,
         "host": dict(stats(totals), per_call=stats(per_call), per_proof_ms=round(sorted(totals)[len(totals) // 2] * 1e3 / B, 4))}
    for name, form in FORMS:
        prover.profile_begin()
        try:
            batch(form)
        finally:
            prof = split(prover.profile_end())
        st = stats(times[name])
        r[name] = dict(st, per_proof_ms=round(st["median_ms"] / B, 4), spread=round((st["max_ms"] - st["min_ms"]) / st["median_ms"], 4), **prof)
    r["host_over_best_batch"] = round(r["host"]["median_ms"] / min(r[n]["median_ms"] for n, _ in FORMS), 2)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 3, 16, 64, 256])
    ap.add_argument("--one-pass", type=int, nargs="*", default=[128, 256], help="batches also verified as ONE device pass (first --rows only)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_verify_batch.json"))
    a = ap.parse_args()
    p = cp.Prover(0)
    cases = []
    try:
        cons_b, map_b, trace_of = satisfied_air()
        cons, mp = cons_b.gpu(p), map_b.gpu(p)
        try:
            for k in a.rows:
                fri = cp.fri_params(k, 1, 4, 16, 84, arity_for(k, 1, 4))
                desc, keep = cp.stark_desc(k, 1, 2, fri, K0, cons, K1, N_RCH, steps=[("map", mp)])
                trace = trace_of(1 << k)
                for B, one in [(B, False) for B in a.batches] + [(B, True) for B in a.one_pass if k == a.rows[0]]:
                    cases.append(run(p, desc, trace, k, B, a.reps, one))
                    print("# rows 2^%d B %d: host %.2f ms/proof, lane %.3f, coop %.3f, auto %.3f" % (
                        k, B, cases[-1]["host"]["per_proof_ms"], cases[-1]["lane"]["per_proof_ms"], cases[-1]["coop"]["per_proof_ms"],
                        cases[-1]["auto"]["per_proof_ms"]), file=sys.stderr, flush=True)
        finally:
            cons.close()
            mp.close()
    finally:
        p.close()
    res = {"what": "cp_stark_verify_batch (one lane per path / twelve lanes per path / the library's choice) against B calls of cp_stark_verify: "
                   "a satisfied synthetic AIR of the SHA-256 STARK's shape (418 + 912 columns, rate_bits 1, cap height 4, 84 queries, 16-bit PoW); "
                   "wall clock around the calls, median of `n` runs after a warm-up round; phases_ms / kernels from one profiled call per form",
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))

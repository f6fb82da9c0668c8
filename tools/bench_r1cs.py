#!/usr/bin/env python3
"""Timing of the device-resident R1CS (cp_r1cs_bls12381_eval_dev / _check_dev, cp_groth16_prove_r1cs_bls12381) at 2^k constraints
against what a caller without it needs at the least: the upload of the three evaluation arrays (one cp_h2d of 3 x 32 B x 2^k from
page-locked memory). Correctness is tests/test_gpu_r1cs.py; this only measures. Prints one JSON line.

The system is synthetic, seeded, satisfied by construction and built in numpy (no pass of Python integers: 2^24 constraints
take seconds to generate). n wires = n constraints; the first half of the wires are booleans (0 / 1), the rest uniform below 2^254. Constraints:
  45 %  linear    A = a combination of 1..6 terms, B = wire 0, C = the same combination, reversed
  35 %  boolean   A = w_b, B = w_b - wire 0, C empty                       (b (b - 1) = 0)
  20 %  scaled    A = a combination, B = k * wire 0 (k one limb), C = the combination with every coefficient times k
Coefficients of a combination: 40 % +1, 20 % -1, 15 % one limb (either sign), 25 % full width; 35 % of the terms on wire 0.
Row length: three linear constraints are long (300, 5 000 and 100 000 terms), the rest as above.

usage: bench_r1cs.py [log sizes, comma separated: default 16,20,24] [--reps N] [--no-prove]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import cityprover as cp  # noqa: E402

R = (lambda x: x**4 - x**2 + 1)(-0xd201000000010000)   # the group order
HBM_BYTES_PER_S = 8e12                                   # the figure the project's other profiles are held against
LONG = (300, 5_000, 100_000)


def limbs4(vals):
    return np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def synthetic_system(log_n, seed=None):
    n = 1 << log_n
    rng = np.random.default_rng(log_n if seed is None else seed)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % R
    base = [1, R - 1] + [2, 3, 5, 12345, (1 << 28) - 1] + [R - 2, R - 7, R - 65537] + [rand() for _ in range(24)]
    scales = [2, 3, 12345]
    table = list(base)
    times = np.zeros((len(scales), len(base)), np.int64)          # index of base[c] * scales[s] in the table
    for si, k in enumerate(scales):
        for ci, c in enumerate(base):
            v = c * k % R
            if v not in table:
                table.append(v)
            times[si, ci] = table.index(v)
    one, minus_one, one_limb, full = 0, 1, np.arange(2, 10), np.arange(10, len(base))
    scale_idx = np.array([table.index(k) for k in scales])
    # witness: wire 0 = 1, booleans in the first half, uniform 254-bit values in the second
    half = max(n // 2, 2)
    w = rng.integers(0, 2**64, (n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 62) - 1)
    w[:half, 1:] = 0
    w[:half, 0] = rng.integers(0, 2, half, dtype=np.uint64)
    w[0] = (1, 0, 0, 0)
    u = rng.random(n)
    kind = np.where(u < 0.45, 0, np.where(u < 0.80, 1, 2))        # 0 linear, 1 boolean, 2 scaled
    la = rng.integers(1, 7, n)
    for pos, ln in zip((n // 2, n // 3, (2 * n) // 3), LONG):
        if n >= 8:
            kind[pos], la[pos] = 0, ln
    len_a = np.where(kind == 1, 1, la)
    len_b = np.where(kind == 1, 2, 1)
    len_c = np.where(kind == 1, 0, la)
    ptr = lambda lens: np.concatenate([np.zeros(1, np.int64), np.cumsum(lens.astype(np.int64))])
    pa, pb, pc = ptr(len_a), ptr(len_b), ptr(len_c)
    ta = int(pa[-1])
    col_a = rng.integers(0, n, ta)
    col_a[rng.random(ta) < 0.35] = 0
    v = rng.random(ta)
    k_a = full[rng.integers(0, len(full), ta)]
    k_a[v < 0.40] = one
    k_a[(v >= 0.40) & (v < 0.60)] = minus_one
    pick = (v >= 0.60) & (v < 0.75)
    k_a[pick] = one_limb[rng.integers(0, len(one_limb), int(pick.sum()))]
    boolean = kind == 1
    wire_b = rng.integers(1, half, int(boolean.sum()))
    col_a[pa[:-1][boolean]], k_a[pa[:-1][boolean]] = wire_b, one
    # B
    col_b, k_b = np.zeros(int(pb[-1]), np.int64), np.full(int(pb[-1]), one, np.int64)
    col_b[pb[:-1][boolean]] = wire_b
    k_b[pb[:-1][boolean] + 1] = minus_one
    scaled = kind == 2
    which = rng.integers(0, len(scales), n)
    k_b[pb[:-1][scaled]] = scale_idx[which[scaled]]
    # C: the A row backwards (linear, scaled), coefficients through the product table where scaled
    off = np.arange(int(pc[-1]), dtype=np.int64) - np.repeat(pc[:-1], len_c)
    src = np.repeat(pa[:-1] + len_a - 1, len_c) - off
    col_c, k_c = col_a[src], k_a[src]
    sc = np.repeat(scaled, len_c)
    k_c[sc] = times[np.repeat(which, len_c)[sc], k_c[sc]]
    mats = [(p.astype(np.uint64), c.astype(np.uint32), k.astype(np.uint32)) for p, c, k in ((pa, col_a, k_a), (pb, col_b, k_b), (pc, col_c, k_c))]
    return {"n": n, "n_wires": n, "coeffs": limbs4(table), "mats": mats, "w": w}


def timed(prover, fn, warm, reps):
    """median of `reps` device-event timings of fn (ms), after `warm` untimed calls"""
    for _ in range(warm):
        fn()
    prover.sync()
    e0, e1 = prover.event(), prover.event()
    ts = []
    for _ in range(reps):
        prover.record(e0)
        fn()
        prover.record(e1)
        ts.append(prover.elapsed_ms(e0, e1))
    for e in (e0, e1):
        prover.lib.cp_event_destroy(prover.ctx, e)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def synthetic_key(prover, n, log_n, n_pub=16):
    from bench_msm import G, G2
    sets = [cp.G1Points.synthetic(prover, G, 3, 1, n), cp.G1Points.synthetic(prover, G, 5, 2, n), cp.G2Points.synthetic(prover, G2, 7, 3, n),
            cp.G1Points.synthetic(prover, G, 11, 4, n), cp.G1Points.synthetic(prover, G, 13, 5, n)]
    pk = cp.Groth16Pk()
    pk.n_wires, pk.n_private, pk.log_domain = n, n - n_pub, log_n
    pk.a_g1, pk.b_g1, pk.b_g2, pk.k_g1, pk.z_g1 = (s.buf.ptr for s in sets)
    pk.a_inf = pk.b_inf = None
    g1 = [(int(G[h]) >> (64 * i)) & (2**64 - 1) for h in range(2) for i in range(6)]
    g2 = [(int(c) >> (64 * i)) & (2**64 - 1) for c in (G2[0][0], G2[0][1], G2[1][0], G2[1][1]) for i in range(6)]
    pk.alpha_g1[:], pk.beta_g1[:], pk.delta_g1[:] = g1, g1, g1
    pk.beta_g2[:], pk.delta_g2[:] = g2, g2
    return pk, sets


def run(prover, log_n, reps=10, prove=True):
    n = 1 << log_n
    t0 = time.perf_counter()
    s = synthetic_system(log_n)
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    r1cs = cp.R1cs(prover, s["n"], s["n_wires"], s["coeffs"], s["mats"])
    t_create = time.perf_counter() - t0
    plain = cp.R1cs(prover, s["n"], s["n_wires"], s["coeffs"], s["mats"], flags=cp.R1CS_NO_TERM_CLASSES)
    info = r1cs.info
    cls = list(info.n_terms_class)
    terms = sum(cls[1:])
    dw = prover.to_device(s["w"])
    ev = [prover.alloc(4 * n) for _ in range(3)]
    out = {"log_constraints": log_n, "wires": n, "terms": {"A": info.nnz[0], "B": info.nnz[1], "C": info.nnz[2]},
           "term_classes": dict(zip(("zero_dropped", "plus_one", "minus_one", "one_limb", "minus_one_limb", "general"), cls)),
           "rows": {"short": info.n_short_rows, "long": info.n_long_rows, "longest": info.longest_row, "long_row_threshold": info.long_row_threshold},
           "device_bytes": info.device_bytes, "generate_s": round(t_gen, 2), "create_s": round(t_create, 2), "reps": reps}
    # the two builds of the system alternate, as the measuring guide asks of an A/B
    ab = {"classes": [], "no_classes": []}
    for _ in range(3):
        ab["classes"].append(timed(prover, lambda: r1cs.eval_dev(dw.ptr, *(b.ptr for b in ev)), 2, reps)[0])
        ab["no_classes"].append(timed(prover, lambda: plain.eval_dev(dw.ptr, *(b.ptr for b in ev)), 2, reps)[0])
    plain.free()
    med, lo, hi = timed(prover, lambda: r1cs.eval_dev(dw.ptr, *(b.ptr for b in ev)), 2, reps)
    out["eval_ms"] = {"median": med, "min": lo, "max": hi}
    out["eval_ab_ms"] = {"term_classes_on": sorted(ab["classes"])[1], "term_classes_off": sorted(ab["no_classes"])[1]}
    assert r1cs.check(dw.ptr) == (0, None), "the synthetic system is not satisfied"
    med, lo, hi = timed(prover, lambda: r1cs.check(dw.ptr), 1, reps)
    out["check_ms"] = {"median": med, "min": lo, "max": hi}
    out["terms_per_s"] = terms / (out["eval_ms"]["median"] * 1e-3)
    out["gathered_bytes_per_s"] = 32 * out["terms_per_s"]
    out["gathered_share_of_hbm_8TBs"] = out["gathered_bytes_per_s"] / HBM_BYTES_PER_S
    # the parent's least cost: the three arrays, already computed and in page-locked memory, uploaded in one copy
    nbytes = 3 * 32 * n
    host = ctypes.c_void_p()
    prover._check(prover.lib.cp_host_alloc(prover.ctx, nbytes, ctypes.byref(host)))
    dst = prover.alloc(3 * 4 * n)
    for k in range(3):
        prover._check(prover.lib.cp_d2h(prover.ctx, host.value + k * 32 * n, ev[k].ptr, 32 * n))     # the real evaluations
    med, lo, hi = timed(prover, lambda: prover._check(prover.lib.cp_h2d(prover.ctx, dst.ptr, host.value, nbytes)), 1, max(3, reps // 2))
    out["upload_3_arrays_ms"] = {"median": med, "min": lo, "max": hi, "bytes": nbytes, "gb_per_s": nbytes / (med * 1e-3) / 1e9}
    out["eval_faster_than_upload"] = bool(out["eval_ms"]["median"] < med)
    prover.lib.cp_host_free(prover.ctx, host)
    dst.free()
    if prove:
        pk, sets = synthetic_key(prover, n, log_n)
        rr, ss = 12345, 67890
        t_old, t_new = [], []
        for it in range(4):                      # the first pair warms both routes up
            r1cs.eval_dev(dw.ptr, *(b.ptr for b in ev))
            prover.sync()
            t0 = time.perf_counter()
            old = cp.groth16_prove(prover, pk, dw.ptr, ev[0].ptr, ev[1].ptr, ev[2].ptr, rr, ss)
            t_old.append(time.perf_counter() - t0)
            if it == 3:
                prover.profile_begin()
            t0 = time.perf_counter()
            new = cp.groth16_prove_r1cs(prover, pk, r1cs, dw.ptr, rr, ss)
            t_new.append(time.perf_counter() - t0)
            if it == 3:
                prof = prover.profile_end()
            assert old == new, "the two routes gave different proofs"
        med = lambda ts: sorted(ts[1:])[1] * 1e3
        front = sum(v["total_ms"] for k, v in prof.items() if k.startswith("r1cs_"))
        out["prove_ms_evaluations_given"] = med(t_old)
        out["prove_r1cs_ms"] = med(t_new)
        out["prove_r1cs_over_prove"] = med(t_new) / med(t_old)
        out["r1cs_kernels_ms_in_prove_r1cs"] = {k: round(v["total_ms"], 3) for k, v in prof.items() if k.startswith("r1cs_")}
        out["share_of_prove_r1cs_in_evaluation_and_check"] = front / (t_new[3] * 1e3)
        for x in sets:
            x.free()
    for d in [dw] + ev:
        d.free()
    r1cs.free()
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="?", default="16,20,24")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-prove", action="store_true")
    a = ap.parse_args()
    p = cp.Prover(0)
    res = [run(p, int(x), reps=a.reps, prove=not a.no_prove) for x in a.sizes.split(",")]
    p.close()
    print(json.dumps({"bench": "r1cs", "results": res}))

#!/usr/bin/env python3
"""Timing of cp_groth16_verify_bls12381 and cp_pairing_product_bls12381. Correctness is tests/test_gpu_groth16_verify.py and
tests/test_gpu_pairing.py; this only measures. The key is made from a trapdoor by the oracle (3 public wires); 64 distinct valid
proofs are simulated from it and tiled to the batch size (the kernels' work does not depend on the values, except for the bits
of the public inputs, which are full width). Per batch size, with and without CP_PAIRING_TRUSTED:
  wall_ms        host clock around the whole call - staging, kernels, verdicts back: one warm-up call, median / min / max of --reps
  kernels        one further call under cp_profile_begin / cp_profile_end: device-event time of every launch by name
  fp_products    F_p products per item counted from the formulas of pairing.h (fp_product_counts below shows the count) and the
                 rate they give over the summed kernel time
The same for bare pairings (k = 1). Prints one JSON line and writes profiles/pairing.json.

usage: bench_pairing.py [batch sizes, comma separated: default 1,64,4096,65536] [--reps N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "city-rollup_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cityprover as cp  # noqa: E402
import pairing_cases as PC  # noqa: E402
import pairing_ref as PR  # noqa: E402

R, P = PR.R, PR.P
N_PUBLIC = 3


def fp_product_counts(n_public=N_PUBLIC):
    """F_p products (squarings count as one) per item, from the formulas of pairing.h and bls12_381.h"""
    m2, s2, mf = 3, 2, 2                      # F_p^2 product (Karatsuba), square, product by an F_p element
    f12_mul, f12_sqr, sparse = 36 * m2, 15 * m2 + 6 * s2, 18 * m2
    dbl_step, add_step = 6 * s2 + 5 * m2 + 2 * mf, 3 * s2 + 10 * m2 + 2 * mf
    adds_x = bin(PR.X_ABS).count("1") - 1     # 5
    miller = 63 * (f12_sqr + sparse + dbl_step) + adds_x * (sparse + add_step)
    fp_inv = 381 + bin(P - 2).count("1")      # square-and-multiply over the bits of p - 2
    f6_mul = 9 * m2
    f6_inv = 3 * s2 + 9 * m2 + (2 + fp_inv + 2)
    f12_inv = 2 * f6_mul + f6_inv + 2 * f6_mul
    frob = 6 * m2
    easy = f12_inv + 2 * f12_mul + frob
    exp_x = 63 * 9 * s2 + adds_x * f12_mul
    hard = 5 * exp_x + 7 * f12_mul + 2 * frob + 9 * s2
    adds_r = bin(R).count("1") - 1
    g1_dbl, g1_add, g2_dbl, g2_add = 5 + 2, 3 + 8, 5 * s2 + 2 * m2, 3 * s2 + 8 * m2
    check_g1, check_g2 = 254 * g1_dbl + adds_r * g1_add + 6, 254 * g2_dbl + adds_r * g2_add + 4 + 2 * m2 + s2
    public_sum = (n_public - 1) * (255 * g1_dbl + 128 * g1_add + 16) + fp_inv + 5
    verify_trusted = 3 * miller + 2 * f12_mul + easy + hard + public_sum + 2 * 6 + (4 + 2 * m2 + s2)
    return {"miller_loop": miller, "final_exponentiation": easy + hard, "subgroup_check_g1": check_g1, "subgroup_check_g2": check_g2,
            "public_input_sum": public_sum, "pairing_trusted": miller + easy + hard, "pairing_checked": miller + easy + hard + check_g1 + check_g2,
            "verify_trusted": verify_trusted, "verify_checked": verify_trusted + 2 * check_g1 + check_g2}


def make_key_and_proofs(prover, pool=64):
    rng = np.random.default_rng(2024)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1
    td = {k: rnd() for k in ("alpha", "beta", "gamma", "delta")}
    ic = [rnd() for _ in range(N_PUBLIC)]
    vk = cp.Groth16Vk()
    vk.alpha_g1[:] = PC.g1_words(PC.g1_mul(td["alpha"])).tolist()
    for name in ("beta", "gamma", "delta"):
        getattr(vk, name + "_g2")[:] = PC.g2_words(PC.g2_mul(td[name])).tolist()
    vk.n_public = N_PUBLIC
    verifier = cp.Groth16Verifier.create(prover, vk, np.stack([PC.g1_words(PC.g1_mul(x)) for x in ic]))
    proofs, pubs = [], []
    for _ in range(pool):
        xs = [rnd() for _ in range(N_PUBLIC - 1)]
        a, b = rnd(), rnd()
        c = (a * b - td["alpha"] * td["beta"] - td["gamma"] * (ic[0] + sum(x * y for x, y in zip(xs, ic[1:])))) * pow(td["delta"], -1, R) % R
        proofs.append(np.concatenate([PC.g1_words(PC.g1_mul(a)), PC.g2_words(PC.g2_mul(b)), PC.g1_words(PC.g1_mul(c))]))
        pubs.append(np.array([[(x >> (64 * j)) & PC.MASK for j in range(4)] for x in xs], np.uint64))
    return verifier, np.stack(proofs), np.stack(pubs)


def measure(prover, call, reps, n, products):
    call()                                   # warm-up
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    prover.profile_begin()
    call()
    prof = prover.profile_end()
    kernels = {k: round(v["total_ms"], 4) for k, v in prof.items() if k.startswith("pairing_")}
    kernel_ms = sum(kernels.values())
    wall.sort()
    med = wall[len(wall) // 2]
    return {"wall_ms": {"median": round(med, 3), "min": round(wall[0], 3), "max": round(wall[-1], 3)}, "items_per_s": round(n / med * 1e3, 1),
            "kernels_ms": kernels, "kernels_total_ms": round(kernel_ms, 3), "fp_products_per_item": products,
            "fp_products_per_s_over_kernel_time": round(n * products / kernel_ms * 1e3) if kernel_ms else None}


def run(prover, verifier, proofs, pubs, n, reps, counts):
    idx = np.arange(n) % len(proofs)
    pr, pu = np.ascontiguousarray(proofs[idx]), np.ascontiguousarray(pubs[idx])
    g1, g2 = np.ascontiguousarray(pr[:, :12]), np.ascontiguousarray(pr[:, 12:36])
    out = {"n": n}
    for name, flags in (("checked", 0), ("trusted", cp.PAIRING_TRUSTED)):
        def verify():
            v = verifier.verify(pr, pu, flags=flags)
            assert not v.any()
        out["verify_" + name] = measure(prover, verify, reps, n, counts["verify_" + name])
        out["pairing_" + name] = measure(prover, lambda: cp.pairing_product(prover, g1, g2, flags=flags, want_gt=False), reps, n, counts["pairing_" + name])
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sizes = [int(x) for x in (args[0] if args else "1,64,4096,65536").split(",")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    p = cp.Prover(0)
    counts = fp_product_counts()
    out = {"tool": "tools/bench_pairing.py", "method": "one warm-up call; wall = host clock around the synchronous call (staging and verdict copies included), "
           "median of reps; kernels = device events of one further profiled call", "n_public": N_PUBLIC, "fp_product_counts": counts,
           "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels() if "pairing" in r["name"]]
    except Exception as e:   # the LLVM tools are a convenience here, not a dependency of the measurement
        out["kernel_registers"] = "unavailable: %s" % e
    verifier, proofs, pubs = make_key_and_proofs(p)
    for n in sizes:
        out["sizes"].append(run(p, verifier, proofs, pubs, n, reps, counts))
    verifier.close()
    p.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pairing.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))

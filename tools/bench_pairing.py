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

With --city, instead: the stored 192-byte form at the same batch sizes (run_city below), written to profiles/pairing_city.json.

With --all, instead: cp_groth16_verify_all_bls12381 (one final exponentiation for the batch) against the per-proof function on the
same proofs (run_all below), and at the largest size a batch with one bad proof; written to profiles/groth16_verify_all.json.

usage: bench_pairing.py [batch sizes, comma separated: default 1,64,4096,65536] [--reps N] [--city | --all]"""
import ctypes
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


HOST_LOOP_CAP = 1024   # proofs the host loop of --city decompresses per repeat (about half a millisecond each, one thread)


def words_to_proof(w):
    val = lambda x: sum(int(v) << (64 * j) for j, v in enumerate(x))
    return (val(w[0:6]), val(w[6:12])), ((val(w[12:18]), val(w[18:24])), (val(w[24:30]), val(w[30:36]))), (val(w[36:42]), val(w[42:48]))


def run_city(prover, verifier, proofs, pubs, n, reps):
    """The stored form (4 x 48 bytes a proof) at batch size n, all in this process, the legs alternating within a repeat:
      a  verify on coordinates that are already unpacked (the path that existed before the stored form was taken on the device)
      b  a host loop of cp_groth16_proof_unpack_city, alone, and followed by a: what a holder of stored proofs did before
      c  verify_city
      d  the device unpack alone (cp_groth16_proofs_unpack_city_bls12381)
    The host loop runs over min(n, HOST_LOOP_CAP) proofs and is scaled to n (its time per proof does not depend on n)."""
    lib = prover.lib
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    blobs64 = np.stack([np.frombuffer(cp.groth16_pack_city(*words_to_proof(w)), np.uint8) for w in proofs])
    idx = np.arange(n) % len(proofs)
    pr, pu, bl = np.ascontiguousarray(proofs[idx]), np.ascontiguousarray(pubs[idx]), np.ascontiguousarray(blobs64[idx])
    n_host = min(n, HOST_LOOP_CAP)
    host_out = np.zeros((n_host, 48), np.uint64)

    def host_loop():
        for i in range(n_host):
            row = host_out[i]
            rc = lib.cp_groth16_proof_unpack_city(bl[i].ctypes.data_as(u8p), row[0:12].ctypes.data_as(u64p), row[12:36].ctypes.data_as(u64p),
                                                  row[36:48].ctypes.data_as(u64p))
            assert rc == 0

    def a():
        assert not verifier.verify(pr, pu).any()

    def c():
        assert not verifier.verify_city(bl, pu).any()

    def d():
        coords, status = cp.groth16_unpack_city_batch(prover, bl)
        assert not status.any()
        return coords

    assert (d() == pr).all()                                     # the same proofs on every path
    host_loop()
    assert (host_out == pr[:n_host]).all()
    legs = {"a_verify_unpacked": a, "b_host_unpack_loop": host_loop, "c_verify_city": c, "d_device_unpack": d}
    for f in legs.values():
        f()                                                      # warm-up of every shape
    walls = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            walls[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in walls.items()}
    out = {"n": n, "reps": reps, "wall_ms": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in walls.items()}}
    host_per_proof_us = med["b_host_unpack_loop"] / n_host * 1e3
    b_total = host_per_proof_us * n / 1e3
    out["b_host_loop"] = {"proofs_timed": n_host, "us_per_proof": round(host_per_proof_us, 2), "ms_scaled_to_n": round(b_total, 3),
                          "then_a_ms": round(b_total + med["a_verify_unpacked"], 3), "then_a_is": "the sum of the two medians"}
    out["us_per_proof"] = {"a": round(med["a_verify_unpacked"] / n * 1e3, 3), "b_then_a": round((b_total + med["a_verify_unpacked"]) / n * 1e3, 3),
                           "c": round(med["c_verify_city"] / n * 1e3, 3), "d": round(med["d_device_unpack"] / n * 1e3, 3)}
    out["c_over_a"] = round(med["c_verify_city"] / med["a_verify_unpacked"], 4)
    out["c_minus_a_us_per_proof"] = round((med["c_verify_city"] - med["a_verify_unpacked"]) / n * 1e3, 3)
    out["b_then_a_over_c"] = round((b_total + med["a_verify_unpacked"]) / med["c_verify_city"], 3)
    prover.profile_begin()
    c()
    prof = prover.profile_end()
    out["c_kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in prof.items() if k.startswith(("pairing_", "groth16_unpack_"))}
    return out


def main_city(sizes, reps):
    p = cp.Prover(0)
    out = {"tool": "tools/bench_pairing.py --city", "method": "one process; per batch size every leg is warmed up once, then the legs alternate within each "
           "of `reps` repeats; wall = host clock around the synchronous call (staging and result copies included); the host loop is timed over "
           "min(n, %d) proofs and scaled to n; kernels = device events of one further profiled verify_city call" % HOST_LOOP_CAP,
           "n_public": N_PUBLIC, "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels() if "k_unpack" in r["name"]]
    except Exception as e:
        out["kernel_registers"] = "unavailable: %s" % e
    verifier, proofs, pubs = make_key_and_proofs(p)
    for n in sizes:
        out["sizes"].append(run_city(p, verifier, proofs, pubs, n, reps))
        print("city", json.dumps(out["sizes"][-1]), flush=True)
    verifier.close()
    p.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pairing_city.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def run_all(prover, verifier, proofs, pubs, n, reps):
    """cp_groth16_verify_all_bls12381 against cp_groth16_verify_bls12381 on the same n valid proofs, one process, the two legs
    alternating within a repeat, with and without CP_PAIRING_TRUSTED. The ratio is all / per_proof: below 1 the aggregated path
    wins. one_bad (asked for at the largest size): the same batch with the C of one proof swapped for its neighbour's, which
    sends verify_all down the fallback path - the aggregated attempt, then the per-proof check."""
    rng = np.random.default_rng(n)
    idx = np.arange(n) % len(proofs)
    pr, pu = np.ascontiguousarray(proofs[idx]), np.ascontiguousarray(pubs[idx])
    w = np.frombuffer(rng.bytes(16 * n), np.uint64).reshape(n, 2) | np.uint64(1)
    out = {"n": n, "reps": reps}

    def timed(legs):
        for f in legs.values():
            f()                                                  # warm-up of every shape
        walls = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                walls[k].append((time.perf_counter() - t0) * 1e3)
        return {k: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in walls.items()}

    for name, flags in (("checked", 0), ("trusted", cp.PAIRING_TRUSTED)):
        def per_proof():
            assert not verifier.verify(pr, pu, flags=flags).any()

        def all_():
            v, path = verifier.verify_all(pr, w, pu, flags=flags)
            assert not v.any() and path == 0
        wall = timed({"per_proof": per_proof, "all": all_})
        prover.profile_begin()
        all_()
        prof = prover.profile_end()
        out[name] = {"wall_ms": wall, "all_over_per_proof": round(wall["all"]["median"] / wall["per_proof"]["median"], 4),
                     "us_per_proof": {k: round(v["median"] / n * 1e3, 3) for k, v in wall.items()},
                     "all_kernels_ms": {k: round(v["total_ms"], 4) for k, v in prof.items() if k.startswith(("pairing_", "groth16_", "msm_"))}}
    return out


def run_all_one_bad(prover, verifier, proofs, pubs, n, reps):
    idx = np.arange(n) % len(proofs)
    pr, pu = np.ascontiguousarray(proofs[idx]), np.ascontiguousarray(pubs[idx])
    pr[n // 2, 36:48] = pr[n // 2 + 1, 36:48]
    w = np.frombuffer(np.random.default_rng(n + 1).bytes(16 * n), np.uint64).reshape(n, 2) | np.uint64(1)
    want = verifier.verify(pr, pu)
    assert want.sum() == 1 and want[n // 2] == 1
    walls = {"per_proof": [], "all": []}
    for r in range(reps + 1):                                    # the first repeat is the warm-up
        t0 = time.perf_counter()
        got = verifier.verify(pr, pu)
        t1 = time.perf_counter()
        v, path = verifier.verify_all(pr, w, pu)
        t2 = time.perf_counter()
        assert (got == want).all() and (v == want).all() and path == 1
        if r:
            walls["per_proof"].append((t1 - t0) * 1e3)
            walls["all"].append((t2 - t1) * 1e3)
    wall = {k: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in walls.items()}
    return {"n": n, "reps": reps, "bad_proofs": 1, "path": 1, "wall_ms": wall, "all_over_per_proof": round(wall["all"]["median"] / wall["per_proof"]["median"], 4)}


def main_all(sizes, reps):
    p = cp.Prover(0)
    out = {"tool": "tools/bench_pairing.py --all", "method": "one process; per batch size both legs are warmed up once, then alternate within each of `reps` "
           "repeats; wall = host clock around the synchronous call (staging and verdict copies included), median / min / max; kernels = device events "
           "of one further profiled verify_all call; the weights are 128 random bits per proof", "n_public": N_PUBLIC, "kernel_registers": None, "sizes": []}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kernel_meta
        new = ("k_scale_g1", "k_fr_weighted_sums", "k_gt_product")
        out["kernel_registers"] = [{k: r[k] for k in ("name", "vgpr", "agpr", "vgpr_spill", "scratch", "lds")} for r in kernel_meta.kernels() if r["name"].endswith(new)]
    except Exception as e:
        out["kernel_registers"] = "unavailable: %s" % e
    verifier, proofs, pubs = make_key_and_proofs(p)
    for n in sizes:
        out["sizes"].append(run_all(p, verifier, proofs, pubs, n, reps))
        print("all", json.dumps(out["sizes"][-1]), flush=True)
    out["one_bad"] = run_all_one_bad(p, verifier, proofs, pubs, max(sizes), reps) if max(sizes) >= 4 else None
    verifier.close()
    p.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "groth16_verify_all.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


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
    if "--city" in sys.argv:
        main_city(sizes, reps)
        sys.exit(0)
    if "--all" in sys.argv:
        main_all(sizes, reps)
        sys.exit(0)
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

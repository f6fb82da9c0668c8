"""A powers-of-tau SRS from a KNOWN (tau, alpha, beta), for tests/test_gpu_point_ntt.py, tests/test_gpu_groth16_srs_setup.py,
tests/test_gpu_groth16_contribute.py and tools/bench_groth16_srs_setup.py: the points are fixed-base multiples of the standard
generators over the scalars tau^k, alpha tau^k, beta tau^k (G1Points.fixed_base / G2Points.fixed_base, the path
tests/test_gpu_fixed_base.py pins against the oracle), read back as affine canonical words. With the trapdoor known, the key the
SRS setup must return is the one the trapdoor setup returns for (tau, alpha, beta, gamma = 1, delta = 1)."""
import numpy as np

import groth16_setup_cases as GC
import oracle_lib as O
import r1cs_cases as RC

R = GC.R


def words(ints, per_point):
    """points as tuples of ints (G1: (x, y); G2: ((x0, x1), (y0, y1))) -> (n, 6 * per_point) u64 affine canonical"""
    flat = [(list(p) if per_point == 2 else [p[0][0], p[0][1], p[1][0], p[1][1]]) for p in ints]
    return np.array([[(int(c) >> (64 * i)) & (2**64 - 1) for c in pt for i in range(6)] for pt in flat], np.uint64).reshape(len(ints), 6 * per_point)


def multiples(prover, group, scalars):
    """([scalars[i]] G as ints, flags) through the fixed-base multiplication on the device"""
    import cityprover as cp
    pts_cls, gen = (cp.G1Points, O.bls_constants()[2]) if group == 1 else (cp.G2Points, O.bls_g2_generator())
    d = prover.to_device(RC.limbs4(scalars))
    try:
        pts, flags = pts_cls.fixed_base(prover, gen, d.ptr, len(scalars))
        try:
            return pts.to_host(), cp.flags_to_host(flags, len(scalars))
        finally:
            pts.free()
            flags.free()
    finally:
        d.free()


def srs_arrays(prover, td, log_size):
    """the five parts of cp_groth16_srs_desc for the trapdoor's (tau, alpha, beta): a dict of u64 arrays"""
    n = 1 << log_size
    tau, alpha, beta = td["tau"], td["alpha"], td["beta"]
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % R)
    g1 = lambda s: words(multiples(prover, 1, s)[0], 2)
    return {"log_size": log_size, "tau_g1": g1(pw), "tau_g2": words(multiples(prover, 2, pw[:n])[0], 4),
            "alpha_tau_g1": g1([alpha * x % R for x in pw[:n]]), "beta_tau_g1": g1([beta * x % R for x in pw[:n]]),
            "beta_g2": words(multiples(prover, 2, [beta])[0], 4)[0]}


def make_srs(prover, arrays, **kw):
    import cityprover as cp
    return cp.Groth16Srs(prover, arrays["log_size"], arrays["tau_g1"], arrays["tau_g2"], arrays["alpha_tau_g1"], arrays["beta_tau_g1"],
                         arrays["beta_g2"], **kw)


def setup_srs(prover, case, srs, n_pub=None, system=None):
    import cityprover as cp
    s = system or case["system"]
    return cp.Groth16Key.setup_srs(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"] if n_pub is None else n_pub, srs)


def setup_trapdoor(prover, case, td=None, n_pub=None, system=None):
    import cityprover as cp
    s = system or case["system"]
    return cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"] if n_pub is None else n_pub,
                               **(td or case["td"]))


def key_bytes(key):
    """everything the key holds, as bytes: two keys of the same setup are equal exactly when these are (the helper of
    tests/test_gpu_groth16_setup.py, copied)"""
    pk, sets = key.pk(), key.point_sets()
    vk = key.vk()
    raw = [sets[k].buf.download().tobytes() for k in ("a_g1", "b_g1", "b_g2", "k_g1", "z_g1")] + [sets["a_inf"].tobytes(), sets["b_inf"].tobytes()]
    singles = [bytes(bytearray(getattr(pk, f))) for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")]
    return raw, singles, repr(vk)


_cases = {}


def case_of(name):
    """the cases of tests/test_gpu_groth16_setup.py, built the same way"""
    if name not in _cases:
        if name == "shapes":
            c = GC.small_case(300, 3, 5, 300, wire0_in_every_a_row=True, a_columns=(GC.LONG, GC.LONG + 1), a_only=True, b_only=True, unused_public=True)
        else:
            n, n_pub, n_in = {"2^3": (8, 3, 3), "2^5": (32, 3, 6), "2^8": (256, 2, 5)}[name]
            c = GC.small_case(n, n_pub, n_in, 100 + n)
        _cases[name] = c
    return _cases[name]

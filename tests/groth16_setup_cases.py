"""Constraint systems with a trapdoor and every logarithm a Groth16 setup must produce, for tests/test_gpu_groth16_setup.py,
tests/test_gpu_fixed_base.py and tools/bench_groth16_setup.py. Everything is Python integers modulo r, computed term by term in
O(terms) (the col() recipe of r1cs_cases.groth16_case is O(n m)); the Lagrange values come from their closed form, one modular
inversion each - not from a transform, which is the library's route. Nothing here touches the GPU or the library."""
import numpy as np

import oracle_lib as O
import r1cs_cases as RC

R = RC.R
LONG = RC.LONG_ROW_THRESHOLD


def log_domain(n):
    return max(0, (n - 1).bit_length())


def lagrange_at(tau, L):
    """L_j(tau), j < 2^L, on the domain <omega>, omega = 7^((r-1)/2^L): (tau^N - 1)/N * omega^j / (tau - omega^j)"""
    N = 1 << L
    omega = pow(7, (R - 1) >> L, R)
    c = (pow(tau, N, R) - 1) * pow(N, -1, R) % R
    out, wj = [], 1
    for _ in range(N):
        out.append(c * wj % R * pow((tau - wj) % R, -1, R) % R)
        wj = wj * omega % R
    return out


def trapdoor(seed):
    rng = np.random.default_rng(seed)
    return {k: int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1 for k in ("tau", "alpha", "beta", "gamma", "delta")}


def expected_logs(system, n_pub, td):
    """u, v, w (all wires), k (private wires), ic (public wires), z (2^L - 1), L = log_domain, zt = tau^N - 1"""
    n, m, cs = system["n"], system["n_wires"], system["coeffs"]
    L = log_domain(n)
    lag = lagrange_at(td["tau"], L)
    cols = []
    for row_ptr, col, coeff in system["mats"]:
        acc = [0] * m
        rp, cc, kk = row_ptr.tolist(), col.tolist(), coeff.tolist()
        for j in range(n):
            lj = lag[j]
            for t in range(rp[j], rp[j + 1]):
                acc[cc[t]] += cs[kk[t]] * lj
        cols.append([x % R for x in acc])
    u, v, w = cols
    zt = (pow(td["tau"], 1 << L, R) - 1) % R
    dinv, ginv = pow(td["delta"], -1, R), pow(td["gamma"], -1, R)
    comb = [(td["beta"] * u[i] + td["alpha"] * v[i] + w[i]) % R for i in range(m)]
    z, tj = [], zt * dinv % R
    for _ in range((1 << L) - 1):
        z.append(tj)
        tj = tj * td["tau"] % R
    return {"u": u, "v": v, "w": w, "k": [c * dinv % R for c in comb[n_pub:]], "ic": [c * ginv % R for c in comb[:n_pub]], "z": z,
            "log_domain": L, "zt": zt}


def proof_logs(system, n_pub, td, exp, r, s):
    """the logarithms of (A, B, C) for the blinding (r, s), as r1cs_cases.groth16_case derives them, and the verification equation
    in the exponent: a b = alpha beta + gamma sum_pub w_i ic_i + c delta"""
    wit = system["w"]
    dot = lambda xs: sum(a * b for a, b in zip(wit, xs)) % R
    au, bv, cw = dot(exp["u"]), dot(exp["v"]), dot(exp["w"])           # a(tau), b(tau), c(tau) of the satisfied system
    dinv = pow(td["delta"], -1, R)
    h_zt = (au * bv - cw) % R                                           # h(tau) (tau^N - 1)
    a_log = (td["alpha"] + au + r * td["delta"]) % R
    b_log = (td["beta"] + bv + s * td["delta"]) % R
    c_log = (sum(x * y for x, y in zip(wit[n_pub:], exp["k"])) + h_zt * dinv + s * a_log + r * b_log - r * s * td["delta"]) % R
    pub = sum(x * y for x, y in zip(wit[:n_pub], exp["ic"])) % R
    assert a_log * b_log % R == (td["alpha"] * td["beta"] + td["gamma"] * pub + c_log * td["delta"]) % R
    return a_log, b_log, c_log


def small_case(n, n_pub, n_in, seed, wire0_in_every_a_row=False, a_columns=(), a_only=False, b_only=False, unused_public=False):
    """A satisfied system of n product constraints (one new wire each, as r1cs_cases.groth16_case builds them): wire 0 = 1, public
    inputs, n_in private inputs, then - in this order - one private wire per entry of a_columns that occurs in exactly that many
    rows of A and nowhere else, a private wire that occurs in A only, one that occurs in B only, and the product wires.
    unused_public: the last public wire occurs nowhere. Every other input occurs in some A row (row j names input j mod their
    number), so no private wire is left without a key point. Returns the case: system, n_pub, trapdoor, expected logs, specials."""
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1
    w = [1] + [rnd() for _ in range(n_pub - 1 + n_in)]
    general = [i for i in range(len(w)) if not (unused_public and i == n_pub - 1)]
    special = {"a_columns": []}
    for ln in a_columns:
        assert ln <= n
        special["a_columns"].append((len(w), ln))
        w.append(rnd())
    for name, on in (("a_only", a_only), ("b_only", b_only)):
        if on:
            special[name] = len(w)
            w.append(rnd())
    if unused_public:
        special["unused_public"] = n_pub - 1
    A, B, C = [], [], []
    for j in range(n):
        ra = {general[j % len(general)]: rnd()}
        for i in rng.choice(len(general), size=min(2, len(general)), replace=False):
            ra.setdefault(general[int(i)], rnd())
        if wire0_in_every_a_row:
            ra.setdefault(0, rnd())
        for wire, ln in special["a_columns"]:
            if j < ln:
                ra[wire] = rnd()
        if a_only and j % 5 == 0:
            ra[special["a_only"]] = rnd()
        rb = {general[int(i)]: rnd() for i in rng.choice(len(general), size=min(2, len(general)), replace=False)}
        if b_only and j % 7 == 0:
            rb[special["b_only"]] = rnd()
        dot = lambda row: sum(c * w[i] for i, c in row.items()) % R
        out = dot(ra) * dot(rb) % R
        A.append(ra); B.append(rb); C.append({len(w): 1})
        general.append(len(w))
        w.append(out)
    system = RC.from_dict_rows(A, B, C, w)
    td = trapdoor(seed + 1000)
    return {"system": system, "n_pub": n_pub, "td": td, "exp": expected_logs(system, n_pub, td), "special": special}


def satisfied_case(n, seed, n_pub):
    """r1cs_cases.satisfied_system (long rows, zero rows, skewed lengths: real infinity patterns in the B query) as a setup case"""
    system = RC.satisfied_system(n, seed)
    td = trapdoor(seed + 1000)
    return {"system": system, "n_pub": n_pub, "td": td, "exp": expected_logs(system, n_pub, td), "special": {}}


# ---- scalars for the fixed-base tests ----
def edge_scalars():
    """every scalar the signed byte recoding and the mixed addition can go wrong on: 0 and r (infinity), 1, 2, r - 1 (= -base),
    r + 1, 2^255, 2^256 - 1, every byte 0x80 / 0x7f (the carry boundary of each digit), and for every shift s in 192 .. 255 the
    scalar k_s = 2 ceil(r / 2^s) 2^s - r where it is below 2^256. Its low s bits are e = ceil(r / 2^s) 2^s - r and e base =
    (k_s - e) base, because r base = 0: the partial sum of the lower windows equals the next table entry, the doubling branch of
    the mixed addition, whatever the window layout"""
    out = [0, 1, 2, R - 1, R, R + 1, 1 << 255, (1 << 256) - 1, int.from_bytes(b"\x80" * 32, "little"), int.from_bytes(b"\x7f" * 32, "little")]
    for s in range(192, 256):
        k = 2 * (-(-R // (1 << s))) * (1 << s) - R
        if 0 <= k < (1 << 256):
            out.append(k)
    return out


def random_scalars(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(n)]

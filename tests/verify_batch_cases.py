"""Shared by the tests of the batched verifier (csrc/fri_verify.h, cp_verify_batch): the instance table and the challenge
record restated in Python from the proof format (tests/proof_format.py), the verdict a cp_verify message names, and twelve
mutations of a reference proof: the eleven tests/test_reference_product_parity.py makes and a flipped index of the last query."""
import ctypes
import re

import numpy as np

import oracle_lib as O
import reference_challenges as R
from proof_format import parse_proof, serialize_proof

P = O.P
KEY_NONE = 0xFFFFFFFF
MAX_ORACLES, MAX_LAYERS, MAX_BATCHES, MAX_RANGES = 8, 8, 4, 16
_u32 = ctypes.c_uint32


class Instance(ctypes.Structure):
    """friv::Instance (csrc/fri_verify.h)"""
    _fields_ = [(n, _u32) for n in ("n_oracles", "n_layers", "n_batches", "n_ranges", "n_queries", "cap_height", "log_n", "final_len",
                                    "q_base", "q_words", "final_off", "depth0")] + \
               [(n, _u32 * MAX_ORACLES) for n in ("leaf_len", "leaf_off", "sib_off", "cap_src", "cap_off")] + \
               [(n, _u32 * MAX_LAYERS) for n in ("arity_bits", "layer_depth", "ev_off", "path_off", "fcap_off")] + \
               [("batch_first", _u32 * (MAX_BATCHES + 1))] + [(n, _u32 * MAX_RANGES) for n in ("r_oracle", "r_first", "r_count")] + \
               [("omega", ctypes.c_uint64), ("arity_g", ctypes.c_uint64 * MAX_LAYERS)]


def root(bits):
    return pow(7, (P - 1) >> bits, P)


def layout(sh, check_cs=False):
    """(Instance, words per proof) of a cp_shape, walked field by field as tests/proof_format.py parses a proof"""
    D = Instance()
    nc, cap_n = sh.num_challenges, 1 << sh.cap_height
    k = [sh.num_constants + sh.num_routed_wires, sh.num_wires, nc * (1 + sh.num_partial_products), nc * sh.quotient_degree_factor]
    leaf = [k[b] + (4 if sh.zero_knowledge and b >= 1 else 0) for b in range(4)]
    lb = sh.degree_bits + sh.rate_bits
    o = 0
    for b in (1, 2, 3):
        o += 1
        D.cap_src[b], D.cap_off[b] = 1, o
        o += 4 * cap_n
    D.cap_src[0] = 2 if check_cs else 0
    for cnt in (sh.num_constants, sh.num_routed_wires, k[1], nc, nc, k[2] - nc, k[3], 0, 0):
        o += 1 + 2 * cnt
    D.n_oracles, D.n_layers, D.n_queries, D.cap_height, D.log_n, D.depth0 = 4, sh.n_arity, sh.num_query_rounds, sh.cap_height, lb, lb - sh.cap_height
    D.omega = root(lb)
    o += 1
    for l in range(sh.n_arity):
        o += 1
        D.fcap_off[l] = o
        o += 4 * cap_n
    o += 1
    D.q_base = o
    r = 1
    for b in range(4):
        D.leaf_len[b] = leaf[b]
        r += 1
        D.leaf_off[b] = r
        r += leaf[b] + 1
        D.sib_off[b] = r
        r += 4 * D.depth0
    r += 1
    bits = lb
    for l in range(sh.n_arity):
        ab = sh.arity_bits[l]
        bits -= ab
        D.arity_bits[l], D.layer_depth[l], D.arity_g[l] = ab, max(bits - sh.cap_height, 0), root(ab)
        r += 1
        D.ev_off[l] = r
        r += (2 << ab) + 1
        D.path_off[l] = r
        r += 4 * D.layer_depth[l]
    D.q_words = r
    o += sh.num_query_rounds * r
    D.final_len = (1 << sh.degree_bits) >> (lb - bits)
    o += 1
    D.final_off = o
    o += 2 * D.final_len + 1
    ranges = [[(0, 0, k[0]), (1, 0, k[1]), (2, 0, k[2]), (3, 0, k[3])], [(2, 0, nc)]]
    D.n_batches, i = len(ranges), 0
    for b, rs in enumerate(ranges):
        D.batch_first[b] = i
        for t in rs:
            D.r_oracle[i], D.r_first[i], D.r_count[i] = t
            i += 1
    D.batch_first[len(ranges)] = D.n_ranges = i
    return D, o + 1 + sh.num_public_inputs


def record(sh, pf, alpha, zeta, betas, x_indices):
    """the challenge record of one parsed proof, on Python integers"""
    o = pf["openings"]
    opened = [[tuple(e) for key in ("constants", "plonk_sigmas", "wires", "plonk_zs", "partial_products", "quotient_polys") for e in o[key]],
              [tuple(e) for e in o["plonk_zs_next"]]]
    alpha, zeta = tuple(int(v) for v in alpha), tuple(int(v) for v in zeta)
    points = [zeta, R.emul(zeta, R.base(root(sh.degree_bits)))]
    rec = list(alpha)
    for b in range(2):
        red, shift = R.ZERO, R.ONE
        for e in reversed(opened[b]):
            red = R.eadd(R.emul(red, alpha), e)
            shift = R.emul(shift, alpha)
        rec += list(points[b]) + list(red) + list(shift)
    for bt in betas:
        rec += [int(bt[0]), int(bt[1])]
    N = 1 << (sh.degree_bits + sh.rate_bits)
    rec += [int(x) % N for x in x_indices]
    return np.array(rec, dtype=np.uint64)


def key_triple(D, key):
    """(status, query, detail) of a failure key, as the library decodes it"""
    if key == KEY_NONE:
        return (0, -1, -1)
    q, ordinal, n_or = key >> 8, key & 0xFF, D.n_oracles
    if ordinal < n_or:
        return (7, q, ordinal)
    if ordinal == n_or:
        return (4, q, -1)
    if ordinal == n_or + 1 + 2 * D.n_layers:
        return (10, q, -1)
    k = ordinal - n_or - 1
    return (9 if k & 1 else 8, q, k >> 1)


_MESSAGES = [
    (r"query (\d+): Merkle path of oracle (\d+)", lambda m: (7, int(m[1]), int(m[2]))),
    (r"query (\d+): opening point", lambda m: (4, int(m[1]), -1)),
    (r"query (\d+): FRI layer (\d+) value", lambda m: (8, int(m[1]), int(m[2]))),
    (r"query (\d+): Merkle path of FRI layer (\d+)", lambda m: (9, int(m[1]), int(m[2]))),
    (r"query (\d+): final polynomial", lambda m: (10, int(m[1]), -1)),
    (r"malformed proof", lambda m: (1, -1, -1)),
    (r"proof-of-work witness is not canonical|proof of work:", lambda m: (6, -1, -1)),
    (r"not canonical", lambda m: (2, -1, -1)),
    (r"public inputs", lambda m: (3, -1, -1)),
    (r"zeta is in the subgroup", lambda m: (4, -1, -1)),
    (r"vanishing identity fails for challenge (\d+)", lambda m: (5, -1, int(m[1]))),
]


def message_triple(msg):
    """the verdict cp_verify's (or the audit hook's) refusal names"""
    for pat, f in _MESSAGES:
        m = re.search(pat, msg)
        if m:
            return f(m)
    raise AssertionError("unknown refusal: " + msg)


def triple(v):
    return (int(v["status"]), int(v["query"]), int(v["detail"]))


def reference_mutations(blob, args):
    """the eleven mutations of tests/test_reference_product_parity.py on one reference proof (leaf value, sibling, opening, layer
    evaluation, final polynomial, FRI cap, alpha, zeta, each beta, a flipped query index) and the last query's index flipped as well:
    [(name, bytes, challenges)]"""
    out = []

    def mutated(name, mutate, a=args):
        d = parse_proof(blob)
        mutate(d)
        out.append((name, serialize_proof(d), tuple(a)))
    mutated("leaf value", lambda d: d["queries"][3]["initial"][1][0].__setitem__(7, (d["queries"][3]["initial"][1][0][7] + 1) % P))
    mutated("sibling", lambda d: d["queries"][0]["initial"][3][1][2].__setitem__(0, 5))
    mutated("opening", lambda d: d["openings"]["wires"][9].__setitem__(0, (d["openings"]["wires"][9][0] + 1) % P))
    mutated("layer evaluation", lambda d: d["queries"][5]["steps"][1][0][3].__setitem__(1, 11))
    mutated("final polynomial", lambda d: d["final_poly"][2].__setitem__(0, (d["final_poly"][2][0] + 1) % P))
    mutated("FRI cap", lambda d: d["commit_caps"][1][4].__setitem__(1, 9))
    bump = lambda e: ((e[0] + 1) % P, e[1])
    for k, name in ((0, "alpha"), (1, "zeta")):
        a = list(args)
        a[k] = bump(a[k])
        mutated(name, lambda d: None, a)
    a = list(args)
    a[2] = [bump(args[2][0]), args[2][1]]
    mutated("beta 0", lambda d: None, a)
    a = list(args)
    a[2] = [args[2][0], bump(args[2][1])]
    mutated("beta 1", lambda d: None, a)
    a = list(args)
    a[3] = [args[3][0] ^ 1] + list(args[3][1:])
    mutated("query index", lambda d: None, a)
    a = list(args)
    a[3] = list(args[3][:-1]) + [args[3][-1] ^ 16]
    mutated("last query index", lambda d: None, a)
    return out

"""Does the reference's second proof sample (city_rollup_common/src/block_template/data.rs:73, the one that carries
public_input_0 and public_input_1) verify under the on-chain verifying key of tests/golden/groth16_verifier_data.json for SOME
assignment of roles? The key is four G1 and three G2 points with no names: alpha plus three IC points, and beta, gamma, delta, for
a circuit with two public inputs. Pure Python (tests/pairing_ref.py), no GPU and no library.

Computed once: the 16 GT values e(P_i, Q_j) (12), e(C, Q_j) (3) and e(A, B). Tried: every choice of alpha among the G1 points,
every order of the other three as IC_0, IC_1, IC_2, every order of the G2 points as beta, gamma, delta, the sign of each of the
five terms, and the two inputs read little- or big-endian (reduced mod r: GT has order r). The inputs in the other order are the
same candidates again - swapping them is swapping IC_1 and IC_2 - so the order of the IC points covers both orders:

    e(A, B) = e(alpha, beta)^+-1 . e(IC_0, gamma)^+-1 . e(IC_1, gamma)^+-x . e(IC_2, gamma)^+-y . e(C, delta)^+-1

4 x 6 x 6 x 32 x 2 = 9 216 distinct candidates. Each side is split in two halves that are tabulated on their own, so the search is a few
thousand products in F_p^12 and a set intersection instead of one product chain per candidate.

RESULT: none of them verifies. The sample and the committed key do not belong together under any of these readings (the sample
predates the key, belongs to another circuit, or the inputs are hashed before they enter the equation): the tree still holds no
Groth16 parity pin that rests on reference data."""
import itertools
import json
import os
import sys

import pairing_cases as PC
import pairing_ref as PR

P, R = PR.P, PR.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def g1_point(b):
    """48 bytes: x little-endian, 0x80 of the last byte: y is the larger root"""
    assert len(b) == 48 and not b[47] & 0x40
    x = int.from_bytes(b, "little") & ((1 << 382) - 1)
    y = PC.fp_sqrt((x**3 + 4) % P)
    assert x < P and y is not None
    if (y > P - y) != bool(b[47] & 0x80):
        y = P - y
    return (x, y)


def g2_point(b):
    """96 bytes: x.c0 (no flags) | x.c1 (flags); the larger root by c1, then c0"""
    assert len(b) == 96 and not b[47] & 0xc0 and not b[95] & 0x40
    x = (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little") & ((1 << 382) - 1))
    y = PC.f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), (4, 4)))
    assert x[0] < P and x[1] < P and y is not None
    neg = PR.f2_sub((0, 0), y)
    if ((y[1], y[0]) > (neg[1], neg[0])) != bool(b[95] & 0x80):
        y = neg
    return (x, y)


def conj(a):
    """the inverse of a value of the pairing (an element of the cyclotomic subgroup): w -> -w"""
    return [c if k % 2 == 0 else PR.f2_sub((0, 0), c) for k, c in enumerate(a)]


def key(a):
    return tuple(a)


def load():
    vk = b"".join(bytes.fromhex(c) for c in json.load(open(os.path.join(GOLDEN, "groth16_verifier_data.json")))["chunks"])
    assert len(vk) == 4 * 48 + 3 * 96
    g1 = [g1_point(vk[o:o + 48]) for o in (0, 48, 96, 144)]
    g2 = [g2_point(vk[o:o + 96]) for o in (192, 288, 384)]
    ins = json.load(open(os.path.join(GOLDEN, "groth16_sample_public_inputs.json")))
    s = json.load(open(os.path.join(GOLDEN, "groth16_proof_samples.json")))[ins["sample"]]
    A, C = g1_point(bytes.fromhex(s["pi_a"])), g1_point(bytes.fromhex(s["pi_c"]))
    B = g2_point(bytes.fromhex(s["pi_b_a0"]) + bytes.fromhex(s["pi_b_a1"]))
    raw = [bytes.fromhex(ins["public_input_%d" % i]) for i in (0, 1)]
    assert all(len(r) == 32 for r in raw)
    return g1, g2, (A, B, C), raw


def input_readings(raw):
    """(x, y) for IC_1, IC_2: little- and big-endian"""
    return {name: tuple(int.from_bytes(r, name) % R for r in raw) for name in ("little", "big")}


def search():
    """every (alpha, ic order, g2 order, signs, reading) that verifies"""
    g1, g2, (A, B, C), raw = load()
    for pt in g1 + [A, C]:
        assert PR.g1_on_curve(pt)
    for pt in g2 + [B]:
        assert PR.g2_on_curve(pt)
    E = [[PR.pairing(p, q) for q in g2] for p in g1]
    EC = [PR.pairing(C, q) for q in g2]
    EAB = PR.pairing(A, B)
    assert PR.f12_mul(EAB, conj(EAB)) == PR.F12_ONE          # the inverse used below is the inverse
    readings = input_readings(raw)
    scalars = sorted({v for xy in readings.values() for v in xy})
    POW = {(i, j, s): PR.f12_pow(E[i][j], s) for i in range(4) for j in range(3) for s in scalars}
    sgn = lambda a, s: a if s > 0 else conj(a)
    found = []
    for b_, g_, d_ in itertools.permutations(range(3)):       # which G2 point is beta, gamma, delta
        # left table: e(A, B) . e(alpha, beta)^-+1 . e(C, delta)^-+1 for every alpha and both signs of each
        left = {}
        for a_ in range(4):
            for sa, sc in itertools.product((1, -1), repeat=2):
                v = PR.f12_mul(PR.f12_mul(EAB, sgn(E[a_][b_], -sa)), sgn(EC[d_], -sc))
                left.setdefault(key(v), []).append((a_, sa, sc))
        # right: e(IC_0, gamma)^+-1 . e(IC_1, gamma)^+-x . e(IC_2, gamma)^+-y
        for ic in itertools.permutations(range(4), 3):
            for name, (x, y) in readings.items():
                for s0, s1, s2 in itertools.product((1, -1), repeat=3):
                    v = PR.f12_mul(PR.f12_mul(sgn(E[ic[0]][g_], s0), sgn(POW[ic[1], g_, x], s1)), sgn(POW[ic[2], g_, y], s2))
                    for a_, sa, sc in left.get(key(v), ()):
                        if a_ not in ic:
                            found.append({"alpha": a_, "ic": ic, "beta": b_, "gamma": g_, "delta": d_, "signs": (sa, s0, s1, s2, sc), "inputs": name})
    return found


def test_the_sample_verifies_under_no_role_assignment_of_the_on_chain_key():
    assert search() == []


def test_the_search_finds_a_planted_assignment(monkeypatch):
    """the same search over a key built around the sample from known logarithms finds exactly the planted roles"""
    raw = load()[3]
    x, y = input_readings(raw)["big"]
    # a key and a proof from known logarithms: A = [a] G1, B = [b] G2, C from the equation
    al, be, ga, de, i0, i1, i2, a, b = PC.scalars(17, 2024)[8:]
    c = (a * b - al * be - ga * (i0 + x * i1 + y * i2)) * pow(de, -1, R) % R
    g1 = [PC.g1_mul(i2), PC.g1_mul(al), PC.g1_mul(i1), PC.g1_mul(i0)]        # alpha second, the IC points out of order
    g2 = [PC.g2_mul(de), PC.g2_mul(be), PC.g2_mul(ga)]
    planted = (g1, g2, (PC.g1_mul(a), PC.g2_mul(b), PC.g1_mul(c)), raw)
    monkeypatch.setattr(sys.modules[__name__], "load", lambda: planted)
    found = search()
    assert found == [{"alpha": 1, "ic": (3, 2, 0), "beta": 1, "gamma": 2, "delta": 0, "signs": (1, 1, 1, 1, 1), "inputs": "big"}]

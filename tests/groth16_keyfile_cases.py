"""Groth16 key files built and taken apart in Python, for tests/test_groth16_keyfile.py and tests/test_gpu_groth16_keyfile.py:
the layout of include/cityprover.h ("Groth16 keys as files") restated from its description alone. A file is built from a
setup case of tests/groth16_setup_cases.py: every point is [its logarithm] G by the oracle's scalar multiplication, compression is
x plus the `y > p - y` bit in Python integers, the checksum is three lines of numpy. Nothing here touches the GPU or the library."""
import numpy as np

import groth16_setup_cases as GC
import oracle_lib as O
import pairing_cases as PC

P = PC.P
MAGIC = int.from_bytes(b"CPG16KEY", "little")
GOLDEN = 0x9E3779B97F4A7C15
SETS = ("a_g1", "b_g1", "b_g2", "k_g1", "z_g1")
FIXED_WORDS = 116


def checksum(words):
    """sum mod 2^64 over every word i != 2 of mix(w_i ^ i * GOLDEN), mix = the splitmix64 finaliser"""
    z = np.asarray(words, np.uint64) ^ (np.arange(len(words), dtype=np.uint64) * np.uint64(GOLDEN))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    z[2] = 0
    return int(z.sum(dtype=np.uint64))


def with_checksum(data):
    """the file with word 2 recomputed: an edited file reaches the checks behind the checksum"""
    w = np.frombuffer(bytes(data), np.uint64).copy()
    w[2] = checksum(w)
    return w.tobytes()


def fp_bytes(v):
    return int(v).to_bytes(48, "little")


def g1_larger(y):
    return y > P - y


def g2_larger(y):
    return g1_larger(y[1]) if y[1] else g1_larger(y[0])


def g1_compressed(pt):
    """48 bytes: x little-endian, 0x80 on the last byte where y is the larger root; None (infinity) is 0x40 alone"""
    if pt is None:
        return bytes(47) + b"\x40"
    b = bytearray(fp_bytes(pt[0]))
    b[47] |= 0x80 if g1_larger(pt[1]) else 0
    return bytes(b)


def g2_compressed(pt):
    """96 bytes: a0, then a1 with the flags on a1"""
    if pt is None:
        return bytes(95) + b"\x40"
    b = bytearray(fp_bytes(pt[0][0]) + fp_bytes(pt[0][1]))
    b[95] |= 0x80 if g2_larger(pt[1]) else 0
    return bytes(b)


def g1_raw(pt):
    return bytes(96) if pt is None else fp_bytes(pt[0]) + fp_bytes(pt[1])


def g2_raw(pt):
    return bytes(192) if pt is None else b"".join(fp_bytes(c) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]))


_points = {}


def key_points(case):
    """every point of the key of a setup case from the trapdoor (None = infinity), computed once per case"""
    if id(case) not in _points:
        G1, G2 = O.bls_constants()[2], O.bls_g2_generator()
        td, exp = case["td"], case["exp"]
        m1 = lambda x: O.bls_g1_mul(G1, x) if x else None
        m2 = lambda x: O.bls_g2_mul(G2, x) if x else None
        _points[id(case)] = {
            "case": case, "G1": G1, "G2": G2,
            "alpha_g1": m1(td["alpha"]), "beta_g1": m1(td["beta"]), "delta_g1": m1(td["delta"]),
            "beta_g2": m2(td["beta"]), "delta_g2": m2(td["delta"]), "gamma_g2": m2(td["gamma"]),
            "ic": [m1(x) for x in exp["ic"]],
            "a_g1": [m1(x) for x in exp["u"]], "b_g1": [m1(x) for x in exp["v"]], "b_g2": [m2(x) for x in exp["v"]],
            "k_g1": [m1(x) for x in exp["k"]], "z_g1": [m1(x) for x in exp["z"]]}
    return _points[id(case)]


def layout(log_domain, n_wires, n_public, raw):
    """byte offsets: {"ic", "ic_flags", each set: (offset, count, bytes per point), "total"}"""
    g1, g2 = (96, 192) if raw else (48, 96)
    out = {"ic": FIXED_WORDS * 8, "ic_flags": FIXED_WORDS * 8 + 96 * n_public}
    off = out["ic_flags"] + 8 * ((n_public + 7) // 8)
    for name, n in zip(SETS, (n_wires, n_wires, n_wires, n_wires - n_public, (1 << log_domain) - 1)):
        size = g2 if name == "b_g2" else g1
        out[name] = (off, n, size)
        off += n * size
    out["total"] = off
    return out


def build_file(case, raw=False):
    """the key file of a setup case, byte for byte what cp_groth16_key_save_file must write"""
    pts = key_points(case)
    m, n_pub, L = case["system"]["n_wires"], case["n_pub"], case["exp"]["log_domain"]
    head = np.array([MAGIC, 1, 0, 1 if raw else 0, L, m, n_pub, 0], np.uint64).tobytes()
    body = [g1_raw(pts[k]) for k in ("alpha_g1", "beta_g1", "delta_g1")] + [g2_raw(pts[k]) for k in ("beta_g2", "delta_g2", "gamma_g2")]
    body += [g1_raw(pt if pt is not None else pts["G1"]) for pt in pts["ic"]]       # under a flag: the generator, as cp_groth16_key_vk returns it
    flags = bytes(int(pt is None) for pt in pts["ic"])
    body.append(flags + bytes(-len(flags) % 8))
    e1, e2 = (g1_raw, g2_raw) if raw else (g1_compressed, g2_compressed)
    for name in SETS:
        body += [(e2 if name == "b_g2" else e1)(pt) for pt in pts[name]]
    data = head + b"".join(body)
    assert len(data) == layout(L, m, n_pub, raw)["total"]
    return with_checksum(data)


def point_at(data, lay, name, i):
    """(offset, size) of point i of a set"""
    off, n, size = lay[name]
    assert 0 <= i < n
    return off + i * size, size


def replace(data, off, new):
    return bytes(data[:off]) + bytes(new) + bytes(data[off + len(new):])


def g1_no_abscissa(start=1):
    """the first x >= start with x^3 + 4 a non-residue: the abscissa of no point of the curve"""
    x = start
    while PC.fp_sqrt((x**3 + 4) % P) is not None:
        x += 1
    return x


def g2_no_abscissa(start=1):
    """the first x = (start, 0), (start + 1, 0), ... with x^3 + 4 (1 + u) a non-square of F_p^2"""
    import pairing_ref as PR
    x = start
    while True:
        xx = (x, 0)
        if PC.f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(xx, xx), xx), (4, 4))) is None:
            return xx
        x += 1


# ---- files that the loader must refuse ----
# what the message of a refused point says after "<set>[<index>] ", per class
CLASS_TEXT = {"flag": "has a flag bit set that may not be set", "range": "has a coordinate that is not canonical", "no_point": "is no point of the curve",
              "infinity": "is the point at infinity", "disagree": "and b_g1 of the same wire disagree", "torsion": "is outside the r-torsion"}


def p_bytes(top=0):
    """x = p, with flag bits on the last byte"""
    b = bytearray(P.to_bytes(48, "little"))
    b[47] |= top
    return bytes(b)


def refusal_edits(case):
    """(label, raw, [(set, index, new bytes of the point)], (class, set, index) the loader must name): each spoils the good file
    of a case with at least 43 wires and 31 Z points. Where two points are spoiled, they lie in different passes of 5 points
    (or, in the last edit, in one pass) and the lowest index is the one to name."""
    exp = case["exp"]
    u_ok = [i for i, x in enumerate(exp["u"]) if x]
    v_ok = [i for i, x in enumerate(exp["v"]) if x]
    v_inf = [i for i, x in enumerate(exp["v"]) if not x]
    pts = key_points(case)
    bad1, bad2 = g1_no_abscissa(5), g2_no_abscissa(5)
    i, j, k, z = u_ok[2], v_ok[3], 4, 9
    assert u_ok[-1] // 5 != i // 5 and v_ok[-1] // 5 != j // 5 and v_inf
    x_of = lambda name, idx: pts[name][idx][0]
    inf1, inf2 = bytes(47) + b"\x40", bytes(95) + b"\x40"
    E = []
    # x >= p, in each of the three classes of set (G1 with flags, G2 - either half -, G1 without flags)
    E.append(("x = p", False, [("a_g1", i, p_bytes())], ("range", "a_g1", i)))
    E.append(("x = p, larger root", False, [("b_g1", j, p_bytes(0x80))], ("range", "b_g1", j)))
    E.append(("x = 2^381 - 1", False, [("k_g1", k, b"\xff" * 47 + b"\x1f")], ("range", "k_g1", k)))
    E.append(("a0 = p", False, [("b_g2", j, p_bytes() + fp_bytes(x_of("b_g2", j)[1]))], ("range", "b_g2", j)))
    E.append(("a1 = p", False, [("b_g2", j, fp_bytes(x_of("b_g2", j)[0]) + p_bytes(0x80))], ("range", "b_g2", j)))
    # an x that is no abscissa
    E.append(("no abscissa", False, [("a_g1", i, fp_bytes(bad1))], ("no_point", "a_g1", i)))
    E.append(("no abscissa, larger root", False, [("z_g1", z, fp_bytes(bad1 | (0x80 << 376)))], ("no_point", "z_g1", z)))
    E.append(("no abscissa", False, [("b_g2", j, fp_bytes(bad2[0]) + fp_bytes(bad2[1]))], ("no_point", "b_g2", j)))
    # 0x40 with other bits set; a flag on a0
    E.append(("0x40 and x", False, [("a_g1", i, fp_bytes(x_of("a_g1", i) | (0x40 << 376)))], ("flag", "a_g1", i)))
    E.append(("0x40 and 0x80", False, [("b_g1", v_inf[0], bytes(47) + b"\xc0")], ("flag", "b_g1", v_inf[0])))
    E.append(("0x40 and a0", False, [("b_g2", v_inf[0], b"\x01" + bytes(94) + b"\x40")], ("flag", "b_g2", v_inf[0])))
    E.append(("0x80 on a0", False, [("b_g2", j, fp_bytes(x_of("b_g2", j)[0] | (0x80 << 376)) + g2_compressed(pts["b_g2"][j])[48:])], ("flag", "b_g2", j)))
    # infinity where none is allowed
    E.append(("0x40 in k", False, [("k_g1", k, inf1)], ("infinity", "k_g1", k)))
    E.append(("0x40 in z", False, [("z_g1", z, inf1)], ("infinity", "z_g1", z)))
    E.append(("zeros in raw k", True, [("k_g1", k, bytes(96))], ("infinity", "k_g1", k)))
    E.append(("zeros in raw z", True, [("z_g1", 0, bytes(96))], ("infinity", "z_g1", 0)))
    # b_g1 and b_g2 disagree, either way round: named where the second of the two is read
    E.append(("b_g1 infinity alone", False, [("b_g1", j, inf1)], ("disagree", "b_g2", j)))
    E.append(("b_g2 infinity alone", False, [("b_g2", j, inf2)], ("disagree", "b_g2", j)))
    E.append(("b_g1 finite alone", False, [("b_g1", v_inf[0], g1_compressed(pts["a_g1"][i]))], ("disagree", "b_g2", v_inf[0])))
    E.append(("raw b_g1 infinity alone", True, [("b_g1", j, bytes(96))], ("disagree", "b_g2", j)))
    # raw form: off the curve, and a coordinate >= p
    off1 = g1_raw((x_of("a_g1", i), (pts["a_g1"][i][1] + 1) % P))
    E.append(("raw off the curve", True, [("a_g1", i, off1)], ("no_point", "a_g1", i)))
    E.append(("raw x and y of two points", True, [("z_g1", z, g1_raw(pts["z_g1"][z])[:48] + g1_raw(pts["z_g1"][z + 1])[48:])], ("no_point", "z_g1", z)))
    q = pts["b_g2"][j]
    E.append(("raw off the twist", True, [("b_g2", j, g2_raw((q[0], (q[1][1], q[1][0]))))], ("no_point", "b_g2", j)))
    E.append(("raw y = p", True, [("k_g1", k, g1_raw(pts["k_g1"][k])[:48] + p_bytes())], ("range", "k_g1", k)))
    E.append(("raw x zero alone", True, [("a_g1", i, bytes(48) + g1_raw(pts["a_g1"][i])[48:])], ("no_point", "a_g1", i)))
    # two spoiled points: the lowest index is named, whatever the classes
    E.append(("two passes", False, [("a_g1", u_ok[-1], fp_bytes(bad1)), ("a_g1", i, p_bytes())], ("range", "a_g1", i)))
    E.append(("two passes", False, [("b_g2", j, fp_bytes(bad2[0]) + fp_bytes(bad2[1])), ("b_g2", v_ok[-1], inf2)], ("no_point", "b_g2", j)))
    E.append(("two passes, raw", True, [("z_g1", 30, bytes(96)), ("z_g1", 11, off1)], ("no_point", "z_g1", 11)))
    E.append(("one pass, two lanes", False, [("k_g1", 6, inf1), ("k_g1", 8, p_bytes())], ("infinity", "k_g1", 6)))
    return E

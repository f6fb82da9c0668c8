"""What each of the 22 plonky2 gate types MEANS on one row, in Python integers: no GPU, no native library, nothing taken from
synth_gates.py / synth_circuit.py. csrc/gates.h, csrc/quotient.h and the oracle state the gates as constraint polynomials; this
file states them as named conditions on integers mod p (a limb is in 0..3, the limbs recompose the output, the claimed element
is the item at the index the bits spell, ...), so that a misreading the three polynomial statements share does not pass.

For every gate, with the parameters of synth_gates.ALL_GATES:
  layout(gate), wire_names(gate)   which local wire index holds what (copy constraints route by index: part of the semantics)
  violations(gate, consts, row, pi_hash)   the named conditions the row breaks; [] = the gate holds
  honest_row(gate, operands)       every helper wire (limbs, inverses, flags, accumulators) filled from the meaning
  typical_operands(gate)           one fixed ordinary operand set, the row `corruptions` starts from
  edge_operands(gate)              the operand sets at which the gate can go wrong
  malicious_rows(gate)             rows that must be refused although every helper wire is as self-consistent as it can be
  corruptions(gate, row)           a fixed list over EVERY wire index below the gate's wire count (+1; for ranged wires also the
                                   first out-of-range value and another in-range value) and one wire at the wire count

The eight in-tree gates are read off the reference's Rust (city_common_circuit/src/u32/gates/, cited per gate). The upstream
gates (plonky2 is not vendored) are stated from what the gate is for and marked UPSTREAM. A condition that continues from a
wire (the S-box input wires of Poseidon, the accumulators of Reducing, the intermediates of CosetInterpolation and
Exponentiation) is checked from the wire's value, as the wire is what the next row or gate can be copy-constrained to.

Readings recorded in DESIGN.md next to the gates: ExponentiationGate does not range its bit wires (a bit b multiplies by
1 + b (base - 1)); the 64-bit Uninterleave gates accept a decomposition of x + p when that still fits 64 bits; no in-tree
gate ranges its INPUT wires, so the edge rows may use inputs above 2^32 where u32 inputs cannot reach the edge."""
import importlib.util
import os

P = 0xFFFFFFFF00000001
U32_MAX = 0xFFFFFFFF
NUM_WIRES = 135  # wires of the standard recursion config; a row handed to `violations` has this many values

(NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC, POSEIDON, COMPARISON, U32_ARITHMETIC, U32_RANGE_CHECK, U32_ADD_MANY,
 U32_SUBTRACTION, U32_INTERLEAVE, UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32, ARITHMETIC_EXT, MUL_EXT, BASE_SUM,
 RANDOM_ACCESS, REDUCING, REDUCING_EXT, POSEIDON_MDS, COSET_INTERPOLATION, EXPONENTIATION) = range(22)

# (type, param, param2, param3): the same 22 tuples as synth_gates.ALL_GATES (test_gate_semantics asserts it)
ALL_GATES = [(NOOP, 0, 0, 0), (CONSTANT, 2, 0, 0), (PUBLIC_INPUT, 0, 0, 0), (COMPARISON, 32, 16, 0), (RANDOM_ACCESS, 4, 4, 2),
             (POSEIDON, 0, 0, 0), (POSEIDON_MDS, 0, 0, 0), (REDUCING, 43, 0, 0), (REDUCING_EXT, 32, 0, 0), (ARITHMETIC, 20, 0, 0),
             (ARITHMETIC_EXT, 10, 0, 0), (MUL_EXT, 13, 0, 0), (BASE_SUM, 63, 2, 0), (COSET_INTERPOLATION, 4, 6, 0),
             (U32_ARITHMETIC, 3, 0, 0), (U32_RANGE_CHECK, 7, 0, 0), (U32_ADD_MANY, 5, 3, 0), (U32_SUBTRACTION, 6, 0, 0),
             (U32_INTERLEAVE, 3, 0, 0), (UNINTERLEAVE_TO_U32, 2, 0, 0), (UNINTERLEAVE_TO_B32, 2, 0, 0), (EXPONENTIATION, 66, 0, 0)]
NAME = {NOOP: "Noop", CONSTANT: "Constant", PUBLIC_INPUT: "PublicInput", ARITHMETIC: "Arithmetic", POSEIDON: "Poseidon",
        COMPARISON: "Comparison", U32_ARITHMETIC: "U32Arithmetic", U32_RANGE_CHECK: "U32RangeCheck", U32_ADD_MANY: "U32AddMany",
        U32_SUBTRACTION: "U32Subtraction", U32_INTERLEAVE: "U32Interleave", UNINTERLEAVE_TO_U32: "UninterleaveToU32",
        UNINTERLEAVE_TO_B32: "UninterleaveToB32", ARITHMETIC_EXT: "ArithmeticExtension", MUL_EXT: "MulExtension",
        BASE_SUM: "BaseSum", RANDOM_ACCESS: "RandomAccess", REDUCING: "Reducing", REDUCING_EXT: "ReducingExtension",
        POSEIDON_MDS: "PoseidonMds", COSET_INTERPOLATION: "CosetInterpolation", EXPONENTIATION: "Exponentiation"}
GATE = {g[0]: g for g in ALL_GATES}

DEFAULT_CONSTS = (0x0123456789ABCDEF % P, 0xFEDCBA9876543210 % P)
DEFAULT_PI_HASH = (11, 0xDEADBEEF12345678 % P, P - 2, 1 << 40)


# ---- deterministic filler values (no sampling: the same lists on every run) ----
def det(seed, n, bound=P):
    out, s = [], (seed * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF
    for _ in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        z = s ^ (s >> 29)
        z = (z * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 32
        out.append(z % bound)
    return out


# ---- F_p^2 = F_p[X] / (X^2 - 7): extension-valued wires are pairs of wires (c0, c1) ----
def e_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def e_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def e_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def e_scale(x, s):
    return (x[0] * s % P, x[1] * s % P)


def inv(x):
    assert x % P
    return pow(x, P - 2, P)


def _pairs(vals):
    return [(vals[2 * i], vals[2 * i + 1]) for i in range(len(vals) // 2)]


def _flat(pairs):
    return [v for p in pairs for v in p]


# ---- Poseidon over Goldilocks, width 12: 4 full rounds, 22 partial, 4 full; x^7; MDS = circulant + diagonal ----
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11
_RC = None


def round_constants():
    """The 360 round constants by their published derivation (csrc/gen_tables.py, plain Python); test_gate_semantics pins
    the permutation built on them to tests/golden/poseidon_zero_hashes.json."""
    global _RC
    if _RC is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "city-rollup_amd", "csrc", "gen_tables.py")
        spec = importlib.util.spec_from_file_location("_gen_tables_for_gate_semantics", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _RC = [int(v) for v in mod.round_constants()]
        assert len(_RC) == 360 and all(0 <= v < P for v in _RC)
    return _RC


def mds(s):
    return [(sum(MDS_CIRC[i] * s[(i + r) % 12] for i in range(12)) + MDS_DIAG[r] * s[r]) % P for r in range(12)]


def _add_rc(s, rnd):
    rc = round_constants()
    return [(s[i] + rc[12 * rnd + i]) % P for i in range(12)]


def poseidon_permutation(state):
    s = [v % P for v in state]
    for rnd in range(30):
        s = _add_rc(s, rnd)
        if 4 <= rnd < 26:
            s[0] = pow(s[0], 7, P)
        else:
            s = [pow(v, 7, P) for v in s]
        s = mds(s)
    return s


# ---- wire layouts ----
def layout(gate):
    """name -> wire index, or list of indices (nested per op / copy where the gate repeats)."""
    t, a, b, c = gate
    if t == NOOP:
        return {}
    if t == CONSTANT:
        return {"value": list(range(a))}
    if t == PUBLIC_INPUT:
        return {"public_inputs_hash": [0, 1, 2, 3]}
    if t == ARITHMETIC:  # UPSTREAM
        return {"multiplicand_0": [4 * i for i in range(a)], "multiplicand_1": [4 * i + 1 for i in range(a)],
                "addend": [4 * i + 2 for i in range(a)], "output": [4 * i + 3 for i in range(a)]}
    if t == POSEIDON:  # UPSTREAM
        return {"input": list(range(12)), "output": list(range(12, 24)), "swap": 24, "delta": [25, 26, 27, 28],
                "full_sbox_0": [[29 + 12 * (r - 1) + i for i in range(12)] for r in (1, 2, 3)],
                "partial_sbox": [65 + r for r in range(22)],
                "full_sbox_1": [[87 + 12 * r + i for i in range(12)] for r in range(4)]}
    if t == COMPARISON:  # comparison.rs:49-93
        cb = -(-a // b)
        return {"first_input": 0, "second_input": 1, "result_bool": 2, "most_significant_diff": 3,
                "first_chunk": [4 + i for i in range(b)], "second_chunk": [4 + b + i for i in range(b)],
                "equality_dummy": [4 + 2 * b + i for i in range(b)], "chunks_equal": [4 + 3 * b + i for i in range(b)],
                "intermediate_value": [4 + 4 * b + i for i in range(b)],
                "most_significant_diff_bit": [4 + 5 * b + i for i in range(cb + 1)]}
    if t == U32_ARITHMETIC:  # arithmetic_u32.rs:44-85
        return {"multiplicand_0": [6 * i for i in range(a)], "multiplicand_1": [6 * i + 1 for i in range(a)],
                "addend": [6 * i + 2 for i in range(a)], "output_low": [6 * i + 3 for i in range(a)],
                "output_high": [6 * i + 4 for i in range(a)], "inverse": [6 * i + 5 for i in range(a)],
                "limb": [[6 * a + 32 * i + j for j in range(32)] for i in range(a)]}
    if t == U32_RANGE_CHECK:  # range_check_u32.rs:40-48
        return {"input_limb": list(range(a)), "aux_limb": [[a + 16 * i + j for j in range(16)] for i in range(a)]}
    if t == U32_ADD_MANY:  # add_many_u32.rs:48-84
        s = b + 3
        return {"addend": [[s * i + j for j in range(b)] for i in range(a)], "carry": [s * i + b for i in range(a)],
                "output_result": [s * i + b + 1 for i in range(a)], "output_carry": [s * i + b + 2 for i in range(a)],
                "limb": [[s * a + 18 * i + j for j in range(18)] for i in range(a)]}
    if t == U32_SUBTRACTION:  # subtraction_u32.rs:45-79
        return {"input_x": [5 * i for i in range(a)], "input_y": [5 * i + 1 for i in range(a)],
                "input_borrow": [5 * i + 2 for i in range(a)], "output_result": [5 * i + 3 for i in range(a)],
                "output_borrow": [5 * i + 4 for i in range(a)], "limb": [[5 * a + 16 * i + j for j in range(16)] for i in range(a)]}
    if t == U32_INTERLEAVE:  # interleave_u32.rs:49-88 (bits big-endian)
        return {"x": [2 * i for i in range(a)], "x_interleaved": [2 * i + 1 for i in range(a)],
                "bit": [[2 * a + 32 * i + k for k in range(32)] for i in range(a)]}
    if t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):  # uninterleave_to_u32.rs:57-90 (bits big-endian)
        return {"x_interleaved": [3 * i for i in range(a)], "x_evens": [3 * i + 1 for i in range(a)],
                "x_odds": [3 * i + 2 for i in range(a)], "bit": [[3 * a + 64 * i + k for k in range(64)] for i in range(a)]}
    if t == ARITHMETIC_EXT:  # UPSTREAM; each name is a pair of wires starting at the index
        return {"multiplicand_0": [8 * i for i in range(a)], "multiplicand_1": [8 * i + 2 for i in range(a)],
                "addend": [8 * i + 4 for i in range(a)], "output": [8 * i + 6 for i in range(a)]}
    if t == MUL_EXT:  # UPSTREAM
        return {"multiplicand_0": [6 * i for i in range(a)], "multiplicand_1": [6 * i + 2 for i in range(a)],
                "output": [6 * i + 4 for i in range(a)]}
    if t == BASE_SUM:  # UPSTREAM (limbs little-endian)
        return {"sum": 0, "limb": [1 + i for i in range(a)]}
    if t == RANDOM_ACCESS:  # UPSTREAM
        vec = 1 << a
        routed = (2 + vec) * b + c
        return {"access_index": [(2 + vec) * k for k in range(b)], "claimed_element": [(2 + vec) * k + 1 for k in range(b)],
                "list_item": [[(2 + vec) * k + 2 + i for i in range(vec)] for k in range(b)],
                "extra_constant": [(2 + vec) * b + i for i in range(c)], "bit": [[routed + a * k + i for i in range(a)] for k in range(b)]}
    if t in (REDUCING, REDUCING_EXT):  # UPSTREAM; output, alpha, old_acc, accs are pairs
        w = 2 if t == REDUCING_EXT else 1
        return {"output": 0, "alpha": 2, "old_acc": 4, "coeff": [6 + w * i for i in range(a)],
                "acc": [6 + w * a + 2 * i for i in range(a - 1)]}
    if t == POSEIDON_MDS:  # UPSTREAM; pairs
        return {"input": [2 * i for i in range(12)], "output": [24 + 2 * i for i in range(12)]}
    if t == COSET_INTERPOLATION:  # UPSTREAM; everything but `shift` is a pair
        n = 1 << a
        ni = (n - 2) // (b - 1)
        return {"shift": 0, "value": [1 + 2 * i for i in range(n)], "evaluation_point": 1 + 2 * n, "evaluation_value": 3 + 2 * n,
                "intermediate_eval": [5 + 2 * n + 2 * k for k in range(ni)], "intermediate_prod": [5 + 2 * n + 2 * (ni + k) for k in range(ni)],
                "shifted_evaluation_point": 5 + 2 * n + 4 * ni}
    if t == EXPONENTIATION:  # UPSTREAM (power bits little-endian)
        return {"base": 0, "power_bit": [1 + i for i in range(a)], "output": 1 + a, "intermediate_value": [2 + a + i for i in range(a)]}
    raise ValueError(gate)


def pair_names(gate):
    """the names of `layout` that stand for an F_p^2 value: two wires, (c0, c1), starting at the index given"""
    t = gate[0]
    L = layout(gate)
    if t in (ARITHMETIC_EXT, MUL_EXT, REDUCING_EXT, POSEIDON_MDS):
        return set(L)
    if t == REDUCING:
        return {"output", "alpha", "old_acc", "acc"}
    if t == COSET_INTERPOLATION:
        return set(L) - {"shift"}
    return set()


def wire_names(gate):
    """{wire index: name}: every wire of the gate exactly once (the layout is a partition of 0..num_wires-1)"""
    out = {}

    def put(i, name):
        assert i not in out, (NAME[gate[0]], i, name, out[i])
        out[i] = name

    def walk(v, name, width):
        if isinstance(v, list):
            for n, x in enumerate(v):
                walk(x, f"{name}[{n}]", width)
        else:
            for h in range(width):
                put(v + h, name if width == 1 else f"{name}.c{h}")
    pairs = pair_names(gate)
    for name, v in layout(gate).items():
        walk(v, name, 2 if name in pairs else 1)
    assert sorted(out) == list(range(len(out))), NAME[gate[0]]
    return out


def num_wires(gate):
    return len(wire_names(gate))


def ranged_wires(gate):
    """(wire index, size of the range) of the wires the definition treats as a limb, a bit or a chunk."""
    t, a, b, c = gate
    L = layout(gate)
    flat = lambda vv: [i for v in vv for i in v]
    if t == POSEIDON:
        return [(L["swap"], 2)]
    if t == COMPARISON:
        cs = 1 << -(-a // b)
        return [(i, cs) for i in L["first_chunk"] + L["second_chunk"]] + [(i, 2) for i in L["most_significant_diff_bit"]]
    if t in (U32_ARITHMETIC, U32_ADD_MANY):
        return [(i, 4) for i in flat(L["limb"])]
    if t == U32_RANGE_CHECK:
        return [(i, 4) for i in flat(L["aux_limb"])]
    if t == U32_SUBTRACTION:
        return [(i, 4) for i in flat(L["limb"])] + [(i, 2) for i in L["output_borrow"]]
    if t in (U32_INTERLEAVE, UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32, RANDOM_ACCESS):
        return [(i, 2) for i in flat(L["bit"])]
    if t == BASE_SUM:
        return [(i, b) for i in L["limb"]]
    if t == EXPONENTIATION:  # bits by purpose; the gate itself does not range them (see the module docstring)
        return [(i, 2) for i in L["power_bit"]]
    return []


# ---- small shared statements ----
def _le_sum(vals, base):
    return sum(v * base ** i for i, v in enumerate(vals)) % P


def _coset(bits):
    n = 1 << bits
    g = pow(7, (P - 1) >> bits, P)  # 7 generates F_p^*: g has order exactly 2^bits
    dom = [pow(g, i, P) for i in range(n)]
    wts = []
    for i in range(n):
        d = 1
        for j in range(n):
            if j != i:
                d = d * (dom[i] - dom[j]) % P
        wts.append(inv(d))
    return dom, wts


def _interp_steps(dom, wts, vals, x, lo, hi, ev, pr):
    """ev = sum_{i < m} w_i v_i prod_{j < m, j != i} (x - x_j), pr = prod_{j < m} (x - x_j), advanced from m = lo to m = hi"""
    for i in range(lo, hi):
        term = e_sub(x, (dom[i], 0))
        ev, pr = e_add(e_mul(ev, term), e_mul(vals[i], e_scale(pr, wts[i]))), e_mul(pr, term)
    return ev, pr


def interpolate(dom, vals, x):
    """The value at x (in F_p^2) of the polynomial of degree < n through (dom[i], vals[i]): Lagrange's formula with inverses."""
    for i, d in enumerate(dom):
        if x == (d, 0):
            return vals[i]

    def e_inv(z):
        nrm = inv((z[0] * z[0] - 7 * z[1] * z[1]) % P)
        return (z[0] * nrm % P, (-z[1]) * nrm % P)
    acc = (0, 0)
    for i in range(len(dom)):
        num, den = (1, 0), 1
        for j in range(len(dom)):
            if j != i:
                num = e_mul(num, e_sub(x, (dom[j], 0)))
                den = den * (dom[i] - dom[j]) % P
        acc = e_add(acc, e_mul(vals[i], e_scale(num, inv(den))))
    return acc


def _chunk_ranges(n, deg):
    """CosetInterpolation: the first `deg` points, then `deg - 1` more after each pair of intermediate wires"""
    ni = (n - 2) // (deg - 1)
    out = [(0, deg)]
    for k in range(ni):
        lo = 1 + (deg - 1) * (k + 1)
        out.append((lo, min(lo + deg - 1, n)))
    return out


# ---- the definition ----
def violations(gate, consts, row, pi_hash):
    t, a, b, c = gate
    w = [int(v) % P for v in row]
    k = [int(v) % P for v in consts]
    L = layout(gate)
    bad = []

    def need(ok, name):
        if not ok:
            bad.append(name)

    def pair(i):
        return (w[i], w[i + 1])
    if t == NOOP:
        pass
    elif t == CONSTANT:
        for i in range(a):
            need(w[i] == k[i], f"wire {i} is constant {i}")
    elif t == PUBLIC_INPUT:
        for i in range(4):
            need(w[i] == int(pi_hash[i]) % P, f"wire {i} is element {i} of the public inputs hash")
    elif t == ARITHMETIC:
        for i in range(a):
            m0, m1, ad, out = (w[4 * i + j] for j in range(4))
            need(out == (k[0] * m0 * m1 + k[1] * ad) % P, f"op {i}: output = c0 m0 m1 + c1 addend")
    elif t == POSEIDON:
        swap = w[24]
        need(swap in (0, 1), "swap is a bit")
        for i in range(4):
            need(w[25 + i] == swap * (w[4 + i] - w[i]) % P, f"delta {i} = swap (input {4 + i} - input {i})")
        st = [(w[i] + w[25 + i]) % P for i in range(4)] + [(w[4 + i] - w[25 + i]) % P for i in range(4)] + w[8:12]
        for rnd in range(30):
            st = _add_rc(st, rnd)  # the state before the S-box layer of round rnd
            if rnd == 0:
                st = [pow(v, 7, P) for v in st]
            elif rnd < 4 or rnd >= 26:
                wires = L["full_sbox_0"][rnd - 1] if rnd < 4 else L["full_sbox_1"][rnd - 26]
                need(st == [w[j] for j in wires], f"S-box inputs of full round {rnd} are the state before its S-box layer")
                st = [pow(w[j], 7, P) for j in wires]
            else:
                need(st[0] == w[65 + rnd - 4], f"S-box input of partial round {rnd - 4} is lane 0 before its S-box")
                st[0] = pow(w[65 + rnd - 4], 7, P)
            st = mds(st)
        need(st == w[12:24], "outputs are the state after the last round")
    elif t == COMPARISON:  # comparison.rs:101-178
        cb = -(-a // b)
        cs = 1 << cb
        f = [w[j] for j in L["first_chunk"]]
        s = [w[j] for j in L["second_chunk"]]
        for i in range(b):
            need(f[i] < cs, f"first chunk {i} is in 0..{cs - 1}")
            need(s[i] < cs, f"second chunk {i} is in 0..{cs - 1}")
        need(_le_sum(f, cs) == w[0], "the first chunks recompose the first input")
        need(_le_sum(s, cs) == w[1], "the second chunks recompose the second input")
        running = 0  # the difference of the most significant differing chunk among chunks 0..i-1
        for i in range(b):
            diff = (s[i] - f[i]) % P
            eq, dummy, inter = w[L["chunks_equal"][i]], w[L["equality_dummy"][i]], w[L["intermediate_value"][i]]
            need(eq == int(diff == 0), f"chunks_equal {i} says whether chunk {i} of both inputs is the same")
            if diff:
                need(dummy * diff % P == 1, f"equality_dummy {i} is the inverse of the chunks' difference")
            need(inter == eq * running % P, f"intermediate {i} keeps the running difference if chunk {i} is equal, else 0")
            running = (inter + (1 - eq) * diff) % P
        need(w[3] == running, "most_significant_diff is the difference at the most significant differing chunk")
        bits = [w[j] for j in L["most_significant_diff_bit"]]
        for i, v in enumerate(bits):
            need(v in (0, 1), f"diff bit {i} is a bit")
        need(_le_sum(bits, 2) == (cs + w[3]) % P, f"the diff bits recompose {cs} + most_significant_diff")
        need(w[2] == bits[cb], "the result is the top diff bit: first <= second")
    elif t == U32_ARITHMETIC:  # arithmetic_u32.rs:93-152
        for i in range(a):
            m0, m1, ad, lo, hi, iv = (w[6 * i + j] for j in range(6))
            limbs = [w[j] for j in L["limb"][i]]
            for j, v in enumerate(limbs):
                need(v < 4, f"op {i}: limb {j} is in 0..3")
            need(_le_sum(limbs[:16], 4) == lo, f"op {i}: the low 16 limbs recompose output_low")
            need(_le_sum(limbs[16:], 4) == hi, f"op {i}: the high 16 limbs recompose output_high")
            need((m0 * m1 + ad) % P == (lo + (hi << 32)) % P, f"op {i}: m0 m1 + addend = lo + 2^32 hi (mod p)")
            need(lo == 0 or iv * (U32_MAX - hi) % P == 1, f"op {i}: hi != 2^32-1 with inverse its witness, or else lo = 0")
    elif t == U32_RANGE_CHECK:  # range_check_u32.rs:57-78
        for i in range(a):
            limbs = [w[j] for j in L["aux_limb"][i]]
            for j, v in enumerate(limbs):
                need(v < 4, f"input {i}: aux limb {j} is in 0..3")
            need(_le_sum(limbs, 4) == w[i], f"input {i}: the 16 aux limbs recompose it")
    elif t == U32_ADD_MANY:  # add_many_u32.rs:93-132
        for i in range(a):
            total = (sum(w[j] for j in L["addend"][i]) + w[L["carry"][i]]) % P
            res, oc = w[L["output_result"][i]], w[L["output_carry"][i]]
            limbs = [w[j] for j in L["limb"][i]]
            for j, v in enumerate(limbs):
                need(v < 4, f"op {i}: limb {j} is in 0..3")
            need(_le_sum(limbs[:16], 4) == res, f"op {i}: the 16 result limbs recompose output_result")
            need(_le_sum(limbs[16:], 4) == oc, f"op {i}: the 2 carry limbs recompose output_carry")
            need(total == (res + (oc << 32)) % P, f"op {i}: addends + carry = result + 2^32 output_carry (mod p)")
    elif t == U32_SUBTRACTION:  # subtraction_u32.rs:89-122
        for i in range(a):
            x, y, br, res, ob = (w[5 * i + j] for j in range(5))
            limbs = [w[j] for j in L["limb"][i]]
            for j, v in enumerate(limbs):
                need(v < 4, f"op {i}: limb {j} is in 0..3")
            need(_le_sum(limbs, 4) == res, f"op {i}: the 16 limbs recompose output_result")
            need(ob in (0, 1), f"op {i}: output_borrow is a bit")
            need(res == (x - y - br + (ob << 32)) % P, f"op {i}: result = x - y - borrow + 2^32 output_borrow (mod p)")
    elif t == U32_INTERLEAVE:  # interleave_u32.rs:90-128
        for i in range(a):
            bits = [w[j] for j in L["bit"][i]]
            for j, v in enumerate(bits):
                need(v in (0, 1), f"op {i}: bit {j} is a bit")
            need(_le_sum(bits[::-1], 2) == w[2 * i], f"op {i}: the bits, most significant first, spell x")
            need(_le_sum(bits[::-1], 4) == w[2 * i + 1], f"op {i}: x_interleaved has bit k of x at position 2k")
    elif t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):  # uninterleave_to_u32.rs:98-143, uninterleave_to_b32.rs:98-144
        base = 2 if t == UNINTERLEAVE_TO_U32 else 4
        for i in range(a):
            bits = [w[j] for j in L["bit"][i]]
            for j, v in enumerate(bits):
                need(v in (0, 1), f"op {i}: bit {j} is a bit")
            need(_le_sum(bits[::-1], 2) == w[3 * i], f"op {i}: the 64 bits, most significant first, spell x_interleaved (mod p)")
            need(_le_sum(bits[0::2][::-1], base) == w[3 * i + 1], f"op {i}: x_evens gathers bit wires 0, 2, .. in base {base}")
            need(_le_sum(bits[1::2][::-1], base) == w[3 * i + 2], f"op {i}: x_odds gathers bit wires 1, 3, .. in base {base}")
    elif t == ARITHMETIC_EXT:
        for i in range(a):
            m0, m1, ad, out = (pair(8 * i + 2 * j) for j in range(4))
            need(out == e_add(e_scale(e_mul(m0, m1), k[0]), e_scale(ad, k[1])), f"op {i}: output = c0 m0 m1 + c1 addend in F_p^2")
    elif t == MUL_EXT:
        for i in range(a):
            m0, m1, out = (pair(6 * i + 2 * j) for j in range(3))
            need(out == e_scale(e_mul(m0, m1), k[0]), f"op {i}: output = c0 m0 m1 in F_p^2")
    elif t == BASE_SUM:
        limbs = [w[j] for j in L["limb"]]
        for j, v in enumerate(limbs):
            need(v < b, f"limb {j} is in 0..{b - 1}")
        need(_le_sum(limbs, b) == w[0], f"the limbs, least significant first, recompose the sum in base {b}")
    elif t == RANDOM_ACCESS:
        for cp in range(b):
            bits = [w[j] for j in L["bit"][cp]]
            for j, v in enumerate(bits):
                need(v in (0, 1), f"copy {cp}: bit {j} is a bit")
            need(_le_sum(bits, 2) == w[L["access_index"][cp]], f"copy {cp}: the bits spell the access index")
            if all(v in (0, 1) for v in bits):
                idx = sum(v << j for j, v in enumerate(bits))
                need(w[L["claimed_element"][cp]] == w[L["list_item"][cp][idx]], f"copy {cp}: the claimed element is the item at the index")
        for i in range(c):
            need(w[L["extra_constant"][i]] == k[i], f"extra constant wire {i} is constant {i}")
    elif t in (REDUCING, REDUCING_EXT):
        alpha, acc = pair(2), pair(4)
        for i in range(a):
            j = L["coeff"][i]
            coeff = pair(j) if t == REDUCING_EXT else (w[j], 0)
            nxt = pair(0) if i == a - 1 else pair(L["acc"][i])
            need(nxt == e_add(e_mul(acc, alpha), coeff), f"accumulator {i} = previous alpha + coefficient {i}" + (" (the output)" if i == a - 1 else ""))
            acc = nxt
    elif t == POSEIDON_MDS:
        for h in range(2):
            out = mds([w[2 * i + h] for i in range(12)])
            for r in range(12):
                need(w[24 + 2 * r + h] == out[r], f"output {r}, component {h}, is row {r} of the MDS matrix times the inputs")
    elif t == COSET_INTERPOLATION:
        n = 1 << a
        dom, wts = _coset(a)
        vals = [pair(j) for j in L["value"]]
        sp = pair(L["shifted_evaluation_point"])
        need(pair(L["evaluation_point"]) == e_scale(sp, w[0]), "evaluation_point = shift * shifted_evaluation_point")
        ev, pr = (0, 0), (1, 0)
        for kk, (lo, hi) in enumerate(_chunk_ranges(n, b)):
            if kk:
                ie, ip = pair(L["intermediate_eval"][kk - 1]), pair(L["intermediate_prod"][kk - 1])
                need(ie == ev, f"intermediate eval {kk - 1} is the partial interpolation sum over the first {lo} points")
                need(ip == pr, f"intermediate prod {kk - 1} is the product of (x - x_j) over the first {lo} points")
                ev, pr = ie, ip
            ev, pr = _interp_steps(dom, wts, vals, sp, lo, hi, ev, pr)
        need(pair(L["evaluation_value"]) == ev, "evaluation_value is the interpolant of the values over shift * H at evaluation_point")
    elif t == EXPONENTIATION:
        base = w[0]
        prev = 1
        for i in range(a):
            bit = w[1 + (a - 1 - i)]  # from the top bit down
            want = prev * prev % P * (1 + bit * (base - 1)) % P
            need(w[2 + a + i] == want, f"intermediate {i} = previous^2 * (base if power bit {a - 1 - i} else 1)")
            prev = w[2 + a + i]
        need(w[1 + a] == w[2 + a + a - 1], "the output is the last intermediate value")
    else:
        raise ValueError(gate)
    return bad


# ---- honest rows ----
def consts_of(gate, operands):
    return tuple((operands or {}).get("consts", DEFAULT_CONSTS))


def pi_hash_of(gate, operands):
    return tuple((operands or {}).get("pi_hash", DEFAULT_PI_HASH))


def _digits(v, base, n):
    return [(v // base ** i) % base for i in range(n)]


def poseidon_row(inputs, swap):
    """inputs: 12 values; swap need not be a bit (the delta wires follow it)."""
    w = [0] * 135
    w[0:12] = [v % P for v in inputs]
    w[24] = swap % P
    for i in range(4):
        w[25 + i] = swap * (w[4 + i] - w[i]) % P
    st = [(w[i] + w[25 + i]) % P for i in range(4)] + [(w[4 + i] - w[25 + i]) % P for i in range(4)] + w[8:12]
    if swap in (0, 1):
        want = poseidon_permutation(w[4:8] + w[0:4] + w[8:12] if swap else w[0:12])
    for rnd in range(30):
        st = _add_rc(st, rnd)
        if 1 <= rnd < 4:
            w[29 + 12 * (rnd - 1):29 + 12 * rnd] = st
        elif 4 <= rnd < 26:
            w[65 + rnd - 4] = st[0]
        elif rnd >= 26:
            w[87 + 12 * (rnd - 26):87 + 12 * (rnd - 25)] = st
        st = [pow(st[0], 7, P)] + st[1:] if 4 <= rnd < 26 else [pow(v, 7, P) for v in st]
        st = mds(st)
    w[12:24] = st
    if swap in (0, 1):
        assert st == want, "the gate's round structure is the Poseidon permutation of the (swapped) inputs"
    return w


def comparison_row(gate, x, y):
    _, a, b, _ = gate
    cb = -(-a // b)
    cs = 1 << cb
    f, s = _digits(x, cs, b), _digits(y, cs, b)
    eq = [int(p == q) for p, q in zip(f, s)]
    dummy = [1 if p == q else inv(q - p) for p, q in zip(f, s)]
    top = max([i for i in range(b) if f[i] != s[i]], default=None)
    msd = 0 if top is None else (s[top] - f[top]) % P
    inter, run = [], 0
    for i in range(b):
        inter.append(run if eq[i] else 0)
        run = run if eq[i] else (s[i] - f[i]) % P
    assert run == msd
    bits = _digits((cs + msd) % P, 2, cb + 1)
    assert bits[cb] == int(x <= y), "the top bit of 2^n + diff says first <= second"
    return [x, y, int(x <= y), msd] + f + s + dummy + eq + inter + bits


def honest_row(gate, operands):
    """All wires below the gate's wire count; operands is a dict (see typical_operands / edge_operands for each gate's keys)."""
    t, a, b, c = gate
    o = operands or {}
    k = consts_of(gate, o)
    if t == NOOP:
        row = []
    elif t == CONSTANT:
        row = list(k[:a])
    elif t == PUBLIC_INPUT:
        row = list(pi_hash_of(gate, o))
    elif t == ARITHMETIC:
        row = [v for m0, m1, ad in o["ops"] for v in (m0, m1, ad, (k[0] * m0 * m1 + k[1] * ad) % P)]
    elif t == POSEIDON:
        row = poseidon_row(o["inputs"], o["swap"])
    elif t == COMPARISON:
        row = comparison_row(gate, o["first"], o["second"])
    elif t == U32_ARITHMETIC:
        routed, limbs = [], []
        for m0, m1, ad in o["ops"]:
            out = (m0 * m1 + ad) % P  # the canonical representative is what lo and hi split
            lo, hi = out & U32_MAX, out >> 32
            routed += [m0, m1, ad, lo, hi, 0 if hi == U32_MAX else inv(U32_MAX - hi)]
            limbs += _digits(out, 4, 32)
        row = routed + limbs
    elif t == U32_RANGE_CHECK:
        row = list(o["values"]) + [d for v in o["values"] for d in _digits(v, 4, 16)]
    elif t == U32_ADD_MANY:
        routed, limbs = [], []
        for addends, carry in o["ops"]:
            out = sum(addends) + carry
            routed += list(addends) + [carry, out & U32_MAX, out >> 32]
            limbs += _digits(out & U32_MAX, 4, 16) + _digits(out >> 32, 4, 2)
        row = routed + limbs
    elif t == U32_SUBTRACTION:
        routed, limbs = [], []
        for x, y, br in o["ops"]:
            d = x - y - br
            ob = int(d < 0)
            res = d + (ob << 32)
            assert 0 <= res <= U32_MAX
            routed += [x, y, br, res, ob]
            limbs += _digits(res, 4, 16)
        row = routed + limbs
    elif t == U32_INTERLEAVE:
        routed, bits = [], []
        for x in o["values"]:
            routed += [x, sum(((x >> i) & 1) << (2 * i) for i in range(32))]
            bits += [(x >> (31 - i)) & 1 for i in range(32)]
        row = routed + bits
    elif t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):
        routed, bits = [], []
        for x in o["values"]:  # a 64-bit pattern; the wire holds it mod p
            bb = [(x >> (63 - i)) & 1 for i in range(64)]
            ev = sum(((x >> (2 * i + 1)) & 1) << i for i in range(32))  # bit wire 0 is bit 63: the "even" wires are the odd bits
            od = sum(((x >> (2 * i)) & 1) << i for i in range(32))
            if t == UNINTERLEAVE_TO_B32:
                ev, od = (sum(((v >> i) & 1) << (2 * i) for i in range(32)) for v in (ev, od))
            routed += [x % P, ev, od]
            bits += bb
        row = routed + bits
    elif t == ARITHMETIC_EXT:
        row = _flat(p for m0, m1, ad in o["ops"] for p in (m0, m1, ad, e_add(e_scale(e_mul(m0, m1), k[0]), e_scale(ad, k[1]))))
    elif t == MUL_EXT:
        row = _flat(p for m0, m1 in o["ops"] for p in (m0, m1, e_scale(e_mul(m0, m1), k[0])))
    elif t == BASE_SUM:
        row = [_le_sum(o["limbs"], b)] + list(o["limbs"])
    elif t == RANDOM_ACCESS:
        routed, bits = [], []
        for idx, items in o["copies"]:
            routed += [idx, items[idx]] + list(items)
            bits += _digits(idx, 2, a)
        row = routed + list(k[:c]) + bits
    elif t in (REDUCING, REDUCING_EXT):
        alpha, acc = o["alpha"], o["old_acc"]
        coeffs = o["coeffs"] if t == REDUCING_EXT else [(v, 0) for v in o["coeffs"]]
        accs = []
        for cf in coeffs:
            acc = e_add(e_mul(acc, alpha), cf)
            accs.append(acc)
        horner = o["old_acc"]
        for cf in coeffs:  # output = old_acc alpha^n + sum coeff_i alpha^(n-1-i)
            horner = e_mul(horner, alpha)
        apow = (1, 0)
        for cf in reversed(coeffs):
            horner = e_add(horner, e_mul(cf, apow))
            apow = e_mul(apow, alpha)
        assert horner == accs[-1]
        row = _flat([accs[-1], alpha, o["old_acc"]]) + (_flat(coeffs) if t == REDUCING_EXT else list(o["coeffs"])) + _flat(accs[:-1])
    elif t == POSEIDON_MDS:
        ins = o["inputs"]
        outs = list(zip(mds([p[0] for p in ins]), mds([p[1] for p in ins])))
        row = _flat(ins) + _flat(outs)
    elif t == COSET_INTERPOLATION:
        n = 1 << a
        dom, wts = _coset(a)
        shift, vals, point = o["shift"], o["values"], o["point"]
        sp = e_scale(point, inv(shift))
        ev, pr = (0, 0), (1, 0)
        ies, ips = [], []
        for kk, (lo, hi) in enumerate(_chunk_ranges(n, b)):
            if kk:
                ies.append(ev)
                ips.append(pr)
            ev, pr = _interp_steps(dom, wts, vals, sp, lo, hi, ev, pr)
        # the polynomial through (shift x_i, v_i) at `point` is the one through (x_i, v_i) at point / shift
        assert ev == interpolate(dom, vals, sp)
        row = [shift] + _flat(vals) + _flat([point, ev]) + _flat(ies) + _flat(ips) + _flat([sp])
    elif t == EXPONENTIATION:
        base, bits = o["base"], o["bits"]
        inter, cur = [], 1
        for i in range(a):
            cur = cur * cur % P * (1 + bits[a - 1 - i] * (base - 1)) % P
            inter.append(cur)
        if all(v in (0, 1) for v in bits):
            assert inter[-1] == pow(base, sum(v << i for i, v in enumerate(bits)), P)
        row = [base] + list(bits) + [inter[-1]] + inter
    else:
        raise ValueError(gate)
    assert len(row) == num_wires(gate), (NAME[t], len(row))
    return [int(v) % P for v in row]


def full_row(gate, row):
    """A gate's row padded to the 135 wires of the config with fixed filler (wires the gate does not constrain)."""
    return list(row) + det(1000 + gate[0], NUM_WIRES - len(row))


# ---- operand sets ----
def _ext_list(seed, n):
    return _pairs(det(seed, 2 * n))


def typical_operands(gate):
    t, a, b, c = gate
    s = 7000 + 13 * t
    if t in (NOOP, CONSTANT, PUBLIC_INPUT):
        return {}
    if t == ARITHMETIC:
        return {"ops": [tuple(det(s + i, 3)) for i in range(a)]}
    if t == POSEIDON:
        return {"inputs": det(s, 12), "swap": 1}
    if t == COMPARISON:  # 14 of the 16 chunks are equal; the two that differ are chunks 6 and 7
        return {"first": 0x12345678, "second": 0x1234A678}
    if t == U32_ARITHMETIC:
        return {"ops": [tuple(det(s + i, 3, 1 << 32)) for i in range(a)]}
    if t == U32_RANGE_CHECK:
        return {"values": det(s, a, 1 << 32)}
    if t == U32_ADD_MANY:
        return {"ops": [(det(s + i, b, 1 << 32), det(s + 50 + i, 1, 1 << 32)[0]) for i in range(a)]}
    if t == U32_SUBTRACTION:
        return {"ops": [tuple(det(s + i, 2, 1 << 32)) + (i & 1,) for i in range(a)]}
    if t == U32_INTERLEAVE:
        return {"values": det(s, a, 1 << 32)}
    if t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):
        return {"values": det(s, a)}
    if t == ARITHMETIC_EXT:
        return {"ops": [tuple(_ext_list(s + i, 3)) for i in range(a)]}
    if t == MUL_EXT:
        return {"ops": [tuple(_ext_list(s + i, 2)) for i in range(a)]}
    if t == BASE_SUM:
        return {"limbs": det(s, a, b)}
    if t == RANDOM_ACCESS:
        return {"copies": [((5 * cp + 3) % (1 << a), det(s + cp, 1 << a)) for cp in range(b)]}
    if t == REDUCING:
        return {"alpha": _ext_list(s, 1)[0], "old_acc": _ext_list(s + 1, 1)[0], "coeffs": det(s + 2, a)}
    if t == REDUCING_EXT:
        return {"alpha": _ext_list(s, 1)[0], "old_acc": _ext_list(s + 1, 1)[0], "coeffs": _ext_list(s + 2, a)}
    if t == POSEIDON_MDS:
        return {"inputs": _ext_list(s, 12)}
    if t == COSET_INTERPOLATION:
        return {"shift": det(s, 1)[0] or 1, "values": _ext_list(s + 1, 1 << a), "point": _ext_list(s + 2, 1)[0]}
    if t == EXPONENTIATION:
        return {"base": det(s, 1)[0], "bits": det(s + 1, a, 2)}
    raise ValueError(gate)


def _rotate(sets, n_ops):
    """edge row e gives op i the edge set (e + i) mod len: every set is seen by op 0, and the ops of a row differ"""
    return [[sets[(e + i) % len(sets)] for i in range(n_ops)] for e in range(len(sets))]


def edge_operands(gate):
    """[(name, operands)]"""
    t, a, b, c = gate
    typ = typical_operands(gate)
    M = U32_MAX
    if t == NOOP:
        return [("no wires", {})]
    if t == CONSTANT:
        return [("its constants", {}), ("constants 0 and p-1", {"consts": (0, P - 1)})]
    if t == PUBLIC_INPUT:
        return [("its hash", {}), ("hash 0, p-1", {"pi_hash": (0, P - 1, 0, P - 1)})]
    if t == ARITHMETIC:
        ones = [(P - 1, P - 1, P - 1)] * a
        return [("constants 0", dict(typ, consts=(0, 0))), ("constants p-1", dict(typ, consts=(P - 1, P - 1))),
                ("operands p-1", {"ops": ones}), ("operands and constants p-1", {"ops": ones, "consts": (P - 1, P - 1)})]
    if t == ARITHMETIC_EXT:
        ones = [((P - 1, P - 1),) * 3] * a
        return [("constants 0", dict(typ, consts=(0, 0))), ("constants p-1", dict(typ, consts=(P - 1, P - 1))),
                ("operands p-1", {"ops": ones}), ("operands and constants p-1", {"ops": ones, "consts": (P - 1, P - 1)})]
    if t == MUL_EXT:
        ones = [((P - 1, P - 1),) * 2] * a
        return [("constants 0", dict(typ, consts=(0, 0))), ("constants p-1", dict(typ, consts=(P - 1, P - 1))),
                ("operands p-1", {"ops": ones}), ("operands and constants p-1", {"ops": ones, "consts": (P - 1, P - 1)})]
    if t == POSEIDON:
        return [("swap 0", dict(typ, swap=0)), ("swap 1", dict(typ, swap=1)), ("all-zero input, swap 0", {"inputs": [0] * 12, "swap": 0}),
                ("all-zero input, swap 1", {"inputs": [0] * 12, "swap": 1}), ("all p-1 input", {"inputs": [P - 1] * 12, "swap": 1})]
    if t == COMPARISON:
        return [(n, {"first": x, "second": y}) for n, x, y in [
            ("equal", 0x89ABCDEF, 0x89ABCDEF), ("equal zeros", 0, 0), ("equal ones", M, M),
            ("chunk 0 only, first smaller", 0x89ABCDEC, 0x89ABCDEF), ("chunk 0 only, first larger", 0x89ABCDEF, 0x89ABCDEC),
            ("top chunk only, first smaller", 0x09ABCDEF, 0xC9ABCDEF), ("top chunk only, first larger", 0xC9ABCDEF, 0x09ABCDEF),
            ("0 and 2^32-1", 0, M), ("2^32-1 and 0", M, 0), ("top says smaller, the rest larger", 0x3FFFFFFF, 0x40000000)]]
    if t == U32_ARITHMETIC:
        return [(f"edge {e}", {"ops": ops}) for e, ops in enumerate(_rotate(_u32_arith_sets(), a))]
    if t == U32_RANGE_CHECK:
        sets = [0, M, 1, 0x80000000, 0x55555555, 0xAAAAAAAA, 3 << 30]
        return [(f"edge {e}", {"values": ops}) for e, ops in enumerate(_rotate(sets, a))]
    if t == U32_ADD_MANY:
        sets = [([0] * b, 0), ([M] * b, M), ([M] + [0] * (b - 1), 1), ([0] * b, M), ([1] * b, M - b)]
        return [(f"edge {e}", {"ops": ops}) for e, ops in enumerate(_rotate(sets, a))]
    if t == U32_SUBTRACTION:
        sets = [(5, 5, 0), (5, 5, 1), (0, M, 1), (M, 0, 0), (0, 0, 0), (0, 0, 1), (M, M, 1), (0, M, 0), (M, 0, 1)]
        return [(f"edge {e}", {"ops": ops}) for e, ops in enumerate(_rotate(sets, a))]
    if t == U32_INTERLEAVE:
        sets = [0, M, 1, 1 << 31, 0x80000001]
        return [(f"edge {e}", {"values": ops}) for e, ops in enumerate(_rotate(sets, a))]
    if t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):
        # all 64 ones is 2^64-1 = 2^32-2 (mod p): the gate takes bit patterns, the wire holds the pattern mod p
        sets = [0, (1 << 64) - 1, 1, 1 << 63, (1 << 63) | 1, P - 1, P, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555]
        return [(f"edge {e}", {"values": ops}) for e, ops in enumerate(_rotate(sets, a))]
    if t == BASE_SUM:
        return [("all limbs 0", {"limbs": [0] * a}), (f"all limbs {b - 1}", {"limbs": [b - 1] * a}),
                ("only the lowest limb", {"limbs": [b - 1] + [0] * (a - 1)}), ("only the highest limb", {"limbs": [0] * (a - 1) + [b - 1]})]
    if t == RANDOM_ACCESS:
        vec = 1 << a
        items = [det(8100 + cp, vec) for cp in range(b)]
        return [("index 0", {"copies": [(0, it) for it in items]}), (f"index {vec - 1}", {"copies": [(vec - 1, it) for it in items]}),
                ("one index per bit", {"copies": [(1 << (cp % a), it) for cp, it in enumerate(items)]}),
                ("equal items", {"copies": [(cp, [7] * vec) for cp in range(b)]})]
    if t == EXPONENTIATION:
        bits = typ["bits"]
        return [("all bits 0", dict(typ, bits=[0] * a)), ("all bits 1", dict(typ, bits=[1] * a)), ("base 0", dict(typ, base=0)),
                ("base p-1", dict(typ, base=P - 1)), ("base 0, all bits 0", {"base": 0, "bits": [0] * a}),
                ("only the top bit", dict(typ, bits=[0] * (a - 1) + [1])), ("only the bottom bit", dict(typ, bits=[1] + [0] * (a - 1))),
                ("base 1", dict(typ, base=1, bits=bits)),
                # the open reading: this gate does not range its bits, a "bit" b multiplies by 1 + b (base - 1)
                ("a bit equal to 2, intermediates follow", dict(typ, bits=[2] + bits[1:]))]
    if t in (REDUCING, REDUCING_EXT):
        zero_coeffs = [0] * a if t == REDUCING else [(0, 0)] * a
        return [("alpha 0", dict(typ, alpha=(0, 0))), ("old_acc 0", dict(typ, old_acc=(0, 0))),
                ("alpha 0 and old_acc 0", dict(typ, alpha=(0, 0), old_acc=(0, 0))), ("coefficients 0", dict(typ, coeffs=zero_coeffs)),
                ("alpha in the base field", dict(typ, alpha=(typ["alpha"][0], 0))), ("alpha p-1", dict(typ, alpha=(P - 1, P - 1)))]
    if t == POSEIDON_MDS:
        return [("all p-1", {"inputs": [(P - 1, P - 1)] * 12}), ("all 0", {"inputs": [(0, 0)] * 12}),
                ("one lane", {"inputs": [(1, 0)] + [(0, 0)] * 11}), ("the last lane, second component", {"inputs": [(0, 0)] * 11 + [(0, 1)]})]
    if t == COSET_INTERPOLATION:
        dom, _ = _coset(a)
        sh = typ["shift"]
        return [("shift 1", dict(typ, shift=1)), ("point on the coset", dict(typ, point=(sh * dom[3] % P, 0))),
                ("point on the coset, first", dict(typ, point=(sh * dom[0] % P, 0))),
                ("point on the coset, last", dict(typ, point=(sh * dom[-1] % P, 0))),
                ("shift p-1", dict(typ, shift=P - 1)), ("values 0", dict(typ, values=[(0, 0)] * (1 << a))),
                ("point 0", dict(typ, point=(0, 0)))]
    raise ValueError(gate)


def _u32_arith_sets():
    """(m0, m1, addend). (2^32-1)^2 + (2^32-1) = 2^64 - 2^32 = p - 1 is the one output with hi = 2^32-1, and then lo = 0. No other
    three u32 operands reach it (m0 m1 <= (2^32-1)^2), but the gate does not range its inputs: 2^32 (2^32-1) and 0 0 + (p-1) do."""
    M = U32_MAX
    return [(0, 0, 0), (M, M, M), (1 << 32, M, 0), (0, 0, P - 1), (M, M, 0), (1, 0, M), (M, 1, 0), (1 << 16, 1 << 16, 0)]


# ---- malicious rows ----
def malicious_rows(gate, consts=DEFAULT_CONSTS, pi_hash=DEFAULT_PI_HASH):
    """[(name, consts, pi_hash, row)]: every one must be refused; the helper wires follow the lie wherever they can. The rows are
    built for the constants and the public-inputs hash given (those of the circuit row they are to be written onto)."""
    t, a, b, c = gate
    out = []
    consts, pi_hash = tuple(consts), tuple(pi_hash)
    typ = dict(typical_operands(gate), consts=consts, pi_hash=pi_hash)
    base = honest_row(gate, typ) if t != NOOP else []
    L = layout(gate)
    M = U32_MAX

    def add(name, row):
        out.append((name, consts, pi_hash, [int(v) % P for v in row]))

    def limb_4(row, limbs, name):
        # a limb of 4 with the next limb one lower keeps every sum: only the range says no
        j = next(j for j in range(len(limbs) - 1) if row[limbs[j]] == 0 and row[limbs[j + 1]] >= 1)
        r = list(row)
        r[limbs[j]], r[limbs[j + 1]] = 4, r[limbs[j + 1]] - 1
        add(name, r)
    if t == U32_ARITHMETIC:
        # m0 m1 + addend = lo - 1 as integers, claimed as lo + 2^32 (2^32-1) = lo - 1 + p: the same residue, another number
        for lo in (1, 2, M):
            r = list(base)
            r[0:6] = [1, lo - 1, 0, lo, M, 0]
            r[L["limb"][0][0]:L["limb"][0][0] + 32] = _digits(lo, 4, 16) + [3] * 16
            add(f"p-alias: hi = 2^32-1 with lo = {lo}", r)
        r = list(base)
        r[0:6] = [1, 0, 0, 1, M, 12345]
        r[L["limb"][0][0]:L["limb"][0][0] + 32] = _digits(1, 4, 16) + [3] * 16
        add("p-alias with a made-up inverse", r)
        limb_4(base, L["limb"][1][:16], "a low limb equal to 4, sums repaired")
        limb_4(base, L["limb"][2][16:], "a high limb equal to 4, sums repaired")
    elif t == U32_RANGE_CHECK:
        limb_4(base, L["aux_limb"][0], "a limb equal to 4, sums repaired")
        limb_4(base, L["aux_limb"][a - 1], "a limb of the last input equal to 4, sums repaired")
    elif t == U32_ADD_MANY:
        limb_4(base, L["limb"][0][:16], "a result limb equal to 4, sums repaired")
        r = list(base)  # carry limbs (4, 0) spell 4 like (0, 1); the inputs are not ranged, so a carry of 4 can be reached
        i0 = L["addend"][a - 1][0]
        r[i0:i0 + b + 3] = [1 << 32] * b + [(4 - b) << 32, 0, 4]
        r[L["limb"][a - 1][0]:L["limb"][a - 1][0] + 18] = [0] * 16 + [4, 0]
        add("a carry limb equal to 4", r)
    elif t == U32_SUBTRACTION:
        limb_4(base, L["limb"][0], "a limb equal to 4, sums repaired")
        r = list(base)
        r[0:5] = [5, 1 << 33, 0, 5, 2]  # 5 - 2^33 + 2 * 2^32 = 5
        r[L["limb"][0][0]:L["limb"][0][0] + 16] = _digits(5, 4, 16)
        add("output_borrow = 2", r)
    elif t == COMPARISON:
        r = list(base)
        r[2] = 1 - r[2]
        add("result flipped", r)
        eqr = comparison_row(gate, 77, 77)
        eqr[2] = 0
        add("equal operands called greater", eqr)
        r = comparison_row(gate, 0x1000, 0x2000)  # chunk 6 holds 1 vs 2: write 5 vs 6, the same difference, inputs repaired
        r[L["first_chunk"][6]], r[L["second_chunk"][6]] = 5, 6
        r[0], r[1] = _le_sum([r[j] for j in L["first_chunk"]], 4), _le_sum([r[j] for j in L["second_chunk"]], 4)
        add("chunks 5 and 6, sums repaired", r)
        r = list(base)  # 4 + msd spelt with a bit of 2
        bits = L["most_significant_diff_bit"]
        if r[bits[1]] == 1:
            r[bits[0]], r[bits[1]] = r[bits[0]] + 2, 0
        else:
            r[bits[1]], r[bits[2]] = 2, r[bits[2]] - 1
            r[2] = r[bits[2]]
        add("a diff bit equal to 2, sum repaired", r)
    elif t == U32_INTERLEAVE:
        r = list(base)
        bits = L["bit"][0]
        j = next(j for j in range(31) if r[bits[j]] == 1 and r[bits[j + 1]] == 0)
        r[bits[j]], r[bits[j + 1]] = 0, 2  # the same x; x_interleaved follows: 4^k * 2 in place of 4^(k+1)
        r[1] = _le_sum([r[i] for i in bits][::-1], 4)
        add("a bit equal to 2, both sums repaired", r)
    elif t in (UNINTERLEAVE_TO_U32, UNINTERLEAVE_TO_B32):
        r = list(base)
        bits = L["bit"][0]
        bs = 2 if t == UNINTERLEAVE_TO_U32 else 4
        j = next(j for j in range(63) if r[bits[j]] == 1 and r[bits[j + 1]] == 0)
        r[bits[j]], r[bits[j + 1]] = 0, 2
        vals = [r[i] for i in bits]
        r[1], r[2] = _le_sum(vals[0::2][::-1], bs), _le_sum(vals[1::2][::-1], bs)
        add("a bit equal to 2, all three sums repaired", r)
    elif t == BASE_SUM:
        r = list(base)
        j = next(j for j in range(a - 1) if r[1 + j] == 0 and r[2 + j] >= 1)
        r[1 + j], r[2 + j] = b, r[2 + j] - 1
        add(f"a limb equal to {b}, sum repaired", r)
        r = list(base)
        r[1] = r[1] + b
        r[0] = (r[0] + b) % P
        add(f"the lowest limb {b} too large, sum follows", r)
    elif t == RANDOM_ACCESS:
        r = list(base)  # copy 0 has index 3 = bits 1, 1, 0, 0: spell it 3, 0, 0, 0
        bits = L["bit"][0]
        assert r[bits[1]] == 1
        r[bits[0]], r[bits[1]] = r[bits[0]] + 2, 0
        add("a bit equal to 2 or 3, index sum repaired", r)
        r = list(base)
        r[L["claimed_element"][1]] = r[L["list_item"][1][(r[L["access_index"][1]] + 1) % (1 << a)]]
        add("the claimed element is the neighbour's", r)
    elif t == POSEIDON:
        add("swap = 2, delta wires repaired", poseidon_row(typ["inputs"], 2))
        add("swap = p-1, delta wires repaired", poseidon_row(typ["inputs"], P - 1))
        r = poseidon_row(typ["inputs"], 1)
        r[12], r[13] = r[13], r[12]
        add("two outputs exchanged", r)
    elif t == EXPONENTIATION:
        r = list(base)
        r[1 + a] = (r[1 + a] * r[0]) % P
        add("output one factor of base too many", r)
    elif t == ARITHMETIC:
        r = list(base)
        r[2], r[6] = r[6], r[2]
        add("the addends of ops 0 and 1 exchanged", r)
    elif t in (REDUCING, REDUCING_EXT):
        r = list(base)
        r[0], r[1] = r[1], r[0]
        add("the components of the output exchanged", r)
    elif t == POSEIDON_MDS:
        r = list(base)
        r[24:26], r[26:28] = r[26:28], r[24:26]
        add("outputs 0 and 1 exchanged", r)
    elif t == COSET_INTERPOLATION:
        r = list(base)
        i = L["evaluation_value"]
        r[i:i + 2] = r[L["value"][0]:L["value"][0] + 2]
        add("the first value claimed as the evaluation", r)
    elif t in (ARITHMETIC_EXT, MUL_EXT):
        r = list(base)
        i = L["output"][0]
        m0, m1 = (r[0], r[1]), (r[2], r[3])
        r[i:i + 2] = e_scale((m0[0] * m1[0] % P, m0[1] * m1[1] % P), consts[0])  # componentwise, not X^2 = 7
        if t == ARITHMETIC_EXT:
            r[i:i + 2] = e_add((r[i], r[i + 1]), e_scale((r[4], r[5]), consts[1]))
        add("a componentwise product in place of the extension product", r)
    elif t == CONSTANT:
        add("constants exchanged", [consts[1], consts[0]])
    elif t == PUBLIC_INPUT:
        add("hash rotated", list(pi_hash[1:]) + [pi_hash[0]])
    return out


# ---- corruptions ----
def corruptions(gate, row):
    """[(wire, new value, kind)] over a row of the gate (its wires only): fixed, no sampling. `row` must be honest-sized."""
    nw = num_wires(gate)
    assert len(row) == nw
    out = [(j, (row[j] + 1) % P, "+1") for j in range(nw)]
    for j, size in ranged_wires(gate):
        out.append((j, size, "first out of range"))
        out.append((j, (row[j] + 1) % size if row[j] < size else 0, "another value in range"))
    if nw < NUM_WIRES:
        out.append((nw, None, "beyond the gate"))  # value: the filler of full_row plus 1
    return out


def apply_corruption(gate, full, corruption):
    j, v, _ = corruption
    r = list(full)
    r[j] = (r[j] + 1) % P if v is None else v
    return r

"""What a constraint of the generic AIR machinery MEANS, stated without the oracle and without the library (include/cityprover.h
cp_air_*; oracle/stark_air.c and the product were written from the same memory of starky, so a shared misreading of a sink kind
passes every byte comparison between them). Python integers mod p, one row at a time:
  * the next row of row n - 1 is row 0;
  * a sink of kind `all` is checked on every row, `transition` on rows 0 .. n - 2, `first` on row 0 only, `last` on row n - 1 only.
Then a PROBE AIR with one column per question a selector answers, its honest trace, and a fixed list of single-cell corruptions
whose verdict follows from the two lines above. Test infrastructure only."""
import numpy as np

import air_programs as A

P = A.P
KIND_OF = {A.ASSERT_ZERO: "all", A.ASSERT_ZERO_TRANSITION: "transition", A.ASSERT_ZERO_FIRST_ROW: "first", A.ASSERT_ZERO_LAST_ROW: "last"}
N_COLUMNS, N_PUBLIC, N_GLOBAL = 8, 2, 1
N_CORRUPTIONS = 7 * 5 + 2


def corrupted_rows(n):
    """the rows where a cell is corrupted"""
    return (0, 1, n // 2, n - 2, n - 1)


def binds(kind, row, n):
    """does a sink of this kind constrain this row of an n-row trace"""
    return {"all": True, "transition": row != n - 1, "first": row == 0, "last": row == n - 1}[kind]


def sink_values(builder, trace, publics=(), globals_=(), challenges=()):
    """-> (values, kinds, degrees): values[k][r] = what sink k (program order) evaluates to on row r, unfiltered; kinds[k] its kind;
    degrees[k] its degree in the row variables (a column is 1, a uniform value 0, a product adds, a sum takes the larger)."""
    if builder.kind != A.CONSTRAINTS:
        raise ValueError("a constraint program is expected")
    n = len(trace[0])
    cols = [[int(v) % P for v in c] for c in trace]
    uni = {A.PUBLIC: [int(v) for v in publics], A.GLOBAL: [int(v) for v in globals_], A.CHALLENGE: [int(v) for v in challenges]}
    values, kinds, degrees = [], [], []
    for r in range(n):
        val, deg, k = [0] * len(builder.ops), [0] * len(builder.ops), 0
        for i, (op, a, b, _) in enumerate(builder.ops):
            if op == A.LOCAL:
                val[i], deg[i] = cols[a][r], 1
            elif op == A.NEXT:
                val[i], deg[i] = cols[a][(r + 1) % n], 1
            elif op in uni:
                val[i] = uni[op][a] % P
            elif op == A.CONST:
                val[i] = builder.consts[a] % P
            elif op == A.ADD:
                val[i], deg[i] = (val[a] + val[b]) % P, max(deg[a], deg[b])
            elif op == A.SUB:
                val[i], deg[i] = (val[a] - val[b]) % P, max(deg[a], deg[b])
            elif op == A.MUL:
                val[i], deg[i] = val[a] * val[b] % P, deg[a] + deg[b]
            elif op == A.NEG:
                val[i], deg[i] = -val[a] % P, deg[a]
            elif op in KIND_OF:
                if r == 0:
                    values.append([0] * n)
                    kinds.append(KIND_OF[op])
                    degrees.append(deg[a])
                values[k][r] = val[a]
                k += 1
            else:
                raise ValueError("op %d of a constraint program: code %d" % (i, op))
    return values, kinds, degrees


def violations(builder, trace, publics=(), globals_=(), challenges=()):
    """-> (the sorted list of (sink index, kind, row) where a sink that binds the row is not zero, the degree of every sink)"""
    values, kinds, degrees = sink_values(builder, trace, publics, globals_, challenges)
    n = len(trace[0])
    return sorted((k, kinds[k], r) for k in range(len(kinds)) for r in range(n) if binds(kinds[k], r, n) and values[k][r]), degrees


def root_of_unity(db):
    """the primitive 2^db-th root both sides use: 7^((p - 1) / 2^32), squared down"""
    g = pow(7, (P - 1) >> 32, P)
    for _ in range(db, 32):
        g = g * g % P
    return g


# sinks of the probe in program order: (column, kind, reads the next row)
PROBE_SINKS = ((0, "all", False), (1, "transition", False), (2, "first", False), (3, "last", False), (4, "transition", True), (5, "all", True),
               (6, "first", False), (6, "transition", True), (6, "last", False))


def probe_air(q, db, top_degree=False, extended=False):
    """the constraints of the probe as a Builder (8 columns, 2 publics, 1 global):
      col 0  c0 = 0 every row              col 4  next(c4) - c4 - 1 = 0 transition (the wrap row breaks it and is not bound)
      col 1  c1 = 0 transition             col 5  next(c5) - w c5 = 0 every row, w a primitive n-th root (holds across the wrap)
      col 2  c2 = 0 first row              col 6  c6 = public0 first; next(c6) = global0 c6 transition; c6 = public1 last
      col 3  c3 = 0 last row               col 7  the mask m: no constraint of its own, never 0
    top_degree: the sinks of columns 0-3 are multiplied by powers of m up to the bound of q (every-row and transition sinks reach
    2^q + 1, first / last row sinks 2^q): the zero set is unchanged, the quotient fills what the degree bound allows.
    extended: one extended column (8) = challenge0 * c7 + next(c4), bound on every row - the NEXT wraps in the map step as well."""
    b = A.Builder(A.CONSTRAINTS, N_COLUMNS + (1 if extended else 0), N_PUBLIC, N_GLOBAL, 1 if extended else 0)
    m = b.local(7)

    def lifted(v, degree):
        for _ in range(degree - 1 if top_degree else 0):
            v = b.mul(v, m)
        return v
    b.assert_zero(lifted(b.local(0), (1 << q) + 1), "all")
    b.assert_zero(lifted(b.local(1), (1 << q) + 1), "transition")
    b.assert_zero(lifted(b.local(2), 1 << q), "first")
    b.assert_zero(lifted(b.local(3), 1 << q), "last")
    b.assert_zero(b.sub(b.sub(b.next(4), b.local(4)), b.const(1)), "transition")
    b.assert_zero(b.sub(b.next(5), b.mul(b.const(root_of_unity(db)), b.local(5))), "all")
    c6 = b.local(6)
    b.assert_zero(b.sub(c6, b.public(0)), "first")
    b.assert_zero(b.sub(b.next(6), b.mul(b.glob(0), c6)), "transition")
    b.assert_zero(b.sub(c6, b.public(1)), "last")
    if extended:
        b.assert_zero(b.sub(b.local(8), b.add(b.mul(b.challenge(0), m), b.next(4))), "all")
    return b


def probe_map():
    """the map step of probe_air(extended=True): extended column 0 = challenge0 * c7 + next(c4); reads trace columns only"""
    m = A.Builder(A.MAP, N_COLUMNS + 1, N_PUBLIC, N_GLOBAL, 1, n_out_columns=1)
    m.store(0, m.add(m.mul(m.challenge(0), m.local(7)), m.next(4)))
    return m


def honest_trace(db, seed):
    """-> (trace (8, n) uint64, publics, globals) satisfying probe_air at every bound row - and breaking it wherever a row is NOT
    bound: c1 is non-zero at n - 1, c2 / c3 are non-zero off their row, c4 does not wrap"""
    n = 1 << db
    rng = np.random.default_rng(seed)
    nz = lambda: int(rng.integers(1, P - 1, dtype=np.uint64))   # non-zero, and still non-zero after an increment
    w, s, pub0, glob0 = root_of_unity(db), nz(), nz(), nz()
    t = [[0] * n for _ in range(N_COLUMNS)]
    t[1][n - 1] = nz()
    t[2] = [0] + [nz() for _ in range(n - 1)]
    t[3] = [nz() for _ in range(n - 1)] + [0]
    t[4] = [7 + i for i in range(n)]
    t[5] = [s * pow(w, i, P) % P for i in range(n)]
    t[6] = [pub0 * pow(glob0, i, P) % P for i in range(n)]
    t[7] = [nz() for _ in range(n)]
    return np.array(t, dtype=np.uint64), (pub0, t[6][n - 1]), (glob0,)


def corruptions(trace, publics):
    """the fixed list [(name, column or None, row or None, trace, publics)]: every column 0-6 at rows 0, 1, n/2, n-2, n-1 (a zero
    cell becomes 1, a non-zero cell is incremented), then public0 + 1 and public1 + 1 with the honest trace"""
    n = trace.shape[1]
    out = []
    for c in range(7):
        for r in corrupted_rows(n):
            t = trace.copy()
            t[c, r] = (int(t[c, r]) + 1) % P
            assert int(t[c, r]) != 0
            out.append(("c%d@%d" % (c, r), c, r, t, tuple(publics)))
    out.append(("public0", None, None, trace, ((publics[0] + 1) % P, publics[1])))
    out.append(("public1", None, None, trace, (publics[0], (publics[1] + 1) % P)))
    return out


def expected_violations(column, row, n, name=None):
    """the hand-written table: the sinks of the corrupted column, on the rows whose evaluation reads the cell (the row itself, and
    the row before it where the sink reads the next row), wherever the sink's kind binds that row"""
    if column is None:
        return [(6, "first", 0)] if name == "public0" else [(8, "last", n - 1)]
    out = set()
    for k, (c, kind, reads_next) in enumerate(PROBE_SINKS):
        if c != column:
            continue
        for r in {row, (row - 1) % n} if reads_next else {row}:
            if binds(kind, r, n):
                out.add((k, kind, r))
    return sorted(out)


def quotient_degree_bound(degrees, kinds, n):
    """the highest coefficient of a quotient that may be non-zero (inclusive): max_k(d_k (n - 1) + e_k) - n, e_k the degree of the
    selector: 0 for all, 1 for transition (x - g^(n-1)), n - 1 for first / last (a Lagrange basis polynomial)"""
    e = {"all": 0, "transition": 1, "first": n - 1, "last": n - 1}
    return max(d * (n - 1) + e[k] for d, k in zip(degrees, kinds)) - n

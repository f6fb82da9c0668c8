"""The query phase of plonky2 verification stated word by word, independent of csrc/fri_verify.h and of its instance table:

  * word_map: a label for every u64 word of a proof, walked in tests/proof_format.py's field order;
  * mutations: what is done to every word;
  * closed_form: the verdict (status, query, detail) one changed word must get while the challenges stay as they were, from the
    label and the query indices alone;
  * verify_queries: the query phase on Python integers (the oracle's hash, Lagrange interpolation, emul / einv), first failure
    in verify_fri_queries' order: per round the oracle paths 0..3, the opening point, per layer the value and then the path,
    then the final polynomial;
  * replay_challenges: the transcript of a proof whose circuit digest is known, with the oracle's challenger.

Used by tests/test_fri_query_words.py (host build of the header) and tests/test_gpu_fri_query_words.py (the kernels)."""
import functools
import struct

import numpy as np

import oracle_lib as O
import reference_challenges as R

P = O.P
OK, MALFORMED, NONCANONICAL = (0, -1, -1), (1, -1, -1), (2, -1, -1)
SALT = 4
OPENING_FIELDS = ["constants", "plonk_sigmas", "wires", "plonk_zs", "plonk_zs_next", "partial_products", "quotient_polys", "lookup_zs",
                  "lookup_zs_next"]
BATCH0 = ["constants", "plonk_sigmas", "wires", "plonk_zs", "partial_products", "quotient_polys"]   # opened at zeta; plonk_zs_next at g zeta
ROUND_KINDS = ("leaf", "salt", "sib", "eval", "path")
FELT_KINDS = ("cap", "open", "fcap", "leaf", "salt", "sib", "eval", "path", "final", "pi")   # what the parser reads as field elements

# The only changes of one word that may be accepted, each with the reason. `hook`: the challenges are supplied, not derived.
ACCEPTED = [
    ("unreached cap entry", "no query index leads to this entry of the cap, so no path is compared with it"),
    ("oracle 0 sibling without a cap", "the constants / sigmas cap is unknown, so that oracle's paths are not climbed (its leaf still enters the combine)"),
    ("pow_witness under the hook", "the proof of work is part of the transcript, which the hook does not replay"),
    ("public input under the hook", "public inputs enter the transcript and the vanishing identity, neither of which the hook checks"),
]


def words_of(blob):
    assert len(blob) % 8 == 0
    return list(struct.unpack("<%dQ" % (len(blob) // 8), blob))


def word_map(blob, salted=False):
    """one label per u64 word of `blob`. salted: the leaves of oracles 1..3 end with SALT salt elements (zero knowledge).
      ("len", what) | ("cap", b, e, limb) | ("open", field, element, limb) | ("fcap", l, e, limb) | ("leaf", q, b, j) |
      ("salt", q, b, j) | ("sib", q, b, level, limb) | ("eval", q, l, i, limb) | ("path", q, l, level, limb) | ("final", i, limb) |
      ("pow",) | ("pi", i)"""
    w = words_of(blob)
    lab = []

    def length(what):
        lab.append(("len", what))
        return w[len(lab) - 1]

    def items(count, limbs, make):
        for e in range(count):
            for k in range(limbs):
                lab.append(make(e, k))
    for b in (1, 2, 3):
        items(length(("cap", b)), 4, lambda e, k: ("cap", b, e, k))
    for f in OPENING_FIELDS:
        items(length(("open", f)), 2, lambda e, k: ("open", f, e, k))
    for l in range(length("fri caps")):
        items(length(("fcap", l)), 4, lambda e, k: ("fcap", l, e, k))
    for q in range(length("rounds")):
        for b in range(length(("oracles", q))):
            n = length(("leaf", q, b))
            ns = SALT if salted and b >= 1 else 0
            items(n, 1, lambda j, k: ("leaf", q, b, j) if j < n - ns else ("salt", q, b, j - (n - ns)))
            items(length(("sib", q, b)), 4, lambda i, k: ("sib", q, b, i, k))
        for l in range(length(("steps", q))):
            items(length(("eval", q, l)), 2, lambda i, k: ("eval", q, l, i, k))
            items(length(("path", q, l)), 4, lambda i, k: ("path", q, l, i, k))
    items(length("final"), 2, lambda i, k: ("final", i, k))
    lab.append(("pow",))
    items(length("public inputs"), 1, lambda i, k: ("pi", i))
    assert len(lab) == len(w), (len(lab), len(w))
    return lab


def mutations(words, labels):
    """[(word, name, new value)]: every word (v + 1) mod p, field elements (and the proof-of-work witness) v ^ 2^40 as well;
    a length prefix + 1"""
    out = []
    for i, (v, lab) in enumerate(zip(words, labels)):
        if lab[0] == "len":
            out.append((i, "+1", v + 1))
        else:
            out.append((i, "+1 mod p", (v + 1) % P))
            out.append((i, "bit 40", v ^ (1 << 40)))
    return out


class Geometry:
    """what the closed form needs of a shape: where a query index leads in every tree"""

    def __init__(self, sh):
        self.lb = sh.degree_bits + sh.rate_bits
        self.cap_height = sh.cap_height
        self.arity_bits = [sh.arity_bits[i] for i in range(sh.n_arity)]
        self.depth0 = self.lb - sh.cap_height
        self.before = [sum(self.arity_bits[:l]) for l in range(len(self.arity_bits))]            # index bits consumed before layer l
        self.depth = [max(self.lb - self.before[l] - self.arity_bits[l] - sh.cap_height, 0) for l in range(len(self.arity_bits))]
        nc = sh.num_challenges
        self.k = [sh.num_constants + sh.num_routed_wires, sh.num_wires, nc * (1 + sh.num_partial_products), nc * sh.quotient_degree_factor]
        self.nc = nc
        self.degree_bits = sh.degree_bits
        self.salted = bool(sh.zero_knowledge)


def accepted_kind(label, indices, G, with_cs_cap, hook):
    """index into ACCEPTED of a changed word that must be accepted, or None"""
    kind = label[0]
    if kind == "cap" and not any(x >> G.depth0 == label[2] for x in indices):
        return 0
    if kind == "fcap":
        l = label[1]
        if not any((x >> (G.before[l] + G.arity_bits[l])) >> G.depth[l] == label[2] for x in indices):
            return 0
    if kind == "sib" and label[2] == 0 and not with_cs_cap:
        return 1
    if kind == "pow" and hook:
        return 2
    if kind == "pi" and hook:
        return 3
    return None


def closed_form(label, new, indices, G, with_cs_cap=True, hook=True):
    """the verdict of a proof in which the word `label` alone was changed to `new`, challenges (and so `indices`) held fixed"""
    kind = label[0]
    if kind == "len":
        return MALFORMED
    if kind in FELT_KINDS and new >= P:
        return NONCANONICAL
    if accepted_kind(label, indices, G, with_cs_cap, hook) is not None:
        return OK
    first_arith = lambda q: (8, q, 0) if G.arity_bits else (10, q, -1)   # where a changed combine shows
    if kind in ("leaf", "salt", "sib"):
        q, b = label[1], label[2]
        if b == 0 and not with_cs_cap:
            assert kind == "leaf"
            return first_arith(q)
        return (7, q, b)
    if kind == "eval":
        q, l, i = label[1], label[2], label[3]
        own = (indices[q] >> G.before[l]) & ((1 << G.arity_bits[l]) - 1)
        return (8, q, l) if i == own else (9, q, l)
    if kind == "path":
        return (9, label[1], label[2])
    if kind == "final":
        return (10, 0, -1)
    if kind == "open":
        return first_arith(0)
    if kind == "cap":
        return (7, min(q for q, x in enumerate(indices) if x >> G.depth0 == label[2]), label[1])
    if kind == "fcap":
        l = label[1]
        return (9, min(q for q, x in enumerate(indices) if (x >> (G.before[l] + G.arity_bits[l])) >> G.depth[l] == label[2]), l)
    raise AssertionError("no closed form outside the hook for %r" % (label,))


# ---- the query phase on Python integers ------------------------------------------------------------------------------------
# Pure functions of their arguments, memoised: a batch of proofs that differ in one word shares nearly every hash.
@functools.lru_cache(maxsize=None)
def _leaf_digest(leaf):
    return tuple(int(v) for v in O.hash_or_noop(np.array(leaf, dtype=np.uint64)))


@functools.lru_cache(maxsize=None)
def _node(left, right):
    return tuple(int(v) for v in O.two_to_one(np.array(left, dtype=np.uint64), np.array(right, dtype=np.uint64)))


def path_ok(leaf, index, siblings, cap):
    cur = _leaf_digest(tuple(leaf))
    for s in siblings:
        cur = _node(tuple(s), cur) if index & 1 else _node(cur, tuple(s))
        index >>= 1
    return index < len(cap) and cur == tuple(int(v) for v in cap[index])


@functools.lru_cache(maxsize=None)
def _reduced(opened, alpha):
    """(sum_j alpha^j opened[j], alpha^len)"""
    red, shift = R.ZERO, R.ONE
    for e in reversed(opened):
        red = R.eadd(R.emul(red, alpha), e)
        shift = R.emul(shift, alpha)
    return red, shift


@functools.lru_cache(maxsize=None)
def _combine(evals, x, alpha, points, opened):
    """plonky2 fri_combine_initial; evals[b]: the unsalted leaf values a batch reads, in batch order. None: a point on the coset"""
    total = R.ZERO
    for ev, point, op in zip(evals, points, opened):
        red, shift = _reduced(op, alpha)
        mine = R.ZERO
        for v in reversed(ev):
            mine = R.eadd(R.emul(mine, alpha), (v, 0))
        den = R.esub((x, 0), point)
        if den == R.ZERO:
            return None
        total = R.eadd(R.emul(total, shift), R.emul(R.esub(mine, red), R.einv(den)))
    return total


@functools.lru_cache(maxsize=None)
def _fold(x, within, ab, evals, beta):
    return R.peval(R.fold_poly(x, within, ab, evals), beta)


@functools.lru_cache(maxsize=None)
def _final(coeffs, x):
    return R.peval(list(coeffs), (x, 0))


def verify_queries(pf, sh, alpha, zeta, betas, indices, cs_cap=None):
    """the first failure of the query phase of parsed proof `pf` as (status, query, detail), or OK"""
    G = Geometry(sh)
    N = 1 << G.lb
    alpha, zeta = tuple(int(v) for v in alpha), tuple(int(v) for v in zeta)
    betas = [tuple(int(v) for v in b) for b in betas]
    omega, g = pow(7, (P - 1) >> G.lb, P), pow(7, (P - 1) >> G.degree_bits, P)
    o = pf["openings"]
    opened = (tuple(tuple(e) for f in BATCH0 for e in o[f]), tuple(tuple(e) for e in o["plonk_zs_next"]))
    points = (zeta, R.emul(zeta, (g, 0)))
    caps = [cs_cap, pf["wires_cap"], pf["zs_pp_cap"], pf["quotient_cap"]]
    final = tuple(tuple(c) for c in pf["final_poly"])
    for q, rnd in enumerate(pf["queries"]):
        x_index = int(indices[q]) % N
        for b, (leaf, sib) in enumerate(rnd["initial"]):
            if caps[b] is not None and not path_ok(leaf, x_index, sib, caps[b]):
                return (7, q, b)
        x = 7 * pow(omega, R.rev(x_index, G.lb), P) % P
        leaves = [rnd["initial"][b][0][:G.k[b]] for b in range(4)]                     # without the salt
        evals = (tuple(v for lf in leaves for v in lf), tuple(leaves[2][:G.nc]))
        old = _combine(evals, x, alpha, points, opened)
        if old is None:
            return (4, q, -1)
        xi = x_index
        for l, ab in enumerate(G.arity_bits):
            ev, path = rnd["steps"][l]
            within, coset = xi & ((1 << ab) - 1), xi >> ab
            if tuple(ev[within]) != old:
                return (8, q, l)
            if not path_ok([v for e in ev for v in e], coset, path, pf["commit_caps"][l]):
                return (9, q, l)
            old = _fold(x, within, ab, tuple(tuple(e) for e in ev), betas[l])
            x, xi = pow(x, 1 << ab, P), coset
        if _final(final, x) != old:
            return (10, q, -1)
    return OK


_CAP_FIELDS = {1: "wires_cap", 2: "zs_pp_cap", 3: "quotient_cap"}


def patched(pf, label, v):
    """parsed proof `pf` with the word `label` set to v; only what lies on the way to the word is copied (parsing two thousand
    proofs that differ in one word costs more than verifying them). The tests hold it against parse_proof on a sample."""
    kind = label[0]

    def put(seq, path):
        seq = list(seq)
        seq[path[0]] = v if len(path) == 1 else put(seq[path[0]], path[1:])
        return seq
    p = dict(pf)
    if kind == "cap":
        p[_CAP_FIELDS[label[1]]] = put(pf[_CAP_FIELDS[label[1]]], label[2:])
    elif kind == "open":
        p["openings"] = dict(pf["openings"])
        p["openings"][label[1]] = put(pf["openings"][label[1]], label[2:])
    elif kind == "fcap":
        p["commit_caps"] = put(pf["commit_caps"], label[1:])
    elif kind in ROUND_KINDS:
        q = label[1]
        rnd = dict(pf["queries"][q])
        if kind in ("leaf", "salt", "sib"):
            b = label[2]
            leaf, sib = rnd["initial"][b]
            if kind == "sib":
                sib = put(sib, label[3:])
            else:
                j = label[3] if kind == "leaf" else len(leaf) - SALT + label[3]
                leaf = put(leaf, (j,))
            rnd["initial"] = list(rnd["initial"])
            rnd["initial"][b] = (leaf, sib)
        else:
            l = label[2]
            ev, path = rnd["steps"][l]
            if kind == "eval":
                ev = put(ev, label[3:])
            else:
                path = put(path, label[3:])
            rnd["steps"] = list(rnd["steps"])
            rnd["steps"][l] = (ev, path)
        p["queries"] = list(pf["queries"])
        p["queries"][q] = rnd
    elif kind == "final":
        p["final_poly"] = put(pf["final_poly"], label[1:])
    elif kind == "pow":
        p["pow_witness"] = v
    elif kind == "pi":
        p["public_inputs"] = put(pf["public_inputs"], label[1:])
    else:
        raise AssertionError(label)
    return p


def reference_verdict(pf, words, labels, changes, sh, alpha, zeta, betas, indices, cs_cap=None):
    """the verdict of proof `pf` (its words, their labels) with changes [(word, value)]: the parser's refusals (a length prefix
    that is not the shape's; then an element >= p), then verify_queries"""
    if any(labels[i][0] == "len" and v != words[i] for i, v in changes):
        return MALFORMED
    if any(v >= P and labels[i][0] in FELT_KINDS for i, v in changes):
        return NONCANONICAL
    for i, v in changes:
        pf = patched(pf, labels[i], v)
    return verify_queries(pf, sh, alpha, zeta, betas, indices, cs_cap)


# ---- the transcript ----------------------------------------------------------------------------------------------------------
def replay_challenges(sh, digest, pf):
    """plonky2's transcript of a proof, with the oracle's challenger: dict(zeta, alpha, betas, indices, pow_response)"""
    c = O.challenger_new()
    nc = sh.num_challenges
    ext = lambda: tuple(int(v) for v in O.challenger_challenges(c, 2))
    O.challenger_observe(c, digest)
    O.challenger_observe(c, O.hash_no_pad(np.array(pf["public_inputs"], dtype=np.uint64)))
    O.challenger_observe(c, pf["wires_cap"])
    plonk_betas, plonk_gammas = O.challenger_challenges(c, nc), O.challenger_challenges(c, nc)
    O.challenger_observe(c, pf["zs_pp_cap"])
    plonk_alphas = O.challenger_challenges(c, nc)
    O.challenger_observe(c, pf["quotient_cap"])
    zeta = ext()
    for f in BATCH0 + ["plonk_zs_next"]:
        if pf["openings"][f]:
            O.challenger_observe(c, pf["openings"][f])
    alpha = ext()
    betas = []
    for cap in pf["commit_caps"]:
        O.challenger_observe(c, cap)
        betas.append(ext())
    O.challenger_observe(c, pf["final_poly"])
    O.challenger_observe(c, [pf["pow_witness"]])
    pow_response = int(O.challenger_challenges(c, 1)[0])
    N = 1 << (sh.degree_bits + sh.rate_bits)
    indices = [int(v) % N for v in O.challenger_challenges(c, len(pf["queries"]))]
    return dict(zeta=zeta, alpha=alpha, betas=betas, indices=indices, pow_response=pow_response,
                plonk=(list(plonk_betas), list(plonk_gammas), list(plonk_alphas)))


# ---- the cases both test modules run -----------------------------------------------------------------------------------------
def index_flips(indices, lb):
    """[(name, indices)]: every bit of every query index flipped, and the first index taken past N"""
    out = []
    for q in range(len(indices)):
        for bit in range(lb):
            ix = list(indices)
            ix[q] ^= 1 << bit
            out.append(("index %d bit %d" % (q, bit), ix))
    out.append(("index 0 + N", [indices[0] + (1 << lb)] + list(indices[1:])))
    return out


def word_pairs(words, labels, indices, G, count=300, seed=1):
    """[(i, vi, j, vj)]: `count` pairs of canonical field-element words changed together by + 1 mod p: a third in one round, among
    them a non-own evaluation of layer l with the own evaluation of layer l + 1 wherever the shape has two layers"""
    rng = np.random.default_rng(seed)
    felt = [i for i, lab in enumerate(labels) if lab[0] in FELT_KINDS]
    by_round = {}
    for i, lab in enumerate(labels):
        if lab[0] in ROUND_KINDS:
            by_round.setdefault(lab[1], []).append(i)
    at = {lab: i for i, lab in enumerate(labels)}
    pairs = []
    if len(G.arity_bits) >= 2:
        for q in range(len(indices)):
            own0 = indices[q] & ((1 << G.arity_bits[0]) - 1)
            own1 = (indices[q] >> G.before[1]) & ((1 << G.arity_bits[1]) - 1)
            pairs.append((at[("eval", q, 0, own0 ^ 1, 0)], at[("eval", q, 1, own1, 1)]))
    while len(pairs) < count // 3:
        q = int(rng.integers(0, len(by_round)))
        i, j = (int(v) for v in rng.choice(by_round[q], 2, replace=False))
        pairs.append((i, j))
    while len(pairs) < count:
        i, j = (int(v) for v in rng.choice(felt, 2, replace=False))
        pairs.append((i, j))
    return [(i, (words[i] + 1) % P, j, (words[j] + 1) % P) for i, j in pairs[:count]]


def verdict_key(t):
    """the order in which the verifier meets its checks: a smaller key is an earlier failure"""
    status, q, d = t
    if status in (1, 2):
        return (-1, status, 0)
    if status == 0:
        return (1 << 30, 0, 0)
    pos = {7: d, 4: 100, 8: 101 + 2 * d, 9: 102 + 2 * d, 10: 1000}[status]
    return (q, pos, 0)

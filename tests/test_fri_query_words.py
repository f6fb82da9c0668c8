"""Every 64-bit word of a plonky2 proof against the query phase of csrc/fri_verify.h compiled for the host (tests/verify_hostsim):
the word is changed, and the verdict must be the one tests/fri_query_words.py derives from the word's label, which must also be what
the query phase on Python integers finds. Then every bit of every query index, 300 pairs of words, and the oracle's own verifier.
CPU only; tests/test_gpu_fri_query_words.py runs the same cases through the kernels."""
import ctypes
import functools
import os
import sys
import time

import numpy as np
import pytest

import fri_query_words as F
import oracle_lib as O
import reference_challenges as R
import test_gpu_verify_batch as B
import verify_batch_cases as V
from proof_format import find_leaf_index, parse_proof
from synth_circuit import build

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "city-rollup_amd"))
P = O.P
_u64p = ctypes.POINTER(ctypes.c_uint64)
DIGEST = [4, 3, 2, 1]

SHAPES = dict(B.SHAPES)
# seven rounds: the lanes of a wave are not whole proofs
SHAPES["db5q7"] = lambda: build(db=5, num_routed=16, num_wires=20, chunk=8, rate_bits=3, arity_bits=(2,), num_query_rounds=7, seed=45)
# no FRI layer at all: the combine is held against the final polynomial directly
SHAPES["nolayers"] = lambda: build(db=5, num_routed=16, num_wires=20, chunk=8, rate_bits=3, arity_bits=(), seed=46)

# accepted single-word changes per shape, by kind (index into fri_query_words.ACCEPTED), with the constants / sigmas cap supplied
# and the challenges held fixed: read off the first run, pinned since
_POW_PI = {"pow_witness under the hook": 2, "public input under the hook": 10}
ACCEPTED_COUNTS = {      # (shape, cap supplied): (words, mutations, accepted by kind)
    ("db5", True): (989, 1913, dict(_POW_PI, **{"unreached cap entry": 64})),
    ("db7", True): (1390, 2706, dict(_POW_PI, **{"unreached cap entry": 40})),
    ("depth0", True): (1114, 2154, dict(_POW_PI, **{"unreached cap entry": 480})),
    ("arity32", True): (1233, 2401, dict(_POW_PI, **{"unreached cap entry": 64})),
    ("zk", True): (1142, 2210, dict(_POW_PI, **{"unreached cap entry": 40})),
    ("noop", True): (927, 1789, dict(_POW_PI, **{"unreached cap entry": 32})),
    ("db5q7", True): (1562, 3023, dict(_POW_PI, **{"unreached cap entry": 32})),
    ("nolayers", True): (916, 1776, dict(_POW_PI, **{"unreached cap entry": 24})),
    ("db5", False): (989, 1913, dict(_POW_PI, **{"unreached cap entry": 64, "oracle 0 sibling without a cap": 192})),
}


class Case:
    """one proof of one shape with everything the tests derive from it once"""

    def __init__(self, name, c, proof):
        import cityprover as cp
        self.name, self.c, self.proof = name, c, proof
        self.sh = B.shape_of(cp, c)
        self.words = F.words_of(proof)
        self.labels = F.word_map(proof, salted=bool(c["shape"].zero_knowledge))
        self.pf = parse_proof(proof)
        self.G = F.Geometry(self.sh)
        self.ch = F.replay_challenges(self.sh, DIGEST, self.pf)
        self.args = (self.ch["alpha"], self.ch["zeta"], self.ch["betas"], self.ch["indices"])
        self.cs_cap = O.commit_batch(c["cs_values"], c["shape"].rate_bits, c["shape"].cap_height, want=("cap",))["cap"]
        self.base = np.array(self.words, dtype=np.uint64)
        opens = [i for i, lab in enumerate(self.labels) if lab[0] == "open"]
        self.open_lo, self.open_hi = min(opens), max(opens) + 1
        self._recs = {}

    def cap(self, with_cap):
        return self.cs_cap if with_cap else None

    def record(self, row, indices=None):
        """the challenge record of a proof whose words are `row`: a function of the openings and the challenges"""
        key = (row[self.open_lo:self.open_hi].tobytes(), None if indices is None else tuple(indices))
        if key not in self._recs:
            pf = dict(self.pf)
            if key[0] != self.base[self.open_lo:self.open_hi].tobytes():
                w = row.copy()
                w[:self.open_lo], w[self.open_hi:] = self.base[:self.open_lo], self.base[self.open_hi:]
                pf = parse_proof(w.tobytes())
            a = self.args if indices is None else self.args[:3] + (list(indices),)
            self._recs[key] = V.record(self.sh, pf, *a)
        return self._recs[key]

    def rows(self, changes):
        """an array [case][words] with the given [(word, value), ...] applied per case"""
        W = np.tile(self.base, (len(changes), 1))
        for r, ch in enumerate(changes):
            for i, v in ch:
                W[r, i] = v
        return W

    def reference(self, changes, with_cap=True, indices=None):
        """the Python verifier's verdict of the proof with [(word, value)] applied"""
        a = self.args if indices is None else self.args[:3] + (list(indices),)
        return F.reference_verdict(self.pf, self.words, self.labels, changes, self.sh, *a, cs_cap=self.cap(with_cap))


@functools.lru_cache(maxsize=None)
def case(name):
    c = SHAPES[name]()
    s = c["shape"]
    if s.zero_knowledge:
        proof, dbg = O.prove_full_zk(s, c["gates"], DIGEST, c["public_inputs"], c["cs_values"], c["wires"], c["salts"])
    else:
        proof, dbg = O.prove_full(s, c["gates"], DIGEST, c["public_inputs"], c["cs_values"], c["wires"])
    cs = Case(name, c, proof)
    cs.dbg = dbg
    return cs


@pytest.fixture(scope="module")
def vh():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("verify_hostsim"))
    lib.vh_instance_size.restype = ctypes.c_size_t
    lib.vh_query_phase_many.restype = None
    lib.vh_query_phase_many.argtypes = [ctypes.POINTER(V.Instance), _u64p, ctypes.c_size_t, _u64p, ctypes.c_size_t, _u64p, ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_uint32)]
    assert lib.vh_instance_size() == ctypes.sizeof(V.Instance)
    return lib


def host_build(vh, cs, W, recs, with_cap, cs_cap=None):
    """the verdicts of the header's host build for proofs W[i] with records recs[i]; cs_cap: another cap than the circuit's"""
    D, words = V.layout(cs.sh, check_cs=with_cap)
    assert W.shape[1] == words
    W, recs = np.ascontiguousarray(W, dtype=np.uint64), np.ascontiguousarray(recs, dtype=np.uint64)
    keys = np.zeros(len(W), np.uint32)
    cap = np.ascontiguousarray(cs.cs_cap if cs_cap is None else cs_cap, dtype=np.uint64) if with_cap else None
    vh.vh_query_phase_many(ctypes.byref(D), W.ctypes.data_as(_u64p), words, recs.ctypes.data_as(_u64p), recs.shape[1],
                           None if cap is None else cap.ctypes.data_as(_u64p), len(W), keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return [V.key_triple(D, int(k)) for k in keys]


def hook(cs, row, indices=None):
    """the host verifier with the challenges supplied (no constants / sigmas cap): parser and query phase of verify.inc"""
    import cityprover as cp
    a = cs.args if indices is None else cs.args[:3] + (list(indices),)
    try:
        cp.verify_fri_queries_with_challenges(cs.sh, row.tobytes(), *a)
        return F.OK
    except cp.CityProverError as e:
        return V.message_triple(str(e))


def single_words(cs, with_cap):
    """every mutation of every word: (mutations, the changed proofs as rows, the closed form's verdicts)"""
    muts = F.mutations(cs.words, cs.labels)
    W = cs.rows([[(i, v)] for i, _, v in muts])
    want = [F.closed_form(cs.labels[i], v, cs.ch["indices"], cs.G, with_cap) for i, _, v in muts]
    return muts, W, want


def mismatches(muts, labels, got, want, limit=8):
    bad = [(labels[m[0]], m[1], g, w) for m, g, w in zip(muts, got, want) if g != w]
    return bad[:limit]


# ---- the definition itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_word_map_against_the_instance_table(name):
    """every offset verify_batch_cases.layout names carries the label the walk gives it; every word has exactly one label"""
    cs = case(name)
    D, words = V.layout(cs.sh, check_cs=True)
    lab, G = cs.labels, cs.G
    assert len(lab) == words == len(cs.words) and len(set(lab)) == len(lab)
    nq = cs.sh.num_query_rounds
    for b in (1, 2, 3):
        assert lab[D.cap_off[b]] == ("cap", b, 0, 0) and lab[D.cap_off[b] - 1] == ("len", ("cap", b))
    for l in range(D.n_layers):
        assert lab[D.fcap_off[l]] == ("fcap", l, 0, 0)
        assert D.arity_bits[l] == G.arity_bits[l] and D.layer_depth[l] == G.depth[l]
    assert D.depth0 == G.depth0 and D.n_queries == nq and D.cap_height == G.cap_height
    for q in range(nq):
        r = D.q_base + q * D.q_words
        assert lab[r] == ("len", ("oracles", q))
        for b in range(4):
            assert lab[r + D.leaf_off[b]] == ("leaf", q, b, 0) and lab[r + D.leaf_off[b] - 1] == ("len", ("leaf", q, b))
            assert lab[r + D.leaf_off[b] + D.leaf_len[b] - 1][0] == ("salt" if G.salted and b else "leaf")
            assert lab[r + D.sib_off[b] - 1] == ("len", ("sib", q, b))
            if D.depth0:
                assert lab[r + D.sib_off[b]] == ("sib", q, b, 0, 0) and lab[r + D.sib_off[b] + 4 * D.depth0 - 1] == ("sib", q, b, D.depth0 - 1, 3)
        for l in range(D.n_layers):
            assert lab[r + D.ev_off[l]] == ("eval", q, l, 0, 0)
            assert lab[r + D.ev_off[l] + (2 << D.arity_bits[l]) - 1] == ("eval", q, l, (1 << D.arity_bits[l]) - 1, 1)
            assert lab[r + D.path_off[l] - 1] == ("len", ("path", q, l))
            if D.layer_depth[l]:
                assert lab[r + D.path_off[l]] == ("path", q, l, 0, 0)
                assert lab[r + D.path_off[l] + 4 * D.layer_depth[l] - 1] == ("path", q, l, D.layer_depth[l] - 1, 3)
        assert lab[r + D.q_words - 1][0] in ("sib", "eval", "path", "len")
    assert lab[D.q_base + nq * D.q_words] == ("len", "final")
    assert lab[D.final_off] == ("final", 0, 0) and lab[D.final_off + 2 * D.final_len - 1] == ("final", D.final_len - 1, 1)
    assert lab[D.final_off + 2 * D.final_len] == ("pow",)
    assert lab[-1] == ("pi", cs.sh.num_public_inputs - 1)
    # the ranges of the combine: the unsalted prefix of every leaf, and the Z polynomials again
    got = [(D.r_oracle[i], D.r_first[i], D.r_count[i]) for i in range(D.n_ranges)]
    assert got == [(b, 0, G.k[b]) for b in range(4)] + [(2, 0, G.nc)]
    for b in range(4):
        assert D.leaf_len[b] == G.k[b] + (F.SALT if G.salted and b else 0)


@pytest.mark.parametrize("which", range(10))
def test_python_verifier_accepts_the_reference_proofs(golden_dir, which):
    """the anchor of verify_queries: plonky2's own ten proofs with their recovered challenges; the word map walks them as well"""
    import cityprover as cp
    blob, pf, ch = R.challenges(golden_dir, which)
    sh = cp.standard_recursion_shape(num_public_inputs=len(pf["public_inputs"]))
    args = (ch["alpha"], ch["zeta"], ch["betas"], ch["x_indices"])
    assert F.verify_queries(pf, sh, *args) == F.OK
    lab = F.word_map(blob)
    assert len(set(lab)) == len(lab) == V.layout(sh)[1]
    if which < 2:   # and it names the check the host verifier names on the twelve mutations of the reference proofs
        for name, bad, a in V.reference_mutations(blob, args):
            with pytest.raises(cp.CityProverError) as e:
                cp.verify_fri_queries_with_challenges(sh, bad, *a)
            assert F.verify_queries(parse_proof(bad), sh, *a) == V.message_triple(str(e.value)), name


@pytest.mark.parametrize("name", list(SHAPES))
def test_challenges_of_a_synthetic_proof(name):
    """the transcript replayed in Python gives the prover's zeta, FRI betas and indices; the indices are where the paths lead; and
    with them (and the FRI alpha, which only the replay knows) the Python verifier accepts the proof, with and without the cap"""
    cs = case(name)
    ch, dbg, nl, nq = cs.ch, cs.dbg, cs.sh.n_arity, cs.sh.num_query_rounds
    assert ch["zeta"] == tuple(dbg.zeta)
    assert ch["betas"] == [tuple(dbg.fri_betas[l]) for l in range(nl)]
    assert ch["indices"] == list(dbg.query_indices[:nq])
    assert ch["pow_response"] == dbg.pow_response
    for q, rnd in enumerate(cs.pf["queries"]):
        leaf, sib = rnd["initial"][1]
        assert find_leaf_index(leaf, sib, cs.pf["wires_cap"], O) == ch["indices"][q]
    assert F.verify_queries(cs.pf, cs.sh, *cs.args, cs_cap=cs.cs_cap) == F.OK
    assert F.verify_queries(cs.pf, cs.sh, *cs.args) == F.OK
    assert O.verify_full(cs.c["shape"], cs.c["gates"], DIGEST, cs.cs_cap, cs.proof) == 0


# ---- every word ----------------------------------------------------------------------------------------------------------------
def counts_by_kind(cs, muts, want, with_cap):
    out = {}
    for (i, _, v), w in zip(muts, want):
        if w == F.OK:
            k = F.accepted_kind(cs.labels[i], cs.ch["indices"], cs.G, with_cap, True)
            out[F.ACCEPTED[k][0]] = out.get(F.ACCEPTED[k][0], 0) + 1
    return out


@pytest.mark.parametrize("name,with_cap", [(n, True) for n in SHAPES] + [("db5", False)])
def test_every_word_every_mutation(vh, name, with_cap):
    cs = case(name)
    t0 = time.time()
    muts, W, want = single_words(cs, with_cap)
    ref = [cs.reference([(i, v)], with_cap) for i, _, v in muts]
    assert not mismatches(muts, cs.labels, ref, want), "Python verifier against the closed form"
    parsed = [r for r, w in enumerate(want) if w[0] not in (1, 2)]
    for r in parsed[::7]:       # the proof the Python verifier saw is the proof the bytes hold
        assert F.patched(cs.pf, cs.labels[muts[r][0]], muts[r][2]) == parse_proof(W[r].tobytes())
    assert len(parsed) < len(muts)
    recs = np.stack([cs.record(W[r]) for r in parsed])
    got = host_build(vh, cs, W[parsed], recs, with_cap)
    assert not mismatches([muts[r] for r in parsed], cs.labels, got, [want[r] for r in parsed]), "host build against the closed form"
    # the parser's verdicts are the library's; without a cap the library's host verifier can take every proof
    through_hook = range(len(muts)) if not with_cap else [r for r, w in enumerate(want) if w[0] in (1, 2)]
    hooked = [hook(cs, W[r]) for r in through_hook]
    assert not mismatches([muts[r] for r in through_hook], cs.labels, hooked, [want[r] for r in through_hook]), "host verifier against the closed form"
    # the accepted set, exactly: the host build accepts what the list allows and nothing else
    accepted = {(muts[r][0], muts[r][1]) for r, g in zip(parsed, got) if g == F.OK}
    allowed = {(i, nm) for i, nm, v in muts
               if F.accepted_kind(cs.labels[i], cs.ch["indices"], cs.G, with_cap, True) is not None and not (cs.labels[i][0] in F.FELT_KINDS and v >= P)}
    assert accepted == allowed
    for i, _ in accepted:
        kind = cs.labels[i][0]
        assert kind not in ("open", "final", "len")
        assert kind not in F.ROUND_KINDS or (not with_cap and kind == "sib" and cs.labels[i][2] == 0)
    by_kind = counts_by_kind(cs, muts, want, with_cap)
    print("\n%s cap=%d: %d words, %d mutations, accepted %s, %.1f s" % (name, with_cap, len(cs.words), len(muts), by_kind, time.time() - t0))
    assert (len(cs.words), len(muts), by_kind) == ACCEPTED_COUNTS[(name, with_cap)]


@pytest.mark.parametrize("name", ["db5", "depth0"])
def test_the_shared_cap_argument(vh, name):
    """the call's own constants / sigmas cap changed word by word: oracle 0's path in the first round that reaches the entry"""
    cs = case(name)
    recs = cs.record(cs.base)[None]
    reached = 0
    for e in range(1 << cs.G.cap_height):
        for limb in range(4):
            cap = cs.cs_cap.copy()
            cap[e, limb] = (int(cap[e, limb]) + 1) % P
            want = F.closed_form(("cap", 0, e, limb), int(cap[e, limb]), cs.ch["indices"], cs.G)
            assert host_build(vh, cs, cs.base[None], recs, True, cap) == [want]
            assert F.verify_queries(cs.pf, cs.sh, *cs.args, cs_cap=cap) == want
            reached += want != F.OK
    assert reached and reached % 4 == 0


# ---- query indices -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_cap", [(n, True) for n in SHAPES] + [("db5", False)])
def test_every_bit_of_every_query_index(vh, name, with_cap):
    """an index is a challenge: it is flipped in the record, bits that choose the cap entry included, and one index is taken past N"""
    cs = case(name)
    flips = F.index_flips(cs.ch["indices"], cs.G.lb)
    assert len(flips) == cs.sh.num_query_rounds * cs.G.lb + 1
    want = [cs.reference([], with_cap, ix) for _, ix in flips]
    assert want[-1] == F.OK and all(w != F.OK for w in want[:-1])
    # a flipped index leaves the first checked oracle's path, in its own round, whichever bit it is
    first = 0 if with_cap else 1
    for (nm, ix), w in zip(flips[:-1], want):
        q = [a != b for a, b in zip(ix, cs.ch["indices"])].index(True)
        assert w == (7, q, first), nm
    W = cs.rows([[]] * len(flips))
    recs = np.stack([cs.record(cs.base, ix) for _, ix in flips])
    assert host_build(vh, cs, W, recs, with_cap) == want
    if not with_cap:
        assert [hook(cs, cs.base, ix) for _, ix in flips] == want


# ---- pairs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_pairs_of_words(vh, name):
    """two words changed together: the verdict is the Python verifier's, and where each change alone is refused it is the earlier of
    the two refusals (no change hides another)"""
    cs = case(name)
    pairs = F.word_pairs(cs.words, cs.labels, cs.ch["indices"], cs.G)
    assert len(pairs) == 300
    W = cs.rows([[(i, vi), (j, vj)] for i, vi, j, vj in pairs])
    want = [cs.reference([(i, vi), (j, vj)]) for i, vi, j, vj in pairs]
    same_round = 0
    for (i, vi, j, vj), w in zip(pairs, want):
        si, sj = (F.closed_form(cs.labels[k], v, cs.ch["indices"], cs.G) for k, v in ((i, vi), (j, vj)))
        if si != F.OK and sj != F.OK:
            assert w == min(si, sj, key=F.verdict_key), (cs.labels[i], cs.labels[j])
        a, b = cs.labels[i], cs.labels[j]
        same_round += a[0] in F.ROUND_KINDS and b[0] in F.ROUND_KINDS and a[1] == b[1]
    assert same_round >= 100
    recs = np.stack([cs.record(W[r]) for r in range(len(pairs))])
    assert host_build(vh, cs, W, recs, True) == want


# ---- the oracle's own verifier -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["db5", "zk"])
def test_oracle_verifier_refuses_every_changed_word(name):
    """or_verify_tail replays the transcript, so a changed word outside the query rounds moves every challenge: only the refusal is
    asserted. Nothing is accepted there: an unreached cap entry and the public inputs are absorbed, the proof of work is checked."""
    cs = case(name)
    muts, W, _ = single_words(cs, True)
    for r, (i, nm, v) in enumerate(muts):
        assert O.verify_full(cs.c["shape"], cs.c["gates"], DIGEST, cs.cs_cap, W[r].tobytes()) != 0, (cs.labels[i], nm)

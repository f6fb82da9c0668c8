"""Every 64-bit word of a proof against the kernels of csrc/fri_verify.h: the cases of tests/test_fri_query_words.py through
cp_verify_batch (proofs proved on the device, the transcript replayed by the library) and through
cp_verify_fri_queries_with_challenges_batch (challenges held fixed), each in one or two calls."""
import time

import numpy as np
import pytest

import fri_query_words as F
import oracle_lib as O
import test_gpu_verify_batch as B
import verify_batch_cases as V
from test_fri_query_words import ACCEPTED_COUNTS, DIGEST, SHAPES, Case, counts_by_kind, mismatches, single_words

pytestmark = pytest.mark.gpu
P = O.P
NON_ROUND = ("cap", "open", "fcap", "final", "pow", "pi")


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def cases(prover):
    """per shape, made once: the circuit on the device and one proof of it, proved there"""
    import cityprover as cp
    made = {}

    def get(name):
        if name not in made:
            c = SHAPES[name]()
            circ = B.load(prover, c, DIGEST)
            if c["shape"].zero_knowledge:
                proof = cp.prove_batch_zk(prover, [circ], [c["public_inputs"]], [c["wires"]], [c["salts"]])[0]
            else:
                proof = cp.prove_batch(prover, [circ], [c["public_inputs"]], [c["wires"]])[0]
            cs = Case(name, c, proof)
            assert (circ.cs_cap() == cs.cs_cap).all()
            assert B.host_triple(cp, circ, proof) == F.OK
            made[name] = (cs, circ)
        return made[name]
    yield get
    for _, circ in made.values():
        circ.close()


def with_originals(rows, original, every=50):
    """the slots of a call: an unchanged proof before every `every - 1` changed ones; -> (slots, position of every row)"""
    slots, where = [], []
    for r in rows:
        if len(slots) % every == 0:
            slots.append(original)
        where.append(len(slots))
        slots.append(r)
    return slots, where


@pytest.mark.parametrize("name", list(SHAPES))
def test_verify_batch_every_word(prover, cases, name):
    """cp_verify_batch, the path a caller takes. A changed word of a query round leaves every challenge as it was, so its verdict
    is the closed form's; any other word moves the transcript and is refused as cp_verify refuses it."""
    import cityprover as cp
    cs, circ = cases(name)
    t0 = time.time()
    muts, W, want = single_words(cs, True)     # pow_witness and the public inputs are not of a round: cp_verify speaks for them
    blobs = [W[r].tobytes() for r in range(len(muts))]
    slots, where = with_originals(blobs, cs.proof)
    got = [V.triple(v) for v in cp.verify_batch(circ, slots)]
    originals = sorted(set(range(len(slots))) - set(where))
    assert originals[:2] == [0, 50] and all(got[s] == F.OK for s in originals)
    mine = [got[s] for s in where]
    in_round = [r for r, (i, _, _) in enumerate(muts) if cs.labels[i][0] in F.ROUND_KINDS + ("len",)]
    assert not mismatches([muts[r] for r in in_round], cs.labels, [mine[r] for r in in_round], [want[r] for r in in_round])
    stride = 1 if name == "db5" else 8
    checked = 0
    for r, (i, nm, _) in enumerate(muts):
        outside = cs.labels[i][0] in NON_ROUND
        if outside:
            assert mine[r] != F.OK, (cs.labels[i], nm)
        if outside or where[r] % stride == 0:
            assert mine[r] == B.host_triple(cp, circ, blobs[r]), (cs.labels[i], nm)
            checked += 1
    assert checked >= len(muts) // stride
    if name == "db5":
        assert [V.triple(v) for v in cp.verify_batch(circ, slots, chunk=97)] == got
    print("\n%s: %d slots, %d held against cp_verify, %.1f s" % (name, len(slots), checked, time.time() - t0))


@pytest.mark.parametrize("name,with_cap", [(n, True) for n in SHAPES] + [("db5", False)])
def test_challenges_held_fixed(prover, cases, name, with_cap):
    """cp_verify_fri_queries_with_challenges_batch: every word, every bit of every index and the 300 pairs in one call"""
    import cityprover as cp
    cs, circ = cases(name)
    t0 = time.time()
    muts, W, want = single_words(cs, with_cap)
    flips = F.index_flips(cs.ch["indices"], cs.G.lb)
    pairs = F.word_pairs(cs.words, cs.labels, cs.ch["indices"], cs.G)
    WP = cs.rows([[(i, vi), (j, vj)] for i, vi, j, vj in pairs])
    ref = [cs.reference([(i, v)], with_cap) for i, _, v in muts]
    assert not mismatches(muts, cs.labels, ref, want), "Python verifier against the closed form"
    want = want + [cs.reference([], with_cap, ix) for _, ix in flips] + [cs.reference([(i, vi), (j, vj)], with_cap) for i, vi, j, vj in pairs]
    blobs = [W[r].tobytes() for r in range(len(muts))] + [cs.proof] * len(flips) + [WP[r].tobytes() for r in range(len(pairs))]
    indices = [cs.ch["indices"]] * len(muts) + [ix for _, ix in flips] + [cs.ch["indices"]] * len(pairs)
    n = len(blobs)
    got = cp.verify_fri_queries_with_challenges_batch(prover, cs.sh, blobs, [cs.ch["alpha"]] * n, [cs.ch["zeta"]] * n, [cs.ch["betas"]] * n, indices,
                                                      cs_cap=cs.cap(with_cap))
    got = [V.triple(v) for v in got]
    assert not mismatches(muts, cs.labels, got[:len(muts)], want[:len(muts)]), "kernels against the closed form"
    assert got[len(muts):] == want[len(muts):]
    accepted = {(muts[r][0], muts[r][1]) for r in range(len(muts)) if got[r] == F.OK}
    allowed = {(i, nm) for i, nm, v in muts
               if F.accepted_kind(cs.labels[i], cs.ch["indices"], cs.G, with_cap, True) is not None and not (cs.labels[i][0] in F.FELT_KINDS and v >= P)}
    assert accepted == allowed
    if (name, with_cap) in ACCEPTED_COUNTS:
        assert (len(cs.words), len(muts), counts_by_kind(cs, muts, want, with_cap)) == ACCEPTED_COUNTS[(name, with_cap)]
    print("\n%s cap=%d: %d proofs in one call, %.1f s" % (name, with_cap, n, time.time() - t0))


@pytest.mark.parametrize("name", ["db5", "depth0"])
def test_the_shared_cap_argument(prover, cases, name):
    """the call's own constants / sigmas cap, changed word by word: refused as oracle 0's path in the first round that reaches the
    entry, accepted where none does; the proof next to it with a changed leaf of oracle 0 is refused for that leaf either way"""
    import cityprover as cp
    cs, circ = cases(name)
    leaf = cs.labels.index(("leaf", cs.sh.num_query_rounds - 1, 0, 1))
    bad = cs.rows([[(leaf, (cs.words[leaf] + 1) % P)]])[0].tobytes()
    a = [[v] * 2 for v in cs.args]
    reached = 0
    for e in range(1 << cs.G.cap_height):
        for limb in range(4):
            cap = cs.cs_cap.copy()
            cap[e, limb] = (int(cap[e, limb]) + 1) % P
            got = cp.verify_fri_queries_with_challenges_batch(prover, cs.sh, [cs.proof, bad], *a, cs_cap=cap)
            want = F.closed_form(("cap", 0, e, limb), int(cap[e, limb]), cs.ch["indices"], cs.G)
            assert V.triple(got[0]) == want, (e, limb)
            assert V.triple(got[1]) == min(want, (7, cs.sh.num_query_rounds - 1, 0), key=F.verdict_key)
            reached += want != F.OK
    assert reached and reached % 4 == 0

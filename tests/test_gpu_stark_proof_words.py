"""Every 64-bit word of one STARK proof against cp_stark_verify_batch (tests/stark_proof_words.py has the layout and the changes): each
word to (v + 1) mod p, each field element also to a value >= p, each length prefix to v + 1. All changed copies go through ONE call
per path form, and every verdict must be the class of cp_stark_verify's answer on the same bytes. No changed proof may be accepted,
except where a changed proof-of-work witness happens to be a valid one - there cp_stark_verify decides."""
import pytest

import air_programs as A
import oracle_lib as O
import stark_proof_words as W
from test_gpu_stark_verify_batch import FORMS, batch, close, toy_descs

pytestmark = pytest.mark.gpu
PREFIX = [1, 2, 3]


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def test_every_word_of_a_toy_proof(prover):
    import cityprover
    db, nq = 4, 3
    gd, od, keep, gp, shape = toy_descs(prover, db, nq=nq, pow_bits=5, arity=(2,))
    try:
        proof = cityprover.stark_prove(prover, gd, A.lookup_trace(1 << db), W.challenger(PREFIX))
        oc = O.challenger_new()
        O.challenger_observe(oc, PREFIX)
        assert proof == O.stark_prove(od, A.lookup_trace(1 << db), oc)
        labels = W.layout(*shape)
        words = W.words_of(proof)
        assert len(words) == len(labels) == W.TOY_WORDS
        ok, ch_ok = W.host_verdict(gd, PREFIX, proof)
        assert ok == W.OK and ch_ok == O.challenger_tuple(oc)
        muts = W.single_word_changes(words, labels)
        assert len(muts) == 2 * W.TOY_WORDS - sum(l[0] == "len" for l in labels)
        blobs = [W.with_words(proof, [(i, v)]) for i, _, v in muts]
        want = [W.host_verdict(gd, PREFIX, b) for b in blobs]
        # the host verifier on its own: a value >= p is that and nothing else, a length prefix is malformed (or, before the FriProof,
        # whatever fails first in a proof read with the right lengths - there is none: every prefix is compared), nothing is accepted
        lucky = 0
        for (i, name, v), (verdict, _) in zip(muts, want):
            if labels[i] == ("pow",):
                assert verdict[0] in (0, 6) and (name != ">=p" or verdict[0] == 6)
                lucky += verdict == W.OK
            else:
                assert verdict != W.OK, (labels[i], name)
                if name == ">=p":
                    assert verdict == (2, -1, -1), (labels[i], verdict)
                if name == "len+1":
                    assert verdict == (1, -1, -1), (labels[i], verdict)
        assert lucky <= 1   # one changed witness; 5 bits of work make it valid with probability 1 / 32
        slots = [proof] + blobs + [proof]
        prefixes = [PREFIX] * len(slots)
        for form in FORMS:
            got, after, before = batch(prover, gd, slots, prefixes, form)
            assert got[0] == W.OK and got[-1] == W.OK and after[0] == ch_ok and after[-1] == ch_ok
            bad = [(labels[i], name, g, w) for (i, name, _), g, (w, _) in zip(muts, got[1:-1], want) if g != w]
            assert not bad, (form, len(bad), bad[:5])
            for k, (w, ch) in enumerate(want):
                assert after[1 + k] == (ch if w == W.OK else before[1 + k]), (form, k)
        # every status the device can give was seen: oracle paths, layer values, layer paths, the final polynomial
        assert {7, 8, 9}.issubset({w[0] for w, _ in want})
    finally:
        close(gp)

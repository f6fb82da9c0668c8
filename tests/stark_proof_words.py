"""The words of a STARK proof (cp_stark_prove's bytes, include/cityprover.h) for the tests of cp_stark_verify_batch: where every 64-bit
word lies and what it is, the changes the word-by-word test applies, and cp_stark_verify's answer on given bytes as the verdict
cp_stark_verify_batch must give. Test infrastructure only.

The toy proof of tests/test_gpu_stark_proof_words.py (the lookup AIR of air_programs.py, 2^4 rows, rate 2, cap height 2, 3 query
rounds, 5-bit proof of work, one arity-4 layer; 7 + 15 trace columns, 4 quotient chunks) has TOY_WORDS = 432 words: 1 + 3 x 17 for the
caps, 3 + 2 x 44 + 8 for the openings, and a FriProof of 1 + 17 + 1, 3 query rounds of 84 (leaves of 7, 15 and 4 elements under paths of
3 siblings, 8 layer values under 1 sibling), 1 + 8 for the final polynomial and the proof-of-work witness."""
import re

P = 0xFFFFFFFF00000001
OK = (0, -1, -1)
TOY_WORDS = 432

# cp_stark_verify's messages -> cp_verify_verdict, written from csrc/stark.inc (stark_verify_front), csrc/fri_prove.inc (cp_fri_verify)
# and csrc/verify.inc (parse_fri_proof, fri_challenges, verify_fri_queries); first match wins
MESSAGES = (
    (r"malformed STARK proof", lambda m: (1, -1, -1)),
    (r"malformed proof", lambda m: (1, -1, -1)),
    (r"a field element of the proof is not canonical", lambda m: (2, -1, -1)),
    (r"zeta lies in the trace domain", lambda m: (4, -1, -1)),
    (r"quotient identity fails at zeta for challenge (\d+)", lambda m: (5, -1, int(m.group(1)))),
    (r"proof-of-work witness is not canonical", lambda m: (6, -1, -1)),
    (r"proof of work: response has fewer than", lambda m: (6, -1, -1)),
    (r"query (\d+): Merkle path of oracle (\d+)", lambda m: (7, int(m.group(1)), int(m.group(2)))),
    (r"query (\d+): opening point \d+ lies on the LDE coset", lambda m: (4, int(m.group(1)), -1)),
    (r"query (\d+): FRI layer (\d+) value mismatch", lambda m: (8, int(m.group(1)), int(m.group(2)))),
    (r"query (\d+): Merkle path of FRI layer (\d+)", lambda m: (9, int(m.group(1)), int(m.group(2)))),
    (r"query (\d+): final polynomial mismatch", lambda m: (10, int(m.group(1)), -1)),
)


def challenger(prefix=()):
    import cityprover
    c = cityprover.ChallengerState()
    if len(prefix):
        c.observe(prefix)
    return c


def host_verdict(gd, prefix, proof, publics=None, globals_=None):
    """cp_stark_verify on these bytes -> ((status, query, detail), the outgoing challenger as a tuple - the incoming one when refused)"""
    import cityprover
    c = challenger(prefix)
    before = c.as_tuple()
    try:
        cityprover.stark_verify(gd, c, proof, publics=publics, globals_=globals_)
    except cityprover.CityProverError as e:
        assert c.as_tuple() == before, "cp_stark_verify moved the challenger of a proof it refused"
        msg = str(e)
        assert msg.startswith("[-7]"), msg    # CP_ERR_VERIFY: anything else is a call that could not run
        for pat, f in MESSAGES:
            m = re.search(pat, msg)
            if m:
                return f(m), before
        raise AssertionError("no status for: " + msg)
    return OK, c.as_tuple()


def layout(db, rb, ch, nq, arity, k0, k1, kq):
    """one label per word of a proof of this shape. ("len", what) is a length prefix; the others are field elements:
    ("cap", oracle, i), ("open", set, i), ("fcap", layer, i), ("leaf", query, oracle, i), ("sib", query, oracle, i), ("eval", query,
    layer, i), ("lsib", query, layer, i), ("final", i); ("pow",) is the proof-of-work witness."""
    n_tr = 2 if k1 else 1
    n_or = n_tr + 1
    kt = k0 + k1
    cap_w = 4 << ch
    lab = [("len", "trace_caps")]
    for o in range(n_or):
        lab.append(("len", "cap"))
        lab += [("cap", o, i) for i in range(cap_w)]
    for s, k in enumerate((kt, kt, kq)):
        lab.append(("len", "open"))
        lab += [("open", s, i) for i in range(2 * k)]
    lab.append(("len", "layers"))
    for l in range(len(arity)):
        lab.append(("len", "fcap"))
        lab += [("fcap", l, i) for i in range(cap_w)]
    lab.append(("len", "queries"))
    leaf = (k0, k1, kq) if k1 else (k0, kq)
    lb = db + rb
    for q in range(nq):
        lab.append(("len", "oracles"))
        for o in range(n_or):
            lab.append(("len", "leaf"))
            lab += [("leaf", q, o, i) for i in range(leaf[o])]
            lab.append(("len", "path"))
            lab += [("sib", q, o, i) for i in range(4 * (lb - ch))]
        lab.append(("len", "steps"))
        bits = lb
        for l, ab in enumerate(arity):
            bits -= ab
            lab.append(("len", "evals"))
            lab += [("eval", q, l, i) for i in range(2 << ab)]
            lab.append(("len", "path"))
            lab += [("lsib", q, l, i) for i in range(4 * max(bits - ch, 0))]
    lab.append(("len", "final"))
    lab += [("final", i) for i in range(2 * ((1 << db) >> sum(arity)))]
    lab.append(("pow",))
    return lab


def words_of(proof):
    import numpy as np
    assert len(proof) % 8 == 0
    return np.frombuffer(proof, dtype="<u8").copy()


def with_words(proof, changes):
    """the proof with words[i] = v for (i, v) in changes"""
    w = words_of(proof)
    for i, v in changes:
        w[i] = v
    return w.tobytes()


def single_word_changes(words, labels):
    """[(word, name, value)]: every word to (v + 1) mod p (a length prefix: to v + 1), every field element and the proof-of-work
    witness also to a value >= p"""
    out = []
    for i, (v, lab) in enumerate(zip(words, labels)):
        v = int(v)
        if lab[0] == "len":
            out.append((i, "len+1", v + 1))
        else:
            out.append((i, "+1", (v + 1) % P))
            out.append((i, ">=p", P + (v % (2**64 - P))))
    return out

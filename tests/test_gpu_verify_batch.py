"""cp_verify_batch and cp_verify_fri_queries_with_challenges_batch (the query phase of plonky2 verification on the device,
csrc/fri_verify.h) against cp_verify, the host audit hook, the oracle's verifier and plonky2's own ten proofs."""
import numpy as np
import pytest

import oracle_lib as O
import reference_challenges as R
import verify_batch_cases as V
from proof_format import parse_proof, serialize_proof
from synth_circuit import build

pytestmark = pytest.mark.gpu
P = O.P
DEVMEM = 3   # CP_FAULT_DEVMEM
OK = (0, -1, -1)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def shape_of(cp, c):
    s = c["shape"]
    return cp.standard_recursion_shape(degree_bits=s.degree_bits, num_constants=s.num_constants, num_routed_wires=s.num_routed_wires,
                                       num_wires=s.num_wires, num_challenges=s.num_challenges, num_partial_products=s.num_partial_products,
                                       quotient_degree_factor=s.quotient_degree_factor, rate_bits=s.rate_bits, cap_height=s.cap_height,
                                       pow_bits=s.pow_bits, num_query_rounds=s.num_query_rounds,
                                       arity_bits=tuple(s.arity_bits[i] for i in range(s.n_arity)), zero_knowledge=s.zero_knowledge,
                                       num_public_inputs=len(c["public_inputs"]))


def load(prover, c, digest):
    import cityprover as cp
    circ = cp.Circuit(prover, shape_of(cp, c), digest, c["cs_values"])
    cp.set_gates(circ, c["gate_list"], 1)
    return circ


def rewitness(c, seed):
    """another witness and other public inputs of the same circuit: the public-input row takes the new hash, and the wires no gate
    and no copy constraint reads (the unrouted ones) are drawn again"""
    rng = np.random.default_rng(seed)
    w = c["wires"].copy()
    pi = [int(x) for x in rng.integers(0, P, len(c["public_inputs"]), dtype=np.uint64)]
    h = O.hash_no_pad(np.array(pi, dtype=np.uint64))
    row = c["gate_of_row"].index(2)
    for j in range(4):
        w[j, row] = h[j]
    nr = c["shape"].num_routed_wires
    w[nr:] = rng.integers(0, P, w[nr:].shape, dtype=np.uint64)
    return w, pi


def host_triple(cp, circ, blob):
    try:
        cp.verify(circ, blob)
        return OK
    except cp.CityProverError as e:
        return V.message_triple(str(e))


def mutate(proof, f):
    d = parse_proof(proof)
    f(d)
    return serialize_proof(d)


def bad_slots(cp, prover, c, circ, other, proof, salts):
    """the refused proofs every batch carries: [(name, bytes)]"""
    muts = {
        "public input": lambda d: d["public_inputs"].__setitem__(0, (d["public_inputs"][0] + 1) % P),
        "opening": lambda d: d["openings"]["wires"][2].__setitem__(0, (d["openings"]["wires"][2][0] + 1) % P),
        "quotient opening": lambda d: d["openings"]["quotient_polys"][1].__setitem__(1, 7),
        "final poly": lambda d: d["final_poly"][0].__setitem__(0, (d["final_poly"][0][0] + 1) % P),
        "pow": lambda d: d.__setitem__("pow_witness", d["pow_witness"] + 1),
        "leaf value": lambda d: d["queries"][1]["initial"][1][0].__setitem__(3, 9),
        "sibling": lambda d: d["queries"][0]["initial"][2][1][0].__setitem__(0, 1),
        "fri step": lambda d: d["queries"][2]["steps"][0][0][1].__setitem__(0, 3),
        "cap": lambda d: d["wires_cap"][0].__setitem__(0, 5),
        # an element >= p of each of the eight kinds
        "p opening": lambda d: d["openings"]["wires"][1].__setitem__(1, P + 3),
        "p cap": lambda d: d["quotient_cap"][0].__setitem__(2, P),
        "p fri cap": lambda d: d["commit_caps"][0][0].__setitem__(0, 2**64 - 1),
        "p leaf": lambda d: d["queries"][0]["initial"][1][0].__setitem__(0, P + 1),
        "p sibling": lambda d: d["queries"][1]["initial"][0][1][0].__setitem__(3, P + 9),
        "p fri eval": lambda d: d["queries"][0]["steps"][0][0][0].__setitem__(1, P + 2),
        "p final poly": lambda d: d["final_poly"][0].__setitem__(0, P + 7),
        "p public input": lambda d: d["public_inputs"].__setitem__(0, P + 1),
        "extra public input": lambda d: d["public_inputs"].append(0),
    }
    out = [(name, mutate(proof, m)) for name, m in muts.items()]
    w = c["wires"].copy()                        # a violated gate: proves, and the vanishing identity refuses it
    row = c["gate_of_row"].index(3)
    w[3, row] = (int(w[3, row]) + 1) % P
    if salts is None:
        out.append(("violated gate", cp.prove_batch(prover, [circ], [c["public_inputs"]], [w])[0]))
    else:
        out.append(("violated gate", cp.prove_batch_zk(prover, [circ], [c["public_inputs"]], [w], [salts])[0]))
    if salts is None:
        out.append(("other digest", cp.prove_batch(prover, [other], [c["public_inputs"]], [c["wires"]])[0]))
    else:
        out.append(("other digest", cp.prove_batch_zk(prover, [other], [c["public_inputs"]], [c["wires"]], [salts])[0]))
    out += [("truncated", proof[:-8]), ("trailing", proof + b"\0" * 8), ("empty", b"")]
    return out


def noop_z_leaf():
    """one challenge: the Z oracle's leaf is 1 + num_partial_products = 2 elements, its own digest (hash_or_noop). synth_circuit.build
    cannot make num_challenges x quotient_degree_factor <= 4 verify (its gates need degree 8), so the noop path of an oracle is this one."""
    return build(db=5, num_routed=16, num_wires=20, chunk=8, nc=1, rate_bits=3, arity_bits=(2,), seed=31)


def zk():
    from test_oracle_full import zk_case
    return zk_case(seed=77, db=5)


SHAPES = {
    "db5": lambda: build(db=5, num_routed=16, num_wires=20, chunk=8, rate_bits=3, arity_bits=(2,), seed=45),
    "db7": lambda: build(db=7, num_routed=24, num_wires=30, chunk=8, rate_bits=3, arity_bits=(2, 2), seed=47),
    # the last layer's tree has as many leaves as the cap has entries: depth 0 (a circuit whose cap is higher still does not load)
    "depth0": lambda: build(db=5, num_routed=16, num_wires=20, chunk=8, rate_bits=3, arity_bits=(2, 2), cap_height=4, seed=48),
    "arity32": lambda: build(db=6, num_routed=16, num_wires=20, chunk=8, rate_bits=3, arity_bits=(5,), seed=49),
    "zk": zk,
    "noop": noop_z_leaf,
}


@pytest.fixture(scope="module")
def batches(prover):
    """per shape, made once: the circuit, 67 proofs of distinct witnesses and public inputs, the refused slots, and for every slot the
    verdict cp_verify names"""
    import cityprover as cp
    made = {}

    def get(name):
        if name in made:
            return made[name]
        c = SHAPES[name]()
        digest = [4, 3, 2, 1]
        circ, other = load(prover, c, digest), load(prover, c, [9, 9, 9, 9])
        wit = [rewitness(c, 1000 + i) for i in range(67)]
        salts = None
        if c["shape"].zero_knowledge:
            rng = np.random.default_rng(5)
            salts = [rng.integers(0, P, c["salts"].shape, dtype=np.uint64) for _ in wit]
            good = cp.prove_batch_zk(prover, [circ] * 67, [w[1] for w in wit], [w[0] for w in wit], salts)
        else:
            good = cp.prove_batch(prover, [circ] * 67, [w[1] for w in wit], [w[0] for w in wit])
        assert len(set(good)) == 67
        c0 = dict(c, wires=wit[0][0], public_inputs=wit[0][1])
        bad = bad_slots(cp, prover, c0, circ, other, good[0], None if salts is None else salts[0])
        assert len(bad) == 23
        expect = {blob: host_triple(cp, circ, blob) for blob in good + [b for _, b in bad]}
        assert all(expect[g] == OK for g in good)
        for nm, b in bad:
            assert expect[b] != OK, nm
            if nm != "extra public input":   # the oracle's shape does not carry the count: [a.., 0] hashes like [a..] there
                assert O.verify_full(c["shape"], c["gates"], digest, circ.cs_cap(), b) != 0, nm
        assert O.verify_full(c["shape"], c["gates"], digest, circ.cs_cap(), good[3]) == 0
        made[name] = dict(c=c, circ=circ, good=good, bad=bad, expect=expect)
        return made[name]
    yield get
    for m in made.values():
        m["circ"].close()


def interleave(good, bad):
    """the refused slots spread among the accepted ones, so that a refused proof has accepted neighbours in its wave"""
    out, step = [], max(1, len(good) // (len(bad) + 1))
    g, b = list(good), list(bad)
    while g or b:
        out += g[:step]
        g = g[step:]
        if b:
            out.append(b.pop(0))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_verify_batch_equals_cp_verify(prover, batches, name):
    import cityprover as cp
    m = batches(name)
    names = {b: nm for nm, b in m["bad"]}
    statuses = set()
    for n_good in (1, 5, 67):
        slots = interleave(m["good"][:n_good], [b for _, b in m["bad"]])
        assert len(slots) == n_good + 23
        got = cp.verify_batch(m["circ"], slots)
        for i, blob in enumerate(slots):
            assert V.triple(got[i]) == m["expect"][blob], (n_good, i, names.get(blob, "good"))
            statuses.add(int(got[i]["status"]))
        assert (got["reserved"] == 0).all()
    assert {0, 1, 2, 3, 5, 7} <= statuses     # 8, 9, 10 and 4 need an untouched transcript: the tests below


def test_layer_path_and_every_query_position(prover, batches):
    """a FRI layer sibling (status 9) and a leaf, both touched in the LAST query round of a proof: the key's query"""
    import cityprover as cp
    m = batches("db7")
    proof = m["good"][1]
    nq = m["c"]["shape"].num_query_rounds
    bad = [mutate(proof, lambda d: d["queries"][nq - 1]["steps"][1][1][0].__setitem__(2, 4)),
           mutate(proof, lambda d: d["queries"][nq - 1]["initial"][3][0].__setitem__(0, 6))]
    slots = [m["good"][0]] + bad + [m["good"][2]]
    got = cp.verify_batch(m["circ"], slots)
    want = [host_triple(cp, m["circ"], b) for b in slots]
    assert [V.triple(v) for v in got] == want
    assert want[1] == (9, nq - 1, 1) and want[2] == (7, nq - 1, 3)


def test_chunking_gives_identical_verdicts(prover, batches):
    import cityprover as cp
    m = batches("db5")
    slots = interleave(m["good"], [b for _, b in m["bad"]])[:67]
    want = [m["expect"][b] for b in slots]
    assert any(t != OK for t in want) and any(t == OK for t in want)
    for chunk in (1, 7, 64, 0):
        prover.profile_begin()
        got = cp.verify_batch(m["circ"], slots, chunk=chunk)
        prof = prover.profile_end()
        assert [V.triple(v) for v in got] == want, chunk
        passes = [slots[i:i + (chunk or 67)] for i in range(0, 67, chunk or 67)]
        on_device = lambda t: t[0] == 0 or t[0] >= 7 or (t[0] == 4 and t[1] >= 0)     # the host phase accepted the proof
        launched = sum(1 for ps in passes if any(on_device(m["expect"][b]) for b in ps))
        assert prof["verify_paths"]["launches"] == launched and prof["verify_arith"]["launches"] == launched, (chunk, prof)


def test_all_malformed_needs_no_launch(prover, batches):
    import cityprover as cp
    m = batches("db5")
    proof = m["good"][0]
    slots = [proof[:-8], b"", proof + b"\0" * 8, proof[:100], b"\1" * 24]
    prover.profile_begin()
    got = cp.verify_batch(m["circ"], slots)
    prof = prover.profile_end()
    assert [V.triple(v) for v in got] == [(1, -1, -1)] * 5
    assert not any(k.startswith("verify_") for k in prof), prof


def test_unaligned_proof_pointers(prover, batches):
    """proof bytes at odd addresses (ctypes hands bytes objects over as they lie): the staging copy aligns them"""
    import ctypes
    import cityprover as cp
    m = batches("db5")
    proofs = m["good"][:3]
    buf = ctypes.create_string_buffer(b"\0" * 3 + b"".join(b"\0" * (1 + 2 * i) + p for i, p in enumerate(proofs)) + b"\0" * 8)
    base = ctypes.addressof(buf)
    ptrs, lens, off = (ctypes.c_char_p * 3)(), (ctypes.c_size_t * 3)(), 3
    for i, p in enumerate(proofs):
        off += 1 + 2 * i
        ptrs[i] = ctypes.cast(base + off, ctypes.c_char_p)
        lens[i] = len(p)
        off += len(p)
    out = np.zeros(3, cp.VERDICT)
    prover._check(prover.lib.cp_verify_batch(m["circ"].handle, ptrs, lens, 3, 0, out.ctypes.data))
    assert [V.triple(v) for v in out] == [OK] * 3


def test_alloc_faults(batches):
    """every device allocation of one cp_verify_batch call refused in turn, as tests/test_gpu_alloc_faults.py does for its entry
    points: out of memory as a status, and the same context then returns the expected verdicts"""
    import cityprover as cp
    lib = cp.load_library()
    m = batches("db5")
    slots = interleave(m["good"][:5], [b for _, b in m["bad"]])
    want = [m["expect"][b] for b in slots]
    refused = 0
    try:
        for j in range(16):
            p = cp.Prover(0)
            circ = load(p, m["c"], [4, 3, 2, 1])
            try:
                cp.batch_pool_trim(p)
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    got = cp.verify_batch(circ, slots)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert str(e).startswith("[-4]") and "memory" in str(e), (j, str(e))
                    refused += 1
                    assert [V.triple(v) for v in cp.verify_batch(circ, slots)] == want, j
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                assert [V.triple(v) for v in got] == want
                break
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                circ.close()
                p.close()
        else:
            pytest.fail("the walk did not end")
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused == 3      # the proofs, the challenge records, the tables and keys


def test_argument_errors_with_a_context(prover, batches):
    import cityprover as cp
    m = batches("db5")
    with pytest.raises(cp.CityProverError, match=r"\[-1\].*no proofs"):
        cp.verify_batch(m["circ"], [])
    bare = cp.Circuit(prover, shape_of(cp, m["c"]), [1, 1, 1, 1], m["c"]["cs_values"])
    with pytest.raises(cp.CityProverError, match=r"\[-1\].*gate set"):
        cp.verify_batch(bare, m["good"][:1])
    bare.close()
    assert V.triple(cp.verify_batch(m["circ"], m["good"][:1])[0]) == OK


# ---- plonky2's own proofs ---------------------------------------------------------------------------------------------
def reference_batches(golden_dir):
    """{public inputs: slots}. The ten reference proofs are of two shapes (eight carry 8 public inputs, two carry 4) and a call takes
    one shape, so they make two calls. The first holds the eight with, between them, the twelve mutated copies of proofs 0 and 1
    (six each) and a zeta that lies on the LDE coset; the second the other two around a proof of the first shape."""
    originals = []
    for which in range(10):
        blob, pf, ch = R.challenges(golden_dir, which)
        originals.append((blob, (ch["alpha"], ch["zeta"], ch["betas"], ch["x_indices"]), len(pf["public_inputs"])))
    n0 = originals[0][2]
    assert originals[1][2] == n0 and originals[2][2] == n0
    muts = V.reference_mutations(originals[0][0], originals[0][1])
    muts1 = V.reference_mutations(originals[1][0], originals[1][1])
    mixed = [muts[i] if i % 2 == 0 else muts1[i] for i in range(12)]
    groups = {}
    for i, (blob, args, n_pi) in enumerate(originals):
        groups.setdefault(n_pi, []).append(("original %d" % i, blob, args))
    first = []
    for i in range(12):
        if i < len(groups[n0]):
            first.append(groups[n0][i])
        first.append(mixed[i])
    # zeta = the point of query 0: the opening point lies on the LDE coset there (status 4 with its query)
    blob, (alpha, _, betas, xs), _ = originals[2]
    x0 = 7 * pow(V.root(R.LOG_N), R.rev(xs[0], R.LOG_N), P) % P
    first.append(("zeta on the coset", blob, (alpha, (x0, 0), betas, xs)))
    out = {n0: first}
    for n_pi, slots in groups.items():
        if n_pi != n0:
            out[n_pi] = slots[:1] + [("another shape's proof", originals[0][0], originals[0][1])] + slots[1:]
    assert sum(1 for sl in out.values() for nm, _, _ in sl if nm.startswith("original")) == 10
    return out


def test_reference_proofs_and_mutations(prover, golden_dir):
    """every verdict equals the host hook's, and the ten originals are accepted. cs_cap = NULL, as the hook has it: the reference
    proofs come without their circuit's constants / sigmas cap."""
    import cityprover as cp
    seen = set()
    for n_pi, slots in reference_batches(golden_dir).items():
        sh = cp.standard_recursion_shape(num_public_inputs=n_pi)
        want = []
        for name, blob, args in slots:
            try:
                cp.verify_fri_queries_with_challenges(sh, blob, *args)
                want.append(OK)
            except cp.CityProverError as e:
                want.append(V.message_triple(str(e)))
        assert [w == OK for w in want] == [nm.startswith("original") for nm, _, _ in slots]
        seen |= {w[0] for w in want}
        for chunk in (0, 5):
            got = cp.verify_fri_queries_with_challenges_batch(prover, sh, [b for _, b, _ in slots], [a[0] for _, _, a in slots], [a[1] for _, _, a in slots],
                                                              [a[2] for _, _, a in slots], [a[3] for _, _, a in slots], cs_cap=None, chunk=chunk)
            assert [V.triple(v) for v in got] == want, (n_pi, chunk)
        if len(slots) > 20:
            assert want[-1] == (4, 0, -1)
    assert {0, 3, 4, 7, 8, 9, 10} <= seen


def test_reference_proofs_with_a_constants_sigmas_cap(prover, golden_dir):
    """the shared cap array of a call (oracle 0): per reference proof, the cap entries its own 28 constants / sigmas paths lead to, climbed with
    the oracle's hash; the proof is accepted under that cap, and a touched sibling of oracle 0 is refused as such"""
    import cityprover as cp
    for which in range(10):
        blob, pf, ch = R.challenges(golden_dir, which)
        sh = cp.standard_recursion_shape(num_public_inputs=len(pf["public_inputs"]))
        cap = np.zeros((16, 4), np.uint64)
        for x, q in zip(ch["x_indices"], pf["queries"]):
            leaf, sib = q["initial"][0]
            cur = O.hash_or_noop(np.array(leaf, np.uint64))
            for lvl, s in enumerate(sib):
                s = np.array(s, np.uint64)
                cur = O.two_to_one(s, cur) if (x >> lvl) & 1 else O.two_to_one(cur, s)
            cap[x >> len(sib)] = cur
        bad = mutate(blob, lambda d: d["queries"][9]["initial"][0][1][3].__setitem__(1, 77))
        args = (ch["alpha"], ch["zeta"], ch["betas"], ch["x_indices"])
        got = cp.verify_fri_queries_with_challenges_batch(prover, sh, [blob, bad, blob], *[[a] * 3 for a in args], cs_cap=cap)
        assert [V.triple(v) for v in got] == [OK, (7, 9, 0), OK], which

"""Every Merkle launch form pinned to the CPU oracle (oracle/cityoracle.c), one forced form per context (cp_ctx_set_option).

The library picks among seven kernels for the tree over column-major leaves (cityprover.hip merkle_cols_batch / merkle_levels):
twelve lanes per leaf or a lane per leaf with 0-3 tree levels fused into the leaf hash, then per level a lane per parent with 0-3
levels fused, twelve lanes per parent, or several levels per cooperative launch. Which one runs depends on the switches below and
on the shape. Every case compares the cap AND every digest (a fused level writes its HBM copy from registers that the next fused
level does not read: a wrong intermediate write leaves the cap intact), and proves from the profile that its form ran: the launch
labels and their counts must equal what `merkle_plan` (the planner restated) predicts. The GPU is touched only inside tests."""
import collections
import os

import numpy as np
import pytest

import fri_instances as F
import oracle_lib as O

pytestmark = pytest.mark.gpu
P = O.P

THREADS = 256          # merkle.h THREADS: a lane-per-node workgroup
COOP_MAX_FUSED = 5     # poseidon_coop.h MAX_FUSED
SALT = 4               # cityprover.SALT_SIZE
DEFAULTS = {"COOP_LEAF_MAX": 8192, "COOP_MAX": 16384, "COOP_FUSE": 5, "MERKLE_FUSE": 1, "MERKLE_LEVEL_FUSE": 0}
LABELS = ("leaf_hash_cols", "leaf_hash_cols_coop", "merkle_level", "merkle_level_fused", "merkle_level_coop", "merkle_levels_coop")

# the switch rows; each names the label that proves its form ran
ROWS = {"coop_leaf": ({}, "leaf_hash_cols_coop")}
for _f in range(4):
    ROWS["lane_leaf_fuse%d" % _f] = ({"COOP_LEAF_MAX": 0, "COOP_MAX": 0, "MERKLE_FUSE": _f}, "leaf_hash_cols")
for _g in range(1, 4):
    ROWS["level_fuse%d" % _g] = ({"COOP_LEAF_MAX": 0, "COOP_MAX": 0, "MERKLE_FUSE": 0, "MERKLE_LEVEL_FUSE": _g}, "merkle_level_fused")
ROWS["coop_level"] = ({"COOP_MAX": 1 << 30, "COOP_FUSE": 0}, "merkle_level_coop")
for _k in range(1, 6):
    ROWS["coop_levels_fused%d" % _k] = ({"COOP_MAX": 1 << 30, "COOP_FUSE": _k}, "merkle_levels_coop")

# switch -> the rows of this module that set it (tests/test_switch_coverage.py: no switch without a test)
FORMS = {name: sorted(r for r, (opts, _) in ROWS.items() if name in opts) for name in DEFAULTS}


def _clip3(v):
    return 0 if v < 0 else 3 if v > 3 else v


def fusable_levels(nodes, cap_n, want):
    if nodes % THREADS:
        return 0
    f = 0
    while f < want and (nodes >> (f + 1)) > cap_n:
        f += 1
    return f


def merkle_plan(n_leaves, leaf_len, n_trees, cap_h, opts, salted=False):
    """launch label -> count of one merkle_cols_batch call (cityprover.hip merkle_cols_batch + merkle_levels, restated)"""
    o = dict(DEFAULTS, **opts)
    cap_n = 1 << cap_h
    got = collections.Counter()
    if n_leaves * n_trees <= o["COOP_LEAF_MAX"] and leaf_len + (SALT if salted else 0) > 4:
        got["leaf_hash_cols_coop"] += 1
        done = 0
    else:
        done = fusable_levels(n_leaves, cap_n, _clip3(o["MERKLE_FUSE"]))
        while done > 0 and (n_leaves >> done) * n_trees < o["COOP_MAX"]:
            done -= 1
        got["leaf_hash_cols"] += 1
    n = n_leaves >> done
    while n > cap_n:
        np_ = n // 2
        if np_ * n_trees <= o["COOP_MAX"] and o["COOP_FUSE"] >= 1:
            while n > cap_n:
                levels = 0
                while levels < o["COOP_FUSE"] and levels < COOP_MAX_FUSED and (n >> levels) > cap_n:
                    levels += 1
                got["merkle_levels_coop"] += 1
                n >>= levels
            break
        fuse = 0 if np_ == cap_n else fusable_levels(np_, cap_n, _clip3(o["MERKLE_LEVEL_FUSE"]))
        while fuse > 0 and (np_ >> fuse) * n_trees < o["COOP_MAX"]:
            fuse -= 1
        if fuse > 0:
            got["merkle_level_fused"] += 1
            n >>= fuse + 1
            continue
        got["merkle_level_coop" if np_ * n_trees <= o["COOP_MAX"] else "merkle_level"] += 1
        n = np_
    return got


def leaf_fuse_eff(n_leaves, n_trees, cap_h, opts):
    o = dict(DEFAULTS, **opts)
    f = fusable_levels(n_leaves, 1 << cap_h, _clip3(o["MERKLE_FUSE"]))
    while f > 0 and (n_leaves >> f) * n_trees < o["COOP_MAX"]:
        f -= 1
    return f


def test_planner_clips_fused_levels_as_documented():
    """the clipping the shapes below are chosen for (CPU only: the restated planner itself)"""
    lane3 = ROWS["lane_leaf_fuse3"][0]
    assert [leaf_fuse_eff(1 << 9, 1, h, lane3) for h in (5, 6, 7, 9)] == [3, 2, 1, 0]
    assert leaf_fuse_eff(1 << 7, 1, 0, lane3) == 0                      # not whole workgroups
    assert merkle_plan(1 << 9, 9, 1, 5, lane3) == {"leaf_hash_cols": 1, "merkle_level": 1}
    assert merkle_plan(1 << 12, 9, 1, 0, {"COOP_MAX": 1 << 30, "COOP_FUSE": 5}) == {"leaf_hash_cols_coop": 1, "merkle_levels_coop": 3}


def measured(prover, fn):
    prover.profile_begin()
    try:
        fn()
    finally:
        prof = prover.profile_end()
    return collections.Counter({k: v["launches"] for k, v in prof.items() if k in LABELS})


def forced(opts):
    import cityprover
    p = cityprover.Prover(0)
    for k, v in opts.items():
        p.set_option(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.lib().or_set_threads(min(16, os.cpu_count() or 1))
    yield
    O.lib().or_set_threads(1)


# (log2 leaves, leaf_len, cap_height): 2^7 is not whole workgroups; 2^9 under three fused levels clips to 3 / 2 / 1 / 0 by the cap
# (cap = all leaves takes the copy path); leaf lengths <= 4 are the leaves that are not hashed
SHAPES = [(7, 5, 0), (7, 1, 3), (9, 9, 5), (9, 4, 6), (9, 8, 7), (9, 5, 9), (12, 135, 0), (12, 1, 4), (12, 4, 0), (14, 9, 4), (14, 5, 0)]
_oracle_cache = {}


def tree_case(log_n, leaf_len, cap_h):
    key = (log_n, leaf_len, cap_h)
    if key not in _oracle_cache:
        cols = O.splitmix64_felts(0x5EED0000 + 1000 * log_n + 10 * leaf_len + cap_h, leaf_len << log_n).reshape(leaf_len, -1)
        _oracle_cache[key] = (cols,) + tuple(O.merkle_tree_cols(cols, cap_h, want_digests=True))
    return _oracle_cache[key]


@pytest.mark.parametrize("row", sorted(ROWS))
def test_merkle_cols_form_matches_oracle_in_every_digest(row):
    opts, label = ROWS[row]
    p = forced(opts)
    ran = 0
    try:
        for log_n, leaf_len, cap_h in SHAPES:
            cols, want_cap, want_dig = tree_case(log_n, leaf_len, cap_h)
            out = {}
            launches = measured(p, lambda: out.update(r=p.merkle_cols(cols, cap_h, want_digests=True)))
            cap, dig = out["r"]
            assert (cap == want_cap).all(), (row, log_n, leaf_len, cap_h)
            if want_dig.shape[0]:
                assert (dig == want_dig).all(), ("digests", row, log_n, leaf_len, cap_h)
            plan = merkle_plan(1 << log_n, leaf_len, 1, cap_h, opts)
            assert launches == plan, (row, log_n, leaf_len, cap_h)
            ran += plan[label] > 0
    finally:
        p.close()
    assert ran >= 3, "the form of row %s ran on %d shapes only" % (row, ran)


# three trees per call (commit_batch_dev): the per-tree stride of every form's writes. (log_n, rate, k, cap_h): leaves = n << rate
BATCH_SHAPES = [(6, 3, 9, 5), (6, 3, 4, 2), (9, 3, 5, 4)]


@pytest.mark.parametrize("row", sorted(ROWS))
def test_commit_batch_form_matches_oracle_per_tree(row):
    opts, label = ROWS[row]
    trees = 3
    p = forced(opts)
    ran = 0
    try:
        for log_n, rate, k, cap_h in BATCH_SHAPES:
            n = 1 << log_n
            N = n << rate
            vals = O.splitmix64_felts(0xBA7C4 + log_n + 16 * k + 256 * cap_h, trees * k * n).reshape(trees * k, n)
            per_tree = 2 * N - (2 << cap_h)
            dv, dl, dd, dcap = p.to_device(vals), p.alloc(trees * k * N), p.alloc(trees * per_tree * 4), p.alloc(trees * (4 << cap_h))
            try:
                launches = measured(p, lambda: p.commit_batch_dev(dv.ptr, k, trees, log_n, rate, cap_h, dl.ptr, dcap.ptr, None, dd.ptr))
                dig = dd.download().reshape(trees, per_tree, 4)
                caps = dcap.download().reshape(trees, 1 << cap_h, 4)
            finally:
                for b in (dv, dl, dd, dcap):
                    b.free()
            for t in range(trees):
                want = O.commit_batch(vals[t * k:(t + 1) * k], rate, cap_h, want=("cap", "digests"))
                assert (caps[t] == want["cap"]).all(), (row, log_n, rate, k, cap_h, t)
                assert (dig[t] == want["digests"]).all(), ("digests", row, log_n, rate, k, cap_h, t)
            plan = merkle_plan(N, k, trees, cap_h, opts)
            assert launches == plan, (row, log_n, rate, k, cap_h)
            ran += plan[label] > 0
    finally:
        p.close()
    assert ran >= 1, "the form of row %s never ran" % row


# salted leaves (k_leaf_hash_cols<true, F>, k_leaf_hash_cols_coop<true>): PolyBatch with salts. (log_n, rate, k, cap_h)
SALTED_SHAPES = [(6, 3, 3, 5), (6, 3, 1, 6), (9, 3, 2, 4)]
SALTED_ROWS = ["coop_leaf", "lane_leaf_fuse0", "lane_leaf_fuse1", "lane_leaf_fuse2", "lane_leaf_fuse3", "level_fuse2", "coop_level"]


@pytest.mark.parametrize("row", SALTED_ROWS)
def test_salted_batch_form_matches_oracle(row):
    import cityprover
    opts, label = ROWS[row]
    p = forced(opts)
    ran = 0
    try:
        for log_n, rate, k, cap_h in SALTED_SHAPES:
            n = 1 << log_n
            N = n << rate
            rng = np.random.default_rng(log_n * 100 + k * 10 + cap_h)
            polys = rng.integers(0, P, (k, n), dtype=np.uint64)
            salts = rng.integers(0, P, (SALT, N), dtype=np.uint64)
            ob = O.Batch(polys, rate, cap_h, salts=salts)
            box = {}
            launches = measured(p, lambda: box.update(b=cityprover.PolyBatch(p, polys, rate, cap_h, salts=salts)))
            gb = box["b"]
            try:
                assert (gb.cap() == ob.cap()).all(), (row, log_n, rate, k, cap_h)
                assert (gb.leaves(0, N) == ob.lde().T).all(), (row, log_n, rate, k, cap_h)   # leaf order, salt included
            finally:
                gb.close()
                ob.close()
            plan = merkle_plan(N, k, 1, cap_h, opts, salted=True)
            assert launches == plan, (row, log_n, rate, k, cap_h)
            ran += plan[label] > 0
    finally:
        p.close()
    assert ran >= 1, "the form of row %s never ran" % row


@pytest.mark.parametrize("row", ["coop_leaf", "lane_leaf_fuse3", "level_fuse3", "coop_level"])
def test_blinded_fri_proof_bytes_under_forced_forms(row):
    """a FRI proof carries Merkle paths of every oracle: blinded (salted) oracles, committed by the forced form"""
    opts, label = ROWS[row]
    spec = F.random_instance(7, degree_bits=7)
    spec["blinding"] = [True] * len(spec["ks"])
    spec["seed"] += 1000 * sorted(ROWS).index(row)   # other data per row: a pooled buffer a row before left cannot pass for a result
    want = F.run_instance(F.OracleBackend(), spec)
    p = forced(opts)
    try:
        out = {}
        launches = measured(p, lambda: out.update(r=F.run_instance(F.GpuBackend(p), spec)))
        got = out["r"]
    finally:
        p.close()
    assert [c.tolist() for c in got["caps"]] == [c.tolist() for c in want["caps"]]
    assert got["proof"] == want["proof"]
    assert launches[label] > 0, (row, dict(launches))

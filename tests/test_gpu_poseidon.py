"""GPU tests of batched Poseidon and the Merkle-tree hashing (mg_poseidon_*, mg_merkle_*) against the pure-Python restatement
of tests/poseidon_ref.py (itself pinned to the reference's BLS12-381 known answer by test_poseidon_host.py), with manta-pay's
four production BN254 parameter sets (tests/golden/manta_parameters)."""
import threading

import numpy as np
import pytest

import merkle_append_ref as A
import poseidon_ref as P
from manta_rs_amd import synth
from test_poseidon_host import POS, bls_kat_params

pytestmark = pytest.mark.gpu

R = P.R_BN254
MODEL = "utxo-accumulator-model.dat"
EDGES = [0, 1, R - 1]


def mont(ints, r=R):
    return synth.to_mont([int(x) for x in ints], r, 4)


def ints(a, r=R):
    return synth.from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4), r)


def rand_ints(n, seed, r=R):
    rng = synth.XorShift(seed)
    return [rng.field(r) for _ in range(n)]


def states_with_edges(t, n, seed):
    """n states of t words: random, with 0, 1 and r - 1 put into every slot of the first states"""
    vals = rand_ints(n * t, seed)
    for s in range(t):
        for e, v in enumerate(EDGES):
            i = s * len(EDGES) + e
            if i < n:
                vals[i * t + s] = v
    return vals


def test_bls12_381_known_answer(gpu):
    """hash.rs:249-258 through mg_poseidon_permute and mg_poseidon_hash (tag 3), parameters built from the JSON"""
    p = bls_kat_params()
    h = gpu.PoseidonHasher(gpu.BLS12_381, 3, 8, 55, p.encode())
    want = [int(x) for x in POS["output"]]
    got = h.permute(mont([3, 1, 2], P.R_BLS381).reshape(1, 3, 4))
    assert ints(got, P.R_BLS381) == want
    d = h.hash(mont([1, 2], P.R_BLS381).reshape(1, 2, 4))
    assert ints(d, P.R_BLS381) == want[:1]


@pytest.mark.parametrize("name", sorted(P.CHECKFILE))
def test_production_hashers_match_the_restatement(gpu, name):
    data, p = P.load(name)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    t = p.t
    tag = mont([p.tag])
    for n in (1, 63, 64, 65, 1000):
        vals = states_with_edges(t, n, seed=n * 7 + t)
        st = mont(vals).reshape(n, t, 4)
        perm = h.permute(st)
        want = [w for i in range(n) for w in p.permute(vals[i * t:(i + 1) * t])]
        assert ints(perm) == want, (name, n)
        # hash = word 0 of permute(tag, inputs), for the whole batch; inputs with edge words in every slot
        inp = mont(states_with_edges(t - 1, n, seed=n * 11 + t)).reshape(n, t - 1, 4)
        dig = h.hash(inp)
        full = np.concatenate([np.broadcast_to(tag.reshape(1, 1, 4), (n, 1, 4)), inp], axis=1)
        assert (dig == h.permute(full)[:, 0]).all(), (name, n)
        assert ints(dig[:5]) == [p.hash(ints(inp[i])) for i in range(min(n, 5))]
        d_in = gpu.DeviceBuffer.from_numpy(inp)
        d_out = h.hash_device(d_in, n)
        assert (d_out.to_numpy(shape=(n, 4)) == dig).all(), (name, n)
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("name", sorted(P.CHECKFILE))
def test_batch_across_a_chunk_boundary(gpu, name):
    """chunk + 3 states: 256 indices checked against the restatement (first, last, both sides of the boundary, seeded
    random); hash = word 0 of permute(tag, inputs) for the whole batch; hash_device = hash"""
    data, p = P.load(name)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    t, chunk = p.t, gpu.POSEIDON_CHUNK
    n = chunk + 3
    rng = np.random.default_rng(t)
    # random canonical elements below r: 4 limbs with the top limb below r's top limb
    st = rng.integers(0, 1 << 63, size=(n, t, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, t, 4), dtype=np.uint64)
    st[..., 3] %= np.uint64(R >> 192)
    st[:3] = mont(states_with_edges(t, 3, seed=t)).reshape(3, t, 4)
    st[chunk - 1] = mont([R - 1] * t).reshape(t, 4)
    st[chunk] = mont([1] * t).reshape(t, 4)
    perm = h.permute(st)
    picks = {0, n - 1, chunk - 2, chunk - 1, chunk, chunk + 1}
    r2 = synth.XorShift(1000 + t)
    while len(picks) < 256:
        picks.add(r2.field(n))
    for i in sorted(picks):
        assert ints(perm[i]) == p.permute(ints(st[i])), (name, i)
    inp = np.ascontiguousarray(st[:, 1:])
    dig = h.hash(inp)
    full = np.concatenate([np.broadcast_to(mont([p.tag]).reshape(1, 1, 4), (n, 1, 4)), inp], axis=1)
    assert (dig == h.permute(full)[:, 0]).all()
    d_in = gpu.DeviceBuffer.from_numpy(inp)
    d_out = h.hash_device(d_in, n)
    assert (d_out.to_numpy(shape=(n, 4)) == dig).all()


def check_tree(gpu, h, p, height, leaves_int, n, idx, r=R):
    ref = P.Tree(p, leaves_int)
    root, paths = gpu.merkle_tree(h, height, mont(leaves_int[:n], r).reshape(n, 4), indices=idx)
    want = ref.root(height, n)
    assert ints(root, r) == [want], (height, n)
    for q, i in enumerate(idx):
        path = ints(paths[q], r)
        assert path == ref.path(height, n, i), (height, n, i)
        assert P.fold(p, leaves_int[i], i, path) == want, (height, n, i)
    return want


def test_trees_of_height_20(gpu):
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    leaves = list(range(1, 4098))
    for n in (0, 1, 2, 3, 5, 1000, 4097):
        idx = sorted({0, n - 1, n // 2, n // 3, max(0, n - 2)}) if n else []
        root = check_tree(gpu, h, p, 20, leaves, n, idx)
        if n == 1:
            assert root == 0x0d1e52ee866bd8b7b874f287ffcfa1a7a9cca3aa64bd1da41ed65f5db6b09082
        if n == 3:
            assert root == 0x2ccab89989b6130f5b9eb16e852b0272194b61a056aa012ffe50d8389691d8da
    d = h.hash(mont([1, 2]).reshape(1, 2, 4))
    assert ints(d) == [0x1744de3ecd28245ea716dbf79cba9ec8fe641e376c1a6eeff74cb8f55afd533f]
    root, _ = gpu.merkle_tree(h, 20, mont(leaves[:4096]).reshape(4096, 4))
    assert ints(root) == [0x1eec8a2100d1e6334e00e33c0888f459d0fd97b27ca9357ce594f748f4573fe0]


@pytest.mark.parametrize("height", [2, 3, 8])
def test_small_trees_up_to_full_capacity(gpu, height):
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    cap = 1 << (height - 1)
    leaves = rand_ints(cap, seed=height)
    for n in range(cap + 1):
        idx = list(range(n)) if height < 8 else sorted({0, n - 1, n // 2, (3 * n) // 4}) if n else []
        check_tree(gpu, h, p, height, leaves, n, idx)


def test_full_capacity_under_the_level_launch(gpu):
    """height 12 at and one below its capacity: level 0 has more than 1 024 nodes, so one level launch runs before the finish
    in LDS, which starts at level 1 with 1 024 nodes, its most"""
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    p = A.Memo(p)  # the two trees share every node over the first 2 046 leaves
    leaves = rand_ints(2048, seed=12)
    for n in (2047, 2048):
        check_tree(gpu, h, p, 12, leaves, n, sorted({0, 1023, 1024, n - 2, n - 1}))


def test_bls12_381_trees_and_forest(gpu):
    """the build on the other field: every tree of height 3 with every path, then the five trees as one forest"""
    r = P.R_BLS381
    p = bls_kat_params()
    h = gpu.PoseidonHasher(gpu.BLS12_381, 3, 8, 55, p.encode())
    leaves = rand_ints(4, seed=3810, r=r)
    want = [check_tree(gpu, h, p, 3, leaves, n, list(range(n)), r=r) for n in range(5)]
    assert want[0] == 0 and len(set(want)) == 5
    off = np.concatenate([[0], np.cumsum(range(5))]).astype(np.uint64)
    roots = gpu.merkle_forest_roots(h, 3, mont([x for n in range(5) for x in leaves[:n]], r).reshape(-1, 4), off)
    assert ints(roots, r) == want


def test_full_tree_of_2_19_leaves(gpu):
    """too large for the restatement: paths are folded to the GPU root in Python, and inner nodes recomputed from returned
    siblings must agree with the next path entry"""
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    H, n = 20, 1 << 19
    rng = np.random.default_rng(19)
    lv = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    lv[:, 3] %= np.uint64(R >> 192)  # canonical Montgomery limbs
    sel = synth.XorShift(1919)
    idx = [0, n - 1] + [sel.field(n) for _ in range(64)]
    root, paths = gpu.merkle_tree(h, H, lv, indices=idx)
    want = ints(root)[0]
    for q, i in enumerate(idx):
        assert P.fold(p, ints(lv[i])[0], i, ints(paths[q])) == want, i
    # inner position (l, j), 1 <= l <= H - 2: leaves a, b under its two children and c under its sibling; then
    # node(l, j) = hash(node(l-1, 2j), node(l-1, 2j+1)) = hash(path(b)[l-1], path(a)[l-1]) must equal path(c)[l]
    trip = []
    for _ in range(1024):
        l = 1 + sel.field(H - 2)
        j = sel.field(n >> l)
        a = (2 * j) << (l - 1)          # under node(l-1, 2j): its path holds node(l-1, 2j+1)
        b = (2 * j + 1) << (l - 1)      # under node(l-1, 2j+1): its path holds node(l-1, 2j)
        c = (j ^ 1) << l                # under node(l, j ^ 1): its path holds node(l, j)
        trip.append((l, a, b, c))
    flat = [x for (_, a, b, c) in trip for x in (a, b, c)]
    _, ps = gpu.merkle_tree(h, H, lv, indices=flat)
    for q, (l, a, b, c) in enumerate(trip):
        pa, pb, pc = ints(ps[3 * q]), ints(ps[3 * q + 1]), ints(ps[3 * q + 2])
        assert p.hash([pb[l - 1], pa[l - 1]]) == pc[l], (l, a)


def test_forests(gpu):
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    rng = synth.XorShift(256)
    counts = []
    for k in range(256):
        u = rng.field(100)
        counts.append(0 if u < 20 else rng.field(5) if u < 75 else rng.field(20) if u < 97 else 20 + rng.field(60))
    counts[7] = 1025  # a tree that takes the level kernel before the top kernel
    assert sum(counts) <= 3000, sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    leaves = rand_ints(int(off[-1]), seed=77)
    roots = gpu.merkle_forest_roots(h, 20, mont(leaves).reshape(-1, 4), off)
    for k in range(256):
        seg = leaves[int(off[k]):int(off[k + 1])]
        assert ints(roots[k]) == [P.Tree(p, seg).root(20, len(seg))], k
    # ~2^20 leaves in 256 uneven trees against one mg_merkle_tree call per tree
    big = [int(x) for x in np.random.default_rng(5).integers(0, 8192, size=256)]
    big[3] = 0
    big[200] = 1 << 14
    off2 = np.concatenate([[0], np.cumsum(big)]).astype(np.uint64)
    n2 = int(off2[-1])
    lv = np.random.default_rng(6).integers(0, 1 << 63, size=(n2, 4), dtype=np.uint64)
    lv[:, 3] %= np.uint64(R >> 192)
    roots2 = gpu.merkle_forest_roots(h, 20, lv, off2)
    for k in range(256):
        r1, _ = gpu.merkle_tree(h, 20, lv[int(off2[k]):int(off2[k + 1])])
        assert (roots2[k] == r1).all(), k


def test_forest_with_two_level_launches(gpu):
    """tree 0 has 2 049 leaves, 1 025 nodes on level 1 and 513 on level 2, so two level launches run before the finish in LDS,
    beside an empty tree, a single leaf, a tree with one level launch of its own and a pair; the roots as a build, then roots
    and states as an append to the empty forest, both against the restatement"""
    data, p = P.load(MODEL)
    h = gpu.PoseidonHasher.decode(gpu.BN254, data)
    H, counts = 20, [2049, 0, 1, 1025, 2]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    leaves = rand_ints(int(off[-1]), seed=2049)
    trees = [P.Tree(p, leaves[int(off[k]):int(off[k + 1])]) for k in range(5)]
    want = [t.root(H, n) for t, n in zip(trees, counts)]
    lv = mont(leaves).reshape(-1, 4)
    assert ints(gpu.merkle_forest_roots(h, H, lv, off)) == want
    roots, state, _, _ = gpu.merkle_forest_append(h, H, gpu.MerkleState.empty(5, H), lv, off)
    assert ints(roots) == want
    assert A.unpack_state(state) == [A.state_of(t, H, n) for t, n in zip(trees, counts)]


def test_concurrent_callers(gpu):
    data, p = P.load(MODEL)
    hashers = {name: gpu.PoseidonHasher.decode(gpu.BN254, P.load(name)[0]) for name in sorted(P.CHECKFILE)}
    h = hashers[MODEL]
    rng = np.random.default_rng(4)
    jobs = []
    for i, name in enumerate(sorted(P.CHECKFILE)):
        t = hashers[name].width
        x = rng.integers(0, 1 << 63, size=(20000 + 1000 * i, t - 1, 4), dtype=np.uint64)
        x[..., 3] %= np.uint64(R >> 192)
        lv = rng.integers(0, 1 << 63, size=(5000 + 777 * i, 4), dtype=np.uint64)
        lv[:, 3] %= np.uint64(R >> 192)
        jobs.append((hashers[name], x, lv, [0, 17, lv.shape[0] - 1]))
    single = [(hh.hash(x), gpu.merkle_tree(h, 20, lv, idx)) for hh, x, lv, idx in jobs]
    got = [None] * len(jobs)
    errs = []

    def work(i):
        try:
            hh, x, lv, idx = jobs[i]
            out = []
            for _ in range(3):
                out.append((hh.hash(x), gpu.merkle_tree(h, 20, lv, idx)))
            got[i] = out
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for i, (d, (root, paths)) in enumerate(single):
        for d2, (root2, paths2) in got[i]:
            assert (d2 == d).all() and (root2 == root).all() and (paths2 == paths).all(), i

"""GPU tests of mg_merkle_forest_append (appending to Merkle trees from their current path, new-leaf paths, refreshed paths)
against tests/poseidon_ref.Tree over the concatenated leaves, with the pure-Python rules of tests/merkle_append_ref.py as a
second oracle; BN254 with the production utxo-accumulator-model hasher unless said."""
import threading

import numpy as np
import pytest

import merkle_append_ref as A
import poseidon_ref as P
from manta_rs_amd import synth
from test_poseidon_host import bls_kat_params

pytestmark = pytest.mark.gpu

R = P.R_BN254
MODEL = "utxo-accumulator-model.dat"
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT


def hasher(gpu):
    data, p = P.load(MODEL)
    return gpu.PoseidonHasher.decode(gpu.BN254, data), A.Memo(p)


def rand_ints(n, seed, r=R):
    rng = synth.XorShift(seed)
    return [rng.field(r) for _ in range(n)]


def every_case(tree, height):
    """every (n_old, b) of the height as a tree of its own over one leaf list: every new leaf's path asked for, every older
    leaf's path refreshed"""
    cap = 1 << (height - 1)
    return [(tree, n_old, b, list(range(n_old, n_old + b)), list(range(n_old)))
            for n_old in range(cap + 1) for b in range(cap - n_old + 1)]


@pytest.mark.parametrize("height", [2, 3, 4])
def test_every_append_of_a_small_height_in_one_forest_call(gpu, height):
    h, p = hasher(gpu)
    cases = every_case(P.Tree(p, rand_ints(1 << (height - 1), seed=40 + height)), height)
    assert len(cases) == {2: 6, 3: 15, 4: 45}[height]
    A.check_forest(gpu, h, height, cases, model=p)


def test_height_20_chained_from_empty(gpu):
    """one tree grown to 4 096 leaves in uneven chunks (the last two take the level kernel before the LDS finish): root and
    state after every step, and the paths of each chunk's first and last leaf refreshed at every later step"""
    h, p = hasher(gpu)
    H = 20
    chunks = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 1025, 1475]
    assert sum(chunks) == 4096
    t = P.Tree(p, range(1, 4097))
    state, n, tracked = gpu.MerkleState.empty(1, H), 0, {}
    for b in chunks:
        new_idx, old = sorted({n, n + b - 1}), sorted(tracked)
        refresh = (old, np.stack([tracked[i] for i in old])) if old else ()
        root, state, paths, ref = gpu.merkle_append(h, H, state, A.mont(t.leaves[n:n + b]), new_idx, refresh)
        n += b
        assert A.ints(root) == [t.root(H, n)], n
        assert A.unpack_state(state) == [A.state_of(t, H, n)], n
        tracked.update(zip(old, ref))
        tracked.update(zip(new_idx, paths))
    assert len(tracked) == 2 * len(chunks) - 2
    want = t.root(H, 4096)
    assert want == 0x1eec8a2100d1e6334e00e33c0888f459d0fd97b27ca9357ce594f748f4573fe0  # as test_trees_of_height_20
    for i, path in tracked.items():
        path = A.ints(path)
        assert path == t.path(H, 4096, i), i
        assert P.fold(p, t.leaves[i], i, path) == want, i


def carry_cases(tree):
    """(n_old, b) around the carries of the count and the seeds they need; prefixes of one leaf list"""
    pairs = [(n_old, b) for n_old in (0, 1, 2, 3, 4, 7, 8, 1023, 1024, 1025, 2047, 2048) for b in (0, 1, 2, 3)]
    for t in range(1, 12):
        pairs += [(1 << t, 1), ((1 << t) - 1, 2)]
    return [(tree, n_old, b, list(range(n_old, n_old + b)), sorted({0, n_old // 2, n_old - 1}) if n_old else [])
            for n_old, b in pairs]


def test_carries_and_seeds_at_height_20(gpu):
    h, p = hasher(gpu)
    t = P.Tree(p, range(1, 2060))
    cases = carry_cases(t)
    assert len(cases) == 48 + 22
    roots, new, _, _ = A.check_forest(gpu, h, 20, cases, model=p)
    state = A.forest_args(gpu, 20, cases)[0]
    for i, (_, n_old, b, _, _) in enumerate(cases):
        if b == 0:  # nothing appended: the state as it was, and the root its fold
            assert new.counts[i] == n_old and (new.last_leaves[i] == state.last_leaves[i]).all(), n_old
            assert (new.current_paths[i] == state.current_paths[i]).all(), n_old
            want = P.fold(p, t.leaves[n_old - 1], n_old - 1, A.ints(state.current_paths[i])) if n_old else 0
            assert A.ints(roots[i]) == [want], n_old


def test_full_capacity_at_height_8(gpu):
    h, p = hasher(gpu)
    t = P.Tree(p, rand_ints(129, seed=8))
    A.check_forest(gpu, h, 8, [(t, 100, 28, [100, 101, 127], [0, 63, 99]), (t, 128, 0, [], [0, 127])], model=p)
    with pytest.raises(gpu.MantaGpuError) as e:
        gpu.merkle_forest_append(h, 8, *A.forest_args(gpu, 8, [(t, 128, 1, [], [])]))
    assert e.value.status == INVALID


def test_forest_of_256_trees_appended_twice(gpu):
    h, p = hasher(gpu)
    H = 20
    rng = synth.XorShift(2560)
    shape = []
    for k in range(256):
        u = rng.field(100)
        n_old = 0 if u < 20 else rng.field(5) if u < 75 else rng.field(20) if u < 97 else 20 + rng.field(21)
        shape.append((n_old, rng.field(13)))
    shape[7] = (37, 1030)  # a tree that takes the level kernel before the LDS finish
    assert sum(n + b for n, b in shape) <= 4500
    vals = rand_ints(sum(n + b + 1 for n, b in shape), seed=78)
    cases, at = [], 0
    for n_old, b in shape:
        t = P.Tree(p, vals[at:at + n_old + b + 1])
        at += n_old + b + 1
        new_idx = [n_old + rng.field(b)] if b and rng.field(3) == 0 else []
        ref_idx = [rng.field(n_old)] if n_old and rng.field(3) == 0 else []
        cases.append((t, n_old, b, new_idx, ref_idx))
    cases[7] = cases[7][:3] + ([37, 600, 1066], [0, 36])
    _, state, _, _ = A.check_forest(gpu, h, H, cases)
    # the returned state is the next call's: one more leaf per tree
    again = [(t, n_old + b, 1, [n_old + b], [0] if n_old + b else []) for t, n_old, b, _, _ in cases]
    args = A.forest_args(gpu, H, again)
    assert (args[0].counts == state.counts).all() and (args[0].last_leaves == state.last_leaves).all()
    assert (args[0].current_paths == state.current_paths).all()
    roots, new, paths, ref = A.check_forest(gpu, h, H, again)
    # new_state = old_state gives the same bytes
    r2, same, p2, f2 = gpu.merkle_forest_append(h, H, state, *args[1:], in_place=True)
    assert same is state
    for x, y in ((roots, r2), (new.counts, state.counts), (new.last_leaves, state.last_leaves),
                 (new.current_paths, state.current_paths), (paths, p2), (ref, f2)):
        assert x.tobytes() == y.tobytes()


def test_agreement_with_merkle_tree_beyond_the_restatement(gpu):
    """64 trees of thousands of random leaves each: states from mg_merkle_tree over the older leaves, then roots and new
    current paths against mg_merkle_tree over all leaves"""
    h, _ = hasher(gpu)
    H = 20
    rng = np.random.default_rng(64)
    n_old = [int(x) for x in rng.integers(0, 8193, size=64)]
    b = [int(x) for x in rng.integers(0, 2049, size=64)]
    n_old[0], b[0], b[1], n_old[2], b[2] = 0, 2048, 0, 8192, 1
    states, new_leaves, trees = [], [], []
    for k in range(64):
        lv = rng.integers(0, 1 << 63, size=(n_old[k] + b[k], 4), dtype=np.uint64)
        lv[:, 3] %= np.uint64(R >> 192)  # canonical Montgomery limbs
        _, path = gpu.merkle_tree(h, H, lv[:n_old[k]], indices=[n_old[k] - 1] if n_old[k] else [])
        states.append(gpu.MerkleState.from_tree(lv[:n_old[k]], path) if n_old[k] else gpu.MerkleState.empty(1, H))
        new_leaves.append(lv[n_old[k]:])
        trees.append(lv)
    off = np.concatenate([[0], np.cumsum(b)]).astype(np.uint64)
    roots, new, _, _ = gpu.merkle_forest_append(h, H, gpu.MerkleState.concat(states), np.concatenate(new_leaves), off)
    for k in range(64):
        n = n_old[k] + b[k]
        root, path = gpu.merkle_tree(h, H, trees[k], indices=[n - 1] if n else [])
        assert (roots[k] == root).all() and new.counts[k] == n, k
        if n:
            assert (new.last_leaves[k] == trees[k][-1]).all() and (new.current_paths[k] == path[0]).all(), k


def test_bls12_381(gpu):
    p = bls_kat_params()
    h = gpu.PoseidonHasher(gpu.BLS12_381, 3, 8, 55, p.encode())
    p = A.Memo(p)
    cases = every_case(P.Tree(p, rand_ints(4, seed=381, r=P.R_BLS381)), 3)
    A.check_forest(gpu, h, 3, cases, r=P.R_BLS381, model=p)


def test_concurrent_appenders(gpu):
    """four threads on one hasher, each repeating the forest call of the carries test"""
    h, p = hasher(gpu)
    args = A.forest_args(gpu, 20, carry_cases(P.Tree(p, range(1, 2060))))
    single = gpu.merkle_forest_append(h, 20, *args)
    got, errs = [None] * 4, []

    def work(i):
        try:
            got[i] = [gpu.merkle_forest_append(h, 20, *args) for _ in range(3)]
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    want = single[0], single[1].counts, single[1].last_leaves, single[1].current_paths, single[2], single[3]
    for outs in got:
        for roots, new, paths, ref in outs:
            for x, y in zip(want, (roots, new.counts, new.last_leaves, new.current_paths, paths, ref)):
                assert x.tobytes() == y.tobytes()

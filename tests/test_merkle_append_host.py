"""CPU tests of mg_merkle_forest_append: every argument check answers MG_ERROR_INVALID_ARGUMENT before any device work, so it
runs without a GPU; and the rules of appending from (count, last leaf, current path) -- restated in pure Python in
tests/merkle_append_ref.py, the GPU tests' second oracle -- give exactly poseidon_ref.Tree over the concatenated leaves."""
import ctypes

import numpy as np
import pytest

import merkle_append_ref as A
import poseidon_ref as P

INVALID = 1  # MG_ERROR_INVALID_ARGUMENT
MODEL = "utxo-accumulator-model.dat"


def rejected(api, *args, **kw):
    with pytest.raises(api.MantaGpuError) as e:
        api.merkle_forest_append(*args, **kw)
    assert e.value.status == INVALID
    return True


def test_append_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    h3 = api.PoseidonHasher.decode(api.BN254, P.load(MODEL)[0])
    h4 = api.PoseidonHasher.decode(api.BN254, P.load("nullifier-commitment-scheme.dat")[0])
    leaves = np.zeros((9, 4), dtype=np.uint64)
    empty = api.MerkleState.empty
    assert rejected(api, h4, 3, empty(1, 3), leaves[:1], [0, 1])  # the tree's inner hash has width 3
    for height in (1, 33):
        assert rejected(api, h3, height, empty(1, height), leaves[:1], [0, 1]), height
    assert rejected(api, h3, 3, empty(1, 3), leaves[:5], [1, 5])  # offsets not from 0
    assert rejected(api, h3, 3, empty(2, 3), leaves[:3], [0, 3, 2])  # decreasing
    assert rejected(api, h3, 3, empty(2, 3), leaves[:9], [0, 5, 9])  # 5 leaves into a tree of 4
    three = api.MerkleState([3], np.zeros((1, 4)), np.zeros((1, 2, 4)))  # height 3 holding 3 of 4: all-zero nodes are a valid path
    assert rejected(api, h3, 3, three, leaves[:2], [0, 2])  # n_old + b over capacity
    assert rejected(api, h3, 3, api.MerkleState([5], np.zeros((1, 4)), np.zeros((1, 2, 4))), leaves[:0], [0, 0])  # n_old itself
    assert rejected(api, h3, 3, api.MerkleState([2 ** 64 - 1], np.zeros((1, 4)), np.zeros((1, 2, 4))), leaves[:2], [0, 2])
    for tree, idx in ((0, 2), (0, 4), (1, 3)):  # a new leaf's path below n_old, at n_new, in a tree that is not there
        assert rejected(api, h3, 3, three, leaves[:1], [0, 1], path_requests=([tree], [idx])), (tree, idx)
    old_path = np.zeros((1, 2, 4), dtype=np.uint64)
    for tree, idx in ((0, 3), (0, 7), (1, 0)):  # a refresh of a leaf that is not older, or of no tree
        assert rejected(api, h3, 3, three, leaves[:1], [0, 1], refresh=([tree], [idx], old_path)), (tree, idx)
    # a current path's entry on a level where the last leaf is a left child is a right sibling: it must be 0
    for n_old, level in ((1, 0), (1, 1), (2, 1), (3, 0)):
        bad = api.MerkleState([n_old], np.zeros((1, 4)), np.zeros((1, 2, 4)))
        for limb in range(4):
            bad.current_paths[:] = 0
            bad.current_paths[0, level, limb] = 1
            assert rejected(api, h3, 3, bad, leaves[:0], [0, 0]), (n_old, level, limb)
    # n_trees = 0 succeeds, and so do empty request lists
    roots, new, paths, ref = api.merkle_forest_append(h3, 20, empty(0, 20), leaves[:0], [0])
    assert roots.shape == (0, 4) and len(new) == 0 and paths.shape == (0, 19, 4) and ref.shape == (0, 19, 4)
    assert rejected(api, h3, 20, empty(0, 20), leaves[:0], [0], path_requests=([0], [0]))  # a request needs a tree


def test_append_null_arrays_with_non_zero_counts():
    from manta_rs_amd import api
    from manta_rs_amd.api import _MerkleStateC, _p, _sz
    h3 = api.PoseidonHasher.decode(api.BN254, P.load(MODEL)[0])
    st = api.MerkleState([1], np.zeros((1, 4)), np.zeros((1, 2, 4)))  # one leaf, so that leaf 1 is new and leaf 0 is older
    new = api.MerkleState.empty(1, 3)
    buf = {name: np.zeros(shape, dtype=np.uint64) for name, shape in
           (("leaves", (1, 4)), ("offsets", (2,)), ("roots", (1, 4)), ("pt", (1,)), ("pi", (1,)), ("paths", (1, 2, 4)),
            ("rt", (1,)), ("ri", (1,)), ("rp", (1, 2, 4)))}
    buf["offsets"][1] = 1

    def call(n_trees=1, old=True, new_=True, k=0, m=0, drop=(), state_drop=None):
        o, n = st._c(), new._c()
        if state_drop:
            setattr(o if state_drop[0] == "old" else n, state_drop[1], None)
        a = {name: (None if name in drop else _p(v)) for name, v in buf.items()}
        return api.LIB.mg_merkle_forest_append(h3._h, ctypes.c_uint(3), _sz(n_trees), ctypes.byref(o) if old else None, a["leaves"],
                                               a["offsets"], a["roots"], ctypes.byref(n) if new_ else None, a["pt"], a["pi"],
                                               _sz(k), a["paths"], a["rt"], a["ri"], _sz(m), a["rp"])

    assert call(old=False) == INVALID and call(new_=False) == INVALID
    for which in ("old", "new"):
        for field, _ in _MerkleStateC._fields_:
            assert call(state_drop=(which, field)) == INVALID, (which, field)
    for name in ("leaves", "offsets", "roots"):
        assert call(drop=(name,)) == INVALID, name
    buf["pi"][0] = 1  # the one new leaf; the refresh is of leaf 0
    for name in ("pt", "pi", "paths"):
        assert call(k=1, drop=(name,)) == INVALID, name
    for name in ("rt", "ri", "rp"):
        assert call(m=1, drop=(name,)) == INVALID, name
    assert not new.counts.any() and not buf["roots"].any()  # a failed call writes nothing
    # with zero counts the arrays may be null
    assert call(n_trees=0, old=False, new_=False, drop=tuple(buf)) == 0


@pytest.mark.parametrize("height", [2, 3, 4])
def test_append_rules_reproduce_the_tree_exhaustively(height):
    """every (n_old, b) of the height: root, new state, the path of every new leaf and the refreshed path of every older leaf
    from the state alone = poseidon_ref.Tree over the concatenated leaves"""
    _, p = P.load(MODEL)
    p = A.Memo(p)
    cap = 1 << (height - 1)
    rng = A.synth.XorShift(height)
    t = P.Tree(p, [rng.field(P.R_BN254) for _ in range(cap)])
    seen = 0
    for n_old in range(cap + 1):
        for b in range(cap - n_old + 1):
            n = n_old + b
            root, state, paths, ref = A.append(p, height, A.state_of(t, height, n_old), t.leaves[n_old:n], range(n_old, n),
                                               [(i, t.path(height, n_old, i)) for i in range(n_old)])
            assert root == t.root(height, n), (n_old, b)
            assert state == A.state_of(t, height, n), (n_old, b)
            assert paths == [t.path(height, n, i) for i in range(n_old, n)], (n_old, b)
            assert ref == [t.path(height, n, i) for i in range(n_old)], (n_old, b)
            for i in range(n):
                assert P.fold(p, t.leaves[i], i, (ref + paths)[i]) == root, (n_old, b, i)
            seen += 1
    assert seen == (cap + 1) * (cap + 2) // 2


def test_append_rules_chained_to_full_capacity_with_a_stand_in_hash():
    """height 12 from empty to 2^11 leaves in 16 uneven steps under a cheap two-to-one hash: every state and root on the way,
    and paths tracked from their insertion and refreshed at every later step"""

    class Toy:
        r = (1 << 61) - 1

        def hash(self, x):
            return (x[0] * 0x9E3779B97F4A7C15 + x[1] * 0xC2B2AE3D27D4EB4F + 0x165667B19E3779F9 + x[0] * x[1]) % self.r + 1

    p, height = Toy(), 12
    steps = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 452]
    assert sum(steps) == 1 << (height - 1) and len(steps) == 16
    t = P.Tree(p, range(1, 2049))
    state, n, tracked = A.state_of(t, height, 0), 0, {}
    for b in steps:
        new_idx = sorted({n, n + b - 1, n + b // 2})
        old = sorted(tracked)
        root, state, paths, ref = A.append(p, height, state, t.leaves[n:n + b], new_idx, [(i, tracked[i]) for i in old])
        n += b
        assert root == t.root(height, n) and state == A.state_of(t, height, n), n
        tracked.update(zip(old, ref))
        tracked.update(zip(new_idx, paths))
        for i, path in tracked.items():
            assert path == t.path(height, n, i), (n, i)
    assert A.append(p, height, state, [])[0] == t.root(height, n)

"""What the tests of mg_merkle_forest_append share (tests/test_merkle_append_host.py, tests/test_gpu_merkle_append.py).

  append        a pure-Python model of appending to a tree that is known only by (count, last leaf, current path): the rules of
                the header, over any two-to-one hash. It never sees an older leaf. Checked exhaustively against
                poseidon_ref.Tree by the host test; the GPU tests use it as a second oracle.
  check_forest  one forest call on the GPU for a list of cases, every output compared with poseidon_ref.Tree over the
                concatenated leaves (root, path), never with the code under test.

Integers are canonical; the arrays that cross the ABI are Montgomery limbs."""
import numpy as np

import poseidon_ref as P
from manta_rs_amd import synth


def mont(vals, r=P.R_BN254):
    return synth.to_mont([int(x) for x in vals], r, 4)


def ints(a, r=P.R_BN254):
    return synth.from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4), r)


class Memo:
    """a Params whose two-to-one hash remembers its answers (the model and Tree then share the work)"""

    def __init__(self, p):
        self.p, self.seen = p, {}

    def hash(self, inputs):
        key = tuple(inputs)
        v = self.seen.get(key)
        if v is None:
            v = self.seen[key] = self.p.hash(list(inputs))
        return v


def state_of(tree, height, n):
    """(count, last leaf, current path) of the tree over the first n leaves; zeros for the empty tree"""
    if n == 0:
        return 0, 0, [0] * (height - 1)
    return n, tree.leaves[n - 1], tree.path(height, n, n - 1)


def ctz(n):
    return (n & -n).bit_length() - 1


def append(p, height, state, new, path_indices=(), refresh=()):
    """state = (n_old, last leaf, current path), new = the appended leaves, refresh = [(index < n_old, its old path)].
    Returns (root, new state, paths of path_indices, refreshed paths)."""
    n_old, last, cur = state
    n_new = n_old + len(new)
    assert n_new <= 1 << (height - 1)
    if n_old:
        assert all(cur[l] == 0 for l in range(height - 1) if not ((n_old - 1) >> l) & 1), "a right sibling in a current path"
    first = [n_old >> l for l in range(height)]                       # s_l
    end = [(n_new + (1 << l) - 1) >> l for l in range(height)]        # one past the level's last node
    levels, seeds = [list(new)], []                                   # levels[l][i] = node(l, s_l + i)
    anc = last                                                        # the last leaf's ancestor on level min(l, ctz(n_old))
    for l in range(height - 1):
        seed = None
        if first[l] & 1:
            seed = cur[l] if n_old % (1 << l) else anc
        seeds.append(seed)
        lv, nxt = levels[l], []
        for j in range(first[l + 1], end[l + 1]):
            c = 2 * j - first[l]                                      # -1: the seed
            left = seed if c < 0 else lv[c]
            right = lv[c + 1] if c + 1 < len(lv) else 0
            nxt.append(p.hash([left, right]))
        levels.append(nxt)
        if n_old and l < ctz(n_old):
            anc = p.hash([cur[l], anc])
    root = 0 if n_new == 0 else levels[-1][0] if levels[-1] else anc

    def sibling(idx, l, keep):
        s = (idx >> l) ^ 1
        if s >= end[l]:
            return 0
        if s >= first[l]:
            return levels[l][s - first[l]]
        return seeds[l] if idx >= n_old else keep

    def path(idx, old=None):
        return [sibling(idx, l, old[l] if old else None) for l in range(height - 1)]

    new_state = (n_new, new[-1], path(n_new - 1)) if new else (n_old, last, list(cur))
    return root, new_state, [path(i) for i in path_indices], [path(i, old) for i, old in refresh]


def pack_state(gpu, states, r=P.R_BN254):
    """[(count, last leaf, path)] -> MerkleState"""
    height = len(states[0][2]) + 1
    flat = [x for _, _, path in states for x in path]
    return gpu.MerkleState([n for n, _, _ in states], mont([last for _, last, _ in states], r),
                           mont(flat, r).reshape(len(states), height - 1, 4))


def unpack_state(st, r=P.R_BN254):
    plen = st.current_paths.shape[1]
    last, flat = ints(st.last_leaves, r), ints(st.current_paths, r)
    return [(int(n), last[i], flat[i * plen:(i + 1) * plen]) for i, n in enumerate(st.counts)]


def forest_args(gpu, height, cases, r=P.R_BN254):
    """cases = [(tree, n_old, b, new leaf indices, older leaf indices)] -> the arguments of merkle_forest_append after the
    hasher and the height: the state and the older leaves' paths are those of poseidon_ref.Tree over the first n_old leaves"""
    state = pack_state(gpu, [state_of(t, height, n_old) for t, n_old, _, _, _ in cases], r)
    leaves = [x for t, n_old, b, _, _ in cases for x in t.leaves[n_old:n_old + b]]
    off = np.concatenate([[0], np.cumsum([b for _, _, b, _, _ in cases])]).astype(np.uint64)
    pt = [i for i, c in enumerate(cases) for _ in c[3]]
    pi = [x for c in cases for x in c[3]]
    rt = [i for i, c in enumerate(cases) for _ in c[4]]
    ri = [x for c in cases for x in c[4]]
    old = [x for t, n_old, _, _, ref in cases for i in ref for x in t.path(height, n_old, i)]
    return (state, mont(leaves, r).reshape(-1, 4), off, (pt, pi) if pt else (),
            (rt, ri, mont(old, r).reshape(len(rt), height - 1, 4)) if rt else ())


def check_forest(gpu, h, height, cases, r=P.R_BN254, model=None):
    """one call for all cases; roots, new states, new paths and refreshed paths against Tree over the n_old + b leaves (and
    against `append` over `model`, a Memo, where given). Returns what the call returned."""
    out = gpu.merkle_forest_append(h, height, *forest_args(gpu, height, cases, r))
    roots, new, paths, refreshed = out
    got_roots, got_state = ints(roots, r), unpack_state(new, r)
    got_paths = ints(paths, r) if paths.size else []
    got_ref = ints(refreshed, r) if refreshed.size else []
    plen, qp, qr = height - 1, 0, 0
    for i, (t, n_old, b, new_idx, ref_idx) in enumerate(cases):
        n = n_old + b
        assert got_roots[i] == t.root(height, n), (i, n_old, b)
        assert got_state[i] == state_of(t, height, n), (i, n_old, b)
        for idx in new_idx:
            assert got_paths[qp * plen:(qp + 1) * plen] == t.path(height, n, idx), (i, n_old, b, idx)
            qp += 1
        for idx in ref_idx:
            assert got_ref[qr * plen:(qr + 1) * plen] == t.path(height, n, idx), (i, n_old, b, idx)
            qr += 1
        if model is not None:
            want = append(model, height, state_of(t, height, n_old), t.leaves[n_old:n],
                          new_idx, [(j, t.path(height, n_old, j)) for j in ref_idx])
            assert want[0] == got_roots[i] and want[1] == got_state[i], (i, n_old, b)
    return out

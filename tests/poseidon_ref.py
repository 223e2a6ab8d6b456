"""A pure-Python restatement of manta-pay's Poseidon and of the hashing inside manta's Merkle trees, for the tests of
mg_poseidon_* / mg_merkle_* (tests/test_poseidon_host.py, tests/test_gpu_poseidon.py). Integers, canonical (not Montgomery).

  permutation  manta-pay/src/crypto/poseidon/mod.rs:383-419, :515-518: round r adds keys[r t + i] to word i, applies x^5 to
               every word (full) or word 0 (partial), then new[i] = sum_j mds[t i + j] st[j]; FULL/2 full, PARTIAL partial,
               FULL/2 full rounds
  hash         hash.rs:111-153: word 0 of the permutation of (domain tag, inputs)
  tree         manta-crypto/src/merkle_tree: level l holds ceil(n / 2^l) nodes, node = hash(left, right) with an absent child
               = 0, a node without leaves = 0; Path = sibling on levels 0 .. H - 2"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_DIR = os.path.join(HERE, "golden", "manta_parameters")
CHECKFILE = json.load(open(os.path.join(PARAM_DIR, "checkfile.json")))
R_BN254 = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
R_BLS381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


class Params:
    def __init__(self, r, width, full, partial, keys, mds, tag):
        self.r, self.t, self.full, self.partial = r, width, full, partial
        self.keys, self.mds, self.tag = keys, mds, tag  # keys[(full + partial) t], mds[t t] row-major

    @classmethod
    def decode(cls, r, data, width, full, partial):
        els = [int.from_bytes(data[32 * i:32 * i + 32], "little") for i in range(len(data) // 32)]
        nk = (full + partial) * width
        assert len(els) == nk + width * width + 1
        return cls(r, width, full, partial, els[:nk], els[nk:nk + width * width], els[-1])

    def encode(self):
        return b"".join(x.to_bytes(32, "little") for x in self.keys + self.mds + [self.tag])

    def permute(self, st):
        r, t = self.r, self.t
        st = [x % r for x in st]
        hf = self.full // 2
        for rnd in range(self.full + self.partial):
            k = self.keys[rnd * t:(rnd + 1) * t]
            st = [(x + y) % r for x, y in zip(st, k)]
            if rnd < hf or rnd >= hf + self.partial:
                st = [pow(x, 5, r) for x in st]
            else:
                st[0] = pow(st[0], 5, r)
            st = [sum(self.mds[t * i + j] * st[j] for j in range(t)) % r for i in range(t)]
        return st

    def hash(self, inputs):
        assert len(inputs) == self.t - 1
        return self.permute([self.tag] + list(inputs))[0]


def load(name, r=R_BN254):
    m = CHECKFILE[name]
    data = open(os.path.join(PARAM_DIR, name), "rb").read()
    return data, Params.decode(r, data, m["width"], m["full_rounds"], m["partial_rounds"])


class Tree:
    """node(l, j) of a tree over `leaves` (the first n of them), memoised on the part of the leaves the node depends on, so
    that trees over growing prefixes of one leaf list cost about height hashes each"""

    def __init__(self, p, leaves):
        self.p, self.leaves, self.memo = p, list(leaves), {}

    def node(self, l, j, n):
        lo = j << l
        if lo >= n:
            return 0
        if l == 0:
            return self.leaves[j]
        m = min(n, (j + 1) << l)  # the node depends on leaves lo .. m - 1 only
        key = (l, j, m)
        v = self.memo.get(key)
        if v is None:
            v = self.p.hash([self.node(l - 1, 2 * j, m), self.node(l - 1, 2 * j + 1, m)])
            self.memo[key] = v
        return v

    def root(self, height, n):
        return self.node(height - 1, 0, n)

    def path(self, height, n, idx):
        return [self.node(l, (idx >> l) ^ 1, n) for l in range(height - 1)]


def fold(p, leaf, idx, path):
    """the root a Path gives: climb from the leaf, hashing with each sibling on the side the index says"""
    cur = leaf
    for l, s in enumerate(path):
        cur = p.hash([s, cur] if (idx >> l) & 1 else [cur, s])
    return cur

"""Appending to the UTXO Merkle forest from its current paths (mg_merkle_forest_append) against the only route there was
before it, mg_merkle_forest_roots over every leaf: one JSON line, also written to profiles/merkle_append_bench.json.

BN254, the production utxo-accumulator-model hasher, height 20, 256 trees, host arrays in and out. A case (N, B) is a forest
that holds N leaves and receives B more, all spread over the shards by mg_merkle_shard_indices. Per case, alternated in this
process:

  append_ms   merkle_forest_append of the B new leaves onto the states of the N old ones
  rebuild_ms  merkle_forest_roots over all N + B leaves
  ratio       rebuild_ms / append_ms

The two routes' roots must be equal before anything is timed. Every figure is the median of --reps calls after one warm-up.

    python tools/merkle_append_bench.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, TREES = 20, 256
CASES = [(1 << 16, 256), (1 << 16, 4096), (1 << 20, 256), (1 << 20, 4096), (1 << 20, 1 << 16)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def rand_mont(rng, n):
    x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    x[:, 3] %= np.uint64(0x30644e72e131a029)  # below r's top limb: canonical
    return x


def by_shard(api, leaves):
    """the leaves grouped by their shard, insertion order kept inside a shard -> (leaves, offsets [TREES + 1])"""
    shards = api.merkle_shard_indices(leaves)
    order = np.argsort(shards, kind="stable")
    counts = np.bincount(shards, minlength=TREES)
    return np.ascontiguousarray(leaves[order]), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api

    api.init(0)
    data = open(os.path.join(ROOT, "tests", "golden", "manta_parameters", "utxo-accumulator-model.dat"), "rb").read()
    h = api.PoseidonHasher.decode(api.BN254, data)
    rng = np.random.default_rng(2027)
    out = {"tool": "merkle_append_bench", "reps": a.reps, "height": HEIGHT, "trees": TREES,
           "hasher": "bn254 Poseidon2 (utxo-accumulator-model.dat, width 3, 8 + 55 rounds)", "cases": []}
    for n_old, b in CASES:
        old, old_off = by_shard(api, rand_mont(rng, n_old))
        new, new_off = by_shard(api, rand_mont(rng, b))
        # the forest before the append, as a ledger or signer holds it: one mg_merkle_tree call per shard, outside the timing
        states = []
        for k in range(TREES):
            seg = old[int(old_off[k]):int(old_off[k + 1])]
            states.append(api.MerkleState.from_tree(seg, api.merkle_tree(h, HEIGHT, seg, [seg.shape[0] - 1])[1])
                          if seg.shape[0] else api.MerkleState.empty(1, HEIGHT))
        state = api.MerkleState.concat(states)
        # all leaves per shard, older first: what the rebuild hashes
        every = np.concatenate([x for k in range(TREES) for x in (old[int(old_off[k]):int(old_off[k + 1])],
                                                                  new[int(new_off[k]):int(new_off[k + 1])])])
        every_off = old_off + new_off

        def append():
            return api.merkle_forest_append(h, HEIGHT, state, new, new_off)[0]

        def rebuild():
            return api.merkle_forest_roots(h, HEIGHT, every, every_off)

        assert (append() == rebuild()).all(), ("roots differ", n_old, b)  # also the warm-up of both
        ta, tr = [], []
        for _ in range(a.reps):
            ta.append(timed(append))
            tr.append(timed(rebuild))
        am, rm = statistics.median(ta), statistics.median(tr)
        out["cases"].append({"held": n_old, "appended": b, "append_ms": round(am, 3), "rebuild_ms": round(rm, 3),
                             "ratio": round(rm / am, 1), "trees_touched": int(np.count_nonzero(np.diff(new_off)))})
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "merkle_append_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

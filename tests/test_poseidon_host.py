"""CPU tests of batched Poseidon / Merkle hashing (mg_poseidon_*, mg_merkle_*): the Python restatement the GPU tests check
against (tests/poseidon_ref.py) is pinned to the reference's BLS12-381 known answer; the committed production parameter
files carry the reference's checkfile digests and the expected MDS / tag; and every argument check of the C ABI answers
MG_ERROR_INVALID_ARGUMENT before any device work, so these run without a GPU."""
import json
import os
import re

import numpy as np
import pytest

import poseidon_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
POS = json.load(open(os.path.join(HERE, "golden", "poseidon_bls381_fr.json")))
INVALID = 1  # MG_ERROR_INVALID_ARGUMENT


def bls_kat_params():
    rc = [int(x) for x in POS["round_constants"]]
    mds = [int(x) for row in POS["mds"] for x in row]
    return P.Params(P.R_BLS381, 3, POS["full_rounds"], POS["partial_rounds"], rc, mds, 3)


def test_restatement_reproduces_the_reference_bls12_381_known_answer():
    """hash.rs:249-258: the permutation of (3, 1, 2) over BLS12-381 Fr, and hash(1, 2) with domain tag 3 = its word 0"""
    p = bls_kat_params()
    want = [int(x) for x in POS["output"]]
    assert p.permute([int(x) for x in POS["input"]]) == want
    assert p.hash([1, 2]) == want[0]


def test_restatement_check_values_of_the_utxo_accumulator_model():
    _, p = P.load("utxo-accumulator-model.dat")
    assert p.hash([1, 2]) == 0x1744de3ecd28245ea716dbf79cba9ec8fe641e376c1a6eeff74cb8f55afd533f
    t = P.Tree(p, range(1, 4))
    assert t.root(20, 1) == 0x0d1e52ee866bd8b7b874f287ffcfa1a7a9cca3aa64bd1da41ed65f5db6b09082
    assert t.root(20, 3) == 0x2ccab89989b6130f5b9eb16e852b0272194b61a056aa012ffe50d8389691d8da
    assert t.root(20, 0) == 0
    for i in range(3):
        assert P.fold(p, i + 1, i, t.path(20, 3, i)) == t.root(20, 3)


@pytest.mark.parametrize("name", sorted(P.CHECKFILE))
def test_production_parameter_fixtures(name):
    """the four committed files: BLAKE3 through the library (mg_blake3) = manta-parameters/data.checkfile; length = keys +
    MDS + tag for the width's round counts; MDS = the Cauchy matrix 1 / (i + t + j) mod r; tag 0"""
    from manta_rs_amd import api
    meta = P.CHECKFILE[name]
    data = open(os.path.join(P.PARAM_DIR, name), "rb").read()
    assert api.blake3(data).hex() == meta["blake3"]
    w, f, p = meta["width"], meta["full_rounds"], meta["partial_rounds"]
    assert (f, p) == api.POSEIDON_ROUNDS[w]
    assert len(data) == 32 * api.poseidon_param_count(w, f, p)
    prm = P.Params.decode(P.R_BN254, data, w, f, p)
    assert prm.mds == [pow(i + w + j, -1, P.R_BN254) for i in range(w) for j in range(w)]
    assert prm.tag == 0
    h = api.PoseidonHasher.decode(api.BN254, data)  # host-only: decoding needs no GPU
    assert (h.width, h.full_rounds, h.partial_rounds) == (w, f, p)


def _create(curve, width, full, partial, data):
    from manta_rs_amd import api
    import ctypes
    h = ctypes.c_void_p()
    rc = api.LIB.mg_poseidon_create(curve, width, full, partial, data, api._sz(len(data)), ctypes.byref(h))
    return rc, h


def test_poseidon_create_rejects_malformed_parameters():
    from manta_rs_amd import api
    data, p = P.load("utxo-accumulator-model.dat")
    rc, h = _create(0, 3, 8, 55, data)
    assert rc == 0 and h.value
    api.LIB.mg_poseidon_destroy(h)
    assert _create(0, 3, 8, 55, data[:-32])[0] == INVALID  # wrong length
    assert _create(0, 3, 8, 55, data + bytes(32))[0] == INVALID
    for pos in (0, 100, len(data) // 32 - 1):  # one element equal to r: a round key, an MDS entry, the tag
        bad = bytearray(data)
        bad[32 * pos:32 * pos + 32] = P.R_BN254.to_bytes(32, "little")
        rc, h = _create(0, 3, 8, 55, bytes(bad))
        assert rc == INVALID and not h.value, pos
    bad = bytearray(data)
    bad[32 * 5:32 * 6] = (P.R_BN254 - 1).to_bytes(32, "little")  # r - 1 is canonical
    rc, h = _create(0, 3, 8, 55, bytes(bad))
    assert rc == 0
    api.LIB.mg_poseidon_destroy(h)
    for w in (2, 7):  # widths outside 3..6, with a length that would match them
        n = api.poseidon_param_count(w, 8, 55)
        assert _create(0, w, 8, 55, bytes(32 * n))[0] == INVALID, w
    for full in (7, 9, 0):  # full rounds odd or zero (length matching)
        n = api.poseidon_param_count(3, full, 55)
        assert _create(0, 3, full, 55, bytes(32 * n))[0] == INVALID, full
    assert _create(2, 3, 8, 55, data)[0] == INVALID  # no such curve
    with pytest.raises(api.MantaGpuError):
        api.PoseidonHasher.decode(api.BN254, data, width=4)


def test_merkle_argument_checks_need_no_gpu():
    from manta_rs_amd import api
    h3 = api.PoseidonHasher.decode(api.BN254, P.load("utxo-accumulator-model.dat")[0])
    h4 = api.PoseidonHasher.decode(api.BN254, P.load("nullifier-commitment-scheme.dat")[0])
    leaves = np.zeros((5, 4), dtype=np.uint64)
    for height, n in ((3, 5), (2, 3), (4, 9)):  # n > 2^(height - 1)
        with pytest.raises(api.MantaGpuError) as e:
            api.merkle_tree(h3, height, leaves[:n] if n <= 5 else np.zeros((n, 4), dtype=np.uint64))
        assert e.value.status == INVALID
    for height in (1, 33):
        with pytest.raises(api.MantaGpuError) as e:
            api.merkle_tree(h3, height, leaves[:1])
        assert e.value.status == INVALID
        with pytest.raises(api.MantaGpuError) as e:
            api.merkle_forest_roots(h3, height, leaves[:1], [0, 1])
        assert e.value.status == INVALID
    with pytest.raises(api.MantaGpuError) as e:
        api.merkle_tree(h4, 20, leaves)  # the tree's inner hash has width 3
    assert e.value.status == INVALID
    with pytest.raises(api.MantaGpuError) as e:
        api.merkle_forest_roots(h4, 20, leaves, [0, 5])
    assert e.value.status == INVALID
    with pytest.raises(api.MantaGpuError) as e:
        api.merkle_tree(h3, 20, leaves, indices=[5])  # a path of a leaf that is not there
    assert e.value.status == INVALID
    for off in ([1, 5], [0, 3, 2], [0, 5, 9]):  # offsets not from 0, decreasing, a tree over capacity (height 3: 4)
        with pytest.raises(api.MantaGpuError) as e:
            api.merkle_forest_roots(h3, 3, np.zeros((9, 4), dtype=np.uint64), off)
        assert e.value.status == INVALID
    # the empty tree and an empty forest are answered without the GPU
    root, paths = api.merkle_tree(h3, 20, np.zeros((0, 4), dtype=np.uint64))
    assert not root.any() and paths.shape == (0, 19, 4)
    assert api.merkle_forest_roots(h3, 20, np.zeros((0, 4), dtype=np.uint64), [0]).shape == (0, 4)


def test_chunk_size_matches_the_header():
    from manta_rs_amd import api
    hdr = open(os.path.join(HERE, "..", "include", "mantagpu.h")).read()
    m = re.search(r"#define MG_POSEIDON_CHUNK \(1u << (\d+)\)", hdr)
    assert m and api.POSEIDON_CHUNK == 1 << int(m.group(1))

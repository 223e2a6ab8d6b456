"""GPU parity of the phase-2 key initialisation (SURVEY f-4): `mg_qap_columns` -- the column sums of scaled group elements of
`specialize_to_phase_2` (mpc.rs:251-294) -- against one oracle MSM per column, and `mg_mpc_initialize` against the oracle's
scalar-side setup at the same toxic waste. Group elements are unique: every comparison is exact, on the limbs."""
import functools

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import ceremony, synth

pytestmark = pytest.mark.gpu
CASES = [(0, 1), (0, 2), (1, 1), (1, 2)]


def csr_of(curve, m, triples):
    """CSR of m rows from (row, column, coefficient) triples in the order given within a row; repeated (row, column) pairs and
    zero coefficients stay stored."""
    r = synth.FR_MODULUS[curve]
    rows = [[] for _ in range(m)]
    for i, j, k in triples:
        rows[i].append((j, k % r))
    row_ptr = np.zeros(m + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum([len(x) for x in rows])
    flat = [e for x in rows for e in x]
    col = np.array([j for j, _ in flat], dtype=np.uint32)
    val = synth.to_mont([k for _, k in flat], r, 4) if flat else np.zeros((0, 4), dtype=np.uint64)
    return synth.CSR(row_ptr, col, val)


def expected(curve, group, terms, n_cols):
    """out[j] = the oracle's MSM over every (basis row, coefficient) of column j, terms = [(basis, triples)]; zeros if empty"""
    r = synth.FR_MODULUS[curve]
    w = O.point_limbs(curve, group)
    per = [([], []) for _ in range(n_cols)]
    for basis, triples in terms:
        for i, j, k in triples:
            per[j][0].append(basis[i])
            per[j][1].append(k % r)
    out = np.zeros((n_cols, w), dtype=np.uint64)
    for j, (pts, ks) in enumerate(per):
        if pts:
            out[j] = O.msm(curve, group, np.stack(pts), synth.ints_to_limbs(ks, 4))
    return out


@functools.lru_cache(maxsize=None)
def shapes_case(curve, group):
    """m = 40, 24 columns: empty first and last column, a one-entry and a three-entry column, the coefficients that take no
    ladder (0, 1, r - 1) and short ones (2, 2^64) beside uniform ones, a basis row at infinity used by two columns"""
    r = synth.FR_MODULUS[curve]
    m, n_cols = 40, 24
    rng = synth.XorShift(900 + 10 * curve + group)
    basis = H.random_points(curve, group, m, seed=910 + curve)
    basis[5] = 0
    special = [0, 1, r - 1, 2, 1 << 64]
    t = [(7, 1, rng.field(r))]                                             # column 1: one entry
    t += [(2, 2, rng.field(r)), (9, 2, 1), (30, 2, rng.field(r))]          # column 2: three entries
    t += [(5, 3, rng.field(r)), (5, 4, 3), (6, 4, rng.field(r))]           # the row at infinity, in columns 3 and 4
    t += [(i, 6 + i, k) for i, k in enumerate(special)]                    # every special coefficient alone in a column ...
    t += [(10 + i, 11, k) for i, k in enumerate(special)]                  # ... and all of them in one
    for i in range(m):
        for _ in range(3):
            t.append((i, 12 + rng.next() % 11, rng.field(r) if rng.next() % 3 else special[rng.next() % 5]))
    return m, n_cols, basis, t, expected(curve, group, [(basis, t)], n_cols)


@pytest.mark.parametrize("curve,group", CASES)
def test_column_sums_match_one_oracle_msm_per_column(gpu, curve, group):
    m, n_cols, basis, t, want = shapes_case(curve, group)
    assert not want[0].any() and not want[n_cols - 1].any() and want[1].any()
    M = csr_of(curve, m, t)
    for epl in (0, 1, 2, 5):
        got = gpu.qap_columns(curve, group, [basis], [M], n_cols, entries_per_lane=epl)
        assert (got == want).all(), (epl, np.flatnonzero((got != want).any(axis=1)))


@functools.lru_cache(maxsize=None)
def long_column_case(curve, group):
    """m = 64, 8 columns. Column 3 has 300 entries: 48 rows of (c P, -c P, P, P, -P, -P) -- the running sum passes through
    infinity, doubles, and cancels in every block, and with 1 to 3 entries per lane each of those pairs also meets across a lane
    boundary, in the merge -- then 12 ordinary entries. Column 5 sums to infinity as a whole; columns 0 and 7 are empty."""
    r = synth.FR_MODULUS[curve]
    m, n_cols = 64, 8
    rng = synth.XorShift(950 + 10 * curve + group)
    basis = H.random_points(curve, group, m, seed=960 + curve)
    t = []
    for i in range(48):
        c = rng.field(r)
        t += [(i, 3, k) for k in (c, r - c, 1, 1, r - 1, r - 1)]
    t += [(50 + i, 3, rng.field(r)) for i in range(12)]
    k5 = rng.field(r)
    t += [(62, 5, k5), (62, 5, r - k5), (63, 5, 5), (63, 5, r - 5)]
    t += [(i, 1 + (i % 2) * 5, rng.field(r)) for i in range(0, 64, 3)]     # columns 1 and 6
    t += [(i, 2, 1) for i in (4, 4, 8)] + [(20, 4, r - 1), (20, 4, 2)]
    want = expected(curve, group, [(basis, t)], n_cols)
    assert want[3].any() and not want[5].any() and sum(1 for e in t if e[1] == 3) == 300
    return m, n_cols, basis, t, want


@pytest.mark.parametrize("curve,group", CASES)
def test_long_column_with_doublings_and_cancellations_on_every_lane_boundary(gpu, curve, group):
    m, n_cols, basis, t, want = long_column_case(curve, group)
    M = csr_of(curve, m, t)
    for epl in (1, 2, 3, 64, 0):
        got = gpu.qap_columns(curve, group, [basis], [M], n_cols, entries_per_lane=epl)
        assert (got == want).all(), (epl, np.flatnonzero((got != want).any(axis=1)))


@pytest.mark.parametrize("curve,group", CASES)
def test_more_than_one_workgroup_and_two_merge_levels(gpu, curve, group):
    """700 entries at one entry per lane: three workgroups of the entry and segmented-sum kernels, 1 400 partials, a merge
    level that is not the last"""
    r = synth.FR_MODULUS[curve]
    m, n_cols = 64, 50
    rng = synth.XorShift(970 + 10 * curve + group)
    basis = H.random_points(curve, group, m, seed=960 + curve)
    t = [(rng.next() % m, rng.next() % n_cols, rng.field(r) if rng.next() % 2 else 1 + rng.next() % 7) for _ in range(700)]
    want = expected(curve, group, [(basis, t)], n_cols)
    M = csr_of(curve, m, t)
    for epl in (1, 0):
        assert (gpu.qap_columns(curve, group, [basis], [M], n_cols, entries_per_lane=epl) == want).all(), epl


@pytest.mark.parametrize("curve,group", CASES)
def test_terms_add_up_and_degenerate_sizes(gpu, curve, group):
    r = synth.FR_MODULUS[curve]
    m, n_cols = 12, 7
    rng = synth.XorShift(980 + 10 * curve + group)
    terms = []
    for s in range(3):
        basis = H.random_points(curve, group, m, seed=985 + s)
        terms.append((basis, [(rng.next() % m, rng.next() % n_cols, rng.field(r)) for _ in range(20)]))
    mats = [csr_of(curve, m, t) for _, t in terms]
    bases = [b for b, _ in terms]
    all3 = gpu.qap_columns(curve, group, bases, mats, n_cols)
    assert (all3 == expected(curve, group, terms, n_cols)).all()
    single = [gpu.qap_columns(curve, group, [b], [M], n_cols) for b, M in zip(bases, mats)]
    for j in range(n_cols):
        assert (all3[j] == O.g_add(curve, group, O.g_add(curve, group, single[0][j], single[1][j]), single[2][j])).all(), j
    # no stored entry at all: every sum is the point at infinity
    empty = csr_of(curve, m, [])
    assert not gpu.qap_columns(curve, group, bases, [empty] * 3, n_cols).any()
    # one row, one column
    k = rng.field(r)
    one = gpu.qap_columns(curve, group, [bases[0][:1]], [csr_of(curve, 1, [(0, 0, k)])], 1)
    assert (one[0] == O.g_mul(curve, group, bases[0][0], synth.ints_to_limbs([k], 4)[0])).all()


KEY_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1", "a_query", "b_g1_query",
              "b_g2_query", "h_query", "l_query")
TOXIC = (0x1111111111111111222333, 0x3333333333333333444555, 0x5555555555555555666777)   # tau, alpha, beta


@functools.lru_cache(maxsize=None)
def accumulator_and_key(curve, m, V, P, seed):
    """a circuit, the accumulator of 2 D powers at TOXIC (built with the oracle) and the oracle's key at (tau, alpha, beta, 1, 1)"""
    r = synth.FR_MODULUS[curve]
    c = synth.make_circuit(curve, m, V, P, seed=seed)
    D = c.D
    tau, alpha, beta = TOXIC
    G1, G2 = O.generator(curve, 1), O.generator(curve, 2)
    lim = lambda ks: synth.ints_to_limbs([k % r for k in ks], 4)
    tp = [pow(tau, i, r) for i in range(2 * D)]
    acc = ceremony.Accumulator(curve, O.fixed_base_mul(curve, 1, G1, lim(tp)), O.fixed_base_mul(curve, 2, G2, lim(tp[:D])),
                               O.fixed_base_mul(curve, 1, G1, lim([alpha * t for t in tp[:D]])),
                               O.fixed_base_mul(curve, 1, G1, lim([beta * t for t in tp[:D]])), O.g_mul(curve, 2, G2, lim([beta])[0]))
    return c, acc, O.groth16_setup(c, synth.to_mont([tau, alpha, beta, 1, 1], r, 4))


def assert_same_key(pk, want, h_len):
    for f in KEY_FIELDS:
        got, ref = np.asarray(getattr(pk, f)), np.asarray(getattr(want, f))
        if f == "h_query":
            got, ref = got[:h_len], ref[:h_len]
        assert (got.reshape(-1) == ref.reshape(-1)).all(), f


@pytest.mark.parametrize("curve", [0, 1])
def test_mpc_initialize_equals_the_oracle_setup(gpu, curve):
    """the tiny circuit of the ceremony test: the key at h_len = D - 1 is the oracle's field by field; at h_len = D the extra
    entry is (tau^(2D-1) - tau^(D-1)) G"""
    r = synth.FR_MODULUS[curve]
    c, acc, want = accumulator_and_key(curve, 27, 20, 4, 81)
    D = c.D
    pk = ceremony.initialize(acc, c)
    assert pk.h_query.shape[0] == D - 1 and pk.h_len == D - 1
    assert_same_key(pk, want, D - 1)
    pkd = ceremony.initialize(acc, c, h_len=D)
    assert pkd.h_query.shape[0] == D
    assert_same_key(pkd, want, D - 1)
    tau = TOXIC[0]
    last = synth.ints_to_limbs([(pow(tau, 2 * D - 1, r) - pow(tau, D - 1, r)) % r], 4)[0]
    assert (pkd.h_query[D - 1] == O.g_mul(curve, 1, O.generator(curve, 1), last)).all()


def test_mpc_initialize_at_d_256_equals_oracle_and_composition(gpu):
    """BN254, D = 256: the oracle's key, the key composed from the element-wise entry points, and the same bytes twice"""
    curve = 0
    c, acc, want = accumulator_and_key(curve, 230, 200, 9, 82)
    assert c.D == 256
    pk = ceremony.initialize(acc, c)
    assert_same_key(pk, want, c.D - 1)
    old = ceremony.initialize_by_composition(acc, c)
    again = ceremony.initialize(acc, c)
    for f in KEY_FIELDS:
        assert np.asarray(getattr(pk, f)).tobytes() == np.asarray(getattr(again, f)).tobytes(), f
        assert (np.asarray(getattr(pk, f)).reshape(-1) == np.asarray(getattr(old, f)).reshape(-1)).all(), f

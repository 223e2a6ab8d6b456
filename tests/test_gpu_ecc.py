"""GPU parity for the group-operation primitives the MSM kernels are made of -- the menu the reference itself
benchmarks and cross-checks (manta-benchmark/src/ecc.rs:30-128, consistency tests :138-172; SURVEY.md row
a-12): mixed addition, general addition, doubling, scalar multiplication and batch normalisation, all through
`mg_ec_elementwise`, every output affine point bit-exact against the CPU oracle."""
import numpy as np
import pytest

import helpers as H
import oracle_lib as O
from manta_rs_amd import synth

pytestmark = pytest.mark.gpu

CASES = [(0, 1), (1, 1), (0, 2), (1, 2)]


def _neg(curve, group, p):
    """-P through the oracle: [r-1]P."""
    r = synth.FR_MODULUS[curve]
    return O.g_mul(curve, group, p, synth.ints_to_limbs([r - 1], 4)[0])


@pytest.mark.parametrize("curve,group", CASES)
def test_addition_is_consistent_for_mixed_and_general_formulas(gpu, curve, group):
    """ecc.rs:138-156: affine+affine, projective+=affine and projective+=projective agree -- here each GPU
    formula against the oracle's sum, including the exceptional inputs (P+P, P+(-P), infinity on either side)."""
    n = 150
    a = H.random_points(curve, group, n, seed=301)
    b = H.random_points(curve, group, n, seed=302)
    b[3] = a[3]                      # P + P  -> must take the doubling path
    b[4] = _neg(curve, group, a[4])  # P + (-P) = infinity
    a[5] = 0                         # infinity + Q
    b[6] = 0                         # P + infinity
    a[7] = 0
    b[7] = 0                         # infinity + infinity
    want = np.stack([O.g_add(curve, group, a[i], b[i]) for i in range(n)])
    assert (want[4] == 0).all() and (want[7] == 0).all()
    mixed = gpu.ec_elementwise(curve, group, gpu.EC_ADD_MIXED, a, b)
    full = gpu.ec_elementwise(curve, group, gpu.EC_ADD, a, b)
    assert (mixed == want).all()
    assert (full == want).all()
    # subtraction = addition of the negated point
    wsub = np.stack([O.g_add(curve, group, a[i], _neg(curve, group, b[i])) if b[i].any() else a[i] for i in range(n)])
    assert (gpu.ec_elementwise(curve, group, gpu.EC_SUB_MIXED, a, b) == wsub).all()


@pytest.mark.parametrize("curve,group", CASES)
def test_doubling_matches_addition_with_itself(gpu, curve, group):
    n = 70
    a = H.random_points(curve, group, n, seed=303)
    a[2] = 0
    want = np.stack([O.g_add(curve, group, a[i], a[i]) for i in range(n)])
    assert (gpu.ec_elementwise(curve, group, gpu.EC_DOUBLE, a) == want).all()
    assert (gpu.ec_elementwise(curve, group, gpu.EC_ADD, a, a) == want).all()


@pytest.mark.parametrize("curve,group", CASES)
def test_scalar_multiplication_is_consistent(gpu, curve, group):
    """ecc.rs:158-172: affine*scalar == projective*scalar -- here double-and-add on the GPU against the oracle,
    with the edge scalars 0, 1, 2, r-1 and r (= the group order: [r]P = infinity)."""
    n = 40
    a = H.random_points(curve, group, n, seed=304)
    k = synth.msm_scalars(curve, n, "U", seed=305)
    r = synth.FR_MODULUS[curve]
    for i, v in enumerate([0, 1, 2, r - 1, r]):
        k[i] = synth.ints_to_limbs([v], 4)[0]
    a[9] = 0
    want = np.stack([O.g_mul(curve, group, a[i], k[i]) for i in range(n)])
    assert (want[0] == 0).all() and (want[4] == 0).all() and (want[1] == a[1]).all()
    got = gpu.ec_elementwise(curve, group, gpu.EC_MUL, a, k)
    assert (got == want).all()


LIMB_BITS = (0, 31, 32, 63, 64, 127, 128, 223, 224, 252)  # one set bit on either side of a 32-bit limb boundary; 2^252 < r


@pytest.mark.parametrize("curve,group", CASES)
def test_scalar_multiplication_at_limb_boundaries(gpu, curve, group):
    """The 256-bit double-and-add walk of every kernel that has one, on scalars whose set bits sit at the ends of
    32-bit limbs: point i times scalar i (EC_MUL), every point times one scalar (EC_MUL_FIXED) and one base times
    every scalar on the per-lane path of fixed_base_mul (n below the table threshold)."""
    from manta_rs_amd import ceremony
    n = 20
    r = synth.FR_MODULUS[curve]
    rng = synth.XorShift(310 + curve)
    ks = [1 << b for b in LIMB_BITS] + [(1 << 32) - 1, (1 << 224) - 1]
    ks += [rng.field(r) for _ in range(n - len(ks))]
    assert len(ks) == n and all(v < r for v in ks)
    k = synth.ints_to_limbs(ks, 4)
    a = H.random_points(curve, group, n, seed=307)
    want = np.stack([O.g_mul(curve, group, a[i], k[i]) for i in range(n)])
    assert (gpu.ec_elementwise(curve, group, gpu.EC_MUL, a, k) == want).all()
    for j, b in enumerate(LIMB_BITS):
        got = ceremony.batch_mul_fixed_scalar(curve, group, a[:3], 1 << b)
        wantb = np.stack([O.g_mul(curve, group, a[i], k[j]) for i in range(3)])
        assert (got == wantb).all(), b
    got = gpu.fixed_base_mul(curve, group, a[0], gpu.DeviceBuffer.from_numpy(k[:12]), 12)
    got = got.to_numpy(shape=(12, gpu.affine_limbs(curve, group)))
    assert (got == O.fixed_base_mul(curve, group, a[0], k[:12])).all()


@pytest.mark.parametrize("curve,group", CASES)
def test_normalising_tail_at_its_batch_boundaries(gpu, curve, group):
    """The XYZZ -> affine tail inverts once per 16 results and skips infinity: sizes around one and two batches, a
    whole batch of infinity results (its running product stays 1), a single infinity result at the ends of a batch,
    a last batch of one element."""
    N = 33
    a0 = H.random_points(curve, group, N, seed=308)
    b0 = H.random_points(curve, group, N, seed=309)
    wsub = np.stack([O.g_add(curve, group, a0[i], _neg(curve, group, b0[i])) for i in range(N)])
    wdbl = np.stack([O.g_add(curve, group, a0[i], a0[i]) for i in range(N)])
    for n in (1, 15, 16, 17, 33):
        holes = [[]] + [[p] for p in sorted({0, 15, 16, n - 1}) if p < n] + ([list(range(16))] if n >= 16 else [])
        for hole in holes:
            a, b, ws, wd = a0[:n].copy(), b0[:n].copy(), wsub[:n].copy(), wdbl[:n].copy()
            b[hole] = a[hole]  # P - P = infinity
            ws[hole] = 0
            assert (gpu.ec_elementwise(curve, group, gpu.EC_SUB_MIXED, a, b) == ws).all(), (n, hole)
            a[hole] = 0        # 2 * infinity = infinity
            wd[hole] = 0
            assert (gpu.ec_elementwise(curve, group, gpu.EC_DOUBLE, a) == wd).all(), (n, hole)


def test_batch_normalisation_of_2_16_points(gpu):
    """ecc.rs:114-119 normalises 2^16 projective points at once: 2^16 doublings on the GPU, every affine output on
    the curve, spot-checked against the oracle, and the sum of all outputs equal to twice the sum of the inputs
    (a size-independent linearity check)."""
    curve, group, n = 1, 1, 1 << 16
    base = H.random_points(curve, group, 64, seed=306)
    a = np.ascontiguousarray(np.tile(base, (n // 64, 1)))
    got = gpu.ec_elementwise(curve, group, gpu.EC_DOUBLE, a)
    for i in (0, 1, 63, 64, n - 1):
        assert (got[i] == O.g_add(curve, group, a[i], a[i])).all()
    assert (got[:64] == got[-64:]).all()
    s_in = gpu.points_sum(curve, group, base)
    s_out = gpu.points_sum(curve, group, got[:64])
    assert (s_out == O.g_add(curve, group, s_in, s_in)).all()


def test_ec_elementwise_rejects_bad_arguments(gpu):
    a = H.random_points(0, 1, 4, seed=1)
    with pytest.raises(gpu.MantaGpuError):
        gpu.ec_elementwise(0, 1, 9, a, a)
    with pytest.raises(gpu.MantaGpuError):
        gpu.ec_elementwise(0, 1, gpu.EC_ADD, a, None)
    with pytest.raises(gpu.MantaGpuError):
        gpu.ec_elementwise(0, 3, gpu.EC_ADD, a, a)

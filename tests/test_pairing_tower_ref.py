"""CPU pins (no GPU) of tests/pairing_tower_ref.py, the plain-integer model the GPU's pairing building blocks are compared with:
its multiplication, its memory order and the final exponentiation's exponent against the CPU oracle and a committed verifying
key; ring identities of its powers; the step counts of the almost-inverse replay that the GPU test's input census relies on."""
import numpy as np
import pytest

import oracle_lib as O
import pairing_tower_ref as T
from manta_rs_amd import synth
from vk_fixtures import VK


def _points(curve, a, b):
    r = synth.FR_MODULUS[curve]
    lim = lambda k: synth.ints_to_limbs([k % r], 4)[0]
    return O.g_mul(curve, 1, O.generator(curve, 1), lim(a)), O.g_mul(curve, 2, O.generator(curve, 2), lim(b))


def test_bn254_power_of_the_textbook_pairing_is_arkworks_value():
    """e^c for c = 2x(6x^2 + 3x + 1): one 190-bit power pins the schoolbook product, the slot order and c at once"""
    t = T.tower(0)
    c = 2 * t.x * (6 * t.x ** 2 + 3 * t.x + 1)
    assert t.final_exponent == c * ((t.p ** 12 - 1) // t.r)
    P, Q = _points(0, 0x1234567890abcdef, 0xfedcba9876543211)
    e = t.from_bytes(O.pairing_bytes(0, P, Q))
    assert t.to_bytes(t.pow(e, c)) == O.pairing_bytes(0, P, Q, ark_exp=True)
    assert t.to_bytes(e) == O.pairing_bytes(0, P, Q)  # bytes -> element -> bytes


def test_bn254_reference_key_file_holds_that_power_of_its_alpha_and_beta():
    t = T.tower(0)
    vk = VK("to-private")
    e = t.from_bytes(O.pairing_bytes(0, vk.alpha, vk.beta))
    assert t.to_bytes(t.pow(e, t.final_exponent // ((t.p ** 12 - 1) // t.r))) == vk.alpha_beta_bytes


def test_bls381_cube_of_the_textbook_pairing():
    t = T.tower(1)
    assert t.final_exponent == 3 * ((t.p ** 12 - 1) // t.r)
    P, Q = _points(1, 0xabcdef0123456789, 0x1122334455667789)
    e = t.from_bytes(O.pairing_bytes(1, P, Q))
    assert t.to_bytes(t.pow(e, 3)) == O.pairing_bytes_pow(1, P, Q, 3)


def _random_element(t, seed):
    rng = synth.XorShift(seed)
    return tuple((rng.field(t.p), rng.field(t.p)) for _ in range(6))


@pytest.mark.parametrize("curve", [0, 1])
def test_ring_identities(curve):
    t = T.tower(curve)
    a = _random_element(t, 41 + curve)
    b = _random_element(t, 43 + curve)
    c = _random_element(t, 47 + curve)
    assert t.mul(a, t.one) == a and t.mul(t.one, a) == a and t.mul(a, b) == t.mul(b, a)
    assert t.mul(t.mul(a, b), c) == t.mul(a, t.mul(b, c))
    w = ((0, 0), (1, 0)) + ((0, 0),) * 4
    assert t.pow(w, 6) == ((t.u0, 1),) + ((0, 0),) * 5            # w^6 = xi
    assert t.mul(a, t.inv(a)) == t.one                             # a a^(p^12 - 2) = 1
    n = t.mul(t.conj(a), a)                                        # a^(p^6) a lies in Fq6: no odd power of w
    assert all(n[m] == (0, 0) for m in (1, 3, 5)) and n != t.zero
    f = t.final_exp(a)
    assert f != t.one and t.pow(f, t.r) == t.one                   # order divides r
    g = t.cyclotomic(a)
    assert t.pow(g, t.phi12) == t.one and t.mul(t.pow_x(g), t.pow(g, -t.x if t.x < 0 else t.phi12 - t.x)) == t.one


@pytest.mark.parametrize("curve", [0, 1])
def test_memory_order_and_montgomery_words_round_trip(curve):
    t = T.tower(curve)
    a = _random_element(t, 53 + curve)
    w = t.words([a, t.one])
    assert w.shape == (2, 12 * t.N) and w.dtype == np.uint32
    assert t.elements(w) == [a, t.one]
    # slot 3 i + j holds the coefficient of w^(i + 2 j); the Montgomery one is R mod p
    assert [t.SLOT_POWER[s] for s in range(6)] == [0, 2, 4, 1, 3, 5]
    assert (w[1][:t.N] == t.raw_words([t.R])[0]).all() and not w[1][t.N:].any()
    ys = t.edge_representatives()
    assert t.fq_values(t.raw_words(ys)) == [t.mont_value(y) for y in ys]
    assert len(ys) == 7 + 2 * (t.N - 1) + 2


@pytest.mark.parametrize("curve", [0, 1])
def test_almost_inverse_step_counts(curve):
    """y = 2^j takes N' + j steps: 1 .. 16 cross the boundary 32 N between the two tails of the kernel's inv_euclid, and the top
    power of two takes the most steps found, 507 (BN254) and 761 (BLS12-381)"""
    t = T.tower(curve)
    n1 = t.bits
    assert (n1, 32 * t.N) == ((254, 256) if curve == 0 else (381, 384))
    assert [t.almost_inverse_steps(1 << j) for j in range(5)] == [n1, n1 + 1, n1 + 2, n1 + 3, n1 + 4]
    assert t.almost_inverse_steps(1 << (n1 - 1)) == (507 if curve == 0 else 761)
    # the replay is the loop whose output is y^-1 2^k: check that on a few values, so that k means what the kernel's tail assumes
    for y in (1, 3, 16, t.p - 1, (t.p + 1) // 2):
        u, v, r, s, k = t.p, y, 0, 1, 0
        while v:
            if not u & 1:
                u, s = u >> 1, s << 1
            elif not v & 1:
                v, r = v >> 1, r << 1
            elif u > v:
                u, r, s = (u - v) >> 1, r + s, s << 1
            else:
                v, s, r = (v - u) >> 1, s + r, r << 1
            k += 1
        assert k == t.almost_inverse_steps(y) and t.bits <= k <= 2 * t.bits
        assert (-r) * y % t.p == pow(2, k, t.p)

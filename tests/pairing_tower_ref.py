"""The pairing's tower in plain Python integers: the model the GPU's building blocks (`mg_pairing_op`) are compared with.

Fq2 = Fq[u]/(u^2 + 1); Fq12 = Fq2[w]/(w^6 - xi), xi = U0 + u, as SIX Fq2 coefficients of w^0 .. w^5 multiplied as schoolbook
polynomials. Every expected value is a product or a plain power in that ring (square-and-multiply):
    Frobenius a^(p^k), conjugation a^(p^6), inverse a^(p^12 - 2), exp_by_x a^x, final exponentiation a^(c (p^12 - 1) / r)
with c = 2x(6x^2 + 3x + 1) on BN254 and 3 on BLS12-381 (what arkworks' hard parts compute; tests/test_pairing_tower_ref.py
pins c, the multiplication and the memory order against the CPU oracle and a committed verifying key). No tower formula, no
Karatsuba, no Frobenius constant: nothing here is shared with manta_rs_amd/csrc/pairing_coop.h.

Two helpers only choose inputs and are never an expected value: `cyclotomic` and `almost_inverse_steps`."""
import numpy as np

from manta_rs_amd import synth

U0 = {0: 9, 1: 1}
X = {0: 0x44e992b44a6909f1, 1: -0xd201000000010000}  # the curve parameter, with its sign


class Tower:
    def __init__(self, curve):
        self.curve = curve
        self.p = p = synth.FQ_MODULUS[curve]
        self.r = synth.FR_MODULUS[curve]
        self.u0, self.x = U0[curve], X[curve]
        self.nl = synth.FQ_LIMBS[curve]   # 64-bit limbs per Fq
        self.N = 2 * self.nl              # 32-bit words per Fq, as the kernels hold them
        self.bits = p.bit_length()        # N'
        self.R = (1 << (32 * self.N)) % p
        self.Rinv = pow(self.R, -1, p)
        self.order = p ** 12 - 1
        assert self.order % self.r == 0
        c = 2 * self.x * (6 * self.x ** 2 + 3 * self.x + 1) if curve == 0 else 3
        self.final_exponent = c * (self.order // self.r)
        self.phi12 = p ** 4 - p ** 2 + 1  # order of the cyclotomic subgroup
        self.one = ((1, 0),) + ((0, 0),) * 5
        self.zero = ((0, 0),) * 6
        self.line_j = (0, 1, 3) if curve == 0 else (0, 2, 3)  # line coefficient t sits at w^line_j[t] (D-type / M-type twist)

    # ---- the ring
    def f2_mul(self, a, b):
        p = self.p
        return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def f2_mul_xi(self, a):
        return self.f2_mul(a, (self.u0, 1))

    def mul(self, a, b):
        """schoolbook: c_m = sum_{i+j=m} a_i b_j + xi sum_{i+j=m+6} a_i b_j, the sums as plain integers"""
        re, im = [0] * 11, [0] * 11
        for i, (a0, a1) in enumerate(a):
            if a0 == 0 and a1 == 0:
                continue
            for j, (b0, b1) in enumerate(b):
                re[i + j] += a0 * b0 - a1 * b1
                im[i + j] += a0 * b1 + a1 * b0
        p, k = self.p, self.u0
        out = []
        for m in range(6):
            x, y = re[m], im[m]
            if m < 5:  # (hr + hi u)(k + u) = (k hr - hi) + (k hi + hr) u
                x += k * re[m + 6] - im[m + 6]
                y += k * im[m + 6] + re[m + 6]
            out.append((x % p, y % p))
        return tuple(out)

    def pow(self, a, e):
        """a^e, e >= 0, by square-and-multiply from the top bit"""
        assert e >= 0
        acc = self.one
        for bit in bin(e)[2:]:
            acc = self.mul(acc, acc)
            if bit == "1":
                acc = self.mul(acc, a)
        return acc

    def inv(self, a):
        assert a != self.zero
        return self.pow(a, self.order - 1)

    def frob(self, a, k):
        return self.pow(a, self.p ** k)

    def conj(self, a):
        return self.frob(a, 6)

    def final_exp(self, a):
        return self.pow(a, self.final_exponent)

    def pow_x(self, a):
        """a^x for a in the cyclotomic subgroup (its order divides p^4 - p^2 + 1, which makes a negative x a positive power)"""
        return self.pow(a, self.x % self.phi12)

    def line(self, coeffs):
        """the sparse element sum_t coeffs[t] w^line_j[t] that a line product multiplies with"""
        el = [(0, 0)] * 6
        for t, c in enumerate(coeffs):
            el[self.line_j[t]] = tuple(c)
        return tuple(el)

    # ---- helpers that choose inputs (never an expected value)
    def cyclotomic(self, a):
        p = self.p
        return self.pow(a, (p ** 6 - 1) * (p ** 2 + 1))

    def almost_inverse_steps(self, y):
        """the step count k of Kaliski's almost-inverse loop on the integer 0 < y < p (y^-1 2^k comes out of it)"""
        u, v, r, s, k = self.p, y, 0, 1, 0
        while v:
            if not u & 1:
                u >>= 1
                s <<= 1
            elif not v & 1:
                v >>= 1
                r <<= 1
            elif u > v:
                u = (u - v) >> 1
                r += s
                s <<= 1
            else:
                v = (v - u) >> 1
                s += r
                r <<= 1
            k += 1
        return k

    # ---- memory: arkworks order, slot 3 i + j holds the coefficient of w^(i + 2 j); Montgomery words through synth
    SLOT_POWER = tuple((s // 3) + 2 * (s % 3) for s in range(6))

    def fq_words(self, vals):
        """field values -> [len, N] uint32 Montgomery words"""
        return synth.to_mont(list(vals), self.p, self.nl).view(np.uint32)

    def raw_words(self, ys):
        """Montgomery representatives y < p themselves -> [len, N] uint32 words"""
        assert all(0 <= y < self.p for y in ys)
        return synth.ints_to_limbs(list(ys), self.nl).view(np.uint32)

    def fq_values(self, words):
        """[.., N] uint32 Montgomery words -> list of field values"""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, self.N)
        return synth.from_mont(w.view(np.uint64), self.p)

    def mont_value(self, y):
        """the field value of the Montgomery representative y"""
        return y * self.Rinv % self.p

    def slots(self, el):
        """element -> the 12 Fq values in memory order"""
        out = []
        for s in range(6):
            out += list(el[self.SLOT_POWER[s]])
        return out

    def from_slots(self, vals):
        assert len(vals) == 12
        el = [None] * 6
        for s in range(6):
            el[self.SLOT_POWER[s]] = (vals[2 * s] % self.p, vals[2 * s + 1] % self.p)
        return tuple(el)

    def words(self, elements):
        """Fq12 elements -> [len, 12 N] uint32"""
        flat = [v for el in elements for v in self.slots(el)]
        return self.fq_words(flat).reshape(len(elements), 12 * self.N)

    def elements(self, words):
        """[len, 12 N] uint32 -> Fq12 elements"""
        vals = self.fq_values(words)
        return [self.from_slots(vals[12 * i:12 * i + 12]) for i in range(len(vals) // 12)]

    def from_bytes(self, data):
        """arkworks' serialisation (12 canonical little-endian Fq) -> element"""
        nb = 8 * self.nl
        assert len(data) == 12 * nb
        return self.from_slots([int.from_bytes(data[i * nb:(i + 1) * nb], "little") for i in range(12)])

    def to_bytes(self, el):
        return b"".join(v.to_bytes(8 * self.nl, "little") for v in self.slots(el))

    def f2_words(self, pairs):
        """Fq2 values -> [len, 2 N] uint32"""
        return self.fq_words([v for c in pairs for v in c]).reshape(len(pairs), 2 * self.N)

    def f2_values(self, words):
        v = self.fq_values(words)
        return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]

    # ---- the Montgomery representatives at which word arithmetic goes wrong
    def edge_representatives(self):
        p, N = self.p, self.N
        low = (1 << (32 * (N - 1))) - 1
        ys = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
        for j in range(1, N):
            ys += [1 << (32 * j), (1 << (32 * j)) - 1]
        ys.append((((p >> (32 * (N - 1))) - 1) << (32 * (N - 1))) | low)  # the largest y < p whose low limbs are all ones
        ys.append(self.R)                                                 # the value 1
        assert all(0 <= y < p for y in ys) and len(set(ys)) == len(ys)
        return ys


_TOWERS = {}


def tower(curve):
    if curve not in _TOWERS:
        _TOWERS[curve] = Tower(curve)
    return _TOWERS[curve]

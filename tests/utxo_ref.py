"""A pure-Python restatement of manta-pay's UTXO statement, for the tests of mg_utxo_model_* / mg_utxos_* / mg_viewing_keys
(tests/test_utxo_host.py, tests/test_gpu_utxo.py). Plain integers, canonical (not Montgomery), built on poseidon_ref (the
`Hasher`s) and edwards_ref (the embedded curve).

  secret / public  manta-accounting/src/transfer/utxo/protocol.rs:93-114: the asset on its side, the default (0, 0) on the other
  commitment       manta-pay/src/config/utxo.rs:367-393: H5 [randomness, asset_id, asset_value, receiving_key.x, receiving_key.y]
  item             utxo.rs:1153-1167: H4 [is_transparent, public_asset.id, public_asset.value, commitment]
  nullifier        utxo.rs:1465-1485: H3 [proof_authorization_key.x, proof_authorization_key.y, item]
  viewing key      utxo.rs:523-545: rem_mod_prime(H2 [proof_authorization_key.x, proof_authorization_key.y]) into the scalar field
  reconstruct      protocol.rs:1461-1487: commit(identifier.randomness, secret(asset).id, secret(asset).value, receiving_key),
                   Utxo::new(identifier.is_transparent, public(asset), commitment); utxo_check (:1489-1499) compares it whole
  mint             protocol.rs:1152-1207: plaintext asset = secret(asset), Utxo::new(is_transparent, public(asset), commitment)

A record is (flag, public id, public value, commitment); a plaintext (randomness, asset id, asset value)."""
import os

import edwards_ref as E
import poseidon_ref as P

R, L = E.R, E.L
OK, BAD_ENCODING, MISMATCH = 0, 1, 2
FILES = ("utxo-commitment-scheme.dat", "utxo-accumulator-item-hash.dat", "nullifier-commitment-scheme.dat",
         "viewing-key-derivation-function.dat", "group-generator.dat")
SHAPES = ((6, 8, 56), (5, 8, 56), (4, 8, 55), (3, 8, 55))  # width, full, partial rounds of H5, H4, H3, H2
U128 = 1 << 128


def read(name):
    return open(os.path.join(P.PARAM_DIR, name), "rb").read()


def rem_mod_l(v):
    """`rem_mod_prime` as the device does it: r < 8 l, so the quotient's three bits are three conditional subtractions"""
    assert 0 <= v < R
    q = 0
    for s in (2, 1, 0):
        if v >= (L << s):
            v -= L << s
            q |= 1 << s
    return v, q


class Model:
    def __init__(self, files=None):
        files = [read(n) for n in FILES] if files is None else list(files)
        self.files = files
        self.h5, self.h4, self.h3, self.h2 = (P.Params.decode(R, d, *s) for d, s in zip(files[:4], SHAPES))
        self.g, st = E.decode(files[4])
        assert st == E.OK

    def commitment(self, randomness, secret_id, secret_value, rk):
        return self.h5.hash([randomness, secret_id, secret_value, rk[0], rk[1]])

    def item(self, utxo):
        return self.h4.hash(list(utxo))

    def nullifier(self, pak, item):
        return self.h3.hash([pak[0], pak[1], item])

    def viewing_key(self, pak):
        return rem_mod_l(self.h2.hash([pak[0], pak[1]]))[0]

    def receiving_key(self, vk):
        return E.mul(self.g, vk)

    def reconstruct(self, flag, plaintext, rk):
        """flag in (0, 1) -> the record"""
        rnd, aid, val = plaintext
        sid, sval, pid, pval = (0, 0, aid, val) if flag else (aid, val, 0, 0)
        return (flag, pid, pval, self.commitment(rnd, sid, sval, rk))

    def mint(self, rk, plaintext, flag):
        """-> (record or None, item or None, status)"""
        if flag not in (0, 1) or plaintext[2] >= U128:
            return None, None, BAD_ENCODING
        utxo = self.reconstruct(flag, plaintext, rk)
        return utxo, self.item(utxo), OK

    def open(self, rk, plaintext, utxo, pak=None):
        """rk = the address's receiving key -> (status, item or None, nullifier or None)"""
        flag = utxo[0]
        if flag not in (0, 1) or plaintext[2] >= U128 or utxo[2] >= U128:
            return BAD_ENCODING, None, None
        if self.reconstruct(flag, plaintext, rk) != tuple(utxo):
            return MISMATCH, None, None
        item = self.item(utxo)
        return OK, item, (None if pak is None else self.nullifier(pak, item))

"""The AES-GCM light notes on the GPU (mg_light_notes_encrypt / mg_light_notes_open): one JSON line, also written to
profiles/light_note_bench.json.

  seal_2^16 / _2^20      light notes sealed per second end to end (host arrays in and out), with and without the ephemeral keys
  open_2^16 / _2^20      light notes opened per second end to end, every note the wallet's own
  scan_2^20              mg_light_notes_open over a ledger-like batch in which 1 / 256 of the partition bytes are the wallet's,
                         against the same batch with partitions = NULL (every lane through the key agreement)
  composition_2^12       what a caller had before: mg_edwards_mul (shared scalar), mg_edwards_encode, then per note hashlib's
                         Blake2s and the host mg_aes256_gcm, alternated in this process with mg_light_notes_open on the same
                         notes; `speedup` = its median over the new call's. The agreed points cross to the host in the old
                         route and stay on the device in the new one.

Every figure is the median of --reps calls after one warm-up call. No bar is set on any of them: parity with the model gates
the feature (tests/test_gpu_light_note.py), not a ratio.

    python tools/light_note_bench.py [--reps 5]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NONCE = b"random nonce"


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def median_ms(fn, reps):
    fn()
    return statistics.median(timed(fn) for _ in range(reps))


def rate(n, ms):
    return {"ms": round(ms, 3), "per_s": round(n / ms * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from manta_rs_amd import api, synth
    import edwards_ref as E
    import utxo_ref as U

    api.init(0)
    model = api.UtxoModel(*[U.read(n) for n in U.FILES])
    rng = np.random.default_rng(2027)
    out = {"tool": "light_note_bench", "reps": a.reps, "curve": "ed_on_bn254", "chunk": api.EDWARDS_CHUNK}

    def scalars(n):
        s = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        s[:, 3] &= np.uint64((1 << 58) - 1)
        s[:, 3] |= np.uint64(1 << 57)  # 250 bits, below l
        return s

    def plaintexts(n):
        pt = rng.integers(0, 1 << 64, size=(n, 3, 4), dtype=np.uint64)
        pt[..., 3] &= np.uint64((1 << 60) - 1)  # reduced Montgomery words
        value = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64) * np.array([1, 1, 0, 0], dtype=np.uint64)
        pt[:, 2] = api.field_op("bn254_fr", "from_canonical", np.ascontiguousarray(value))  # a u128
        return pt

    vk = scalars(1)
    g = synth.to_mont(list(E.generator()), E.R, 4).reshape(1, 8)
    g_vk = api.edwards_mul(api.EDWARDS_MUL_FIXED_BASE, g, vk)  # the wallet's receiving key
    notes = {}
    for lg in (16, 20):
        n = 1 << lg
        keys = np.ascontiguousarray(np.broadcast_to(g_vk, (n, 8)))
        rnd, pt = scalars(n), plaintexts(n)
        seal_ms = median_ms(lambda: model.light_encrypt(keys, rnd, pt), a.reps)
        seal_no_epk_ms = median_ms(lambda: model.light_encrypt(keys, rnd, pt, epks=False), a.reps)
        epk, ct, st = model.light_encrypt(keys, rnd, pt)
        assert not st.any()
        open_ms = median_ms(lambda: model.light_open(vk[0], epk, ct), a.reps)
        got, ok, _, tried = model.light_open(vk[0], epk, ct)
        assert ok.all() and (got == pt).all() and tried == n
        out[f"seal_2^{lg}"] = dict(rate(n, seal_ms), without_epk=rate(n, seal_no_epk_ms))
        out[f"open_2^{lg}"] = rate(n, open_ms)
        notes[lg] = (epk, ct, pt)

    # the scan: 1 / 256 of the ledger carries the wallet's byte
    n = 1 << 20
    epk, ct, pt = notes[20]
    mine = int(model.address_partitions(g_vk)[0])
    parts = rng.integers(1, 256, size=n, dtype=np.uint64).astype(np.uint8)
    parts = ((parts.astype(np.uint16) + mine) % 256).astype(np.uint8)  # never the wallet's byte ...
    parts[::256] = mine  # ... but on every 256th lane
    scan_ms = median_ms(lambda: model.light_open(vk[0], epk, ct, partitions=parts), a.reps)
    full_ms = median_ms(lambda: model.light_open(vk[0], epk, ct), a.reps)
    got, ok, st, tried = model.light_open(vk[0], epk, ct, partitions=parts)
    assert tried == n // 256 and ok.sum() == tried and (got[::256] == pt[::256]).all() and (st[1::256] == api.NOTE_OTHER_PARTITION).all()
    out["scan_2^20"] = {"matching": tried, "with_partitions": rate(n, scan_ms), "partitions_null": rate(n, full_ms),
                        "speedup": round(full_ms / scan_ms, 1)}

    # the composition a caller had before, at 2^12, alternated with the new call
    n = 1 << 12
    epk, ct, pt = (x[:n] for x in notes[16])

    def composed():
        agreed = api.edwards_mul(api.EDWARDS_MUL_SHARED_SCALAR, epk, vk)
        enc = api.edwards_encode(agreed)
        res = []
        for i in range(n):
            key = hashlib.blake2s(enc[32 * i:32 * i + 32]).digest()
            res.append(api.aes256_gcm_decrypt(key, NONCE, ct[i].tobytes()))
        return res

    want = composed()
    got, ok, _, _ = model.light_open(vk[0], epk, ct)
    canon = api.field_op("bn254_fr", "to_canonical", np.ascontiguousarray(got.reshape(-1, 4))).reshape(n, 3, 4)
    for i in range(0, n, 97):
        body, good = want[i]
        assert good and ok[i] and body == canon[i, 0].tobytes() + canon[i, 1].tobytes() + canon[i, 2, :2].tobytes(), i
    old, new = [], []
    for _ in range(a.reps):
        old.append(timed(composed))
        new.append(timed(lambda: model.light_open(vk[0], epk, ct)))
    om, nm = statistics.median(old), statistics.median(new)
    out["composition_2^12"] = {"route": "mg_edwards_mul + mg_edwards_encode + hashlib blake2s + host mg_aes256_gcm per note",
                               "ms": round(om, 1), "per_s": round(n / om * 1e3), "mg_light_notes_open_ms": round(nm, 3),
                               "speedup": round(om / nm, 1)}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "light_note_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

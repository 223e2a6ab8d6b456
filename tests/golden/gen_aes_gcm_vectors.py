"""Writes tests/golden/aes_gcm_vectors.json: AES-256-GCM vectors (12-byte nonce, no associated data, 16-byte tag) computed by
OpenSSL's libcrypto (EVP_aes_256_gcm) through ctypes. The tests read only the JSON, so they need no OpenSSL. Deterministic:
keys, nonces and plaintexts come from random.Random(20241); run `python tests/golden/gen_aes_gcm_vectors.py` to rewrite the file.

40 vectors: every plaintext length of 0, 1, 15, 16, 17, 48, 80, 96 with five keys each; the first three of each length under
manta-pay's fixed nonce b"random nonce", the other two under random nonces."""
import ctypes
import ctypes.util
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (0, 1, 15, 16, 17, 48, 80, 96)
FIXED_NONCE = b"random nonce"
EVP_CTRL_GCM_GET_TAG = 0x10


def openssl_seal(lib, key, nonce, plaintext):
    ctx = lib.EVP_CIPHER_CTX_new()
    assert ctx
    try:
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_aes_256_gcm(), None, key, nonce) == 1  # the default IV length is 12
        out, n = ctypes.create_string_buffer(len(plaintext) + 16), ctypes.c_int(0)
        assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), plaintext, len(plaintext)) == 1
        done = n.value
        assert lib.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, done), ctypes.byref(n)) == 1
        done += n.value
        assert done == len(plaintext)
        tag = ctypes.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        return out.raw[:done] + tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def main():
    lib = ctypes.CDLL(ctypes.util.find_library("crypto"))
    lib.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
    lib.EVP_aes_256_gcm.restype = ctypes.c_void_p
    lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
    lib.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    lib.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    lib.EVP_CIPHER_CTX_ctrl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.OpenSSL_version.restype = ctypes.c_char_p
    rng = random.Random(20241)
    vectors = []
    for length in LENGTHS:
        for k in range(5):
            key, nonce, pt = rng.randbytes(32), (FIXED_NONCE if k < 3 else rng.randbytes(12)), rng.randbytes(length)
            vectors.append({"key": key.hex(), "nonce": nonce.hex(), "plaintext": pt.hex(),
                            "sealed": openssl_seal(lib, key, nonce, pt).hex()})
    # NIST's GCM test cases 13 and 14 (all-zero key and nonce; empty and one zero block), as a check of this script itself
    assert openssl_seal(lib, bytes(32), bytes(12), b"").hex() == "530f8afbc74536b9a963b4f1c4cb738b"
    assert openssl_seal(lib, bytes(32), bytes(12), bytes(16)).hex() == "cea7403d4d606b6e074ec5d3baf39d18d0d1c8a799996bf0265b98b5d48ab919"
    doc = {"source": "EVP_aes_256_gcm, " + lib.OpenSSL_version(0).decode(), "cipher": "AES-256-GCM, 12-byte nonce, no AAD, sealed = ciphertext | 16-byte tag",
           "vectors": vectors}
    with open(os.path.join(HERE, "aes_gcm_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(len(vectors), "vectors written")


if __name__ == "__main__":
    main()

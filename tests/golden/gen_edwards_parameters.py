"""Makes the parameters of manta-pay's embedded curve and note encryption travel with the tests:
    python tests/golden/gen_edwards_parameters.py <checkout of manta-parameters>
Copies group-generator.dat (32 bytes: the ark-ec 0.3 twisted Edwards encoding of the ed_on_bn254 generator manta-pay uses),
incoming-base-encryption-scheme.dat (8 712 bytes: the width-4 Poseidon permutation and `FixedEncryption::initial_state`) and
viewing-key-derivation-function.dat (a width-3 `Hasher`) byte for byte into tests/golden/manta_parameters/, and records their
BLAKE3 digests as manta-parameters/data.checkfile lists them in edwards_checkfile.json beside them. checkfile.json (the four
`Hasher` files of gen_manta_parameters.py) is left alone."""
import json, os, re, shutil, sys
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "manta_parameters")
FILES = {  # file: (bytes, what it is)
    "group-generator.dat": (32, "GroupGenerator: ed_on_bn254 affine point, ark-ec 0.3 twisted Edwards encoding (config/utxo.rs)"),
    "incoming-base-encryption-scheme.dat": (32 * (63 * 4 + 16) + 8 + 4 * 32, "IncomingBaseEncryptionScheme: FixedDuplexer<1, Poseidon3>: keys | MDS | u64 4 | initial state (config/utxo.rs:744-758)"),
    "viewing-key-derivation-function.dat": (32 * (63 * 3 + 9 + 1), "ViewingKeyDerivationFunction: Hasher<Poseidon2, .., 2> (config/utxo.rs:497-562)"),
}
check = {}
for line in open(f"{REF}/data.checkfile"):
    m = re.match(r"([0-9a-f]{64})\s+data/pay/parameters/(\S+)$", line.strip())
    if m:
        check[m.group(2)] = m.group(1)
meta = {}
for name, (size, what) in FILES.items():
    shutil.copyfile(f"{REF}/data/pay/parameters/{name}", f"{OUT}/{name}")
    assert os.path.getsize(f"{OUT}/{name}") == size, name
    meta[name] = {"blake3": check[name], "bytes": size, "what": what,
                  "source": f"manta-parameters/data/pay/parameters/{name}; digest: manta-parameters/data.checkfile"}
json.dump(meta, open(f"{OUT}/edwards_checkfile.json", "w"), indent=1)
print("ok")

"""Makes manta-pay's production Poseidon parameters travel (the GPU box has no reference checkout). Run in the build container:
    python tests/golden/gen_manta_parameters.py
Copies the four `Hasher` parameter files of manta-pay's UTXO model (manta-parameters/data/pay/parameters/*.dat, the manta
codec of `Hasher<Poseidon{2,3,4,5}, ..>`: round keys | MDS | domain tag, 32-byte elements) byte for byte into
tests/golden/manta_parameters/, and records their BLAKE3 digests as manta-parameters/data.checkfile lists them, with the width
and round counts manta-pay gives each (manta-pay/src/config/poseidon.rs:26-48), in checkfile.json beside them."""
import json, os, re, shutil
REF = "/root/reference/manta-parameters"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "manta_parameters")
FILES = {  # file: (width, full rounds, partial rounds, what it hashes)
    "utxo-accumulator-model.dat": (3, 8, 55, "UtxoAccumulatorModel: Merkle inner hash, Hasher<Poseidon2, InnerHashDomainTag, 2> (utxo.rs:1200-1248)"),
    "nullifier-commitment-scheme.dat": (4, 8, 55, "NullifierCommitmentScheme, Poseidon3 (utxo.rs:1374-1395)"),
    "utxo-accumulator-item-hash.dat": (5, 8, 56, "UtxoAccumulatorItemHash, Hasher<Poseidon4, .., 4> (utxo.rs:1062-1083)"),
    "utxo-commitment-scheme.dat": (6, 8, 56, "UtxoCommitmentScheme, Poseidon5 (utxo.rs:277-297)"),
}
check = {}
for line in open(f"{REF}/data.checkfile"):
    m = re.match(r"([0-9a-f]{64})\s+data/pay/parameters/(\S+)$", line.strip())
    if m:
        check[m.group(2)] = m.group(1)
os.makedirs(OUT, exist_ok=True)
meta = {}
for name, (w, f, p, what) in FILES.items():
    shutil.copyfile(f"{REF}/data/pay/parameters/{name}", f"{OUT}/{name}")
    assert os.path.getsize(f"{OUT}/{name}") == 32 * ((f + p) * w + w * w + 1), name
    meta[name] = {"blake3": check[name], "width": w, "full_rounds": f, "partial_rounds": p, "hasher": what,
                  "source": f"manta-parameters/data/pay/parameters/{name}; digest: manta-parameters/data.checkfile"}
json.dump(meta, open(f"{OUT}/checkfile.json", "w"), indent=1)
print("ok")

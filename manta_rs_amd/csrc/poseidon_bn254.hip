// Poseidon and Merkle-tree kernels instantiated over the BN254 scalar field.
#include "poseidon.h"
namespace mg {
hipError_t poseidon_launch_bn254(const PoseidonLaunch &a) { return poseidon_launch<Bn254FrCfg>(a); }
} // namespace mg

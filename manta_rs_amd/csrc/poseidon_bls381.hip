// Poseidon and Merkle-tree kernels instantiated over the BLS12-381 scalar field.
#include "poseidon.h"
namespace mg {
hipError_t poseidon_launch_bls381(const PoseidonLaunch &a) { return poseidon_launch<Bls381FrCfg>(a); }
} // namespace mg

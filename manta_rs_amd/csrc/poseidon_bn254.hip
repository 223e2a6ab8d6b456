// Poseidon and Merkle-tree kernels instantiated over the BN254 scalar field.
#include "poseidon.h"
namespace mg {
template struct PoseidonKernels<Bn254FrCfg>;
} // namespace mg

// Poseidon and Merkle-tree kernels instantiated over the BLS12-381 scalar field.
#include "poseidon.h"
namespace mg {
template struct PoseidonKernels<Bls381FrCfg>;
} // namespace mg

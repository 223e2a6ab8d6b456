// Point codec instantiation: Bls381, G1 and G2 (arkworks format only: the Perpetual Powers of Tau files are over Bn254).
#include "point_codec.h"
namespace mg {
int point_codec_bls381(const PointCodecArgs &a) {
    if (a.format != 0) return MG_ERR_ARG;
    return point_codec_dispatch<Bls381, codec::Arkworks>(a);
}
} // namespace mg

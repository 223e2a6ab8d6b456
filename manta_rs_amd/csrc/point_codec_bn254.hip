// Point codec instantiation: Bn254, G1 and G2, in the arkworks format and in that of the Perpetual Powers of Tau files.
#include "point_codec.h"
namespace mg {
int point_codec_bn254(const PointCodecArgs &a) {
    if (a.format == 1) return point_codec_dispatch<Bn254, codec::Ppot>(a);
    return point_codec_dispatch<Bn254, codec::Arkworks>(a);
}
} // namespace mg

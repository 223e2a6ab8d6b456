// Point codec instantiation: Bls381, G1 and G2.
#include "point_codec.h"
namespace mg {
int point_codec_bls381(const PointCodecArgs &a) { return point_codec_dispatch<Bls381>(a); }
} // namespace mg

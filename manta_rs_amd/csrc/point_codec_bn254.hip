// Point codec instantiation: Bn254, G1 and G2.
#include "point_codec.h"
namespace mg {
int point_codec_bn254(const PointCodecArgs &a) { return point_codec_dispatch<Bn254>(a); }
} // namespace mg

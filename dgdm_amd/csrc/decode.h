// The constant tables of the finger-geometry decode (decode.hip) and the one expression every kernel that evaluates a decoded
// point uses, so that finger_mesh.hip's base ring / sheet is bit for bit what dgdm_finger_decode_2d / _3d write.
#pragma once
#include "common.h"

namespace dgdm {

struct DecodeTable {
    DevBuf mat;          // [npts][K] float: weights of the K control values
    DevBuf fixed;        // [npts][F] float: the coordinates that do not depend on the sample (2-D: x; 3-D: x, z)
    int npts = 0, K = 0;
};

// kind 2: K control values per finger, n spline points; kind 3: K = 21, n = sample_size (npts = n^2).  Built once per (kind, K, n)
// on the host in double precision, kept for the life of the process.
int decode_table(int kind, int K, int n, DecodeTable **out);

// y of one decoded point: sum_k m[k] (scale s[k] + offset), one fmaf per term in k order
__device__ __forceinline__ float decode_y(const float *__restrict__ s, const float *__restrict__ m, int K, float scale, float offset) {
    float y = 0.f;
    for (int k = 0; k < K; ++k) y = fmaf(m[k], fmaf(scale, s[k], offset), y);
    return y;
}

}  // namespace dgdm

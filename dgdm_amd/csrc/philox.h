// Philox4x64-10 (Salmon et al., SC'11; the Random123 constants), one block of four 64-bit outputs: the one copy behind the mesh
// sampler (mesh.hip) and the scheduler step's keyed noise (smallnet.hip).  numpy's convention (numpy.random.Philox(key=[k0, k1],
// counter=[c0, c1, c2, c3]).random_raw()): the counter counts up BEFORE a block is made, so raw outputs 4b .. 4b + 3 of a stream are
// the block of counter (c0 + b + 1, c1, c2, c3) while c0 does not wrap.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace dgdm {

struct U64x4 { uint64_t v[4]; };

__host__ __device__ inline void mulhilo64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    *hi = __umul64hi(a, b);
#else
    *hi = (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
    *lo = a * b;
}

__host__ __device__ inline U64x4 philox4x64_10(U64x4 c, uint64_t k0, uint64_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        uint64_t hi0, lo0, hi1, lo1;
        mulhilo64(0xD2E7470EE14C6C93ull, c.v[0], &hi0, &lo0);
        mulhilo64(0xCA5A826395121157ull, c.v[2], &hi1, &lo1);
        c = U64x4{{hi1 ^ c.v[1] ^ k0, lo1, hi0 ^ c.v[3] ^ k1, lo0}};
    }
    return c;
}

}  // namespace dgdm

// within_cluster_dev.hpp -- the staged row scores of the fixed-effects regression's errors clustered on ANY key (within_cluster.hip):
// how a row's score x~_i e_i lies in memory, once, for the kernel that writes it and the kernel that gathers it.
//
// The scores are staged ROW-MAJOR: row r holds its P entries at rows[r * cluster_row_stride(P)], padded to an even count, so a row
// starts on a 16-byte boundary and moves as two-double words.  A gathered row is then 1 - 3 cache lines instead of the P + 1 lines the
// column-major frame would cost (the access pattern of w2_chunk2_kernel on the row-major f64 copy).
#pragma once
#include "wave_tile_dev.hpp"

namespace pds {

typedef double d2 __attribute__((ext_vector_type(2)));

// v[0 .. P) -> the staged row r (the padding entry of an odd P is written as 0.0: a gathered row reads it)
template <int P>
__device__ __forceinline__ void cluster_row_store(double* __restrict__ rows, int64_t r, const double* v) {
    constexpr int PS = cluster_row_stride(P);
    d2* out = reinterpret_cast<d2*>(rows + r * PS);
#pragma unroll
    for (int c = 0; c < PS; c += 2) {
        d2 t;
        t.x = v[c];
        t.y = c + 1 < P ? v[c + 1] : 0.0;
        out[c >> 1] = t;
    }
}

// the staged row r -> v[0 .. cluster_row_stride(P)): the loads are issued back to back
template <int P>
__device__ __forceinline__ void cluster_row_load(gptr<double> rows, int64_t r, double* v) {
    constexpr int PS = cluster_row_stride(P);
    const gptr<d2> in = (gptr<d2>)(rows + r * PS);
#pragma unroll
    for (int c = 0; c < PS; c += 2) {
        const d2 t = in[c >> 1];
        v[c] = t.x;
        v[c + 1] = t.y;
    }
}

}  // namespace pds

// wave_tile_dev.hpp -- the wave-tile Gram idiom of the per-group f64 kernels (grouped_irls.hip, mixed.hip, grouped_report_pass.hip), once.
//
// One wave owns a group (or a piece of one), lane = row.  64 rows per step are written into a wave-private LDS tile, feature-major
// ([f * stride + row]), and fed to v_mfma_f64_16x16x4 four rows at a time: lane (f = lane & 15, kq = lane >> 4) supplies feature f of
// row 4 m + kq as the A and the B operand.  Operands (s x, x) give the 16 x 16 block sum_r s_r x_r x_r'; a second instruction with
// operands (x, [side columns]) gives the right-hand sides sum_r x_r b_r' in the first columns of a second accumulator.  Scalar sums
// are per-lane registers folded by wave_sum().  Nothing here owns LDS or synchronises: the carving of the tile, its stride, which
// rows are resident and where PDS_WAVE_LDS_SYNC() goes are the kernels' decisions.
#pragma once
#include "common.hpp"

#include <type_traits>

namespace pds {

typedef double d4 __attribute__((ext_vector_type(4)));  // the four D registers of a lane

// sum over the wave in a fixed order (no atomics: repeated calls give the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return __shfl(v, 0, 64);  // (lane 0's order for every lane)
}

// Doubles per feature row of a tile of `rows` row slots (a multiple of 32): rows + 2, = 2 (mod 32).  An operand read is a
// ds_read_b64, served in two groups of 32 lanes with the bank pair = (index in doubles) mod 32.  A group holds the 16 features of
// two adjacent kq, at f * stride + kq + const = 2 f + kq (mod 32): 32 different bank pairs, no conflict.  (A stride = 1 (mod 32)
// makes the lane = row column writes conflict-free as well as this one does, but its operand reads collide two by two.)
constexpr int wave_tile_stride(int rows) { return rows + 2; }

struct TileNoScale {};  // A operand = x: no multiply
struct TileNoSide {};   // no second accumulator: no second matrix instruction

// The matrix-instruction loop over the `rows` live rows of a step (steps of 4; rows past `rows` in the last step hold zeros).
// tile: the step's first row slot of feature 0; operand rows f >= P read as 0.0.
//   scale(row)        the A-side factor s of a row, or TileNoScale
//   side(f, row, s)   the B operand of the second accumulator (column f of the side block; s = scale(row), already loaded), or
//   side(f, row)      with TileNoScale, or TileNoSide (acc2 is then not touched)
template <int P, typename Scale, typename Side>
__device__ __forceinline__ void wave_tile_gram(const double* tile, int stride, int rows, int lane, Scale scale, Side side, d4& acc,
                                               d4& acc2) {
    constexpr bool kSide = !std::is_same_v<Side, TileNoSide>;
    const int f = lane & 15, kq = lane >> 4;
    const int steps = (rows + 3) >> 2;
    for (int m = 0; m < steps; ++m) {
        const int row = 4 * m + kq;
        const double xv = f < P ? tile[f * stride + row] : 0.0;
        double av = xv, bv = 0.0;
        if constexpr (std::is_same_v<Scale, TileNoScale>) {
            if constexpr (kSide) bv = side(f, row);
        } else {
            const double s = scale(row);
            av = s * xv;
            if constexpr (kSide) bv = side(f, row, s);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, xv, acc, 0, 0, 0);
        if constexpr (kSide) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, bv, acc2, 0, 0, 0);
    }
}

// the 16 x 16 block alone
template <int P, typename Scale>
__device__ __forceinline__ void wave_tile_gram(const double* tile, int stride, int rows, int lane, Scale scale, d4& acc) {
    d4 none = {0.0, 0.0, 0.0, 0.0};  // (never touched)
    wave_tile_gram<P>(tile, stride, rows, lane, scale, TileNoSide{}, acc, none);
}

// D layout of v_mfma_f64_16x16x4: col = lane & 15, row = (lane >> 4) + 4 reg.  fn(row, col, value...) for the lane's four
// entries of each of the accumulators given (by value: they stay registers).
template <typename F, typename... Acc>
__device__ __forceinline__ void wave_tile_for_d(int lane, F&& fn, Acc... acc) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) fn((lane >> 4) + 4 * reg, lane & 15, acc[reg]...);
}

}  // namespace pds

// score_meat_dev.hpp -- the score / meat idiom of the one-pass robust-error kernels (cluster_meat.hip, within_pass.hip), once.
//
// A wave streams the rows of a cluster 64 per step through a wave-private LDS tile (the wave-tile idiom of wave_tile_dev.hpp:
// feature-major, row stride kScoreTileStride, the residual e behind the features).  The cluster's score s = sum_i x_i e_i comes from
// one v_mfma_f64_16x16x4 per four rows with operands (x, [e | 0 ..]) (score_tile_step).  The meat M = sum_g s_g s_g' is S'S with the
// CLUSTER as the K dimension: a finished score is parked in LDS (kScoreBatch slots of kScorePark doubles); every four clusters one
// matrix instruction with operands (s, s) adds their outer products to the 16 x 16 feature block (ScoreMeat).  sum e^2 is a
// compensated sum (value + error term, two-sum at every level: lane, butterfly, records): r2 = 1 - sum e^2 / (n var y) magnifies the
// sum's last bits by (1 - r2) / r2.  The wave writes ONE record in the layout of common.hpp (kMixedRecStride).
//
// HAS_BIAS says whether a bias entry exists AT ALL: with it the score has a 17th entry sum e, the meat a bias column (a second matrix
// instruction with B = [s_bias | 0 ..]) and a bias diagonal, and whether this call uses them is ScoreMeat::bias at run time.  Without
// it none of that is formed, kept in registers or written (a centred score's bias entry is sum e = 0).
// Which slots are zeroed, the two-sum order and the chunk order decide the "two calls give equal bits" and "empty groups change no
// bit" guarantees of both callers: this is the only copy.  Nothing here uses a floating-point atomic.
#pragma once
#include "wave_tile_dev.hpp"

#include <algorithm>

namespace pds {

constexpr int kScoreTileStride = wave_tile_stride(64);  // doubles per feature row of the tile: 64 rows per step
constexpr int kScorePark = kClusterScoreStride;         // doubles per parked score: 16 features, the bias entry, one of padding
constexpr int kScoreBatch = 4;                          // scores per outer-product instruction: its K dimension

// the record slots of common.hpp's layout the passes fill besides the 16 x 16 feature block: the bias column, sum e^2 and its error
// term, the bias diagonal
constexpr int kScoreRecBias = kMixedRecXY, kScoreRecEE = kMixedRecYY, kScoreRecEC = kMixedRecCY, kScoreRecBB = kMixedRecC;

// s + v exactly: the rounded sum in s, its error added to c (Knuth's two-sum: no branch, any magnitudes)
__device__ __forceinline__ void two_sum(double& s, double& c, double v) {
    const double t = s + v;
    const double bb = t - s;
    c += (s - (t - bb)) + (v - bb);
    s = t;
}

// sum e^2 as value + error term
struct CompSq {
    double s = 0.0, c = 0.0;
    __device__ __forceinline__ void add(double e) {
        const double q = e * e;
        c += fma(e, e, -q);  // (the product's own rounding error)
        two_sum(s, c, q);
    }
    // the butterfly of wave_sum() on (value, error term) pairs: lane 0 ends with the wave's sum
    __device__ __forceinline__ void wave_fold() {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double so = __shfl_xor(s, o, 64), co = __shfl_xor(c, o, 64);
            c += co;
            two_sum(s, c, so);
        }
    }
};

// a score in the D layout of the side block (column 0: entry (lane >> 4) + 4 reg in the lanes with lane & 15 == 0) and its bias entry
// sb (wave-uniform; 0 without one) -> the kScorePark doubles at `out` (a park slot or a row of the chunk scores)
__device__ __forceinline__ void score_store_d(double* out, int lane, const d4& sc, double sb) {
    if ((lane & 15) == 0) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(lane >> 4) + 4 * reg] = sc[reg];
    }
    if (lane == 0) out[16] = sb, out[17] = 0.0;
}

// four rows of a step's tile (features 0 .. P - 1, then e, at xt[c * kScoreTileStride + row]) -> the score sc: ONE matrix instruction
// with operands (x, [e | 0 ..]).  The lane (f = lane & 15, kq = lane >> 4) supplies feature f of `row` = 4 m + kq; a caller walks
// m over the (rows + 3) / 4 steps of its live rows (the row slots past them hold zeros).
template <int P>
__device__ __forceinline__ void score_rows4(const double* xt, int row, int f, d4& sc) {
    const double xv = f < P ? xt[f * kScoreTileStride + row] : 0.0;
    const double bv = f == 0 ? xt[P * kScoreTileStride + row] : 0.0;
    sc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, bv, sc, 0, 0, 0);
}

// the meat a wave carries across its clusters, and the batch of parked scores in front of it (park: kScoreBatch * kScorePark doubles
// of LDS)
template <bool HAS_BIAS>
struct ScoreMeat {
    d4 m = {0.0, 0.0, 0.0, 0.0};   // the 16 x 16 feature block (D layout)
    d4 mb = {0.0, 0.0, 0.0, 0.0};  // HAS_BIAS: column 0 is the bias column
    double bb = 0.0;               // HAS_BIAS: the bias diagonal (wave-uniform)
    int bias = 0;                  // HAS_BIAS: this call has a bias (wave-uniform)
    int parked = 0;                // scores in the park (wave-uniform)

    // the parked scores -> the meat; slots [parked, kScoreBatch) are zeroed first
    __device__ __forceinline__ void flush(double* park, int lane) {
        if (parked == 0) return;
        for (int k = parked; k < kScoreBatch; ++k)
            if (lane < kScorePark) park[k * kScorePark + lane] = 0.0;
        PDS_WAVE_LDS_SYNC();
        const int f = lane & 15, kq = lane >> 4;
        const double sv = park[kq * kScorePark + f];
        m = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, sv, m, 0, 0, 0);
        if constexpr (HAS_BIAS) {
            if (bias) {
                const double bv = f == 0 ? park[kq * kScorePark + 16] : 0.0;
                mb = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, bv, mb, 0, 0, 0);
            }
        }
        PDS_WAVE_LDS_SYNC();  // (the operand reads are done before the next score is parked)
        parked = 0;
    }

    // the score in the next park slot (its bias entry: sb) is complete; a full park is flushed
    __device__ __forceinline__ void parked_one(double* park, int lane, double sb) {
        if constexpr (HAS_BIAS) bb = fma(sb, sb, bb);
        if (++parked == kScoreBatch) flush(park, lane);
    }

    // a finished score in D layout (score_store_d) -> the park
    __device__ __forceinline__ void park_d(double* park, int lane, const d4& sc, double sb = 0.0) {
        score_store_d(park + parked * kScorePark, lane, sc, sb);
        parked_one(park, lane, sb);
    }

    // the wave's record: the feature block, with HAS_BIAS the bias column and diagonal, sum e^2 and its error term
    __device__ __forceinline__ void write_record(double* rec, int lane, CompSq ee) const {
        if constexpr (HAS_BIAS) {
            wave_tile_for_d(
                lane,
                [&](int i, int c, double w, double side) {
                    rec[kMixedRecW + i * 16 + c] = w;
                    if (c == 0) rec[kScoreRecBias + i] = side;
                },
                m, mb);
        } else {
            wave_tile_for_d(lane, [&](int i, int c, double w) { rec[kMixedRecW + i * 16 + c] = w; }, m);
        }
        ee.wave_fold();
        const double es = __shfl(ee.s, 0, 64), ec = __shfl(ee.c, 0, 64);  // (lane 0's order for the record)
        // the slots the pass does not use: the record sum reads all of them
        constexpr int first = HAS_BIAS ? kMixedRecCM : kMixedRecXY;
        if (lane < kMixedRecStride - first) {
            const int slot = first + lane;
            rec[slot] = slot == kScoreRecEE ? es : (slot == kScoreRecEC ? ec : (HAS_BIAS && slot == kScoreRecBB ? bb : 0.0));
        }
    }
};

// one wave walks the long clusters (grid stride): the chunk scores (n_chunks x kScorePark) added in chunk order, lane = entry, then
// parked and multiplied like any other score; one record per wave.  Bias: `int` with HAS_BIAS (ScoreMeat::bias), nothing without --
// the kernel then has no such argument.
template <bool HAS_BIAS, typename... Bias>
__global__ __launch_bounds__(64) void score_long_meat_kernel(const int64_t* __restrict__ long_c0, const int64_t* __restrict__ long_nc,
                                                             int64_t n_long, const double* __restrict__ scores, Bias... bias,
                                                             double* __restrict__ partials) {
    static_assert(sizeof...(Bias) == (HAS_BIAS ? 1 : 0), "a bias argument exactly when there is a bias entry");
    __shared__ double park[kScoreBatch * kScorePark];
    const int lane = threadIdx.x;
    ScoreMeat<HAS_BIAS> mt;
    if constexpr (HAS_BIAS) mt.bias = (bias, ...);
    for (int64_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const int64_t c0 = long_c0[j], nc = long_nc[j];
        double s = 0.0;
        if (lane < kScorePark)
            for (int64_t k = 0; k < nc; ++k) s += scores[(c0 + k) * kScorePark + lane];
        const double sb = __shfl(s, 16, 64);
        if (lane < kScorePark) park[mt.parked * kScorePark + lane] = s;
        mt.parked_one(park, lane, sb);
    }
    mt.flush(park, lane);
    mt.write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, CompSq{});
}

}  // namespace pds

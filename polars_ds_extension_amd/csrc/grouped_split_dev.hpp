// grouped_split_dev.hpp -- how the fused grouped kernel (grouped_fused.hip) deals the frame's rows to its waves: ONE definition,
// used by the kernel, by its launcher and by pds_grouped_fused_split (the host restatement the CPU tests check).
//
// Wave w of W owns the groups whose first row lies in [row(w), row(w + 1)) of the frame's row range; row() is monotone with
// row(0) = 0 and row(W) = total, so the waves partition the groups whatever the shares are.
//
// The shares are NOT equal when the grid fills the device.  The kernel runs two one-wave blocks per SIMD; the dispatcher places
// blocks [0, W/2) first, one per SIMD, and blocks [W/2, W) beside them as each SIMD's second -- younger -- wave.  The SIMD issues
// the older wave first, so the younger one advances more slowly as long as both are resident: with equal shares the first
// half of the grid ended after 2076 us and the second half after 2353 us of a 2460 us launch (1134 / 1280 of 1306 us at 8
// features; profiles/fused_tail_parent.txt), 10 % of all wave-slot time stood idle behind the slow half.  `late_permille` is the
// share of the rows, in 1/1000, that goes to the second half of the grid; 0 = equal shares by the plain w total / W rule.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDS_HD __host__ __device__
#else
#define PDS_HD
#endif

namespace pds {

// share of the rows given to the second half of a device-filling grid (blocks [W - W/2, W)): chosen by A/B among 500 ... 430 on three frames,
// profiles/fused_tail_ab.txt
constexpr int kFusedLatePermille = 455;

// first row (relative to offsets[0]) of wave w's range, 0 <= w <= W; total = rows of the frame
PDS_HD inline int64_t fused_split_row(int64_t w, int64_t W, int64_t total, int late_permille) {
    const int64_t H = W / 2;  // waves of the second half
    if (late_permille <= 0 || late_permille >= 1000 || H == 0) return (total * w) / W;
    const int64_t E = W - H;  // waves of the first half
    const int64_t late_rows = (total / 1000) * late_permille + ((total % 1000) * late_permille) / 1000;
    const int64_t early_rows = total - late_rows;
    if (w <= E) return (early_rows * w) / E;
    return early_rows + (late_rows * (w - E)) / H;
}

// the launcher's rule: the unequal shares apply to a grid that fills every wave slot of the device (`slots`, an even number of
// waves per SIMD) -- only then is the second half of the grid the set of younger waves.  `opt` is the context option
// "grouped_fused_late_permille" (1 .. 999 forces a share on any grid of two or more waves: tests, A/B runs).
inline int fused_late_permille(int64_t waves, int64_t slots, int64_t opt) {
    if (waves < 2) return 0;
    if (opt >= 1 && opt <= 999) return (int)opt;
    return (waves == slots && slots % 2 == 0) ? kFusedLatePermille : 0;
}

}  // namespace pds

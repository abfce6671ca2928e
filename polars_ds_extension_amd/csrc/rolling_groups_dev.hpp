// rolling_groups_dev.hpp -- group boundaries of the grouped rolling / expanding fits (pds_rolling_lr_grouped_*,
// pds_recursive_lr_grouped_*).  The one source of boundaries is the int64 offsets array (G + 1 entries, group g = rows
// [off[g], off[g+1]), empty groups allowed); there is no per-row group-id stream.  A wave finds the group of its first row by
// a binary search once per tile, then walks the offsets forward with its rows: per stage one coalesced load of the next 64
// offsets (a ballot counts the groups that start inside the stage), and a lane's own rows search only the groups the stage
// spans -- none or one for groups longer than a stage.  All of it is integer work: the FP64 unit that bounds the rolling
// kernels does not see it.
#pragma once
#include <cstdint>

namespace pds {

struct RollGroups {
    const int64_t* off;  // G + 1 offsets, device resident (nullptr: the ungrouped fit)
    int64_t ng;          // G
    uint8_t* tile_flag;  // expanding totals pass: 1 where a group starts inside the tile / segment
};

// the group of row r: the largest g in [lo, hi] with off[g] <= r (off[lo] <= r is required; empty groups share an offset
// with the group after them, which is the one returned)
__device__ __forceinline__ int64_t grp_find(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t r) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// wave-uniform (all 64 lanes): the group of row r >= off[g].  One coalesced load of the next 64 offsets settles the common case
// (fewer than 64 groups start in (off[g], r]); past that -- short or many empty groups -- a binary search over the rest, so the
// cost stays O(log G) however many empty groups lie in between
__device__ __forceinline__ int64_t grp_advance(const int64_t* __restrict__ off, int64_t ng, int64_t g, int64_t r) {
    const int lane = threadIdx.x & 63;
    const int64_t j = g + 1 + lane;
    const bool le = j < ng && off[j] <= r;
    const int c = __popcll(__ballot(le));  // offsets are monotone: the lanes that pass are a prefix
    return c < 64 ? g + c : grp_find(off, g + 64, ng - 1, r);
}

}  // namespace pds

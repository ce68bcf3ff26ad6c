// "The n smallest hash keys of a short row", shared by dr_neighbor_sample's one-wave rows and dr_mlm_mask: the row's 32-bit hashes lie
// in LDS, a key is (hash, index) compared lexicographically -- the 64-bit value (hash << 32 | index) -- and every lane ranks its own
// entries against all of them.  Exactly n keys rank below n, so the takers write themselves out in ascending index with one ballot
// per 64 entries.  Integer only: the result is a function of the hashes alone.
#pragma once
#include "dr_common.h"

// the lanes of a wave below `lane` as a ballot mask
__device__ __forceinline__ uint64_t dr_lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// how many of the keys (h[k], k), k < d, lie below (hj, j): the hash decides, the index breaks a tie
__device__ __forceinline__ int dr_key_rank(const uint32_t* __restrict__ h, int d, uint32_t hj, int j) {
    int rank = 0;
    for (int k = 0; k < d; ++k) {
        const uint32_t hk = h[k];
        rank += (hk < hj || (hk == hj && k < j)) ? 1 : 0;
    }
    return rank;
}

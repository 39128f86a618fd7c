// The failing-link rule of dl_drop_rounds and dl_link_mask (include/dlamd.h), defined once for the
// kernel (mix_drop.hip) and the host (launch.cpp): a counter-based hash of (seed, round, link),
// all arithmetic uint32 modulo 2^32.  Plain C++, no HIP types.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DL_HASH_FN __host__ __device__ inline
#else
#define DL_HASH_FN inline
#endif

namespace dl {

DL_HASH_FN uint32_t link_fmix(uint32_t a) {
    a ^= a >> 16;
    a *= 0x85EBCA6Bu;
    a ^= a >> 13;
    a *= 0xC2B2AE35u;
    a ^= a >> 16;
    return a;
}

// the part of the hash every link of round t shares (uniform: a scalar register in the kernel)
DL_HASH_FN uint32_t link_round_key(uint32_t seed, uint32_t t) {
    return link_fmix(seed + 0x9E3779B9u * (t + 1u));
}

// u(seed, t, lo, hi) from the round key
DL_HASH_FN uint32_t link_u(uint32_t key, uint32_t lo, uint32_t hi) {
    return link_fmix(link_fmix(key ^ lo) ^ hi);
}

// Is the CSR entry (row i, column j) of round `key` down?  An entry on the diagonal never is; a
// link {i, j} is when its own draw or either end's is below the threshold (0: never).
DL_HASH_FN bool link_down(uint32_t key, uint32_t i, uint32_t j, uint32_t thr_edge,
                          uint32_t thr_node) {
    if (i == j) return false;
    const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
    bool down = link_u(key, lo, hi) < thr_edge;
    if (thr_node != 0u)
        down = down || link_u(key, i, i) < thr_node || link_u(key, j, j) < thr_node;
    return down;
}

}  // namespace dl

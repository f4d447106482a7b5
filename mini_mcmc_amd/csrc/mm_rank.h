/*
 * mm_rank.h -- what the rank diagnostics (mm_rank.hip) share between device and host code.
 *
 * Sort keys: the f32 bit pattern mapped to a uint32 whose unsigned order is the order of the floats, -0.0 and +0.0 equal
 * (Vehtari et al. 2021 rank all draws of a parameter; ties share the average rank, so equal VALUES must give equal keys):
 *   -0.0 -> +0.0, then negative numbers: all bits flipped, the others: sign bit set.
 * -inf < negative normals < negative denormals < 0 < positive denormals < ... < +inf; NaNs land at either end and are
 * flagged instead of ranked.  Integer tests only: no float compare that a flush-to-zero mode could change.
 */
#ifndef MM_RANK_H
#define MM_RANK_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_RANK_HD __host__ __device__ inline
#else
#define MM_RANK_HD inline
#endif

MM_RANK_HD uint32_t mm_rank_key_of_bits(uint32_t bits)
{
    if ((bits << 1) == 0u)
        bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

MM_RANK_HD uint32_t mm_rank_bits_of_key(uint32_t key)
{
    return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
}

MM_RANK_HD bool mm_rank_bits_are_nan(uint32_t bits)
{
    return (bits & 0x7fffffffu) > 0x7f800000u;
}

/* mm_stats.hip: the shape limits of mmcmc_split_rhat_mean_ess beyond n < 2^31 and dim < 2^16 (its residue transform's
 * bins), for entry points that run it on arrays of the same shape and must refuse before they allocate */
bool mm_stats_shape_fits(size_t n, size_t dim);

#endif

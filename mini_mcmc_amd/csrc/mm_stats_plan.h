/* mm_stats_plan.h -- which kernels reduce a sample to the split-R-hat / ESS statistics (mm_stats.hip), with what grids, and
 * where each of them writes inside the device workspace: one record per call, made by one function from the shape, the
 * element type and the selector value the caller read ONCE (mmcmc_stats_set_kernel).  mm_stats_ws_floats, the size the entry
 * points give that workspace, stands next to the uses it has to cover.  Pure host functions: no HIP include and no
 * environment, so tests/cpp/stats_plan.cpp walks them with a plain C++17 compiler (every block inside the workspace under
 * every selector, grids within the launch limits, ...), and tests/cpp/stats_launch_trace.cpp pins what mm_stats.hip launches
 * from a plan.  Internal linkage: nothing here joins the library's exported symbols.
 *
 * The counts chosen here (n_wg, n_slabs, parts, the "256 compute units' worth" constants) fix which terms a wave sums in f32:
 * they are part of the numerical result, the same on every device, and why R-hat / ESS are the same bits everywhere. */
#ifndef MM_STATS_PLAN_H
#define MM_STATS_PLAN_H

#include "../../include/mmcmc.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

/* the measurement-only knobs (mm_tuning.h), read by mm_stats.hip and handed in as numbers */
struct mm_stats_knobs {
    int fft_nwg_percent = 100; /* MMCMC_FFT_NWG_MULT: workgroups of the short transform per resident slot, in percent */
    int waves = 0;             /* MMCMC_STATS_WAVES: waves (= slabs) of the direct kernels, and no cap of a path's own; 0: not set,
                                  4096 and the caps (a variable set to 0 arrives as 4096: set, and the default count) */
};

constexpr size_t kStatsLongMaxM = 131072; /* N = 2^18: the inverse (mm_fft_finish_long_kernel) is O(m N) per parameter */
constexpr size_t kStatsFftLdsCx = 72;     /* complex numbers of LDS per wave and R1: mm_fft_plan<R1>::LDS_CX / R1 (mm_stats_fft.h) */
/* LDS of a workgroup of mm_chain_fft_long_kernel: the spectrum S[4096] and the wave's exchange block */
constexpr size_t kStatsLongLds = ((size_t)4096 + 2 * 32 * kStatsFftLdsCx) * sizeof(float);
static_assert(kStatsLongLds <= 64 * 1024, "mm_chain_fft_long_kernel is launched without raising its dynamic LDS limit");
constexpr unsigned int kStatsWbChunks = 32;  /* MM_WB_CHUNKS: blocks per parameter of the tail kernel's cross-chain sums */

/* The transform paths count bins (dim x N, N = 2048 N1 up to 2^18 beyond 1024 draws per half-chain) in 32 bits: a shape
 * whose count would wrap is refused from the shape alone, whichever kernel is selected, before anything is allocated */
static inline bool stats_bins_fit(size_t n, size_t dim)
{
    const size_t m = n / 2;
    if (m <= 1024 || m > kStatsLongMaxM)
        return true; /* one wave-level transform (N <= 2048, dim < 2^16) or no transform at all */
    const uint64_t N = 2048ull * std::max<uint64_t>(2, (m + 1023) / 1024);
    return (uint64_t)dim * N < (1ull << 32);
}

/* MMCMC_ERR_SHAPE for a shape no path takes: what stats_partials_impl and both entry points answer before anything else
 * is looked at but their arguments */
static inline int mm_stats_shape_status(size_t n, size_t dim)
{
    return n / 2 < 1 || n >= (1ull << 31) || dim >= (1u << 16) || !stats_bins_fit(n, dim) ? MMCMC_ERR_SHAPE : MMCMC_OK;
}

/* tiles of 8 time steps x 16 lags of one parameter's (t, lag) triangle (the tile kernels' own count) */
static inline unsigned int stats_tile_count(size_t m)
{
    unsigned int n = 0;
    for (size_t kb = 0; 16 * kb < m; ++kb)
        n += (unsigned int)((m - 16 * kb + 7) / 8);
    return n;
}

/* number of waves (= per-wave lag-sum slabs) of the direct kernels before a path's own cap */
static inline unsigned int stats_n_slabs(size_t n_chains, const mm_stats_knobs &k)
{
    /* 4 waves per SIMD hide the LDS / global latencies of the half-chain loop; more only lengthens the slab reduction
     * (measured at [65536, 400, 3]: 1024 waves 1.65 ms, 2048 0.96, 4096 0.69 + 0.08, 8192 0.82 + 0.21) */
    return (unsigned int)std::min<size_t>(2 * n_chains, k.waves ? (size_t)k.waves : 4096);
}

enum mm_stats_path {
    MM_STATS_FFT,      /* mm_chain_fft_kernel<T, r1, dt, wpe, top> */
    MM_STATS_FFT_LONG, /* mm_chain_fft_long_kernel<T>: N1 = 2 */
    MM_STATS_FFT_RES,  /* mm_half_chain_means_kernel<T> (or the moments kernel), then mm_chain_fft_res_kernel<T, 32, 2, 1> */
    MM_STATS_TILE1,    /* mm_half_chain_tile1_kernel<T, tpl, npre>: one parameter per wave */
    MM_STATS_TILE,     /* mm_half_chain_tile_kernel<T, tpl, vec>: register tiles, all parameters */
    MM_STATS_MFMA,     /* mm_half_chain_mfma_kernel<T>: lag sums on the matrix cores */
    MM_STATS_LDS,      /* mm_half_chain_kernel<T>: the half-chain staged in LDS */
    MM_STATS_ANY       /* mm_half_chain_moments_any_kernel<T>, then mm_lag_sums_any_kernel<T>: from global memory, any length */
};

enum mm_stats_finish {
    MM_STATS_FINISH_NONE, /* the tail kernel's output is the result: n_parts partial totals [m, dim] */
    MM_STATS_FINISH_FFT,  /* mm_fft_finish_kernel: one inverse per parameter from the partial bin totals */
    MM_STATS_FINISH_LONG  /* mm_fft_psum_kernel (f64 bin totals into P), then mm_fft_finish_long_kernel */
};

struct mm_stats_launch {
    unsigned int gx = 0, gy = 1, gz = 1, block = 0; /* block = 0: no such launch */
    size_t lds = 0;                                 /* dynamic LDS bytes */
};

struct mm_stats_plan {
    int status; /* not MMCMC_OK: the call returns it and launches nothing */
    explicit mm_stats_plan(int st = MMCMC_OK) : status(st) {}
    mm_stats_path path = MM_STATS_ANY;
    /* which instance: r1 / dt / wpe / top (short transform), tpl / npre (tile1), tpl / vec (tile), moments (residues:
     * the means come from the moments kernel, dim > 16) */
    int r1 = 0, dt = 0, wpe = 0;
    bool top = false, vec = false, moments = false;
    unsigned int tpl = 0, npre = 0;
    /* the path's own number: n_pt (short transform), N1 (long transform and residues), parts (tile1), n_tiles (MFMA), m_pad (LDS) */
    unsigned int arg = 0;
    mm_stats_launch pre, first, tail, sum, finish; /* in this order; pre: means / moments; sum: mm_fft_psum_kernel */
    bool raise_lds = false;                        /* first.lds > 64 KB: hipFuncAttributeMaxDynamicSharedMemorySize first */
    unsigned int rows = 0, row_len = 0;            /* what the tail kernel sums: n_slabs x m, or n_wg x N */
    unsigned int nb_red = 0;                       /* its blocks that sum rows; the others are the cross-chain sums' */
    mm_stats_finish finish_kind = MM_STATS_FINISH_NONE;
    bool writes_total = false; /* the finish writes the total [m, dim]; otherwise the tail writes n_parts partial totals */
    /* blocks of the workspace, in floats: the first stage's rows (at 0), the transform paths' partial bin totals and their f64 sum */
    size_t len_slabs = 0, off_bins = 0, len_bins = 0, off_P = 0, len_P = 0;
    size_t ws_floats = 0; /* all it uses */
};

/* the power-spectrum path (mm_chain_fft_kernel), half-chains of 2 .. 1024 draws, as stats.rs:549 switches above 100: the
 * instance (r1, dt, wpe), arg = n_pt parameter tiles, rows = n_wg workgroups per tile of row_len = N bins per parameter */
static inline void stats_fft_geom(mm_stats_plan &p, size_t n_chains, size_t m, size_t dim, const mm_stats_knobs &k)
{
    p.r1 = m <= 256 ? 8 : m <= 512 ? 16 : 32;
    p.row_len = 64u * (unsigned int)p.r1;
    /* parameters per wave: as many as the registers hold without spilling (R1 = 8: 4 at two waves per SIMD, 3 at three;
     * R1 = 16: 3; R1 = 32: 1), the tiles of a larger dimension as even as possible */
    const size_t dt_max = p.r1 == 8 ? 4 : p.r1 == 16 ? 3 : 1;
    p.arg = (unsigned int)((dim + dt_max - 1) / dt_max);
    p.dt = (int)((dim + p.arg - 1) / p.arg);
    p.wpe = p.r1 == 8 && p.dt <= 3 ? 3 : 2;
    /* resident workgroups of four waves: waves per SIMD x CUs, shared between the parameter tiles.  The workgroup count
     * fixes which chains a wave sums in f32, so it must not depend on the device (CU count, partition mode): 256 compute
     * units' worth, an MI355X's, on every device */
    p.rows = std::max(1u, 256u * (unsigned int)p.wpe / p.arg);
    p.rows = std::max(1u, (unsigned int)((unsigned long long)p.rows * (unsigned int)k.fft_nwg_percent / 100u));
    p.rows = (unsigned int)std::min<size_t>(p.rows, (n_chains + 3) / 4);
}

/* the long-chain paths, half-chains of 1025 .. 2048 draws (mm_chain_fft_long_kernel, N1 = 2) and up to kStatsLongMaxM
 * (mm_chain_fft_res_kernel: one (residue, parameter) per wave, spectrum in registers, N1 >= 3): arg = N1, row_len = N =
 * 2048 N1 bins per parameter, rows = n_wg chain groups */
static inline void stats_long_geom(mm_stats_plan &p, size_t n_chains, size_t m, size_t dim)
{
    /* N >= 2 m, N1 the SMALLEST such count (not the next power of two: a residue wave reads the whole chain, so time goes
     * as N1 x the data: m = 10 000 took N1 = 16 where 10 do, [16384, 20000, 3] 20.7 -> 9.0 ms) */
    p.arg = (unsigned int)std::max<size_t>(2, (m + 1023) / 1024);
    p.row_len = 2048u * p.arg;
    size_t g = 512;
    if (p.arg >= 3) {
        /* chain groups: as many as keep ONE resident round of one-wave workgroups busy -- one per SIMD by their registers,
         * 1024 on an MI355X, N1 residues per parameter; a constant, not a device query, because the group count fixes the
         * f32 summation grouping -- in multiples of 8 (the kernel's XCD mapping), at most 512 */
        g = std::min<size_t>(512, std::max<size_t>(8, 1024 / (dim * p.arg) / 8 * 8));
    } else {
        /* at most 512 chain groups, and no more than fit the one-wave workgroups an MI355X holds at once with this kernel's
         * LDS (256 CUs x workgroups per CU: 1024; a launch of 1536 ran a second, half-empty round), a multiple of 8 */
        const size_t resident = 256 * std::max<size_t>(1, (160u << 10) / kStatsLongLds);
        if (g * dim > resident)
            g = std::max<size_t>(8, resident / dim / 8 * 8);
    }
    p.rows = (unsigned int)std::min<size_t>(g, n_chains); /* fewer for few chains */
}

/* Floats of device workspace a call with n_parts partial totals may use, WHICHEVER kernel is selected: a
 * mmcmc_stats_set_kernel() from another thread between an entry point's sizing and its call can change which kernel runs
 * but never make the buffer too small.  The three terms are the `ws_floats` of mm_stats_make_plan's three groups of paths:
 * the direct kernels (rows <= stats_n_slabs), the short transform, the long transforms with their f64 block. */
static inline size_t mm_stats_ws_floats(size_t n_chains, size_t n, size_t dim, unsigned int n_parts, const mm_stats_knobs &k)
{
    const size_t m = n / 2;
    size_t need = (size_t)stats_n_slabs(n_chains, k) * dim * m;
    if (dim == 0)
        return 0; /* no call: the geometries below divide by the dimension */
    mm_stats_plan p;
    if (m >= 2 && m <= 1024) {
        stats_fft_geom(p, n_chains, m, dim, k);
        need = std::max(need, ((size_t)p.rows + n_parts) * dim * p.row_len);
    } else if (m > 1024 && m <= kStatsLongMaxM) {
        stats_long_geom(p, n_chains, m, dim);
        need = std::max(need, ((size_t)p.rows + n_parts + 2) * dim * p.row_len);
    }
    return need;
}

/* sel: the selector value (MMCMC_STATS_KERNEL_*); aligned16: the sample starts on a 16-byte boundary; work_limit: lag
 * products the any-length path may be asked for, 0 = no limit (mmcmc_stats_set_direct_work_limit) */
static inline mm_stats_plan mm_stats_make_plan(size_t n_chains, size_t n, size_t dim, int dtype, int sel, unsigned int n_parts,
                                               bool want_wb, bool aligned16, const mm_stats_knobs &k, uint64_t work_limit)
{
    mm_stats_plan p;
    const size_t m = n / 2;
    if (n_chains == 0 || dim == 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return mm_stats_plan{MMCMC_ERR_INVALID_ARG};
    if (mm_stats_shape_status(n, dim) != MMCMC_OK)
        return mm_stats_plan{MMCMC_ERR_SHAPE};
    const bool transform = sel == MMCMC_STATS_KERNEL_AUTO || sel == MMCMC_STATS_KERNEL_FFT;
    if (transform && m >= 2 && m <= 1024 && (sel == MMCMC_STATS_KERNEL_FFT || m > 100)) {
        /* power spectrum per workgroup -> bin totals in n_parts partial sums (the tail kernel, with bins for lags) -> one
         * inverse per parameter */
        stats_fft_geom(p, n_chains, m, dim, k);
        p.path = MM_STATS_FFT;
        p.top = m > 64 * (size_t)(p.r1 / 2 - 1); /* only a lane's last point can be padding */
        p.first = {p.rows * p.arg, 1, 1, 256, 4 * (size_t)p.r1 * kStatsFftLdsCx * 2 * sizeof(float)};
        p.finish_kind = MM_STATS_FINISH_FFT;
        p.finish.lds = (2 * (size_t)p.row_len + 256) * sizeof(double);
    } else if (transform && m > 1024 && m <= kStatsLongMaxM) {
        stats_long_geom(p, n_chains, m, dim);
        p.finish_kind = MM_STATS_FINISH_LONG;
        p.sum = {(unsigned int)((dim * p.row_len + 255) / 256), 1, 1, 256, 0};
        if (p.arg >= 3) {
            /* means by a streaming pass (dim <= 16: 64 dim threads per half-chain; wider samples through the any-length
             * moments kernel), then one wave per (chain group, residue, parameter) */
            p.path = MM_STATS_FFT_RES;
            p.moments = dim > 16;
            if ((uint64_t)2 * n_chains >= (1ull << 31) || (uint64_t)p.rows * dim * p.arg >= (1ull << 31) ||
                (p.moments && (uint64_t)2 * n_chains * dim >= (1ull << 31)))
                return mm_stats_plan{MMCMC_ERR_SHAPE};
            const unsigned int c2 = (unsigned int)(2 * n_chains);
            p.pre = p.moments ? mm_stats_launch{c2 * (unsigned int)dim, 1, 1, 64, 0} : mm_stats_launch{c2, 1, 1, 64u * (unsigned int)dim, 0};
            p.first = {p.rows * (unsigned int)dim * p.arg, 1, 1, 64, 32 * kStatsFftLdsCx * 2 * sizeof(float)};
        } else {
            p.path = MM_STATS_FFT_LONG;
            p.first = {p.rows * (unsigned int)dim, 1, 1, 64, kStatsLongLds};
        }
    } else {
        unsigned int n_slabs = stats_n_slabs(n_chains, k);
        const bool no_force = sel != MMCMC_STATS_KERNEL_DIRECT && sel != MMCMC_STATS_KERNEL_MFMA;
        /* register tiles on the vector ALU where a lane's share of the D x tiles(m) tiles fits its registers (at most 8
         * tiles of 16 lag sums: [., 400, 3] just fits) */
        const unsigned int tiles_1 = stats_tile_count(m);
        const unsigned int tpl = (unsigned int)((dim * (size_t)tiles_1 + 63) / 64);
        const size_t pitch_t = 12 * ((m + 8 + 16 + 8 + 7) / 8) + 4; /* the tile kernels' row pitch */
        const size_t lds_tile = (dim * pitch_t + dim * m + 64 * 16) * sizeof(float);
        /* one parameter per wave, a parameter's tiles dealt to `parts` waves of three slots (mm_half_chain_tile1_kernel: four
         * waves per SIMD): half-chains up to 512 long -- eight column loads per lane, 16 waves' rows in a CU's LDS --;
         * MMCMC_STATS_KERNEL_TILE keeps the all-parameters kernel where that one applies */
        const unsigned int tpl_1 = tiles_1 <= 64 ? 1u : tiles_1 <= 128 ? 2u : 3u;
        const unsigned int parts = (tiles_1 + 64u * tpl_1 - 1u) / (64u * tpl_1);
        const size_t lds_1 = (pitch_t + m + 64 * 16 + 64) * sizeof(float);
        /* lag sums on the matrix cores (one 16 x 16 tile per 256 lags) unless the half-chain is too long for LDS */
        const unsigned int n_tiles = (unsigned int)((m + 255) / 256);
        const size_t row = 240 + 256 * (size_t)(n_tiles - 1) + m + 36, row_pitch = row + row / 16 + 1;
        const size_t lds_mfma = ((size_t)dim * row_pitch + (size_t)dim * m) * sizeof(float);
        /* the half-chain staged whole, at an odd row pitch */
        const unsigned int m_pad = (unsigned int)(m + 64 + ((m + 64) % 2 == 0 ? 1 : 0));
        const size_t lds_whole = ((size_t)dim * m_pad + (size_t)dim * m) * sizeof(float);
        if (no_force && sel != MMCMC_STATS_KERNEL_TILE && m <= 512 && 16 * lds_1 <= 160 * 1024 && (size_t)parts * dim <= n_slabs) {
            /* slabs x parts x parameters waves = the resident 16 per CU; the tail sums slabs x parts rows per (d, lag) */
            p.path = MM_STATS_TILE1;
            const size_t cap = k.waves ? (size_t)n_slabs : 4096 / dim;
            n_slabs = (unsigned int)std::max<size_t>(1, std::min<size_t>(n_slabs, cap) / parts) * parts;
            p.tpl = m > 256 ? 3 : tpl_1;
            p.npre = m > 256 ? 8 : 4;
            p.arg = parts;
            p.first = {n_slabs * (unsigned int)dim, 1, 1, 64, lds_1};
        } else if (no_force && tpl <= 8 && lds_tile <= 40 * 1024) {
            /* 8 tiles = 128 lag sums + operands = 218 registers, two waves per SIMD: exactly the resident waves, each with a
             * longer list of half-chains (measured at [65 536, 400, 3]: 1024 waves 0.62 ms, 2048 0.39, 4096 0.43, 8192 0.54) */
            p.path = MM_STATS_TILE;
            if (!k.waves)
                n_slabs = std::min(n_slabs, 2048u);
            p.tpl = tpl <= 2 ? 2 : tpl <= 4 ? 4 : 8;
            /* 16-byte loads where every half-chain's [m, D] block starts on a 16-byte boundary and is whole vectors long */
            p.vec = dtype == MMCMC_F32 && (n * dim) % 4 == 0 && ((n - m) * dim) % 4 == 0 && (m * dim) % 4 == 0 && aligned16 &&
                    m * dim <= 4 * 256;
            p.first = {n_slabs, 1, 1, 64, lds_tile};
        } else if (lds_mfma <= 64 * 1024 && sel != MMCMC_STATS_KERNEL_DIRECT) {
            p.path = MM_STATS_MFMA;
            p.arg = n_tiles;
            p.first = {n_slabs, 1, 1, 64, lds_mfma};
        } else if (lds_whole <= 160 * 1024 && m <= 16384) {
            p.path = MM_STATS_LDS;
            p.arg = m_pad;
            p.first = {n_slabs, 1, 1, 64, lds_whole};
        } else {
            /* nothing stages such a half-chain (or only one wave per half-chain would: [2, 32770, 1] 46 ms against 1 ms here):
             * moments and lag sums straight from global memory.  32-bit quantities of this path: the moments kernel's grid
             * (2 C D workgroups) and dim * m (the tail kernel's element count); and a WORK bound -- the lag sums cost
             * C * D * m^2 products like the reference's brute-force branch (stats.rs:622-654), ~6e12 per second on an MI355X:
             * past the limit the call is refused instead of occupying the device for minutes.  Under AUTO / FFT this path is
             * reached only beyond kStatsLongMaxM draws per half-chain */
            if ((uint64_t)dim * m >= (1ull << 32) || (uint64_t)2 * n_chains * dim >= (1ull << 31))
                return mm_stats_plan{MMCMC_ERR_SHAPE};
            if (work_limit != 0 && (long double)n_chains * (long double)dim * (long double)m * (long double)m > (long double)work_limit)
                return mm_stats_plan{MMCMC_ERR_UNSUPPORTED};
            n_slabs = std::min(n_slabs, 16u);
            p.pre = {(unsigned int)(2 * n_chains * dim), 1, 1, 64, 0};
            p.first = {(unsigned int)((m + 255) / 256), (unsigned int)dim, n_slabs, 256, 0};
        }
        p.rows = n_slabs, p.row_len = (unsigned int)m;
    }
    p.raise_lds = p.first.lds > 64 * 1024;
    const unsigned int total = (unsigned int)(dim * p.row_len); /* < 2^32: stats_bins_fit, dim x m above */
    p.nb_red = (total + 63) / 64 * n_parts;
    p.tail = {p.nb_red + (want_wb ? (unsigned int)dim * kStatsWbChunks : 0u), 1, 1, 256, 0};
    p.len_slabs = (size_t)p.rows * total;
    /* without a workspace the tile kernels' rows are allocated as stats_n_slabs gives them, before those paths' own caps */
    const bool tiles = p.path == MM_STATS_TILE1 || p.path == MM_STATS_TILE;
    p.ws_floats = tiles ? (size_t)stats_n_slabs(n_chains, k) * total : p.len_slabs;
    if (p.finish_kind != MM_STATS_FINISH_NONE) {
        p.writes_total = true;
        p.finish = {(unsigned int)dim * (unsigned int)((m + 31) / 32), 1, 1, 256, p.finish.lds};
        p.off_bins = p.len_slabs, p.len_bins = (size_t)n_parts * total;
        p.ws_floats += p.len_bins;
        if (p.finish_kind == MM_STATS_FINISH_LONG) {
            p.off_P = (p.ws_floats + 1) / 2 * 2; /* doubles: on an 8-byte boundary of a workspace that starts on one */
            p.len_P = 2 * (size_t)total;
            p.ws_floats = p.off_P + p.len_P;
        }
    }
    return p;
}

#endif /* MM_STATS_PLAN_H */

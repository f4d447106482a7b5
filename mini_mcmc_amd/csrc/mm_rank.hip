/*
 * mm_rank.hip -- rank-normalised diagnostics on the GPU (C ABI: mmcmc_rank_normalize, mmcmc_quantiles,
 * mmcmc_rank_diagnostics): Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), "Rank-normalization, folding, and
 * localization: an improved R-hat for assessing convergence of MCMC".  Not in the reference, whose stats.rs:416-546 stops at
 * the mean-based split R-hat and the mean ESS.
 *
 * Per parameter d of sample [C, n, D] (S = C n pooled draws, cast to f32 like RunStats::from, stats.rs:365):
 *   mm_rank_extract_kernel    column d -> (order-preserving uint32 key, index payload); raises the parameter's NaN flag;
 *                             the folded pass takes |x - med| first
 *   a stable LSD radix sort of the pairs, four 8-bit passes, each
 *     mm_radix_hist_kernel    digit counts of every tile of 4096 keys -> hist[digit][tile]
 *     mm_scan_*_kernel        exclusive scan of hist read as one array (digit-major: the tile's first output slot per digit)
 *     mm_radix_scatter_kernel ranks every key among the equal digits before it in the tile -- inside a wave by matching the
 *                             digit with eight ballots, across rounds and waves by per-wave counters that only the leading
 *                             lane of a digit group updates (no LDS atomics: nothing depends on the order they complete in) --,
 *                             orders the tile by digit in LDS and writes each digit's run to its slot
 *   mm_tie_reduce_kernel / mm_tie_parts_kernel / mm_tie_apply_kernel
 *                             head flags key[i] != key[i - 1]; a forward max-scan carries the first position `lo` of the tie
 *                             group, a backward min-scan the last `hi`; rank2 = lo + hi = 2 x the average 1-based rank,
 *                             exact in uint32 for S < 2^31; z = normcdfinv((rank2 / 2 - 3/8) / (S + 1/4)) in f64, rounded
 *                             once to f32 and scattered to z[c, t, d] through the payload
 * Order statistics (quantiles, the fold's median) are read from the sorted keys by the host, two words per probability.
 * Everything after that is the library's own split R-hat / ESS (mmcmc_split_rhat_mean_ess) on the transformed arrays.
 *
 * The result is a pure function of the input: integer counts and scans only, bit-reproducible across runs, streams and
 * devices.  Parameters go one after another on the caller's stream; work buffers hold one parameter (2 x S x 8 bytes +
 * histograms).  Single device: ranks are global over chains, device groups are out of scope.
 */
#include "../../include/mmcmc.h"
#include "mm_host.h"
#include "mm_rank.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {

constexpr unsigned int RS_THREADS = 256;            /* four waves */
constexpr unsigned int RS_ITEMS = 16;               /* keys per thread and tile */
constexpr unsigned int RS_TILE = RS_THREADS * RS_ITEMS;
constexpr unsigned int RS_WAVES = RS_THREADS / 64;
constexpr unsigned int RS_WCHUNK = 64 * RS_ITEMS;   /* consecutive keys of a tile one wave ranks */
constexpr unsigned int SC_ITEMS = 8;                /* scan / tie kernels: consecutive elements per thread */
constexpr unsigned int SC_TILE = RS_THREADS * SC_ITEMS;

struct OpAdd {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct OpMax {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct OpMin {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};

/* Exclusive scan over the 256 threads of a block (REV: from the last thread down), double-buffered in buf [2][256];
 * *total = the reduction over all threads.  Every thread of the block must call it. */
template <class Op, bool REV>
__device__ uint32_t block_scan_excl(uint32_t v, uint32_t ident, Op op, uint32_t *buf, uint32_t *total)
{
    const int t = (int)threadIdx.x;
    int p = 0;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < (int)RS_THREADS; off <<= 1) {
        uint32_t a = buf[p * RS_THREADS + t];
        const int o = REV ? t + off : t - off;
        if (o >= 0 && o < (int)RS_THREADS)
            a = op(a, buf[p * RS_THREADS + o]);
        buf[(p ^ 1) * RS_THREADS + t] = a;
        p ^= 1;
        __syncthreads();
    }
    const int nb = REV ? t + 1 : t - 1;
    const uint32_t ex = (nb >= 0 && nb < (int)RS_THREADS) ? buf[p * RS_THREADS + nb] : ident;
    *total = buf[p * RS_THREADS + (REV ? 0 : (int)RS_THREADS - 1)];
    __syncthreads();
    return ex;
}

/* ---- key extraction ---- */

/* column d of sample [S, D] (T = float or double, cast to f32 first) -> keys[i], idx[i] = i.  fold: |x - med| in f32. */
template <class T>
__global__ __launch_bounds__(256) void mm_rank_extract_kernel(const T *__restrict__ sample, uint32_t S, uint32_t D, uint32_t d,
                                                              int fold, float med, uint32_t *__restrict__ keys,
                                                              uint32_t *__restrict__ idx, uint32_t *__restrict__ nan_flag)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    bool saw_nan = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < S; i += stride) {
        float x = (float)sample[(size_t)i * D + d];
        if (fold)
            x = fabsf(x - med);
        const uint32_t bits = __float_as_uint(x);
        saw_nan |= mm_rank_bits_are_nan(bits);
        keys[i] = mm_rank_key_of_bits(bits);
        idx[i] = i;
    }
    if (saw_nan)
        atomicOr(nan_flag, 1u); /* idempotent: the flag does not depend on who comes first */
}

/* ---- radix sort ---- */

/* hist[digit * n_tiles + tile] = keys of the tile with that digit.  Integer counts: the LDS atomics' order is immaterial. */
__global__ __launch_bounds__(RS_THREADS) void mm_radix_hist_kernel(const uint32_t *__restrict__ keys, uint32_t S, int shift,
                                                                   uint32_t *__restrict__ hist, uint32_t n_tiles)
{
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x, tile0 = blockIdx.x * RS_TILE;
    h[tid] = 0;
    __syncthreads();
#pragma unroll
    for (unsigned int r = 0; r < RS_ITEMS; ++r) {
        const uint32_t i = tile0 + r * RS_THREADS + tid;
        if (i < S)
            atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)tid * n_tiles + blockIdx.x] = h[tid];
}

/* in-place exclusive scan of a[0 .. len): block sums, a scan of the block sums by one workgroup, the blocks' own scans */
__global__ __launch_bounds__(RS_THREADS) void mm_scan_reduce_kernel(const uint32_t *__restrict__ a, uint32_t len,
                                                                    uint32_t *__restrict__ parts)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    const uint32_t i0 = blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e)
        if (i0 + e < len)
            s += a[i0 + e];
    uint32_t total;
    (void)block_scan_excl<OpAdd, false>(s, 0u, OpAdd(), buf, &total);
    if (threadIdx.x == 0)
        parts[blockIdx.x] = total;
}

__global__ __launch_bounds__(RS_THREADS) void mm_scan_parts_kernel(uint32_t *__restrict__ parts, uint32_t n_parts)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_parts; base += RS_THREADS) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < n_parts ? parts[j] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_excl<OpAdd, false>(v, 0u, OpAdd(), buf, &total);
        if (j < n_parts)
            parts[j] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(RS_THREADS) void mm_scan_apply_kernel(uint32_t *__restrict__ a, uint32_t len,
                                                                   const uint32_t *__restrict__ parts)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    const uint32_t i0 = blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
    uint32_t v[SC_ITEMS], s = 0;
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e) {
        v[e] = i0 + e < len ? a[i0 + e] : 0u;
        s += v[e];
    }
    uint32_t total;
    uint32_t run = parts[blockIdx.x] + block_scan_excl<OpAdd, false>(s, 0u, OpAdd(), buf, &total);
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e) {
        if (i0 + e < len)
            a[i0 + e] = run;
        run += v[e];
    }
}

/* One pass: the tile's keys, in input order, go behind the equal digits of every earlier tile (base = scanned hist) and of
 * the tile itself.  Wave w ranks keys [w, w + 1) x 1024 of the tile, 64 consecutive keys per round: a key's rank among the
 * wave's equal digits so far = the wave's counter + the equal digits in lower lanes; the leading lane of each digit group
 * then advances the counter by the group's size.  One writer per counter and round, reads before the write in program
 * order: no atomics, no dependence on completion order. */
__global__ __launch_bounds__(RS_THREADS) void mm_radix_scatter_kernel(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                                      uint32_t *__restrict__ kout, uint32_t *__restrict__ vout,
                                                                      uint32_t S, int shift, const uint32_t *__restrict__ base,
                                                                      uint32_t n_tiles)
{
    __shared__ uint32_t wcnt[RS_WAVES][256];
    __shared__ uint32_t dstart[256]; /* first slot of the digit in the tile's digit-ordered copy */
    __shared__ uint32_t gbase[256];  /* first output slot of the tile's keys with the digit */
    __shared__ uint32_t buf[2 * RS_THREADS];
    __shared__ uint32_t sk[RS_TILE], sv[RS_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t tile0 = blockIdx.x * RS_TILE;
    const uint32_t n_valid = S - tile0 < RS_TILE ? S - tile0 : RS_TILE;
    for (unsigned int i = tid; i < RS_WAVES * 256; i += RS_THREADS)
        (&wcnt[0][0])[i] = 0;
    uint32_t key[RS_ITEMS], val[RS_ITEMS], rk[RS_ITEMS];
#pragma unroll
    for (unsigned int r = 0; r < RS_ITEMS; ++r) {
        const uint32_t j = w * RS_WCHUNK + r * 64u + lane;
        const bool valid = j < n_valid;
        key[r] = valid ? kin[tile0 + j] : 0xffffffffu;
        val[r] = valid ? vin[tile0 + j] : 0u;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (unsigned int r = 0; r < RS_ITEMS; ++r) {
        const bool valid = w * RS_WCHUNK + r * 64u + lane < n_valid;
        const uint32_t dg = (key[r] >> shift) & 255u;
        unsigned long long same = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (unsigned int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1u;
            const unsigned long long bb = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? bb : ~bb;
        }
        const uint32_t old = wcnt[w][dg];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t lower = (uint32_t)__popcll(same & lt);
        if (valid && lower == 0)
            wcnt[w][dg] = old + (uint32_t)__popcll(same);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        rk[r] = old + lower;
    }
    __syncthreads();
    { /* thread = digit: the waves' counts -> their offsets inside the digit; the digits' totals -> dstart */
        uint32_t tot = 0;
#pragma unroll
        for (unsigned int q = 0; q < RS_WAVES; ++q) {
            const uint32_t c = wcnt[q][tid];
            wcnt[q][tid] = tot;
            tot += c;
        }
        uint32_t all;
        dstart[tid] = block_scan_excl<OpAdd, false>(tot, 0u, OpAdd(), buf, &all);
        gbase[tid] = base[(size_t)tid * n_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (unsigned int r = 0; r < RS_ITEMS; ++r) {
        if (w * RS_WCHUNK + r * 64u + lane < n_valid) {
            const uint32_t dg = (key[r] >> shift) & 255u;
            const uint32_t pos = dstart[dg] + wcnt[w][dg] + rk[r]; /* < n_valid: the counts are of the valid keys */
            sk[pos] = key[r];
            sv[pos] = val[r];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_valid; i += RS_THREADS) {
        const uint32_t k = sk[i], dg = (k >> shift) & 255u;
        const uint32_t dst = gbase[dg] + (i - dstart[dg]); /* < S: base is the scan of the same keys' counts */
        kout[dst] = k;
        vout[dst] = sv[i];
    }
}

/* ---- tie groups, scores, scatter ---- */

/* tile b of 2048 sorted keys: bmax[b] = the last head position (1-based; 0 = none), bmin[b] = the first tail position
 * (0xffffffff = none); head: key[i] != key[i - 1], tail: key[i] != key[i + 1] */
__global__ __launch_bounds__(RS_THREADS) void mm_tie_reduce_kernel(const uint32_t *__restrict__ k, uint32_t S,
                                                                   uint32_t *__restrict__ bmax, uint32_t *__restrict__ bmin)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    const uint32_t i0 = blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
    uint32_t hmax = 0u, tmin = 0xffffffffu;
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e) {
        const uint32_t i = i0 + e;
        if (i < S) {
            const uint32_t ki = k[i];
            if (i == 0 || k[i - 1] != ki)
                hmax = i + 1;
            if ((i == S - 1 || k[i + 1] != ki) && tmin == 0xffffffffu)
                tmin = i + 1;
        }
    }
    uint32_t tot_max, tot_min;
    (void)block_scan_excl<OpMax, false>(hmax, 0u, OpMax(), buf, &tot_max);
    (void)block_scan_excl<OpMin, false>(tmin, 0xffffffffu, OpMin(), buf, &tot_min);
    if (threadIdx.x == 0) {
        bmax[blockIdx.x] = tot_max;
        bmin[blockIdx.x] = tot_min;
    }
}

/* bmax -> exclusive forward max-scan (what reaches tile b from the tiles before it), bmin -> exclusive backward min-scan */
__global__ __launch_bounds__(RS_THREADS) void mm_tie_parts_kernel(uint32_t *__restrict__ bmax, uint32_t *__restrict__ bmin,
                                                                  uint32_t n_tiles)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < n_tiles; base += RS_THREADS) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < n_tiles ? bmax[j] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_excl<OpMax, false>(v, 0u, OpMax(), buf, &total);
        if (j < n_tiles)
            bmax[j] = carry > ex ? carry : ex;
        carry = carry > total ? carry : total;
    }
    carry = 0xffffffffu;
    for (uint32_t base = 0; base < n_tiles; base += RS_THREADS) {
        const uint32_t r = base + threadIdx.x; /* r counts tiles from the last one */
        const uint32_t v = r < n_tiles ? bmin[n_tiles - 1u - r] : 0xffffffffu;
        uint32_t total;
        const uint32_t ex = block_scan_excl<OpMin, false>(v, 0xffffffffu, OpMin(), buf, &total);
        if (r < n_tiles)
            bmin[n_tiles - 1u - r] = carry < ex ? carry : ex;
        carry = carry < total ? carry : total;
    }
}

/* rank2 = lo + hi of every sorted key, its normal score, both scattered through the payload to [S, D] column d (z and / or
 * rank2 may be NULL).  A flagged parameter (any NaN draw) gets z = NaN and rank2 = 0 everywhere. */
__global__ __launch_bounds__(RS_THREADS) void mm_tie_apply_kernel(const uint32_t *__restrict__ k, const uint32_t *__restrict__ idx,
                                                                  uint32_t S, const uint32_t *__restrict__ bmax,
                                                                  const uint32_t *__restrict__ bmin, const uint32_t *__restrict__ nan_flag,
                                                                  uint32_t D, uint32_t d, float *__restrict__ z,
                                                                  uint32_t *__restrict__ rank2)
{
    __shared__ uint32_t buf[2 * RS_THREADS];
    const uint32_t i0 = blockIdx.x * SC_TILE + threadIdx.x * SC_ITEMS;
    uint32_t head[SC_ITEMS], tail[SC_ITEMS];
    uint32_t hmax = 0u, tmin = 0xffffffffu;
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e) {
        const uint32_t i = i0 + e;
        head[e] = 0u;
        tail[e] = 0xffffffffu;
        if (i < S) {
            const uint32_t ki = k[i];
            if (i == 0 || k[i - 1] != ki)
                head[e] = i + 1;
            if (i == S - 1 || k[i + 1] != ki)
                tail[e] = i + 1;
        }
        hmax = head[e] > hmax ? head[e] : hmax;
        tmin = tail[e] < tmin ? tail[e] : tmin;
    }
    uint32_t total;
    uint32_t lo = block_scan_excl<OpMax, false>(hmax, 0u, OpMax(), buf, &total);
    uint32_t hi = block_scan_excl<OpMin, true>(tmin, 0xffffffffu, OpMin(), buf, &total);
    const uint32_t cmax = bmax[blockIdx.x], cmin = bmin[blockIdx.x];
    lo = lo > cmax ? lo : cmax;
    hi = hi < cmin ? hi : cmin;
    uint32_t his[SC_ITEMS];
#pragma unroll
    for (int e = (int)SC_ITEMS - 1; e >= 0; --e) {
        hi = tail[e] < hi ? tail[e] : hi;
        his[e] = hi;
    }
    const bool flagged = *nan_flag != 0u;
    const double denom = (double)S + 0.25;
#pragma unroll
    for (unsigned int e = 0; e < SC_ITEMS; ++e) {
        const uint32_t i = i0 + e;
        lo = head[e] > lo ? head[e] : lo;
        if (i < S) {
            const uint32_t r2 = lo + his[e];
            const size_t dst = (size_t)idx[i] * D + d;
            if (rank2)
                rank2[dst] = flagged ? 0u : r2;
            if (z) {
                const double u = ((double)r2 * 0.5 - 0.375) / denom; /* Blom; in (0, 1) */
                z[dst] = flagged ? __uint_as_float(0x7fc00000u) : (float)normcdfinv(u);
            }
        }
    }
}

/* out[e] = x[e] <= q[e % D] ? 1 : 0 (x cast to f32 first, compared as double with the f64 quantile) */
template <class T>
__global__ __launch_bounds__(256) void mm_rank_indicator_kernel(const T *__restrict__ sample, size_t total, uint32_t D,
                                                                const double *__restrict__ q, float *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const float x = (float)sample[e];
        out[e] = (double)x <= q[e % D] ? 1.0f : 0.0f;
    }
}

/* ---- host ---- */

/* every device buffer of a call; freed when the call returns (each entry point ends with a stream synchronise) */
struct RankBufs {
    std::vector<void *> owned;
    ~RankBufs()
    {
        for (void *p : owned)
            (void)hipFree(p);
    }
    template <class T> hipError_t get(T **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess)
            owned.push_back(p);
        *out = (T *)p;
        return e;
    }
};

/* the sort's work buffers for S keys */
struct RankSort {
    uint32_t S = 0, n_tiles = 0, hist_len = 0, n_parts = 0, n_tie_tiles = 0;
    uint32_t *k[2] = {nullptr, nullptr}, *v[2] = {nullptr, nullptr};
    uint32_t *hist = nullptr, *parts = nullptr, *bmax = nullptr, *bmin = nullptr;
    uint32_t *flag = nullptr; /* the NaN flag of the parameter being worked on */
    hipError_t alloc(RankBufs &b, size_t s)
    {
        S = (uint32_t)s;
        n_tiles = (S + RS_TILE - 1) / RS_TILE;
        hist_len = 256u * n_tiles; /* <= 2^27 */
        n_parts = (hist_len + SC_TILE - 1) / SC_TILE;
        n_tie_tiles = (S + SC_TILE - 1) / SC_TILE;
        hipError_t e;
        for (int i = 0; i < 2; ++i) {
            if ((e = b.get(&k[i], S)) != hipSuccess || (e = b.get(&v[i], S)) != hipSuccess)
                return e;
        }
        if ((e = b.get(&hist, hist_len)) != hipSuccess || (e = b.get(&parts, n_parts)) != hipSuccess ||
            (e = b.get(&bmax, n_tie_tiles)) != hipSuccess || (e = b.get(&bmin, n_tie_tiles)) != hipSuccess ||
            (e = b.get(&flag, 1)) != hipSuccess)
            return e;
        return hipSuccess;
    }
};

/* column d of the sample -> sorted (key, index) pairs in w.k[0] / w.v[0]; the parameter's NaN flag in *w.flag */
int rank_sort_column(RankSort &w, const void *d_sample, int dtype, uint32_t D, uint32_t d, int fold, float med,
                     hipStream_t stream)
{
    MM_HIP(hipMemsetAsync(w.flag, 0, sizeof(uint32_t), stream));
    const unsigned int eb = std::min<unsigned int>((w.S + 255u) / 256u, 4096u);
    if (dtype == MMCMC_F32)
        hipLaunchKernelGGL(mm_rank_extract_kernel<float>, dim3(eb), dim3(256), 0, stream, (const float *)d_sample, w.S, D, d,
                           fold, med, w.k[0], w.v[0], w.flag);
    else
        hipLaunchKernelGGL(mm_rank_extract_kernel<double>, dim3(eb), dim3(256), 0, stream, (const double *)d_sample, w.S, D,
                           d, fold, med, w.k[0], w.v[0], w.flag);
    MM_HIP(hipGetLastError());
    int src = 0;
    for (int pass = 0; pass < 4; ++pass, src ^= 1) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(mm_radix_hist_kernel, dim3(w.n_tiles), dim3(RS_THREADS), 0, stream, w.k[src], w.S, shift, w.hist,
                           w.n_tiles);
        hipLaunchKernelGGL(mm_scan_reduce_kernel, dim3(w.n_parts), dim3(RS_THREADS), 0, stream, w.hist, w.hist_len, w.parts);
        hipLaunchKernelGGL(mm_scan_parts_kernel, dim3(1), dim3(RS_THREADS), 0, stream, w.parts, w.n_parts);
        hipLaunchKernelGGL(mm_scan_apply_kernel, dim3(w.n_parts), dim3(RS_THREADS), 0, stream, w.hist, w.hist_len, w.parts);
        hipLaunchKernelGGL(mm_radix_scatter_kernel, dim3(w.n_tiles), dim3(RS_THREADS), 0, stream, w.k[src], w.v[src],
                           w.k[src ^ 1], w.v[src ^ 1], w.S, shift, w.hist, w.n_tiles);
        MM_HIP(hipGetLastError());
    }
    return MMCMC_OK; /* four passes: back in buffer 0 */
}

/* ranks and scores of the sorted column -> column d of z / rank2 [S, D] (device; either may be NULL) */
int rank_apply_column(RankSort &w, uint32_t D, uint32_t d, float *d_z, uint32_t *d_rank2, hipStream_t stream)
{
    hipLaunchKernelGGL(mm_tie_reduce_kernel, dim3(w.n_tie_tiles), dim3(RS_THREADS), 0, stream, w.k[0], w.S, w.bmax, w.bmin);
    hipLaunchKernelGGL(mm_tie_parts_kernel, dim3(1), dim3(RS_THREADS), 0, stream, w.bmax, w.bmin, w.n_tie_tiles);
    hipLaunchKernelGGL(mm_tie_apply_kernel, dim3(w.n_tie_tiles), dim3(RS_THREADS), 0, stream, w.k[0], w.v[0], w.S, w.bmax,
                       w.bmin, w.flag, D, d, d_z, d_rank2);
    MM_HIP(hipGetLastError());
    return MMCMC_OK;
}

/* type-7 quantiles (numpy's default) of the sorted column in w.k[0]: h = (S - 1) p, j = floor(h), g = h - j,
 * q = a + g (b - a) in f64 with a, b the f32 order statistics j and j + 1.  Waits for the stream.  out[i] for probs[i];
 * *flagged = the parameter has a NaN draw (every quantile NaN then). */
int rank_read_quantiles(RankSort &w, const double *probs, size_t n_probs, double *out, bool *flagged, hipStream_t stream)
{
    std::vector<uint32_t> got(2 * n_probs + 1);
    std::vector<double> g(n_probs);
    for (size_t i = 0; i < n_probs; ++i) {
        const double h = (double)(w.S - 1u) * probs[i];
        const double fl = std::floor(h);
        const uint32_t j = (uint32_t)fl, j1 = j + 1u < w.S ? j + 1u : j;
        g[i] = h - fl;
        MM_HIP(hipMemcpyAsync(&got[2 * i], w.k[0] + j, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        MM_HIP(hipMemcpyAsync(&got[2 * i + 1], w.k[0] + j1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    MM_HIP(hipMemcpyAsync(&got[2 * n_probs], w.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MM_HIP(hipStreamSynchronize(stream));
    *flagged = got[2 * n_probs] != 0u;
    for (size_t i = 0; i < n_probs; ++i) {
        float af, bf;
        const uint32_t ab = mm_rank_bits_of_key(got[2 * i]), bb = mm_rank_bits_of_key(got[2 * i + 1]);
        std::memcpy(&af, &ab, 4);
        std::memcpy(&bf, &bb, 4);
        const double a = (double)af, b = (double)bf;
        out[i] = *flagged ? std::numeric_limits<double>::quiet_NaN() : (g[i] == 0.0 || a == b) ? a : a + g[i] * (b - a);
    }
    return MMCMC_OK;
}

/* arguments every entry point shares; the shape is judged before the device is looked for or anything is allocated */
int rank_check_args(const void *sample, int dtype, size_t n_chains, size_t n, size_t dim)
{
    if (!sample || n_chains == 0 || n == 0 || dim == 0 || (dtype != MMCMC_F32 && dtype != MMCMC_F64))
        return MMCMC_ERR_INVALID_ARG;
    if (n >= (1ull << 31) || n_chains >= (1ull << 31) || n_chains * n >= (1ull << 31) || dim >= (1u << 16))
        return MMCMC_ERR_SHAPE;
    return MMCMC_OK;
}

int rank_check_probs(const double *probs, size_t n_probs)
{
    if (n_probs > 0 && !probs)
        return MMCMC_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
            return MMCMC_ERR_INVALID_ARG;
    return MMCMC_OK;
}

/* the sample on the device: the caller's pointer, or a copy of the host array */
int rank_device_sample(RankBufs &bufs, const void *sample, int sample_is_device, size_t bytes, hipStream_t stream,
                       const void **out)
{
    if (sample_is_device) {
        *out = sample;
        return MMCMC_OK;
    }
    char *p = nullptr;
    MM_HIP(bufs.get(&p, bytes));
    MM_HIP(hipMemcpyAsync(p, sample, bytes, hipMemcpyHostToDevice, stream));
    *out = p;
    return MMCMC_OK;
}

} // namespace

extern "C" {

int mmcmc_rank_normalize(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                         int folded, float *z, int z_is_device, uint32_t *rank2, int device, void *stream_v)
{
    int st = rank_check_args(sample, dtype, n_chains, n, dim);
    if (st == MMCMC_OK && !z)
        st = MMCMC_ERR_INVALID_ARG;
    if (st != MMCMC_OK)
        return st;
    if ((st = mm_check_device(device)) != MMCMC_OK)
        return st;
    DevGuard g(device);
    hipStream_t stream = (hipStream_t)stream_v;
    const size_t S = n_chains * n, total = S * dim;
    RankBufs bufs;
    RankSort w;
    const void *d_sample = nullptr;
    if ((st = rank_device_sample(bufs, sample, sample_is_device, total * (dtype == MMCMC_F32 ? 4 : 8), stream, &d_sample)) !=
        MMCMC_OK)
        return st;
    MM_HIP(w.alloc(bufs, S));
    float *d_z = z;
    uint32_t *d_r2 = rank2;
    if (!z_is_device) {
        MM_HIP(bufs.get(&d_z, total));
        if (rank2)
            MM_HIP(bufs.get(&d_r2, total));
    }
    const double half = 0.5;
    for (uint32_t d = 0; d < (uint32_t)dim; ++d) {
        if ((st = rank_sort_column(w, d_sample, dtype, (uint32_t)dim, d, 0, 0.f, stream)) != MMCMC_OK)
            return st;
        if (folded) {
            double med = 0.0;
            bool flagged = false;
            if ((st = rank_read_quantiles(w, &half, 1, &med, &flagged, stream)) != MMCMC_OK)
                return st;
            /* a flagged parameter: med is NaN, every folded draw is NaN, the folded pass flags it again */
            if ((st = rank_sort_column(w, d_sample, dtype, (uint32_t)dim, d, 1, (float)med, stream)) != MMCMC_OK)
                return st;
        }
        if ((st = rank_apply_column(w, (uint32_t)dim, d, d_z, d_r2, stream)) != MMCMC_OK)
            return st;
    }
    if (!z_is_device) {
        MM_HIP(hipMemcpyAsync(z, d_z, total * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (rank2)
            MM_HIP(hipMemcpyAsync(rank2, d_r2, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    MM_HIP(hipStreamSynchronize(stream)); /* the work buffers are freed on return */
    return MMCMC_OK;
}

int mmcmc_quantiles(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                    const double *probs, size_t n_probs, double *out, int device, void *stream_v)
{
    int st = rank_check_args(sample, dtype, n_chains, n, dim);
    if (st == MMCMC_OK)
        st = rank_check_probs(probs, n_probs);
    if (st == MMCMC_OK && n_probs > 0 && !out)
        st = MMCMC_ERR_INVALID_ARG;
    if (st != MMCMC_OK)
        return st;
    if ((st = mm_check_device(device)) != MMCMC_OK)
        return st;
    if (n_probs == 0)
        return MMCMC_OK;
    DevGuard g(device);
    hipStream_t stream = (hipStream_t)stream_v;
    const size_t S = n_chains * n, total = S * dim;
    RankBufs bufs;
    RankSort w;
    const void *d_sample = nullptr;
    if ((st = rank_device_sample(bufs, sample, sample_is_device, total * (dtype == MMCMC_F32 ? 4 : 8), stream, &d_sample)) !=
        MMCMC_OK)
        return st;
    MM_HIP(w.alloc(bufs, S));
    std::vector<double> q(n_probs);
    for (uint32_t d = 0; d < (uint32_t)dim; ++d) {
        bool flagged = false;
        if ((st = rank_sort_column(w, d_sample, dtype, (uint32_t)dim, d, 0, 0.f, stream)) != MMCMC_OK ||
            (st = rank_read_quantiles(w, probs, n_probs, q.data(), &flagged, stream)) != MMCMC_OK)
            return st;
        for (size_t i = 0; i < n_probs; ++i)
            out[i * dim + d] = q[i];
    }
    return MMCMC_OK;
}

int mmcmc_rank_diagnostics(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                           float *rhat_rank, float *rhat_parts, float *ess_bulk, float *ess_tail, float *ess_tail_parts,
                           const double *probs, size_t n_probs, double *quantiles, int device, void *stream_v)
{
    int st = rank_check_args(sample, dtype, n_chains, n, dim);
    if (st == MMCMC_OK)
        st = rank_check_probs(probs, n_probs);
    if (st == MMCMC_OK && n_probs > 0 && !quantiles)
        st = MMCMC_ERR_INVALID_ARG;
    if (st == MMCMC_OK && (n < 2 || !mm_stats_shape_fits(n, dim)))
        st = MMCMC_ERR_SHAPE;
    if (st != MMCMC_OK)
        return st;
    if ((st = mm_check_device(device)) != MMCMC_OK)
        return st;
    DevGuard g(device);
    hipStream_t stream = (hipStream_t)stream_v;
    const size_t S = n_chains * n, total = S * dim;
    RankBufs bufs;
    RankSort w;
    const void *d_sample = nullptr;
    if ((st = rank_device_sample(bufs, sample, sample_is_device, total * (dtype == MMCMC_F32 ? 4 : 8), stream, &d_sample)) !=
        MMCMC_OK)
        return st;
    MM_HIP(w.alloc(bufs, S));
    float *d_a = nullptr, *d_b = nullptr; /* [S, dim] each: z then I(x <= q05); z_f then I(x <= q95) */
    double *d_q = nullptr;                /* [2, dim]: q05, q95 */
    MM_HIP(bufs.get(&d_a, total));
    MM_HIP(bufs.get(&d_b, total));
    MM_HIP(bufs.get(&d_q, 2 * dim));
    /* the probabilities read from every sorted column: 5 %, 50 %, 95 % for the tail indicators and the fold, then the caller's */
    std::vector<double> p(3 + n_probs), q(3 + n_probs), q_tail(2 * dim);
    p[0] = 0.05;
    p[1] = 0.5;
    p[2] = 0.95;
    for (size_t i = 0; i < n_probs; ++i)
        p[3 + i] = probs[i];
    std::vector<char> flagged(dim, 0);
    for (uint32_t d = 0; d < (uint32_t)dim; ++d) {
        bool fl = false;
        if ((st = rank_sort_column(w, d_sample, dtype, (uint32_t)dim, d, 0, 0.f, stream)) != MMCMC_OK ||
            (st = rank_apply_column(w, (uint32_t)dim, d, d_a, nullptr, stream)) != MMCMC_OK ||
            (st = rank_read_quantiles(w, p.data(), p.size(), q.data(), &fl, stream)) != MMCMC_OK)
            return st;
        flagged[d] = fl;
        q_tail[d] = q[0];
        q_tail[dim + d] = q[2];
        for (size_t i = 0; i < n_probs; ++i)
            quantiles[i * dim + d] = q[3 + i];
        if ((st = rank_sort_column(w, d_sample, dtype, (uint32_t)dim, d, 1, (float)q[1], stream)) != MMCMC_OK ||
            (st = rank_apply_column(w, (uint32_t)dim, d, d_b, nullptr, stream)) != MMCMC_OK)
            return st;
    }
    std::vector<float> r_bulk(dim), r_fold(dim), e_bulk(dim), e_lo(dim), e_hi(dim), scratch(dim);
    if ((st = mmcmc_split_rhat_mean_ess(d_a, 1, MMCMC_F32, n_chains, n, dim, r_bulk.data(), e_bulk.data(), device, stream_v)) !=
            MMCMC_OK ||
        (st = mmcmc_split_rhat_mean_ess(d_b, 1, MMCMC_F32, n_chains, n, dim, r_fold.data(), scratch.data(), device, stream_v)) !=
            MMCMC_OK)
        return st;
    MM_HIP(hipMemcpyAsync(d_q, q_tail.data(), 2 * dim * sizeof(double), hipMemcpyHostToDevice, stream));
    const unsigned int ib = (unsigned int)std::min<size_t>((total + 255) / 256, 8192);
    if (dtype == MMCMC_F32) {
        hipLaunchKernelGGL(mm_rank_indicator_kernel<float>, dim3(ib), dim3(256), 0, stream, (const float *)d_sample, total,
                           (uint32_t)dim, d_q, d_a);
        hipLaunchKernelGGL(mm_rank_indicator_kernel<float>, dim3(ib), dim3(256), 0, stream, (const float *)d_sample, total,
                           (uint32_t)dim, d_q + dim, d_b);
    } else {
        hipLaunchKernelGGL(mm_rank_indicator_kernel<double>, dim3(ib), dim3(256), 0, stream, (const double *)d_sample, total,
                           (uint32_t)dim, d_q, d_a);
        hipLaunchKernelGGL(mm_rank_indicator_kernel<double>, dim3(ib), dim3(256), 0, stream, (const double *)d_sample, total,
                           (uint32_t)dim, d_q + dim, d_b);
    }
    MM_HIP(hipGetLastError());
    if ((st = mmcmc_split_rhat_mean_ess(d_a, 1, MMCMC_F32, n_chains, n, dim, scratch.data(), e_lo.data(), device, stream_v)) !=
            MMCMC_OK ||
        (st = mmcmc_split_rhat_mean_ess(d_b, 1, MMCMC_F32, n_chains, n, dim, scratch.data(), e_hi.data(), device, stream_v)) !=
            MMCMC_OK)
        return st;
    MM_HIP(hipStreamSynchronize(stream));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t d = 0; d < dim; ++d) {
        /* the conventional sqrt(var+ / W): the inverse of the reference's (quirk Q7), as standard_split_rhat reports it */
        const float rb = flagged[d] ? nan : 1.0f / r_bulk[d], rf = flagged[d] ? nan : 1.0f / r_fold[d];
        const float eb = flagged[d] ? nan : e_bulk[d], el = flagged[d] ? nan : e_lo[d], eh = flagged[d] ? nan : e_hi[d];
        if (rhat_rank)
            rhat_rank[d] = (rb != rb || rf != rf) ? nan : (rb > rf ? rb : rf);
        if (rhat_parts) {
            rhat_parts[d] = rb;
            rhat_parts[dim + d] = rf;
        }
        if (ess_bulk)
            ess_bulk[d] = eb;
        if (ess_tail)
            ess_tail[d] = (el != el || eh != eh) ? nan : (el < eh ? el : eh);
        if (ess_tail_parts) {
            ess_tail_parts[d] = el;
            ess_tail_parts[dim + d] = eh;
        }
    }
    return MMCMC_OK;
}

} /* extern "C" */

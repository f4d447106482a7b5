/*
 * mm_draw_stats.hip -- per-chain summary of NUTS's per-draw records (include/mmcmc.h: mmcmc_nuts_draw,
 * mmcmc_nuts_draw_summary): counts of transitions, divergences and depth-cap hits, leapfrog total, the means of the
 * acceptance statistic and of the step size, and the energy Bayesian fraction of missing information (E-BFMI).
 *
 * One wave per chain.  A chain's records are contiguous, 16 bytes each: a trip of the wave is one 16-byte load per lane,
 * 1 KB per wave.  Every sum is float64.  The denominator of E-BFMI, sum (E_t - mean)^2, is two-pass: the first pass over
 * the chain gives the mean (with every other sum), the second reads the records again -- a chain of a few thousand rows
 * is a few tens of KB and comes back from L2.  The numerator, sum (E_t - E_{t-1})^2, needs each lane's left neighbour: it
 * comes from the lane below (__shfl_up), and lane 0 takes the last lane's energy of the previous trip, which the wave
 * carries along, so no record is loaded twice for it.  Integer fields are summed as integers.
 */
#include "mm_host.h"

#include <cstdint>
#include <limits>

namespace {

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}
__device__ __forceinline__ unsigned int wave_max(unsigned int v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return __shfl(v, 0, 64);
}

/* rec [n_chains, n_rows] as uint4 = (accept_stat, step_size, energy, tree); out [n_chains] */
__global__ __launch_bounds__(64 * kWavesPerBlock) void mm_draw_summary_kernel(const uint4 *__restrict__ rec, unsigned long long n_chains,
                                                                               unsigned long long n_rows,
                                                                               mmcmc_nuts_chain_summary *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long c = (unsigned long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (c >= n_chains) /* the whole wave: a partial last block */
        return;
    const uint4 *const row = rec + c * n_rows;
    const unsigned long long trips = (n_rows + 63) / 64;

    /* first pass: everything but the two sums of squares */
    double s_e = 0.0, s_acc = 0.0, s_eps = 0.0;
    unsigned long long n_lf = 0;
    unsigned int n_tr = 0, n_div = 0, n_cap = 0, max_depth = 0;
    for (unsigned long long k = 0; k < trips; ++k) {
        const unsigned long long i = k * 64 + lane;
        if (i < n_rows) {
            const uint4 r = row[i];
            if (!(r.w >> 31)) {
                const unsigned int depth = (r.w >> 16) & 15u;
                n_tr += 1u;
                n_div += (r.w >> 24) & 1u;
                n_cap += (r.w >> 25) & 1u;
                max_depth = depth > max_depth ? depth : max_depth;
                n_lf += r.w & 0xffffu;
                s_acc += (double)__uint_as_float(r.x);
                s_eps += (double)__uint_as_float(r.y);
                s_e += (double)__uint_as_float(r.z);
            }
        }
    }
    const unsigned long long tr = wave_sum((unsigned long long)n_tr), dv = wave_sum((unsigned long long)n_div),
                             cp = wave_sum((unsigned long long)n_cap);
    n_lf = wave_sum(n_lf);
    max_depth = wave_max(max_depth);
    s_acc = wave_sum(s_acc);
    s_eps = wave_sum(s_eps);
    s_e = wave_sum(s_e);
    const double mean_e = s_e / (double)tr;

    /* second pass: sum (E - mean)^2 over the transitions, sum (E_t - E_{t-1})^2 over the rows whose predecessor is a
     * transition too (the one record without a transition is row 0, which has no predecessor) */
    double den = 0.0, num = 0.0, carry_e = 0.0;
    int carry_has = 0;
    for (unsigned long long k = 0; k < trips; ++k) {
        const unsigned long long i = k * 64 + lane;
        double e = 0.0;
        int has = 0;
        if (i < n_rows) {
            const uint4 r = row[i];
            has = (r.w >> 31) ? 0 : 1;
            e = (double)__uint_as_float(r.z);
        }
        double prev_e = __shfl_up(e, 1, 64);
        int prev_has = __shfl_up(has, 1, 64);
        if (lane == 0) {
            prev_e = carry_e;
            prev_has = carry_has;
        }
        if (has) {
            const double d = e - mean_e;
            den += d * d;
            if (prev_has) {
                const double q = e - prev_e;
                num += q * q;
            }
        }
        carry_e = __shfl(e, 63, 64);
        carry_has = __shfl(has, 63, 64);
    }
    den = wave_sum(den);
    num = wave_sum(num);
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        mmcmc_nuts_chain_summary s;
        s.n_transitions = (uint32_t)tr;
        s.n_divergent = (uint32_t)dv;
        s.n_depth_cap = (uint32_t)cp;
        s.max_depth_seen = max_depth;
        s.n_leapfrog = n_lf;
        s.mean_accept = tr ? s_acc / (double)tr : nan;
        s.mean_step = tr ? s_eps / (double)tr : nan;
        s.ebfmi = (tr >= 2 && den != 0.0) ? num / den : nan;
        out[c] = s;
    }
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p)
            (void)hipFree(p);
    }
};

} // namespace

extern "C" int mmcmc_nuts_draw_summary(const mmcmc_nuts_draw *rec, int rec_is_device, size_t n_chains, size_t n_rows, int device,
                                       mmcmc_nuts_chain_summary *out)
{
    if (!out || n_chains == 0 || (!rec && n_rows != 0) || (rec_is_device && ((uintptr_t)rec & 15u))) /* 16-byte loads */
        return MMCMC_ERR_INVALID_ARG;
    const int dc = mm_check_device(device);
    if (dc != MMCMC_OK)
        return dc;
    /* rows < 2^32 (the counters are uint32_t), and the byte count must fit size_t */
    if ((uint64_t)n_rows >= (1ull << 32) || (n_rows != 0 && n_chains > std::numeric_limits<size_t>::max() / sizeof(mmcmc_nuts_draw) / n_rows) ||
        (n_chains + kWavesPerBlock - 1) / kWavesPerBlock > 0x7fffffffull)
        return MMCMC_ERR_SHAPE;
    DevGuard g(device);
    if (!g.ok)
        return MMCMC_ERR_INVALID_ARG;
    const size_t bytes = n_chains * n_rows * sizeof(mmcmc_nuts_draw);
    DevBuf staged, d_out;
    const void *d_rec = rec;
    if (!rec_is_device && bytes) {
        MM_HIP(hipMalloc(&staged.p, bytes));
        MM_HIP(hipMemcpy(staged.p, rec, bytes, hipMemcpyHostToDevice));
        d_rec = staged.p;
    }
    MM_HIP(hipMalloc(&d_out.p, n_chains * sizeof(mmcmc_nuts_chain_summary)));
    const unsigned int grid = (unsigned int)((n_chains + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(mm_draw_summary_kernel, dim3(grid), dim3(64 * kWavesPerBlock), 0, nullptr, (const uint4 *)d_rec,
                       (unsigned long long)n_chains, (unsigned long long)n_rows, (mmcmc_nuts_chain_summary *)d_out.p);
    MM_HIP(hipGetLastError());
    MM_HIP(hipMemcpy(out, d_out.p, n_chains * sizeof(mmcmc_nuts_chain_summary), hipMemcpyDeviceToHost));
    return MMCMC_OK;
}

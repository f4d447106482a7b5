/*
 * mm_inst.inc -- instantiates the sampling kernels for one element type (MM_INST_T) and builds the dispatch
 * table the C ABI looks kernels up in.  Dimensions are compile-time so that a chain's vectors stay in VGPRs.
 */
#define MM_NOISE_SCALAR_CUBICS 1 /* mm_rng.h: the normals' cubics stay scalar (no pairing moves) */
#include "mm_kernels.h"
#include "mm_split_kernels.h"

/* the scheduled split kernel's launcher where it is instantiated, else null */
template <class T, class Tgt, int QP, int NN, int RBF, int NT, bool ON> struct mm_split_sched_fn {
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, hipStream_t) = nullptr;
};
template <class T, class Tgt, int QP, int NN, int RBF, int NT> struct mm_split_sched_fn<T, Tgt, QP, NN, RBF, NT, true> {
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, hipStream_t) =
        &mm_launch_run_split_sched<T, Tgt, QP, NN, RBF, NT>;
};

/* the scheduled PIPE = 2 launcher where variant 2 can be a handle's default: not above dim 16 (the plain kernel is the default
 * there) and not for the dense Gaussian at 16 / 32 (the lane-group kernel is; its f32 PIPE = 2 form spills with a schedule) */
template <class T, class Tgt, bool ON> struct mm_pp_sched_fn {
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, unsigned int, unsigned int,
                                       hipStream_t) = nullptr;
};
template <class T, class Tgt> struct mm_pp_sched_fn<T, Tgt, true> {
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, unsigned int, unsigned int,
                                       hipStream_t) = &mm_launch_run_sched<T, Tgt>;
};

/* the split kernel's launcher where it is instantiated (dim <= 8: the noise ring of larger dims does not fit), else null */
template <class T, class Tgt, int SAMPLER, int LCT, bool ON> struct mm_split_fn {
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, hipStream_t) = nullptr;
    static constexpr hipError_t (*sched)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, hipStream_t) = nullptr;
};
template <class T, class Tgt, int SAMPLER, int LCT> struct mm_split_fn<T, Tgt, SAMPLER, LCT, true> {
    /* f32: three noise waves per pair (1024-thread workgroups, four waves per SIMD; mm_split_kernels.h); f64 keeps one
     * (a 1024-thread workgroup caps a wave at 128 registers) */
    static constexpr int nn = sizeof(T) == 4 ? MM_SPLIT_NOISE_WAVES : 1;
    static constexpr int qp = SAMPLER == MM_SAMPLER_MH ? mm_split_mh_qp<T, Tgt::dim, nn>::value : 0;
    /* HMC with three noise waves, where it fits (f32, D <= 3): ring half 8 and two tiles, the last noise wave writes them out
     * (mm_split_hmc_pf: config 3 -2.5 %) */
    static constexpr bool pf = SAMPLER == MM_SAMPLER_HMC && nn == 3 && mm_split_hmc_pf<T, Tgt::dim>::ok;
    static constexpr hipError_t (*ptr)(const mm_run_args<T> &, hipStream_t) =
        &mm_launch_run_split<T, Tgt, SAMPLER, LCT, qp, nn, (pf ? 8 : 0), (pf ? 2 : MM_SPLIT_NTILE(SAMPLER == MM_SAMPLER_MH))>;
    /* the scheduled form of the run-time L HMC instance above (f32 only: the split kernel is the f32 default) */
    static constexpr hipError_t (*sched)(const mm_run_args<T> &, const mm_sched_step<T> *, unsigned int, hipStream_t) =
        mm_split_sched_fn<T, Tgt, qp, nn, (pf ? 8 : 0), (pf ? 2 : MM_SPLIT_NTILE(false)),
                          SAMPLER == MM_SAMPLER_HMC && LCT == 0 && sizeof(T) == 4>::ptr;
};

#define MM_ENTRY(KIND, DIM)                                                                                       \
    {                                                                                                             \
        KIND, DIM, &mm_launch_run<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, MM_SAMPLER_MH>,                     \
            &mm_launch_run<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, MM_SAMPLER_HMC>,                           \
            &mm_launch_run<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, MM_SAMPLER_MH, 2, 0>,                      \
            &mm_launch_run<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, MM_SAMPLER_HMC, 2, 0>,                     \
            /* the unrolled L = 10 integrator only where it is small: not at D >= 16, not for the dense Gaussian (D^2 terms) */ \
            &mm_launch_run<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, MM_SAMPLER_HMC, 2, ((DIM <= 8 && KIND != MM_GAUSSIAN_ND) ? 10 : 0)>, \
            &mm_launch_logp_grad<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>>,                                     \
            mm_tile<MM_INST_T, DIM>::lds_bytes_per_wave,                                                          \
            mm_split_fn<MM_INST_T, mm_target<MM_INST_T, KIND, (DIM <= 8 ? DIM : 1)>, MM_SAMPLER_MH, 0, (DIM <= 8)>::ptr,  \
            mm_split_fn<MM_INST_T, mm_target<MM_INST_T, KIND, (DIM <= 8 ? DIM : 1)>, MM_SAMPLER_HMC, 0, (DIM <= 8)>::ptr, \
            mm_split_fn<MM_INST_T, mm_target<MM_INST_T, KIND, (DIM <= 8 ? DIM : 1)>, MM_SAMPLER_HMC,                      \
                        ((DIM <= 8 && KIND != MM_GAUSSIAN_ND) ? 10 : 0), (DIM <= 8)>::ptr,                                \
            /* scheduled runs (mmcmc_hmc_run_scheduled): the run-time L instances read (eps, L) per transition */          \
            mm_pp_sched_fn<MM_INST_T, mm_target<MM_INST_T, KIND, DIM>, (DIM <= 16 && !(KIND == MM_GAUSSIAN_ND && DIM >= 16))>::ptr, \
            mm_split_fn<MM_INST_T, mm_target<MM_INST_T, KIND, (DIM <= 8 ? DIM : 1)>, MM_SAMPLER_HMC, 0, (DIM <= 8)>::sched \
    }

#define MM_ENTRY_ND(KIND)                                                                                         \
    MM_ENTRY(KIND, 1), MM_ENTRY(KIND, 2), MM_ENTRY(KIND, 3), MM_ENTRY(KIND, 4), MM_ENTRY(KIND, 5),                \
        MM_ENTRY(KIND, 6), MM_ENTRY(KIND, 7), MM_ENTRY(KIND, 8), MM_ENTRY(KIND, 16), MM_ENTRY(KIND, 32)

static const mm_kernel_entry<MM_INST_T> g_table[] = {
    MM_ENTRY(MM_GAUSSIAN2D, 2),
    MM_ENTRY(MM_DIFFABLE_GAUSSIAN2D, 2),
    MM_ENTRY(MM_ROSENBROCK2D, 2),
    MM_ENTRY_ND(MM_ISOTROPIC_GAUSSIAN),
    MM_ENTRY_ND(MM_ROSENBROCK_ND),
    MM_ENTRY_ND(MM_STANDARD_NORMAL),
    MM_ENTRY_ND(MM_GAUSSIAN_ND),
};

#define MM_NOISE(DIM)                                                                                             \
    {                                                                                                             \
        DIM, &mm_launch_noise<MM_INST_T, DIM>                                                                     \
    }
static const mm_noise_entry<MM_INST_T> g_noise[] = {
    MM_NOISE(1), MM_NOISE(2), MM_NOISE(3), MM_NOISE(4), MM_NOISE(5), MM_NOISE(6), MM_NOISE(7), MM_NOISE(8),
    MM_NOISE(16), MM_NOISE(32),
};

/*
 * mmcmc.h -- C ABI of libmmcmc.so: the MI355X-native many-chain engine for mini-mcmc's per-chain inner loop.
 *
 * This is the drop-in boundary.  The reference (mini-mcmc v0.8.3, Rust) has no FFI of its own: its boundary is
 * the trait + constructor surface of the crate.  Each entry point below names the reference item it stands in
 * for (file:line in the reference tree); INTEGRATION.md shows the `extern "C"` block and the safe Rust wrapper
 * (`GpuMetropolisHastings`, `GpuHmc`, `GpuNuts`) a maintainer would add on top.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types; no exceptions cross the boundary
 *   - every function returns an int status: MMCMC_OK (0), negative = invalid argument / unsupported,
 *     positive = the hipError_t of the failing HIP call.  mmcmc_status_string() names them.
 *   - sample layout is the reference's: [n_chains, n_collect, dim] row-major (core.rs:176-186, hmc.rs:157)
 *   - a handle owns its device state (current positions, iteration counter, seed), so calling run() twice
 *     continues the chains exactly as the Rust sampler structs do
 *   - handles are not thread-safe; one handle = one device; `stream` arguments are hipStream_t passed as
 *     void* (NULL = the handle's own stream, a BLOCKING stream: it orders itself with work on the legacy default
 *     stream, so a caller working on the default stream -- e.g. torch's -- sees the results without a host
 *     synchronisation); run() is asynchronous when `out` is device memory and no host-side result (accept
 *     counts) is requested -- call mmcmc_*_sync() or synchronise the stream.
 *   - the library has NO CPU fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef MMCMC_H
#define MMCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101 (round 6): + mmcmc_{mh,hmc}_group_run_async, mmcmc_*_group_stats_phases, mmcmc_device_pci_bus_id,
 *   MMCMC_ERR_GROUP_BROKEN; mmcmc_*_group_run blocks again whatever its arguments (100 inferred "asynchronous" from
 *   out_host == NULL && accept_counts == NULL); mmcmc_nuts_set_repacking (100, measured slower, removed) stays removed.
 * 102 (round 6): + mmcmc_rtc_compiler_info; long-chain diagnostics take N1 = ceil(n/2 / 1024) residues (any count).
 * Later additions that keep 102 (a binding probes them with dlsym): mmcmc_hmc_set_step_size, mmcmc_hmc_set_n_leapfrog,
 *   mmcmc_hmc_params, mmcmc_hmc_set_state, mmcmc_hmc_run_scheduled; settable chain state and stream position
 *   ("chain state and stream position" below): mmcmc_mh_set_proposal_std, mmcmc_mh_params, mmcmc_mh_set_state,
 *   mmcmc_nuts_set_state, mmcmc_nuts_set_adapt_state, mmcmc_nuts_params, mmcmc_nuts_set_target_accept_p,
 *   mmcmc_mh_discrete_set_state, mmcmc_gibbs_mixture_set_state, mmcmc_{mh,hmc,nuts,mh_discrete,gibbs_mixture}_stream_position,
 *   mmcmc_{mh,hmc,nuts,mh_discrete,gibbs_mixture}_set_iteration, mmcmc_{mh,hmc,nuts}_group_set_state,
 *   mmcmc_{mh,hmc,nuts}_group_stream_position, mmcmc_{mh,hmc,nuts}_group_set_iteration, mmcmc_{mh,hmc,nuts}_group_params,
 *   mmcmc_hmc_group_set_step_size, mmcmc_hmc_group_set_n_leapfrog, mmcmc_mh_group_set_proposal_std,
 *   mmcmc_nuts_group_adapt_state, mmcmc_nuts_group_set_adapt_state, mmcmc_nuts_group_set_target_accept_p;
 *   rank-normalised diagnostics: mmcmc_rank_normalize, mmcmc_quantiles, mmcmc_rank_diagnostics;
 *   mmcmc_group_bind_collectives; the diagonal metric: mmcmc_{hmc,nuts}_set_metric, mmcmc_{hmc,nuts}_metric; the dense
 *   metric: mmcmc_{hmc,nuts}_set_metric_dense, mmcmc_{hmc,nuts}_metric_dense; NUTS's per-draw statistics:
 *   mmcmc_nuts_set_draw_stats, mmcmc_nuts_draw_stats_enabled, mmcmc_nuts_draw_stats, mmcmc_nuts_draw_summary,
 *   mmcmc_nuts_group_set_draw_stats.
 * A binding checks mmcmc_version() >= the version it was generated from (rust/mini-mcmc-hip: assert_abi, in every constructor). */
#define MMCMC_VERSION 102 /* 0.1.2 */

/* ---- status ---- */
#define MMCMC_OK 0
#define MMCMC_ERR_INVALID_ARG (-1)  /* NULL pointer, zero chains, negative count, ...            */
#define MMCMC_ERR_UNSUPPORTED (-2)  /* target kind / dim / dtype combination has no kernel        */
#define MMCMC_ERR_SHAPE (-3)        /* the analogue of ndarray::ShapeError from core.rs:184       */
#define MMCMC_ERR_NO_DEVICE (-4)    /* no HIP device: the engine never falls back to the CPU      */
#define MMCMC_ERR_STATE (-5)        /* call made in the wrong state (e.g. timing before any run)  */
#define MMCMC_ERR_GROUP_BROKEN (-6) /* a device group whose shards stand at different iterations (a run failed on some) */

/* ---- element types ---- */
#define MMCMC_F32 0
#define MMCMC_F64 1

/* ---- built-in targets: the closed registry standing in for `impl Target` / `impl BatchedGradientTarget`
 *      / `impl GradientTarget` (distributions.rs:65-108).  params[] meaning per kind:
 *   MMCMC_GAUSSIAN2D           mean0, mean1, cov00, cov01, cov10, cov11     distributions.rs:158-206
 *   MMCMC_DIFFABLE_GAUSSIAN2D  mean0, mean1, cov00, cov01, cov10, cov11     distributions.rs:212-316
 *   MMCMC_ISOTROPIC_GAUSSIAN   std                                          distributions.rs:344-402
 *   MMCMC_ROSENBROCK2D         a, b                                         distributions.rs:490-524
 *   MMCMC_ROSENBROCK_ND        (none)                                       distributions.rs:528-547
 *   MMCMC_STANDARD_NORMAL      (none)                                       nuts.rs:1024-1037 (test target)
 *   MMCMC_GAUSSIAN_ND          matrix = precision A, row-major dim x dim    (not in the reference; config 5) */
#define MMCMC_GAUSSIAN2D 0
#define MMCMC_DIFFABLE_GAUSSIAN2D 1
#define MMCMC_ISOTROPIC_GAUSSIAN 2
#define MMCMC_ROSENBROCK2D 3
#define MMCMC_ROSENBROCK_ND 4
#define MMCMC_STANDARD_NORMAL 5
#define MMCMC_GAUSSIAN_ND 6

typedef struct mmcmc_target_desc {
    int32_t kind;
    int32_t dim;
    double params[8];
    const double *matrix; /* host pointer, only for MMCMC_GAUSSIAN_ND */
} mmcmc_target_desc;

/* `impl Proposal` (distributions.rs:92-101): the reference's IsotropicGaussian (distributions.rs:344-392), or a kind
 * handed out by mmcmc_proposal_register_source (>= MMCMC_USER_PROPOSAL_BASE): a proposal of the caller's own, `std` = its
 * one run-time parameter */
#define MMCMC_PROPOSAL_ISOTROPIC_GAUSSIAN 0
#define MMCMC_USER_PROPOSAL_BASE 1000
typedef struct mmcmc_proposal_desc {
    int32_t kind;
    int32_t reserved;
    double std;
} mmcmc_proposal_desc;

/* summary of one diagnostic (stats.rs:373-381 BasicStats) */
typedef struct mmcmc_basic_stats {
    float min, median, max, mean, std;
} mmcmc_basic_stats;
/* stats.rs:338-342 RunStats */
typedef struct mmcmc_run_stats {
    mmcmc_basic_stats ess;
    mmcmc_basic_stats rhat;
} mmcmc_run_stats;

/* timing of the most recent run(): device time of the sampling kernel(s), measured with HIP events on the
 * stream the kernels were launched on */
typedef struct mmcmc_timing {
    float kernel_ms;      /* sum over launches */
    uint32_t n_launches;
    uint32_t reserved;
    uint64_t out_bytes;   /* sample bytes written by the kernels */
    uint64_t state_bytes; /* chain state bytes loaded + stored */
} mmcmc_timing;

/* ---- library ---- */
int mmcmc_version(void);
const char *mmcmc_status_string(int status);
int mmcmc_device_count(int *count);
/* hipDeviceGetPCIBusId of `device` as "dddd:bb:dd.f" into buf (len >= 16): a scaling run prints it per shard so that two
 * "devices" that are one GPU cannot pass for two */
int mmcmc_device_pci_bus_id(int device, char *buf, size_t len);

/* ---- core.rs:394-435  init_with_seed / init_det (seed 42): n*d StandardNormal draws of the reference's own
 *      stream (rand 0.9 SmallRng = xoshiro256++, rand_distr 0.5 ziggurat), row-major, as double. Host only. */
int mmcmc_init_with_seed(size_t n, size_t d, uint64_t seed, double *out);

/* ---- Metropolis-Hastings -----------------------------------------------------------------------------
 * MetropolisHastings::new(target, proposal, initial_states)   metropolis_hastings.rs:149-159
 * init: host, [n_chains, dim] of `dtype` elements */
typedef struct mmcmc_mh mmcmc_mh;
int mmcmc_mh_create(mmcmc_mh **out, const mmcmc_target_desc *target, const mmcmc_proposal_desc *proposal,
                    const void *init, size_t n_chains, int dtype, int device);
/* MetropolisHastings::seed   metropolis_hastings.rs:187-193 */
int mmcmc_mh_seed(mmcmc_mh *h, uint64_t seed);
/* multi-GPU sharding: global id of this handle's first chain (stream key = chain_offset + local index) */
int mmcmc_mh_set_chain_offset(mmcmc_mh *h, uint64_t chain_offset);
/* ChainRunner::run(n_collect, n_discard) -> Array3 [n_chains, n_collect, dim]   core.rs:176-186 (+ :55-73)
 * out: [n_chains, n_collect, dim] of dtype, device memory if out_is_device else host (may be NULL: no samples).
 * accept_counts: host, [n_chains], accepted proposals per chain over the whole call (may be NULL). */
int mmcmc_mh_run(mmcmc_mh *h, size_t n_collect, size_t n_discard, void *out, int out_is_device,
                 uint64_t *accept_counts, void *stream);
/* the same into rows [row0, row0 + n_rows) of a DEVICE buffer out [n_chains, n_total_rows, dim]: one sample filled by
 * several launches (run_progress' segments); n_rows = 0 with n_discard > 0 only advances the chains */
int mmcmc_mh_run_rows(mmcmc_mh *h, size_t n_rows, size_t n_discard, void *out_device, size_t n_total_rows, size_t row0,
                      void *stream);
/* what the handle was created with (any pointer may be NULL) */
int mmcmc_mh_shape(mmcmc_mh *h, size_t *n_chains, int *dim, int *dtype, int *device);
/* MarkovChain::current_state for every chain   core.rs:43-44 ; host [n_chains, dim] */
int mmcmc_mh_state(mmcmc_mh *h, void *out);
int mmcmc_mh_sync(mmcmc_mh *h);
int mmcmc_mh_timing(mmcmc_mh *h, mmcmc_timing *t);
/* run() brackets its launches with two HIP events for mmcmc_*_timing (default on); off = no event packets on the
 * stream between back-to-back runs (mmcmc_*_timing then returns MMCMC_ERR_STATE) */
int mmcmc_mh_enable_timing(mmcmc_mh *h, int on);
int mmcmc_mh_destroy(mmcmc_mh *h);

/* ---- HMC ---------------------------------------------------------------------------------------------
 * HMC::new(target, initial_positions, step_size, n_leapfrog)   hmc.rs:87-109 */
typedef struct mmcmc_hmc mmcmc_hmc;
int mmcmc_hmc_create(mmcmc_hmc **out, const mmcmc_target_desc *target, const void *init, size_t n_chains,
                     double step_size, int n_leapfrog, int dtype, int device);
/* HMC::set_seed   hmc.rs:118-121 (inert in the reference, quirk Q6; here it keys the stream) */
int mmcmc_hmc_seed(mmcmc_hmc *h, uint64_t seed);
int mmcmc_hmc_set_chain_offset(mmcmc_hmc *h, uint64_t chain_offset);
/* HMC::run(n_collect, n_discard) -> Tensor [n_chains, n_collect, dim]   hmc.rs:137-158 */
int mmcmc_hmc_run(mmcmc_hmc *h, size_t n_collect, size_t n_discard, void *out, int out_is_device,
                  uint64_t *accept_counts, void *stream);
int mmcmc_hmc_run_rows(mmcmc_hmc *h, size_t n_rows, size_t n_discard, void *out_device, size_t n_total_rows, size_t row0,
                       void *stream);
int mmcmc_hmc_shape(mmcmc_hmc *h, size_t *n_chains, int *dim, int *dtype, int *device);
/* HMC::step   hmc.rs:304-377 : one transition of every chain */
int mmcmc_hmc_step(mmcmc_hmc *h, void *stream);
/* HMC::positions   hmc.rs:49 ; host [n_chains, dim] */
int mmcmc_hmc_state(mmcmc_hmc *h, void *out);
int mmcmc_hmc_sync(mmcmc_hmc *h);
int mmcmc_hmc_timing(mmcmc_hmc *h, mmcmc_timing *t);
int mmcmc_hmc_enable_timing(mmcmc_hmc *h, int on);
int mmcmc_hmc_destroy(mmcmc_hmc *h);

/* The reference's public fields (hmc.rs:41-49: pub step_size, pub n_leapfrog, pub positions) as setters, and scheduled runs.
 * These entry points are additive: MMCMC_VERSION stays 102, and a binding that must also load an older library probes them
 * with dlsym.  None of them touches the seed, the chain offset or the iteration counter.
 *   set_step_size / set_n_leapfrog: mmcmc_hmc_create's checks (step size finite and > 0, n_leapfrog >= 0); they apply from
 *     the next transition on.  mmcmc_hmc_params reads both back (either pointer may be NULL).
 *   set_state: [n_chains, dim] of the handle's dtype, host memory (is_device = 0; copied before the call returns) or device
 *     memory on the handle's device (is_device = 1), ordered on `stream` (NULL: the handle's own) like a run.
 *   run_scheduled: step_sizes / n_leapfrogs are host arrays of n_discard + n_collect entries.  Defined as, for each k: set
 *     (step_sizes[k], n_leapfrogs[k]), do one transition, keep the state as sample row k - n_discard when k >= n_discard --
 *     and equal to that loop bit for bit (samples, final state, accept counts, iteration counter).  Afterwards the handle's
 *     own step size and leapfrog count are what they were.  Output arguments as mmcmc_hmc_run.  The default kernels of the
 *     fixed-dimension targets (variants 5 and 2) read the pair per transition in one launch; every other variant runs one
 *     launch per maximal run of equal pairs (one per transition at worst). */
int mmcmc_hmc_set_step_size(mmcmc_hmc *h, double step_size);
int mmcmc_hmc_set_n_leapfrog(mmcmc_hmc *h, int n_leapfrog);
int mmcmc_hmc_params(mmcmc_hmc *h, double *step_size, int *n_leapfrog);
int mmcmc_hmc_set_state(mmcmc_hmc *h, const void *positions, int is_device, void *stream);
int mmcmc_hmc_run_scheduled(mmcmc_hmc *h, size_t n_collect, size_t n_discard, const double *step_sizes,
                            const int32_t *n_leapfrogs, void *out, int out_is_device, uint64_t *accept_counts, void *stream);

/* A diagonal mass matrix for HMC and NUTS (not in the reference, which integrates with the identity metric).  Additive as the
 * setters above: MMCMC_VERSION stays 102; seed, chain offset, iteration counter and NUTS's adaptation records are untouched.
 *   The metric is a scale per coordinate, scale[dim] (host doubles), each finite and > 0 -- also once converted to the
 *     handle's element type (HMC) / tensor type (NUTS), which happens once, here.  It is M = diag(1 / s_i^2) written in whitened
 *     momentum: the noise stream, the kinetic energy 1/2 sum p_i^2 and the accept rule stay as they are, and only the step
 *     length becomes per-coordinate, e_i = eps * s_i (one multiplication in the element type), h_i = e_i / 2:
 *       HMC:  first kick p_i = fma(h_i, g_i, p_i), drift x_i = fma(e_i, p_i, x_i), kick p_i = fma(last ? h_i : e_i, g_i, p_i);
 *       NUTS: the leapfrog (the step-size search of init_chain goes through it) with e_i = +-eps * s_i, and the stop
 *             criterion with diff_i = (x_plus_i - x_minus_i) * r_i, r_i = 1 / s_i in the tensor type; the summation order,
 *             dual averaging, the slice variable and the tree bookkeeping are untouched.
 *     With a metric of the target's posterior standard deviations a step size of order 1 is the natural scale.
 *   A metric of all ones gives the bits of a handle without one.  NULL removes the metric.
 *   It applies from the next transition on and to everything that advances the handle: step, run, run_rows, run_progress,
 *     and run_scheduled (one launch per maximal run of equal pairs).
 *   Every value is checked before anything changes: a non-finite or non-positive one returns MMCMC_ERR_INVALID_ARG.
 *   Kernels: a handle with a metric runs a unit compiled at run time on the first set_metric of its (target kind, dimension)
 *     -- seconds, once per process -- around the target's own functor (a built-in kind, or a kind registered from source:
 *     plain, log-density alone, with data), verified bit for bit before the handle relies on it.  While a metric is set
 *     the handle's kernel variant is 7 and set_kernel_variant to anything else returns MMCMC_ERR_UNSUPPORTED; after NULL the
 *     handle has its previous variant again.  MMCMC_ERR_UNSUPPORTED, and nothing changed: a dimension above 32, no run-time
 *     compiler on the machine, a unit that fails its check.  Device groups have no metric.
 *   mmcmc_*_metric writes scale_out[dim] -- the doubles last set, ones when none is -- and returns 1 if a metric is set, 0 if
 *     not, < 0 on error. */
int mmcmc_hmc_set_metric(mmcmc_hmc *h, const double *scale); /* [dim], or NULL = identity */
int mmcmc_hmc_metric(mmcmc_hmc *h, double *scale_out);
/* A dense mass matrix from a Cholesky factor.  Additive as the diagonal metric: MMCMC_VERSION stays 102.
 *   chol is a lower-triangular factor L, row-major [dim, dim] host doubles, with positive diagonal: Sigma = L L^T stands for the
 *     posterior covariance, M = Sigma^-1, written in whitened momentum exactly as the diagonal metric is -- noise, kinetic
 *     energy 1/2 sum p_i^2 and accept rule untouched:
 *       HMC:  drift x_i = fma(eps, (L p)_i, x_i); kick p_j = fma(k, (L^T g)_j, p_j), k = eps / 2 for the first and the last kick
 *             and eps for the merged ones;
 *       NUTS: the leapfrog (and so the step-size search) with the same two products and eps signed; the stop criterion with
 *             diff = L^-1 (x_plus - x_minus).  L^-1 is formed once, here, in float64 by forward substitution and then converted
 *             to the tensor type.
 *     Every sum starts at its diagonal term and takes the others by ascending index, each with one fma (mm_samplers.h):
 *     an identity factor gives the bits of a handle without a metric, a factor diag(s) with every s_i a power of two the bits
 *     of the diagonal metric s.
 *   One metric per handle: a dense one replaces a diagonal one and the other way round; NULL to either setter removes
 *     whichever is set, and the handle has the variant it had before.  What a metric applies to is as above.
 *   Every check happens before any change.  MMCMC_ERR_INVALID_ARG: a non-finite entry, a non-zero entry above the diagonal, a
 *     diagonal entry <= 0, a factor or inverse that is not finite with positive diagonal once converted to the handle's
 *     element type (HMC) / tensor type (NUTS).  MMCMC_ERR_UNSUPPORTED, nothing changed: a dimension above 32, no run-time
 *     compiler, a unit that fails its check.  Device groups and MH have no metric.
 *   Kernels: a dense-metric unit of its own, compiled on the first set_metric_dense of a (target kind, dimension) and
 *     verified bit for bit before the handle relies on it; the variant is 7 while the metric is set.
 *   mmcmc_*_metric_dense writes chol_out[dim * dim], the doubles last set, and returns 1; returns 0 and writes nothing if no
 *     dense metric is set; < 0 on error.  While a dense metric is set mmcmc_*_metric returns 2 and writes the marginal standard
 *     deviations, the row norms of L. */
int mmcmc_hmc_set_metric_dense(mmcmc_hmc *h, const double *chol); /* row-major dim x dim; NULL removes the metric */
int mmcmc_hmc_metric_dense(mmcmc_hmc *h, double *chol_out);

/* ---- NUTS ------------------------------------------------------------------------------------------------
 * NUTS::new(target, initial_positions, target_accept_p)   nuts.rs:123-129 over NUTSChain::new nuts.rs:410-434.
 * init: host [n_chains, dim] doubles (the reference's Vec<Vec<T>>).  mode selects the reference's type split:
 *   0 = f32 tensors + f64 scalars  (`NUTS<f64, Autodiff<NdArray>, _>`: NdArray elements are f32)
 *   1 = f32 tensors + f32 scalars  (`NUTS<f32, Autodiff<NdArray>, _>`)
 *   2 = f64 tensors + f64 scalars  (BASELINE.json config 5 "f64"; no default reference backend has f64 elements)
 * Samples are of the tensor type (f32 for modes 0/1, f64 for mode 2).
 * Any bits are accepted as a start, here and by mmcmc_nuts_set_state.  A chain whose start has no real log-density in the
 *   tensor type -- a NaN or infinite coordinate, or a finite one where the density overflows -- does not move: the step-size
 *   search (nuts.rs:695-761, which in the reference never returns from such a start) ends with epsilon = 0, every
 *   transition stops at its first leaf (1 leapfrog), every collected row is the start, bit for bit, and the run ends.
 *   The other chains of the handle are not affected. */
typedef struct mmcmc_nuts mmcmc_nuts;
int mmcmc_nuts_create(mmcmc_nuts **out, const mmcmc_target_desc *target, const double *init, size_t n_chains,
                      double target_accept_p, int mode, int device);
/* the diagonal metric: see mmcmc_hmc_set_metric.  A search of the step size (epsilon = -1 in the adaptation records) that runs
 * after the metric is set runs under it. */
int mmcmc_nuts_set_metric(mmcmc_nuts *h, const double *scale); /* [dim], or NULL = identity */
int mmcmc_nuts_metric(mmcmc_nuts *h, double *scale_out);
/* the dense metric: see mmcmc_hmc_set_metric_dense */
int mmcmc_nuts_set_metric_dense(mmcmc_nuts *h, const double *chol); /* row-major dim x dim; NULL removes the metric */
int mmcmc_nuts_metric_dense(mmcmc_nuts *h, double *chol_out);
/* NUTS::set_seed   nuts.rs:347-353 (keys the counter-based stream; chains differ by their global index) */
int mmcmc_nuts_seed(mmcmc_nuts *h, uint64_t seed);
int mmcmc_nuts_set_chain_offset(mmcmc_nuts *h, uint64_t chain_offset);
/* maximum tree depth (doublings per transition), 1..12, default 10.  The reference's `while s` (nuts.rs:578) is
 * unbounded; a lane that never terminates would stall its whole wave, so the engine caps it. */
int mmcmc_nuts_set_max_depth(mmcmc_nuts *h, int max_depth);
/* Kernel mapping (not in the reference).  0 = one chain per lane, the lanes of a wave taking their transitions in step
 * (every target / mode); 4 = one chain per lane, every lane advancing through its transitions on its own, one leaf per
 * tick (dim <= 8; results identical to 0); 5 = the same with the leaves taken in pairs, level 0 of the pending-subtree
 * stack in registers and the auxiliary uniforms in an LDS ring (dim <= 8; the default there; results identical to 0
 * and 4).  6 = one chain per lane at RUN-TIME dimension, the
 * transition's vectors in an HBM store (csrc/mm_nuts_generic.h): the N-dimensional built-in targets (isotropic / standard
 * / dense Gaussian, RosenbrockND) at ANY dimension, all three modes; the default where there is no compiled instance of
 * 0 (those exist for every dim <= 8 and 10, 16, 20, 24 / 32 for the dense Gaussian), selectable everywhere, results
 * identical to 0 where both exist.  1 = lane-group mapping with
 * the gradient on the matrix cores: 16 chains per wave, four lanes per chain, v_mfma_f64_16x16x4 for A x, the whole
 * run in one launch, every wave keeping its 16 chains.  2 and 3 = the same arithmetic with tree-depth compaction
 * (BASELINE.json config 5): a transition is cut at the doubling boundaries and the chains that still double are
 * re-packed into full waves -- 2: one launch per tree level and transition; 3: one persistent kernel whose waves take
 * work units from per-level queues, chains advancing independently of each other (the fastest from a few thousand
 * chains on; below 2048 chains it runs as 1).
 * 1..3 exist for mode 2 + MMCMC_GAUSSIAN_ND with dim 16 or 32, where 3 is the default; elsewhere setting them returns
 * MMCMC_ERR_UNSUPPORTED (so do 4 and 5 above dim 8).  1, 2 and 3 give bit-identical results.  They sum the D-term dot products in a different
 * order than 0 (four interleaved partial sums vs sequential), so their samples differ from 0's in the last bits and,
 * over long trajectories of a stiff target, visibly; each is bit-exact against its own host build
 * (oracle/engine_host.cpp modes 3 and 2).  With variant 3 mmcmc_nuts_run returns after the kernel has finished.
 * 7 (the default of targets compiled at run time: mmcmc_target_register_source, and built-in targets at dimensions 9 .. 31
 * without a compiled instance): the asynchronous-lane kernel with the leaves in pairs (as 5), compiled with the target's functor
 * on first use.  A unit is checked once against the run-time-dimension kernel (6), bit for bit, before a handle relies on
 * it; if that fails a built-in target runs 6 and a user target is refused (MMCMC_ERR_UNSUPPORTED).
 * mmcmc_nuts_kernel_variant returns the mapping in use (>= 0) or a negative status.
 * mmcmc_nuts_set_compaction (variants 2, 3): doublings below `first_level` run before the first re-packing (default 5;
 * variant 3, until this is called, picks the mode of the depths seen so far minus one, after a 16-transition pilot on a
 * fresh handle); variant 2 splits the chains into `n_groups` contiguous groups (1..16; 0 = one per 16 384 chains), each
 * with its own launch sequence on its own stream.  Neither setting changes a result. */
int mmcmc_nuts_set_kernel_variant(mmcmc_nuts *h, int variant);
int mmcmc_nuts_kernel_variant(mmcmc_nuts *h);
int mmcmc_nuts_set_compaction(mmcmc_nuts *h, int first_level, int n_groups);
/* progress = 0: NUTS::run -> NUTSChain::run (nuts.rs:163-170, 457-471): n_collect + n_discard - 1 transitions, and
 *               with n_discard == 0 row 0 is the initial position (the reference's off-by-one, test_chain_1);
 * progress = 1: the stepping of run_progress (nuts.rs:491-522): all n_collect + n_discard transitions;
 * progress = 2: the same with EVERY state recorded, burn-in included (what run_progress' per-chain trackers are fed,
 *               nuts.rs:491-506): out then has n_collect + n_discard rows per chain.
 * out: [n_chains, n_collect, dim] of the tensor type, device or host memory (may be NULL). */
int mmcmc_nuts_run(mmcmc_nuts *h, size_t n_collect, size_t n_discard, void *out, int out_is_device, int progress,
                   void *stream);
int mmcmc_nuts_shape(mmcmc_nuts *h, size_t *n_chains, int *dim, int *mode, int *device);
/* NUTSChain::position for every chain (nuts.rs:369); host [n_chains, dim] of the tensor type */
int mmcmc_nuts_state(mmcmc_nuts *h, void *out);
/* per-chain adaptation state: host [n_chains, 4] doubles = epsilon, epsilon_bar, h_bar, mu (nuts.rs:374-386) */
int mmcmc_nuts_adapt_state(mmcmc_nuts *h, double *out);
/* diagnostics (not in the reference): gradient evaluations per chain so far; histogram[13] of tree depths */
int mmcmc_nuts_leapfrog_counts(mmcmc_nuts *h, uint64_t *out);
int mmcmc_nuts_depth_histogram(mmcmc_nuts *h, uint32_t *out);
int mmcmc_nuts_sync(mmcmc_nuts *h);
int mmcmc_nuts_timing(mmcmc_nuts *h, mmcmc_timing *t);
int mmcmc_nuts_destroy(mmcmc_nuts *h);

/* Per-draw sampler statistics (not in the reference).  Additive: MMCMC_VERSION stays 102.
 * One 16-byte record per chain and per ROW of the sample that mmcmc_nuts_run / mmcmc_nuts_run_progress returns, laid out
 * [n_chains, n_rows] and indexed exactly like the sample's first two axes. */
typedef struct mmcmc_nuts_draw {
    float accept_stat; /* alpha / n_alpha exactly as dual averaging is fed it (the last doubling only, the kept quirk), computed in the
                          scalar type, converted once */
    float step_size;   /* the epsilon this transition's tree was built with, scalar type -> float */
    float energy;      /* the Hamiltonian level of the trajectory: -(logp(x) - 1/2 p0.p0) at the transition's start, x the position
                          before it and p0 the momentum drawn for it -- the level the tree holds, exact; NOT evaluated at the
                          selected point.  Scalar type -> float */
    uint32_t tree;     /* bits 0..15 leapfrog steps of this transition (<= 4095), 16..19 tree depth, 24 divergent, 25 depth cap,
                          31 no transition */
} mmcmc_nuts_draw;
/*   divergent (bit 24): some leaf of the transition left the slice by more than 1000, (ln u - 1000) < joint' failed (a NaN
 *     joint' fails it); such a leaf ends the tree, so there is at most one.  depth cap (bit 25): depth >= max_depth.
 *   no transition (bit 31): the row is not the result of a transition -- row 0 of a progress = 0 run with n_discard == 0, the
 *     initial position.  Its floats are NaN except step_size, which holds the current epsilon; its other bits are 0.
 * mmcmc_nuts_set_draw_stats(h, on): recording from the next run on; off frees the buffer.  The handle owns a device buffer of
 *   n_chains * n_rows * 16 bytes that grows on demand: 420 MB at 65 536 chains x 400 rows, more than that run's 3-D f32
 *   sample.  Recording changes no result and touches nothing else: seed, chain offset, iteration counter, adaptation records,
 *   leapfrog counts, depth histogram and checkpoints are what they are without it.
 *   While recording is on the handle runs the stats unit of its target, compiled on the first enable of a (target kind,
 *   dimension, compiler, metric kind) and verified bit for bit before use: mmcmc_nuts_kernel_variant reports 7,
 *   set_kernel_variant to anything else returns MMCMC_ERR_UNSUPPORTED, and the variant the handle had comes back when
 *   recording is switched off.  A metric may be set or cleared while recording is on and the other way round; each setter
 *   leaves the other's state intact.  MMCMC_ERR_UNSUPPORTED, and nothing changed: a dimension above 32, no run-time compiler,
 *   a unit that does not build or fails its verification.  Device groups do not record (mmcmc_nuts_group_set_draw_stats).
 * mmcmc_nuts_draw_stats_enabled: 1 / 0, or a negative status.
 * mmcmc_nuts_draw_stats: the records of the last run made with recording on, [n_chains, *n_rows], to host or device memory
 *   (16-byte aligned); out may be NULL to ask for n_rows alone.  MMCMC_ERR_SHAPE if there was no such run.  Waits for the run.
 * mmcmc_nuts_draw_summary: per chain, over the records that have a transition, on `device` (one wave per chain, float64
 *   sums): rec [n_chains, n_rows] in host or device memory, out host [n_chains].  ebfmi = sum_{t >= 2} (E_t - E_{t-1})^2 /
 *   sum_t (E_t - mean E)^2 over consecutive transition records, NaN with fewer than two transitions or a zero denominator;
 *   the two means are NaN without a transition.  MMCMC_ERR_INVALID_ARG: NULL out, NULL rec with n_rows > 0, zero chains, a
 *   device pointer that is not 16-byte aligned, a device index out of range; MMCMC_ERR_NO_DEVICE without a device;
 *   MMCMC_ERR_SHAPE: n_rows >= 2^32 or a byte count beyond size_t. */
typedef struct mmcmc_nuts_chain_summary {
    uint32_t n_transitions, n_divergent, n_depth_cap, max_depth_seen;
    uint64_t n_leapfrog;
    double mean_accept, mean_step, ebfmi;
} mmcmc_nuts_chain_summary;
int mmcmc_nuts_set_draw_stats(mmcmc_nuts *h, int on);
int mmcmc_nuts_draw_stats_enabled(mmcmc_nuts *h);
int mmcmc_nuts_draw_stats(mmcmc_nuts *h, mmcmc_nuts_draw *out, int out_is_device, size_t *n_rows);
int mmcmc_nuts_draw_summary(const mmcmc_nuts_draw *rec, int rec_is_device, size_t n_chains, size_t n_rows, int device,
                            mmcmc_nuts_chain_summary *out);

/* knobs shared by the samplers:
 * iterations per kernel launch (0 = the whole run in one launch, the default) -- never changes a result;
 * kernel variant: 2 = noise of two iterations packed and software-pipelined (default up to dim 16 in f64, at dim 16 in
 *   f32), 0 = plain (default at dim 32), 5 = workgroups of four transition waves fed by noise waves through an LDS ring
 *   (f32: three noise waves each, 1024 threads, four waves per SIMD; f64: one, 512 threads, two per SIMD) (csrc/mm_split_kernels.h; up to dim 8, the default there in f32, elsewhere
 *   MMCMC_ERR_UNSUPPORTED) -- all bit-identical;
 *   HMC only: 3 = the lane-group mapping with the gradient on the matrix cores (16 chains per wave, four lanes per
 *   chain, v_mfma_f64_16x16x4 / v_mfma_f32_16x16x4; csrc/mm_hmc_lg.h), for MMCMC_GAUSSIAN_ND of dim 16 or 32 in f64 and
 *   f32, where it is the default (elsewhere MMCMC_ERR_UNSUPPORTED).  Like the NUTS mappings it sums the D-term dot
 *   products as four partial sums (f64: interleaved coordinates, f32: blocks of four), so its samples differ from
 *   variants 0 / 2 by rounding; it is bit-exact against its own host build (oracle/engine_host.cpp:
 *   eh_hmc_grouped_run, eh_hmc_grouped_run_f32);
 *   6 = one chain per lane at RUN-TIME dimension (csrc/mm_generic.h), the default for a dimension without a compiled
 *   instance; HMC only: 8 = one chain per WORKGROUP, the coordinates across up to 1024 threads (csrc/mm_wide.hip) -- few
 *   chains of a huge dimension, the shape of the reference's own timing tests (hmc.rs:882-916: 6 chains, D = 10 000) --
 *   for RosenbrockND / IsotropicGaussian / StandardNormal at 4 <= dim <= 32 768, the default there from dim 128 on with
 *   fewer than 1024 chains.  It reduces the three sums of a transition across the workgroup, so its samples differ from
 *   variant 6's by rounding (same stream, same transition). */
int mmcmc_mh_set_iters_per_launch(mmcmc_mh *h, uint32_t iters);
int mmcmc_hmc_set_iters_per_launch(mmcmc_hmc *h, uint32_t iters);
int mmcmc_mh_set_kernel_variant(mmcmc_mh *h, int variant);
int mmcmc_hmc_set_kernel_variant(mmcmc_hmc *h, int variant);
int mmcmc_hmc_kernel_variant(mmcmc_hmc *h); /* the variant in use (>= 0) or a negative status */

/* ---- user-defined targets (csrc/mm_rtc.hip) ------------------------------------------------------------------
 * The reference's `Target` / `GradientTarget` (distributions.rs:65-108) are open traits.  The GPU analogue of
 * `impl GradientTarget for MyDensity`: the HIP source of
 *     template <class T> struct mmcmc_user_target {
 *         static constexpr int dim = <dim>;
 *         MM_HD static T logp(const mm_tparams<T> &P, const T *x);                // unnorm_logp
 *         MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g);     // unnorm_logp_and_grad, returns logp
 *     };
 * (P.p[0..8) = `params` of the mmcmc_target_desc a sampler is later created with, P.mat = its `matrix` [dim, dim] or
 * NULL; everything in csrc/mm_math.h / mm_targets.h -- mm_fma, mm_logf, mm_exp, ... -- is in scope) is compiled with
 * hipRTC into the engine's own MH / HMC kernel skeleton for f32 and f64 and its one-chain-per-lane NUTS kernel for the
 * three type modes (NUTS kernel variant 7), and registered under a new target kind (>= MMCMC_USER_KIND_BASE), which
 * mmcmc_mh_create, mmcmc_hmc_create, mmcmc_nuts_create (nuts.rs:123-129 takes any GradientTarget), mmcmc_*_group_create
 * and mmcmc_logp_grad_batch then accept like a built-in kind (dim 1..32).  `log` (may be NULL) receives the compiler's diagnostics.
 * MMCMC_ERR_INVALID_ARG: the source does not compile (see log); MMCMC_ERR_UNSUPPORTED: no libhiprtc on this machine. */
#define MMCMC_USER_KIND_BASE 1000
int mmcmc_target_register_source(const char *name, int dim, const char *hip_source, int *kind_out, char *log, size_t log_len);

/* The same from the log-density ALONE: the GPU analogue of the default body of `GradientTarget::unnorm_logp_and_grad`, which
 * differentiates `unnorm_logp` through burn's autodiff (distributions.rs:78-88).  `hip_source` defines
 *     template <class T> struct mmcmc_user_logp {
 *         static constexpr int dim = <dim>;
 *         template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x);   // written ONCE over the scalar type S
 *     };
 * and the library appends the adapter mmcmc_user_target<T>: logp is logp<T>, logp_grad is forward-mode automatic
 * differentiation of the same body with S = mm_dual<T, W> (csrc/mm_autodiff.h: a value and W tangents, in registers).  The
 * functor then goes exactly the way of mmcmc_target_register_source -- the same kernels, the same checks, the same status
 * codes (MMCMC_ERR_NO_DEVICE without a GPU) -- and the kind is accepted wherever a user kind is: MH, HMC, NUTS, the device
 * groups, mmcmc_logp_grad_batch, and as the target of mmcmc_proposal_register_source.
 *   Differentiable: + - * / and unary minus in every S / T combination, mm_fma, mm_logT, mm_expT, mm_sqrtT, mm_absT,
 *   mm_maxT, mm_minT, mm_softplusT (log(1 + e^a)), mm_sigmoidT; S(c) makes a constant; < > <= >= compare values, so a body may branch on them.  Anything else called
 *   on an S (mm_logf, sinf, ...) has no dual overload: the unit does not compile and the compiler's text arrives in `log`.
 *   Constants and parameters written as T (T(100) * t, P.p[0] * x[0]) cost one multiplication per tangent, the same written
 *   as S (S(100) * t) two operations: prefer T where the body allows it.
 *   Cost: ceil(dim / W) passes, W = min(dim, 8), each about (1 + W) x logp -- against about 2 x logp for a hand-written
 *   gradient.  A density whose gradient is needed at speed keeps mmcmc_target_register_source.
 *   Loops over the coordinates must be fully unrolled -- write MM_UNROLL in front of them.  A loop left rolled indexes the
 *   array of dual numbers at run time, and the compiler then keeps that array in private (scratch) memory instead of
 *   registers: the RosenbrockND body at dim 32 without the pragma costs 1168 B (f32) / 2592 B (f64) per lane.
 *   Singular points: the tangent of mm_sqrtT(a) divides by sqrt(a) and that of mm_logT(a) by a, so both are inf / NaN at
 *   a = 0, as the derivatives themselves are.
 *   Kinks: mm_absT at 0 and mm_maxT / mm_minT at a tie take ONE side's derivative (d|x| = +dx at 0; a tie takes the second
 *   argument's tangents); a branch differentiates the side it takes.
 *   The value returned next to the gradient equals logp<T> bit for bit, and host and device agree bit for bit
 *   (-ffp-contract=off; every derivative formula has one fixed operation order). */
int mmcmc_target_register_logp_source(const char *name, int dim, const char *hip_source, int *kind_out, char *log, size_t log_len);

/* A target that carries DATA: the GPU analogue of `struct LogisticRegression { x, y }` implementing `GradientTarget` -- a Rust
 * struct owns whatever it likes, a run-time compiled functor sees P.p[0..8) and P.mat.  For a kind registered here P.mat is
 * an array of `data_len` elements of the caller's own, not a dim x dim matrix.  `flavour` says what `hip_source` defines:
 * MMCMC_SOURCE_LOGP_GRAD mmcmc_user_target<T> (as for mmcmc_target_register_source), MMCMC_SOURCE_LOGP mmcmc_user_logp<T>
 * (as for mmcmc_target_register_logp_source); csrc/mm_data.h (mm_data_row) and csrc/mm_autodiff.h are included in front of it.
 *   The length is the KIND's, fixed here.  In every mmcmc_target_desc of this kind `matrix` must point at `data_len` host
 *   doubles (NULL: MMCMC_ERR_INVALID_ARG from every create and from mmcmc_logp_grad_batch).  mmcmc_mh_create,
 *   mmcmc_hmc_create, mmcmc_nuts_create, the group constructors (one copy per device), mmcmc_logp_grad_batch and a proposal
 *   registered over the kind upload that many values, converted once to the element type the functor runs in (f32 for f32
 *   handles and NUTS modes 0 / 1, f64 otherwise).  The handle owns its device copy: the host array may be freed or
 *   overwritten as soon as create returns.  Two handles of one kind over different arrays sample different densities; the
 *   compiled unit is shared.
 *   `data_len` is a CAPACITY: a model with a run-time number of rows passes it in `params` and reads fewer elements.
 *   Reading P.mat beyond data_len is the caller's fault, as reading `matrix` beyond dim x dim is for every other kind.
 *   The row index of mm_data_row must not depend on x, and the bounds of the loop over the rows come from P.p or constants:
 *   every lane of a wave then reads the same address and the row arrives through the scalar data path.
 *   Leave the loop over the ROWS rolled and unroll the loops over the coordinates (MM_UNROLL), as above.
 *   Status codes: those of mmcmc_target_register_source; in addition data_len == 0, an unknown flavour or a data_len whose
 *   byte count overflows size_t is MMCMC_ERR_INVALID_ARG.  A failed device allocation at create returns the HIP error. */
#define MMCMC_SOURCE_LOGP_GRAD 0 /* source defines mmcmc_user_target<T> (as mmcmc_target_register_source) */
#define MMCMC_SOURCE_LOGP 1      /* source defines mmcmc_user_logp<T> (as mmcmc_target_register_logp_source) */
int mmcmc_target_register_data_source(const char *name, int dim, size_t data_len, int flavour, const char *hip_source, int *kind_out, char *log, size_t log_len);
/* the data length of `kind`: what mmcmc_target_register_data_source fixed, 0 for a built-in kind and for every kind
 * registered without data; MMCMC_ERR_INVALID_ARG (and 0) for a kind nobody registered */
int mmcmc_target_data_len(int kind, size_t *data_len_out);

/* Which compiler builds run-time compiled units (process-wide; default AUTO).  AUTO: `hipcc --genco` in a child process
 * wherever hipcc is found (PATH, then /opt/rocm/bin), hipRTC (libhiprtc.so, bound at run time) otherwise.  A hipRTC was
 * caught miscompiling one kernel of these units that hipcc compiles correctly, hence the order; it was the copy PyTorch
 * bundles (ROCm 7.0.2's compiler, which a Python process that imported torch resolves libhiprtc.so.7 to), not the system's
 * 7.2, which emits hipcc's code (csrc/mm_rtc.hip at g_compiler).
 * HIPCC / HIPRTC pin one of them (registration then returns MMCMC_ERR_UNSUPPORTED where it is missing). */
#define MMCMC_RTC_COMPILER_AUTO 0
#define MMCMC_RTC_COMPILER_HIPCC 1
#define MMCMC_RTC_COMPILER_HIPRTC 2
int mmcmc_rtc_set_compiler(int which);
/* which compiler built the unit behind a kind handed out by a mmcmc_*_register_source call: MMCMC_RTC_COMPILER_HIPCC or
 * MMCMC_RTC_COMPILER_HIPRTC (MMCMC_ERR_INVALID_ARG: no such kind) */
int mmcmc_rtc_unit_compiler(int kind);
/* (version 102) which copy of hipRTC this process would compile with -- the file the dynamic loader resolved, e.g.
 * .../torch/lib/libhiprtc.so once PyTorch is imported --, the HIP version (major * 10^7 + minor * 10^5 + patch) of the
 * runtime the process bound (hipRTC and its compiler library come from the same bundle) and of the compiler the library was
 * built with (what a `hipcc --genco` child normally is).  Any pointer may be NULL.  MMCMC_ERR_UNSUPPORTED (empty path): no
 * usable libhiprtc.  Needs no GPU.  A unit built by the hipRTC of an older runtime than the library's compiler says so in the
 * `log` of its register call. */
int mmcmc_rtc_compiler_info(char *hiprtc_path, size_t path_len, int *process_hip_version, int *built_hip_version);

/* ---- user-defined proposals (csrc/mm_rtc.hip) --------------------------------------------------------------------
 * `Proposal` is an open trait too (distributions.rs:92-101), and the reference keeps BOTH q-terms in the acceptance
 * ratio because a proposal may be asymmetric (metropolis_hastings.rs:303-315; its own integration tests define custom
 * proposals, tests/metrohast_poisson_test.rs:50-85).  The GPU analogue of `impl Proposal for MyProposal`: the HIP source of
 *     template <class T> struct mmcmc_user_proposal {
 *         MM_HD static void sample(T sigma, const T *x, const T *z, T *out);   // x' ~ q(. | x) from z[dim] i.i.d. N(0, 1)
 *         MM_HD static T logp(T sigma, const T *from, const T *to);            // log q(to | from)
 *     };
 * (sigma = `std` of the mmcmc_proposal_desc the sampler is created with; MM_USER_DIM = dim; the engine's headers are in
 * scope) is compiled for ONE target -- `target_kind` a built-in kind at dimension `dim`, or a kind handed out by
 * mmcmc_target_register_source -- into the engine's MH skeletons for f32 and f64, whose transition then is
 * MHMarkovChain::step with both q-terms in the reference's order:
 *     log_accept_ratio = (lp(x') + log q(x | x')) - (lp(x) + log q(x' | x));   accept iff log_accept_ratio > ln u
 * The noise z and u are the engine's stream (mm_rng.h), so a run is reproducible and independent of launch partition
 * and sharding like every other.  *proposal_kind_out (>= MMCMC_USER_PROPOSAL_BASE) goes into mmcmc_proposal_desc.kind;
 * mmcmc_mh_create accepts it together with a description of exactly that target kind and dimension
 * (MMCMC_ERR_UNSUPPORTED / MMCMC_ERR_SHAPE otherwise).  Status codes as for mmcmc_target_register_source. */
int mmcmc_proposal_register_source(const char *name, int target_kind, int dim, const char *hip_source, int *proposal_kind_out,
                                   char *log, size_t log_len);

/* ---- device groups: one call runs every chain on N GPUs (csrc/mm_group.hip) ------------------------------------
 * `run` of the reference executes ALL chains of the sampler (ChainRunner::run core.rs:176-186, HMC::run hmc.rs:137-158).
 * A group shards n_chains contiguously over `devices` (device i: global chains [first_i, first_i + n_i), stream keyed by
 * the global index, so the sample does not depend on the number of devices), runs the shards with no data-path
 * collective, and reduces split-R-hat / ESS (stats.rs:416-546) over all chains: per-device
 * sufficient statistics, RCCL ncclAllGather of the per-half-chain means / sums of squares + ncclAllReduce of the lag
 * sums over xGMI; the cross-chain sums of withinvar are then reduced on shard 0 (f64 partial sums of the means relative
 * to the mean of the first half of global chain 0 -- the shift the single-GPU kernel uses -- grouped per rank, so equal to
 * the single-GPU result to rounding, not bit for bit) and the finish is the single-GPU one.  (RCCL is bound at run time; if it is missing, or a
 * device is listed twice -- several shards on one GPU --, the statistics travel through the host; *used_rccl says which:
 * 1 = RCCL; 0 = the host by design (a device listed twice); -1 = the host as a FALLBACK because no RCCL library could be
 * loaded; -2 = the host because ncclCommInitAll failed -- check it in a scaling run.)
 *   init: host [n_chains, dim] of dtype.  run: the sample stays on the devices (mmcmc_hmc_group_shard gives each shard's
 *   device pointer [n_i, n_collect, dim]); out_host, if not NULL, also receives [n_chains, n_collect, dim];
 *   accept_counts: host [n_chains] or NULL.  A second run continues the chains.
 *   _run BLOCKS: it returns when every shard's results are there, also with out_host == NULL and accept_counts == NULL
 *   (the shards' device pointers may then be read from any stream).
 *   _run_async (MH / HMC; version 101 -- version 100 inferred this from two NULL arguments of _run) enqueues every shard's
 *   launch on that shard's stream and returns (as mmcmc_hmc_run does on a caller's stream), so runs issued back to back keep
 *   all devices busy; mmcmc_*_group_sync waits for them and reports their errors.  _state, _split_rhat_mean_ess and a later
 *   run are ordered behind the queued work by the streams; read a shard's device pointer only after _sync.
 *   A run (either spelling) that fails after SOME shards have advanced leaves them at different iterations: what was queued
 *   is waited for, the failing status returned, and every later run / diagnostics call of the group returns
 *   MMCMC_ERR_GROUP_BROKEN (_state, _shard, _destroy still work).
 *   _stats_phases: host wall-clock milliseconds of the last _split_rhat_mean_ess, ms3 = {every shard's local statistics,
 *   the exchange (collectives + cross-chain sums, or the host copies), the finish}.
 *   _stream_timer(g, 0, NULL) records a start event on every shard's stream, _stream_timer(g, 1, ms) the end events, waits
 *   and writes each shard's elapsed device milliseconds into ms [n_devices].
 *   _exchange: how the diagnostics' statistics will travel -- decided in _create, where the RCCL communicators are made
 *   (ncclCommInitAll; *status as *used_rccl above, *n_rccl_ranks = ranks of the communicator or 0). */
/* The collectives are bound ONCE per process: by the first group that is created (librccl, found by the loader), or before
 * that by this call from the library at `library_path` -- dlopen(RTLD_NOW | RTLD_LOCAL) and dlsym ON THAT HANDLE for
 * ncclCommInitAll, ncclCommDestroy, ncclAllGather, ncclAllReduce, so the named library's functions are taken even where
 * another librccl is already mapped.  MMCMC_ERR_INVALID_ARG: library_path is NULL, the library cannot be loaded, one of the
 * four symbols is missing, or the collectives are already bound (by this call or by an earlier group creation).
 * ranks_may_share_a_device != 0: a device listed twice no longer sends the statistics through the host (*used_rccl 1, not
 * 0).  Bind that way ONLY a library that accepts several ranks on one device; RCCL itself refuses them. */
int mmcmc_group_bind_collectives(const char *library_path, int ranks_may_share_a_device);
typedef struct mmcmc_hmc_group mmcmc_hmc_group;
int mmcmc_hmc_group_create(mmcmc_hmc_group **out, const mmcmc_target_desc *target, const void *init, size_t n_chains,
                           double step_size, int n_leapfrog, int dtype, const int *devices, int n_devices);
int mmcmc_hmc_group_seed(mmcmc_hmc_group *g, uint64_t seed);
int mmcmc_hmc_group_set_chain_offset(mmcmc_hmc_group *g, uint64_t first_global_chain);
int mmcmc_hmc_group_run(mmcmc_hmc_group *g, size_t n_collect, size_t n_discard, void *out_host, uint64_t *accept_counts);
int mmcmc_hmc_group_run_async(mmcmc_hmc_group *g, size_t n_collect, size_t n_discard);
int mmcmc_hmc_group_stats_phases(mmcmc_hmc_group *g, double *ms3);
int mmcmc_hmc_group_state(mmcmc_hmc_group *g, void *out); /* host [n_chains, dim] */
int mmcmc_hmc_group_split_rhat_mean_ess(mmcmc_hmc_group *g, float *rhat, float *ess, int *used_rccl); /* of the last run */
int mmcmc_hmc_group_shard(mmcmc_hmc_group *g, int i, int *device, size_t *first_chain, size_t *n_chains, void **sample_dev);
int mmcmc_hmc_group_sync(mmcmc_hmc_group *g);
int mmcmc_hmc_group_stream_timer(mmcmc_hmc_group *g, int stop, float *ms_per_device);
int mmcmc_hmc_group_exchange(mmcmc_hmc_group *g, int *status, int *n_rccl_ranks);
int mmcmc_hmc_group_destroy(mmcmc_hmc_group *g);
typedef struct mmcmc_mh_group mmcmc_mh_group;
int mmcmc_mh_group_create(mmcmc_mh_group **out, const mmcmc_target_desc *target, const mmcmc_proposal_desc *proposal,
                          const void *init, size_t n_chains, int dtype, const int *devices, int n_devices);
int mmcmc_mh_group_seed(mmcmc_mh_group *g, uint64_t seed);
int mmcmc_mh_group_set_chain_offset(mmcmc_mh_group *g, uint64_t first_global_chain);
int mmcmc_mh_group_run(mmcmc_mh_group *g, size_t n_collect, size_t n_discard, void *out_host, uint64_t *accept_counts);
int mmcmc_mh_group_run_async(mmcmc_mh_group *g, size_t n_collect, size_t n_discard);
int mmcmc_mh_group_stats_phases(mmcmc_mh_group *g, double *ms3);
int mmcmc_mh_group_state(mmcmc_mh_group *g, void *out);
int mmcmc_mh_group_split_rhat_mean_ess(mmcmc_mh_group *g, float *rhat, float *ess, int *used_rccl);
int mmcmc_mh_group_sync(mmcmc_mh_group *g);
int mmcmc_mh_group_stream_timer(mmcmc_mh_group *g, int stop, float *ms_per_device);
int mmcmc_mh_group_exchange(mmcmc_mh_group *g, int *status, int *n_rccl_ranks);
int mmcmc_mh_group_destroy(mmcmc_mh_group *g);
/* NUTS::run / run_progress (nuts.rs:163-170, 194-338) of every chain on N devices: `init` host [n_chains, dim] doubles
 * and `mode` as in mmcmc_nuts_create; out_host [n_chains, n_collect, dim] of the mode's tensor type (f32 for modes 0 and
 * 1, f64 for mode 2) or NULL; progress as in mmcmc_nuts_run.  Chain i's results do not depend on the number of devices. */
typedef struct mmcmc_nuts_group mmcmc_nuts_group;
int mmcmc_nuts_group_create(mmcmc_nuts_group **out, const mmcmc_target_desc *target, const double *init, size_t n_chains,
                            double target_accept_p, int mode, const int *devices, int n_devices);
int mmcmc_nuts_group_seed(mmcmc_nuts_group *g, uint64_t seed);
int mmcmc_nuts_group_set_chain_offset(mmcmc_nuts_group *g, uint64_t first_global_chain);
int mmcmc_nuts_group_set_max_depth(mmcmc_nuts_group *g, int max_depth);
int mmcmc_nuts_group_run(mmcmc_nuts_group *g, size_t n_collect, size_t n_discard, void *out_host, int progress);
int mmcmc_nuts_group_stats_phases(mmcmc_nuts_group *g, double *ms3);
int mmcmc_nuts_group_set_draw_stats(mmcmc_nuts_group *g, int on); /* MMCMC_ERR_UNSUPPORTED: a device group records no per-draw statistics */
int mmcmc_nuts_group_state(mmcmc_nuts_group *g, void *out); /* host [n_chains, dim] of the tensor type */
int mmcmc_nuts_group_leapfrog_counts(mmcmc_nuts_group *g, uint64_t *out); /* host [n_chains] */
int mmcmc_nuts_group_split_rhat_mean_ess(mmcmc_nuts_group *g, float *rhat, float *ess, int *used_rccl);
int mmcmc_nuts_group_sync(mmcmc_nuts_group *g);
int mmcmc_nuts_group_stream_timer(mmcmc_nuts_group *g, int stop, float *ms_per_device);
int mmcmc_nuts_group_exchange(mmcmc_nuts_group *g, int *status, int *n_rccl_ranks);
int mmcmc_nuts_group_destroy(mmcmc_nuts_group *g);

/* ---- diagnostics: stats.rs ------------------------------------------------------------------------------
 * split_rhat_mean_ess(sample[chains, n, params]) -> (rhat[params], ess[params])   stats.rs:416-423
 * (splitcat :396-402, withinvar :429-477, rhat :425-427 = sqrt(W/var+) as the reference defines it, ess :496-546).
 * sample: [n_chains, n, dim] of dtype, device or host memory; rhat, ess: host [dim] (f32 like the reference).
 * Shapes: dim < 2^16, n < 2^31, and where the half-chain takes the residue transform (1024 < n/2 <= 131072)
 * dim x 2048 x max(2, ceil(n/2 / 1024)) < 2^32 -- from dim = 16384 up that cuts the longest half-chains -- whichever kernel
 * is selected; MMCMC_ERR_SHAPE beyond, decided from the shape before anything is allocated (also for _stats_partials). */
int mmcmc_split_rhat_mean_ess(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n,
                              size_t dim, float *rhat, float *ess, int device, void *stream);
/* The two halves of the above, for multi-GPU runs (chains sharded over ranks):
 * partials: device-side sufficient statistics of the LOCAL chains -- means, ssq: device [2*n_chains, dim] in splitcat
 * order (first halves of all local chains, then second halves), acov_sum: device [n/2, dim] un-normalised lag sums
 * over the local half-chains.  All-gather the first two, all-reduce(sum) the third, then
 * finish (host): the arithmetic of stats.rs:449-465, :425-427, :509-545 on the global statistics (f32; the cross-chain
 * sums in f64 as on the device, so the result does not drift from the single-GPU one as the chain count grows). */
int mmcmc_stats_partials(const void *sample, int dtype, size_t n_chains, size_t n, size_t dim, float *means,
                         float *ssq, float *acov_sum, int device, void *stream);
int mmcmc_stats_finish(const float *means, const float *ssq, const float *acov_sum, size_t n_half_chains, size_t m,
                       size_t dim, float *rhat, float *ess);
/* finish from the cross-chain SUMS instead of the per-half-chain statistics, for runs where gathering 2 * chains * dim
 * numbers on every rank is the expensive part: dsum[d] = sum over ALL half-chains of (mean - overall mean)^2,
 * wsum[d] = sum of the biased half-chain variances ssq / m (two all-reduces: the overall mean first), acov_sum as
 * above.  Same arithmetic from there on (stats.rs:459-465, :425-427, :509-545). */
int mmcmc_stats_finish_sums(const double *dsum, const double *wsum, const float *acov_sum, size_t n_half_chains, size_t m,
                            size_t dim, float *rhat, float *ess);
/* Which kernel computes the lag sums (process-wide; every one of them implements the same biased, mean-removed
 * estimator of stats.rs:548-654 and they agree to f32 rounding -- tests/test_gpu_parity.py::test_stats_kernels_agree):
 *   AUTO    what the reference does (stats.rs:549): direct sums for half-chains up to 100 draws (register tiles on the
 *           vector ALU), the power spectrum above (one wave-level FFT per chain and parameter, one inverse for all);
 *   FFT / TILE1 / TILE / MFMA / DIRECT   that kernel wherever its shape limits allow, AUTO's choice elsewhere
 *           (FFT: 2 <= n/2 <= 131072 -- one wave-level transform up to 1024, N1 = ceil(n/2 / 1024) = 2 .. 128 residues of
 *           2048-point transforms beyond (any count, not a power of two), one residue and parameter per wave with its spectrum in registers (version 101; 100 ended
 *           at 16384); TILE1: n/2 <= 512; TILE: up to 8 tiles per lane; MFMA: LDS layout up to 64 KB).  Half-chains longer
 *           than 131072 draws -- and, under DIRECT, any the staging kernels cannot hold in a workgroup's LDS -- are reduced
 *           straight from global memory (O(chains x dim x n^2), meant for a few very long chains): any n < 2^31 with
 *           dim x n/2 < 2^32 and 2 x chains x dim < 2^31 (MMCMC_ERR_SHAPE beyond), and chains x dim x (n/2)^2 within the
 *           direct-work limit (default 2^46, about ten seconds of device time; MMCMC_ERR_UNSUPPORTED beyond;
 *           mmcmc_stats_set_direct_work_limit(0) removes the limit).
 * For measurements and for the agreement test; results never depend on it beyond rounding.  Process-wide and meant to
 * be set once: a call that races with it picks one kernel or the other (its work buffer fits both).  Under one selection
 * R-hat / ESS are bit-reproducible across devices too: no kernel's summation grouping depends on the device. */
#define MMCMC_STATS_KERNEL_AUTO 0
#define MMCMC_STATS_KERNEL_FFT 1
#define MMCMC_STATS_KERNEL_TILE1 2
#define MMCMC_STATS_KERNEL_TILE 3
#define MMCMC_STATS_KERNEL_MFMA 4
#define MMCMC_STATS_KERNEL_DIRECT 5
int mmcmc_stats_set_kernel(int kind);
/* lag products the O(n^2) from-global-memory path may be asked for before it returns MMCMC_ERR_UNSUPPORTED (process-wide;
 * default 2^46; 0 = no limit: the call then runs however long it takes) */
int mmcmc_stats_set_direct_work_limit(uint64_t max_lag_products);
/* basic_stats stats.rs:310-336 (host) and RunStats::from stats.rs:360-371 */
int mmcmc_basic_stats_from(const float *data, size_t len, mmcmc_basic_stats *out);
int mmcmc_run_stats_from(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                    mmcmc_run_stats *out, int device, void *stream);

/* ---- rank-normalised diagnostics (csrc/mm_rank.hip; not in the reference) -----------------------------------------
 * Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021): the mean-based split R-hat above cannot see chains that agree in
 * location and differ in scale or tails, and a mean ESS says nothing about the 5 % / 95 % quantiles.  For sample
 * [n_chains, n, dim] (device or host, dtype; cast to f32 first like RunStats::from, stats.rs:365; f64 input is ranked by its
 * f32 casts), S = n_chains x n, every parameter on its own:
 *   ranks       all S draws pooled; -0.0 == +0.0; equal values share the average of their 1-based positions;
 *               rank2 = first + last position of the tie group = 2 x the average rank, exact in uint32
 *   scores      z = Phi^-1((rank2 / 2 - 3/8) / (S + 1/4)) evaluated in f64 on the device, rounded once to f32
 *   folded      the same for |x - med| (f32), med = the pooled median (quantile rule below, rounded to f32)
 *   quantiles   numpy's default (type 7): h = (S - 1) p, j = floor(h), q = a + (h - j) (b - a) in f64 from the sorted f32
 *               draws a, b at j, j + 1
 *   rhat_bulk / rhat_folded   the CONVENTIONAL split R-hat sqrt(var+ / W) of z / of the folded z (the inverse of what
 *               mmcmc_split_rhat_mean_ess reports, quirk Q7); rhat_rank = their maximum
 *   ess_bulk    the library's split ESS of z;  ess_tail = min over q in {q05, q95} of the split ESS of the 0 / 1 indicator
 *               I(x <= q).  "The library's split ESS" is exactly mmcmc_split_rhat_mean_ess (splitcat, the reference's
 *               Geyer pairing, the AUTO kernel choice): the definitions are Vehtari et al.'s, the ESS estimator is the
 *               reference's, so the figures are not promised to equal Stan's or ArviZ's digit for digit.
 *   A parameter with any NaN draw gets NaN in every output and rank2 = 0; +-inf sort like numbers.  A constant parameter
 *   goes through the pipeline as it is (NaN wherever 0 / 0 arises).
 * The hot path is a stable LSD radix sort of (key, index) pairs, four 8-bit passes, hand-written for gfx950; results are a
 * pure function of the input, bit-reproducible across runs, streams and devices.  The calls block: they return when the
 * outputs are there.  Work memory: 16 x S bytes + histograms for the sort (one parameter at a time); _rank_diagnostics
 * additionally two f32 arrays of the sample's shape.
 * SINGLE DEVICE: ranks are global over chains, so a sample sharded over a device group has to be gathered first; the
 * mmcmc_*_group handles have no rank diagnostics.
 * Status: MMCMC_ERR_INVALID_ARG  NULL sample / z, a probability outside [0, 1], n_probs > 0 with NULL probs (or NULL output);
 *         MMCMC_ERR_SHAPE        n_chains x n >= 2^31, dim >= 2^16, for _rank_diagnostics also n < 2 and every shape limit of
 *                                mmcmc_split_rhat_mean_ess -- decided from the shape before anything is allocated;
 *         MMCMC_ERR_NO_DEVICE    no device, like every compute entry point.
 * These entry points are additive: MMCMC_VERSION stays 102. */
/* z: f32 [n_chains, n, dim], device memory if z_is_device else host; rank2 (may be NULL): uint32, same shape, same place as z;
 * folded != 0: the scores (and ranks) of |x - med| */
int mmcmc_rank_normalize(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                         int folded, float *z, int z_is_device, uint32_t *rank2, int device, void *stream);
/* out: host [n_probs, dim] */
int mmcmc_quantiles(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                    const double *probs, size_t n_probs, double *out, int device, void *stream);
/* every output host [dim] and nullable; rhat_parts [2, dim] = bulk, folded; ess_tail_parts [2, dim] = lower (q05), upper (q95);
 * quantiles [n_probs, dim] when n_probs > 0 */
int mmcmc_rank_diagnostics(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                           float *rhat_rank, float *rhat_parts, float *ess_bulk, float *ess_tail, float *ess_tail_parts,
                           const double *probs, size_t n_probs, double *quantiles, int device, void *stream);

/* ---- running diagnostics: MultiChainTracker (stats.rs:189-306) -------------------------------------------------
 * What run_progress shows while sampling (hmc.rs:242-281: `p(accept)` and `max(rhat)` after every step).  The tracker
 * keeps per-chain running mean / mean of squares (the reference's f32 recurrences, exactly), the exponentially
 * averaged acceptance indicator and the running R-hat sqrt(var+ / W) (the conventional one, unlike split_rhat's,
 * quirk Q7) on the device; it is fed blocks of consecutive states and polled by the host between launches.
 *   mmcmc_tracker_steps: MultiChainTracker::step (stats.rs:236-262) for rows t0 .. t0+k-1 of every chain of
 *       states [n_chains, n_rows, dim] of dtype (device or host pointer) -- e.g. a slice of a sampler's output, or the
 *       current positions with n_rows = 1.
 *   mmcmc_tracker_stats: rhat [dim] (MultiChainTracker::rhat :280-286), its maximum (max_rhat :270-274) and p_accept;
 *       needs at least two steps.  Any of the outputs may be NULL. */
typedef struct mmcmc_tracker mmcmc_tracker;
int mmcmc_tracker_create(mmcmc_tracker **out, size_t n_chains, size_t dim, int device);
int mmcmc_tracker_steps(mmcmc_tracker *h, const void *states, int states_is_device, int dtype, size_t n_rows, size_t t0,
                        size_t k, void *stream);
int mmcmc_tracker_stats(mmcmc_tracker *h, float *rhat, float *max_rhat, float *p_accept, void *stream);
/* The per-chain flavour the generic run_progress uses (core.rs:90-140, 255-300): ChainTracker::new(initial_state) =
 * mmcmc_tracker_init_last (before any step; states [n_chains, dim]), then mmcmc_tracker_steps as above;
 * mmcmc_tracker_chain_stats = collect_rhat (stats.rs:150-178, with its chains*params - 1 divisor, quirk Q9), its
 * NaN-skipping maximum, and the average of the per-chain acceptance EMAs (stats.rs:109-123, started from the first
 * comparison of coordinate 0: quirk Q12). */
int mmcmc_tracker_init_last(mmcmc_tracker *h, const void *states, int states_is_device, int dtype, void *stream);
int mmcmc_tracker_chain_stats(mmcmc_tracker *h, float *rhat, float *max_rhat, float *avg_p_accept, void *stream);
int mmcmc_tracker_n(mmcmc_tracker *h, uint64_t *n);
int mmcmc_tracker_shape(mmcmc_tracker *h, size_t *n_chains, size_t *dim, int *device);
/* withinvar_from_cs (stats.rs:155-178) over the per-chain ChainStats (mean, sm2 = (mean_sq - mean^2) n / (n - 1), n):
 * within [dim], var [dim] (host) -- the pair collect_rhat and ess_from_chainstats share.  Needs at least two steps. */
int mmcmc_tracker_within_var(mmcmc_tracker *h, float *within, float *var, void *stream);
/* stats::ess_from_chainstats(sample, chain_stats) (stats.rs:668-671): the UN-split ESS of sample [n_chains, n, dim]
 * (device or host memory, dtype) with within / var from the per-chain trackers that were fed the run
 * (mmcmc_tracker_init_last + mmcmc_tracker_steps, or the tracker mmcmc_*_run_progress hands back); ess: host [dim].
 * The autocovariance follows the reference's switch on n (stats.rs:549), Geyer's truncation as stats.rs:523-545. */
int mmcmc_ess_from_chainstats(const void *sample, int sample_is_device, int dtype, size_t n_chains, size_t n, size_t dim,
                              mmcmc_tracker *tracker, float *ess, int device, void *stream);

/* ---- run_progress ------------------------------------------------------------------------------------------------
 * ChainRunner::run_progress (core.rs:208-360, the MH flavour), HMC::run_progress (hmc.rs:222-294), NUTS::run_progress
 * (nuts.rs:172-345 over NUTSChain::run_progress :473-526): burn-in + sampling with the reference's running diagnostics,
 * returning the sample and RunStats.  The tracker feeding orders live here once (csrc/mm_progress.hip):
 *   HMC  burn-in unobserved; one MultiChainTracker fed the positions sampling starts from, then every collected state;
 *   MH   per-chain ChainTrackers built on the state before the first step, fed EVERY state, burn-in included;
 *   NUTS as MH (all n_discard + n_collect states; the run is one launch, the trackers are fed after it).
 * cb (may be NULL) is called after every `every` transitions (0: ten times per run) with what the reference's bar shows:
 * p(accept) and max(rhat) -- the MultiChainTracker's for HMC (stats.rs:270-286), the average per-chain EMA and
 * collect_rhat's NaN-skipping maximum for MH and NUTS (core.rs:268-293).
 * out: [n_chains, n_collect, dim] of the sampler's dtype (NUTS: f32 for modes 0 / 1, f64 for mode 2), device or host, may
 * be NULL; stats (may be NULL; needs n_collect >= 2): RunStats::from(sample); tracker_out (may be NULL): receives the
 * tracker that was fed (the caller destroys it with mmcmc_tracker_destroy), e.g. for mmcmc_ess_from_chainstats.
 * stream NULL: a stream of the call's own; the call returns when everything has finished.  Device memory beside the sample:
 * MH a block of `every` burn-in states, NUTS all n_discard + n_collect states of every chain (its adaptation makes the
 * run one launch): n_chains x (n_discard + n_collect) x dim elements -- hipErrorOutOfMemory if that does not fit. */
typedef void (*mmcmc_progress_fn)(void *user, uint64_t transitions_done, uint64_t transitions_total, float p_accept,
                                  float max_rhat);
int mmcmc_mh_run_progress(mmcmc_mh *h, size_t n_collect, size_t n_discard, size_t every, mmcmc_progress_fn cb, void *user,
                          void *out, int out_is_device, mmcmc_run_stats *stats, mmcmc_tracker **tracker_out, void *stream);
int mmcmc_hmc_run_progress(mmcmc_hmc *h, size_t n_collect, size_t n_discard, size_t every, mmcmc_progress_fn cb, void *user,
                           void *out, int out_is_device, mmcmc_run_stats *stats, mmcmc_tracker **tracker_out, void *stream);
int mmcmc_nuts_run_progress(mmcmc_nuts *h, size_t n_collect, size_t n_discard, size_t every, mmcmc_progress_fn cb, void *user,
                            void *out, int out_is_device, mmcmc_run_stats *stats, mmcmc_tracker **tracker_out, void *stream);
int mmcmc_tracker_destroy(mmcmc_tracker *h);

/* ---- Metropolis-Hastings on integer states ---------------------------------------------------------------------
 * MHMarkovChain / MetropolisHastings are generic over the state type (metropolis_hastings.rs:28-48, 149-160); the
 * reference's own discrete users are the targets + proposals below.  One chain per lane, state i32, log-densities
 * f64 (a table per target, built with the reference's operation order), step = metropolis_hastings.rs:303-315.
 *   MMCMC_POISSON_REFLECT  params {lambda}: PoissonDist + PoissonRandomWalk      tests/metrohast_poisson_test.rs:18-85
 *   MMCMC_BINOMIAL_CLAMP   params {n, p}:   BinomialDist + BinomialRandomWalk    tests/metrohast_poisson_test.rs:150-212
 *                          (n < 1024: the log-density table lives in LDS; larger n: MMCMC_ERR_UNSUPPORTED)
 *   MMCMC_POISSON_NONNEG   params {lambda}: PoissonTarget + NonnegativeProposal  examples/poisson_mh.rs:8-76
 * (lambda <= 256: states above 1023 have probability zero here.)  init: host [n_chains] i32;
 * out: [n_chains, n_collect] i32 (the reference's Array3<i32>[C, n, 1]).  Integer states and accept counts are
 * bit-exact against the host build of the same header (oracle/engine_host.cpp) and against the oracle's independent
 * restatement on the same stream. */
#define MMCMC_POISSON_REFLECT 16
#define MMCMC_BINOMIAL_CLAMP 17
#define MMCMC_POISSON_NONNEG 18
/* An integer-state model of the caller's own (csrc/mm_rtc.hip, csrc/mm_discrete_kernels.h): `impl Target<i32, f64>` +
 * `impl Proposal<i32, f64>` as the reference's own tests write them (tests/metrohast_poisson_test.rs:18-85), as HIP source
 *     struct mmcmc_user_discrete {
 *         MM_HD static double logp(const double *params, int k);                  // Target::unnorm_logp
 *         MM_HD static int sample(const double *params, int current, int step);   // Proposal::sample; step = +1 / -1, p = 1/2 each
 *         MM_HD static double logq(const double *params, int from, int to);       // Proposal::logp = log q(to | from)
 *     };
 * (mm_log, mm_ln_factorial, MM_NEG_INF, ... of the engine's headers in scope).  *kind_out (>= MMCMC_USER_KIND_BASE) is a `kind` for
 * mmcmc_mh_discrete_create, whose `params` (eight doubles) reach the functor unchanged; the transition is
 * MHMarkovChain::step with both q-terms on the built-in models' stream, so a restatement of a built-in model reproduces
 * it bit for bit (tests/test_user_proposal.py). */
int mmcmc_discrete_register_source(const char *name, const char *hip_source, int *kind_out, char *log, size_t log_len);
typedef struct mmcmc_mh_discrete mmcmc_mh_discrete;
int mmcmc_mh_discrete_create(mmcmc_mh_discrete **out, int kind, const double *params, const int32_t *init,
                             size_t n_chains, int device);
/* kernel mapping: 1 = noise waves + transition waves, four waves per SIMD (default; used from 4096 chains on), 0 = one wave per
 * SIMD; bit-identical */
int mmcmc_mh_discrete_set_kernel_variant(mmcmc_mh_discrete *h, int variant);
int mmcmc_mh_discrete_seed(mmcmc_mh_discrete *h, uint64_t seed);                 /* MetropolisHastings::seed :187-193 */
int mmcmc_mh_discrete_set_chain_offset(mmcmc_mh_discrete *h, uint64_t chain_offset);
/* ChainRunner::run core.rs:176-186: n_discard + n_collect transitions, the last n_collect states kept */
int mmcmc_mh_discrete_run(mmcmc_mh_discrete *h, size_t n_collect, size_t n_discard, int32_t *out, int out_is_device,
                          void *stream);
int mmcmc_mh_discrete_state(mmcmc_mh_discrete *h, int32_t *out);                 /* host [n_chains] */
int mmcmc_mh_discrete_accept_counts(mmcmc_mh_discrete *h, uint64_t *out);        /* host [n_chains], since creation */
int mmcmc_mh_discrete_sync(mmcmc_mh_discrete *h);
int mmcmc_mh_discrete_destroy(mmcmc_mh_discrete *h);

/* ---- Gibbs sampling with a built-in full conditional --------------------------------------------------------
 * GibbsSampler / GibbsMarkovChain (gibbs.rs:31-203) take a user-written `Conditional`; the one the reference ships --
 * the two-component Gaussian mixture over the state [x, z] of gibbs.rs:231-285 and examples/mixture_gibbs.rs:24-76 --
 * is built in.  params = {mu0, sigma0, mu1, sigma1, pi0}; init: host [n_chains, 2] f64 (the reference starts from
 * init_det(n, 2)); out: [n_chains, n_collect, 2] f64.  One sweep = x | z then z | x (gibbs.rs:96-101). */
typedef struct mmcmc_gibbs_mixture mmcmc_gibbs_mixture;
int mmcmc_gibbs_mixture_create(mmcmc_gibbs_mixture **out, const double *params, const double *init, size_t n_chains,
                               int device);
int mmcmc_gibbs_mixture_set_kernel_variant(mmcmc_gibbs_mixture *h, int variant); /* as mmcmc_mh_discrete_set_kernel_variant */
int mmcmc_gibbs_mixture_seed(mmcmc_gibbs_mixture *h, uint64_t seed);            /* GibbsSampler::set_seed gibbs.rs:179-187 */
int mmcmc_gibbs_mixture_set_chain_offset(mmcmc_gibbs_mixture *h, uint64_t chain_offset);
int mmcmc_gibbs_mixture_run(mmcmc_gibbs_mixture *h, size_t n_collect, size_t n_discard, double *out, int out_is_device,
                            void *stream);                                      /* ChainRunner::run core.rs:176-186 */
int mmcmc_gibbs_mixture_state(mmcmc_gibbs_mixture *h, double *out);             /* host [n_chains, 2] */
int mmcmc_gibbs_mixture_sync(mmcmc_gibbs_mixture *h);
int mmcmc_gibbs_mixture_destroy(mmcmc_gibbs_mixture *h);

/* ---- chain state and stream position: checkpoint and resume ------------------------------------------------------
 * The engine's noise is a function of (seed, global chain id, iteration) alone, so a handle's future is fixed by its
 * positions, seed, chain offset, iteration counter and sampler fields, plus NUTS's per-chain adaptation records.  Each
 * can be read and set below; a handle given all of another's continues exactly as that one would, bit for bit (samples,
 * states, accept counts, adaptation), in another process or on another number of devices.  Additive to 102.
 * Every setter makes its constructor's checks, leaves the handle unchanged when they fail, applies from the next
 * transition on and touches nothing else (not the seed, chain offset or iteration unless that is what it sets).
 *   mh_set_proposal_std: Sampler::scale of MH (metropolis_hastings.rs:101-109 `pub proposal`), finite and > 0 as in
 *     mmcmc_mh_create; mmcmc_mh_params reads it.  mh_set_state / nuts_set_state: [n_chains, dim] of the handle's dtype (NUTS:
 *     the mode's tensor type), host or device memory, ordered as mmcmc_hmc_set_state.
 *   nuts_set_adapt_state: the exact inverse of mmcmc_nuts_adapt_state, host [n_chains, 4] doubles = epsilon, epsilon_bar,
 *     h_bar, mu.  Every value finite (also in the mode's scalar type), epsilon > 0 or exactly the sentinel -1 (not yet
 *     searched, nuts.rs:415-433).  Round trips are bit-exact in every mode (f32 through f64 is exact).  Ordered behind
 *     every queued run of the device.  mmcmc_nuts_params reads target_accept_p and max_depth;
 *     nuts_set_target_accept_p makes mmcmc_nuts_create's check (0 < p < 1).
 *   mh_discrete_set_state: host [n_chains] i32; gibbs_mixture_set_state: host [n_chains, 2] f64 (behind every queued run).
 *   *_stream_position: seed, chain offset and iteration (the next transition's index; NUTS: self.m, which the adaptation
 *     also reads against n_discard); any pointer may be NULL.  *_set_iteration refuses values >= 2^32, the limit every run
 *     already keeps.
 * Not state: the accept counts (per run) and NUTS's leapfrog counts and depth histogram (cumulative diagnostics); the
 * lane-group records of NUTS variants 1..3 (every transition writes its record before reading it) and the compaction
 * level and pilot of variant 3 (they never change a result); the kernel variant and iters_per_launch (results identical).
 * Groups fan out to their shards: set_state takes the global host [n_chains, dim] and copies each shard's rows on that
 * shard's stream, behind its queued asynchronous runs; _stream_position gives the group's first global chain
 * (mmcmc_*_group_set_chain_offset) and the shards' common iteration; the NUTS group's adaptation is global [n_chains, 4].
 * The group field setters check their argument once, so no shard changes unless every shard does.  On a broken group
 * (MMCMC_ERR_GROUP_BROKEN above) every setter and _stream_position return MMCMC_ERR_GROUP_BROKEN. */
int mmcmc_mh_set_proposal_std(mmcmc_mh *h, double std);
int mmcmc_mh_params(mmcmc_mh *h, double *std);
int mmcmc_mh_set_state(mmcmc_mh *h, const void *x, int is_device, void *stream);
int mmcmc_nuts_set_state(mmcmc_nuts *h, const void *x, int is_device, void *stream);
int mmcmc_nuts_set_adapt_state(mmcmc_nuts *h, const double *in);
int mmcmc_nuts_params(mmcmc_nuts *h, double *target_accept_p, int *max_depth);
int mmcmc_nuts_set_target_accept_p(mmcmc_nuts *h, double target_accept_p);
int mmcmc_mh_discrete_set_state(mmcmc_mh_discrete *h, const int32_t *x);
int mmcmc_gibbs_mixture_set_state(mmcmc_gibbs_mixture *h, const double *x);
int mmcmc_mh_stream_position(mmcmc_mh *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
int mmcmc_hmc_stream_position(mmcmc_hmc *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
int mmcmc_nuts_stream_position(mmcmc_nuts *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
int mmcmc_mh_discrete_stream_position(mmcmc_mh_discrete *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
int mmcmc_gibbs_mixture_stream_position(mmcmc_gibbs_mixture *h, uint64_t *seed, uint64_t *chain_offset, uint64_t *iteration);
int mmcmc_mh_set_iteration(mmcmc_mh *h, uint64_t iteration);
int mmcmc_hmc_set_iteration(mmcmc_hmc *h, uint64_t iteration);
int mmcmc_nuts_set_iteration(mmcmc_nuts *h, uint64_t iteration);
int mmcmc_mh_discrete_set_iteration(mmcmc_mh_discrete *h, uint64_t iteration);
int mmcmc_gibbs_mixture_set_iteration(mmcmc_gibbs_mixture *h, uint64_t iteration);
int mmcmc_hmc_group_set_state(mmcmc_hmc_group *g, const void *in);
int mmcmc_mh_group_set_state(mmcmc_mh_group *g, const void *in);
int mmcmc_nuts_group_set_state(mmcmc_nuts_group *g, const void *in);
int mmcmc_hmc_group_set_step_size(mmcmc_hmc_group *g, double step_size);
int mmcmc_hmc_group_set_n_leapfrog(mmcmc_hmc_group *g, int n_leapfrog);
int mmcmc_hmc_group_params(mmcmc_hmc_group *g, double *step_size, int *n_leapfrog);
int mmcmc_mh_group_set_proposal_std(mmcmc_mh_group *g, double std);
int mmcmc_mh_group_params(mmcmc_mh_group *g, double *std);
int mmcmc_nuts_group_adapt_state(mmcmc_nuts_group *g, double *out);
int mmcmc_nuts_group_set_adapt_state(mmcmc_nuts_group *g, const double *in);
int mmcmc_nuts_group_params(mmcmc_nuts_group *g, double *target_accept_p, int *max_depth);
int mmcmc_nuts_group_set_target_accept_p(mmcmc_nuts_group *g, double target_accept_p);
int mmcmc_hmc_group_stream_position(mmcmc_hmc_group *g, uint64_t *seed, uint64_t *first_global_chain, uint64_t *iteration);
int mmcmc_mh_group_stream_position(mmcmc_mh_group *g, uint64_t *seed, uint64_t *first_global_chain, uint64_t *iteration);
int mmcmc_nuts_group_stream_position(mmcmc_nuts_group *g, uint64_t *seed, uint64_t *first_global_chain, uint64_t *iteration);
int mmcmc_hmc_group_set_iteration(mmcmc_hmc_group *g, uint64_t iteration);
int mmcmc_mh_group_set_iteration(mmcmc_mh_group *g, uint64_t iteration);
int mmcmc_nuts_group_set_iteration(mmcmc_nuts_group *g, uint64_t iteration);

/* ---- sample sink: io/csv.rs:47-69 save_csv -- header `chain,observation,dim_0,...`, one record per (chain,
 *      observation), values in Rust `Display` formatting (shortest round-trip, no exponent).  sample: HOST
 *      [n_chains, n, dim] of dtype. */
int mmcmc_save_csv(const void *sample, int dtype, size_t n_chains, size_t n, size_t dim, const char *filename);

/* ---- densities, for parity tests ---------------------------------------------------------------------
 * BatchedGradientTarget::unnorm_logp_batch (distributions.rs:65-76) / unnorm_logp_and_grad (:81-87)
 * x: host [n, dim]; logp: host [n]; grad: host [n, dim] or NULL; all of `dtype` */
int mmcmc_logp_grad_batch(const mmcmc_target_desc *target, int dtype, const void *x, size_t n, void *logp,
                          void *grad, int device);

/* ---- the engine's random stream, for parity tests: noise of (seed, chain, iteration) exactly as the kernels
 *      draw it.  z: host [n_chains, dim] of dtype, u: host [n_chains] of dtype; computed on the device. */
int mmcmc_draw_noise(uint64_t seed, uint64_t chain_offset, uint32_t iteration, size_t n_chains, int dim, int dtype,
                     void *z, void *u, int device);
/* The noise of the METROPOLIS-HASTINGS sampler: in f32 at dim <= 2 it draws from a stream of its own -- one Philox block per
 * TWO transitions, the accept uniform's low byte from a second block (csrc/mm_rng.h, "paired stream": half the generator
 * work of the step) --; everywhere else this is mmcmc_draw_noise. */
int mmcmc_draw_noise_mh(uint64_t seed, uint64_t chain_offset, uint32_t iteration, size_t n_chains, int dim, int dtype, void *z,
                        void *u, int device);

#ifdef __cplusplus
}
#endif
#endif /* MMCMC_H */

"""`HMC` -- host-side mirror of src/hmc.rs:87-158, 304-377 over the GPU engine."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import checkpoint as K
from .core import _Sampler
from .distributions import IsotropicGaussian, Target


class HMC(_Sampler):
    """HMC::new(target, initial_positions, step_size, n_leapfrog) (hmc.rs:87-109)."""

    _prefix = "hmc"
    _cprefix = _ckpt_sampler = "hmc"

    def __init__(self, target: Target, initial_positions, step_size: float, n_leapfrog: int, device: int = 0):
        super().__init__()
        init = np.ascontiguousarray(initial_positions)
        if init.dtype not in (np.float32, np.float64):
            init = init.astype(np.float32)
        if init.ndim != 2:
            raise ValueError("initial_positions must be [n_chains, dim]")
        self.n_chains, self.dim = init.shape
        self.dtype = init.dtype.type
        self.device = device
        if target.dim != self.dim:
            if type(target).__name__ in ("RosenbrockND", "StandardNormal"):
                target = type(target)(self.dim)
            elif isinstance(target, IsotropicGaussian):
                target = IsotropicGaussian(target.std, self.dim)
            else:
                raise ValueError(f"target dim {target.dim} != state dim {self.dim}")
        self.target = target
        d = target.desc()
        st = L.lib().mmcmc_hmc_create(C.byref(self._h), C.byref(d), init.ctypes.data, self.n_chains,
                                      float(step_size), int(n_leapfrog),
                                      L.F32 if self.dtype == np.float32 else L.F64, device)
        L.check(st, "mmcmc_hmc_create")

    def set_seed(self, seed: int) -> "HMC":
        """hmc.rs:118-121."""
        L.check(L.lib().mmcmc_hmc_seed(self._h, int(seed)), "mmcmc_hmc_seed")
        return self

    @property
    def kernel_variant(self) -> int:
        """The variant in use (set_kernel_variant takes the same numbers; results do not depend on it).  One chain per lane:
        0 plain, 2 noise of two iterations paired + pipelined (1 is kept as an alias: stored and reported as 1, runs as 2),
        5 noise waves + transition waves (up to dim 8; the f32 default there).  3: lane groups + MFMA (GaussianND of dim 16
        or 32, where it is the default).  6: run-time dimension (the default without a fixed-dimension kernel: dims other
        than 1..8, 16, 32; selectable elsewhere while a chain's vectors fit LDS).  7: a run-time compiled unit -- a
        UserTarget's only variant, and the default of a built-in target at dims 9..31, where 6 stays selectable.
        8: wide, one chain per workgroup (IsotropicGaussian, RosenbrockND, StandardNormal from dim 4; the default where no
        fixed-dimension kernel exists, from dim 128 with fewer than 1024 chains)."""
        return int(L.lib().mmcmc_hmc_kernel_variant(self._h))

    def step(self) -> None:
        """hmc.rs:304-377: one transition of every chain."""
        L.check(L.lib().mmcmc_hmc_step(self._h, None), "mmcmc_hmc_step")
        L.check(L.lib().mmcmc_hmc_sync(self._h), "mmcmc_hmc_sync")

    # The reference's public fields (hmc.rs:41-49): setting one applies from the next transition on; seed, chain offset and
    # iteration counter are untouched.
    def _params(self):
        eps, n = C.c_double(), C.c_int()
        L.check(L.lib().mmcmc_hmc_params(self._h, C.byref(eps), C.byref(n)), "mmcmc_hmc_params")
        return eps.value, n.value

    @property
    def step_size(self) -> float:
        """hmc.rs:43 `step_size`."""
        return self._params()[0]

    @step_size.setter
    def step_size(self, eps: float) -> None:
        L.check(L.lib().mmcmc_hmc_set_step_size(self._h, float(eps)), "mmcmc_hmc_set_step_size")

    @property
    def n_leapfrog(self) -> int:
        """hmc.rs:46 `n_leapfrog`."""
        return self._params()[1]

    @n_leapfrog.setter
    def n_leapfrog(self, n: int) -> None:
        L.check(L.lib().mmcmc_hmc_set_n_leapfrog(self._h, int(n)), "mmcmc_hmc_set_n_leapfrog")

    @property
    def metric(self):
        """The diagonal metric: scales [dim] float64 (M = diag(1 / s_i^2); the step of coordinate i is step_size * s_i), or
        None when none is set.  Setting it (an array of finite scales > 0, or None to clear) applies from the next transition
        on, to step / run / run_progress / run_scheduled alike; a metric of ones gives the bits of no metric.  With the
        posterior's standard deviations as scales a step_size of order 1 is the natural scale (warmup.warmup_hmc).  Up to
        dim 32; the first use compiles the target's metric unit (seconds); kernel_variant is 7 while a metric is set."""
        return K.get_metric(self)

    @metric.setter
    def metric(self, scale) -> None:
        K.set_metric(self, scale)

    @property
    def metric_chol(self):
        """The dense metric: a lower-triangular factor L [dim, dim] float64 with positive diagonal -- Sigma = L L^T stands for
        the posterior covariance, M = Sigma^-1 in whitened momentum: the drift moves x by step_size * (L p), a kick moves p
        by k * (L^T g) --, or None when none is set; the getter returns exactly what was set.  A handle has one metric:
        setting this replaces a diagonal `metric` and the other way round, and None to either removes whichever is set.
        An identity factor gives the bits of no metric.  Up to dim 32; the first use compiles the target's dense-metric
        unit (seconds); kernel_variant is 7 while a metric is set (warmup.warmup_hmc(..., dense=True))."""
        return K.get_metric_chol(self)

    @metric_chol.setter
    def metric_chol(self, chol) -> None:
        K.set_metric_chol(self, chol)

    @property
    def positions(self) -> np.ndarray:
        """hmc.rs:49 `positions` [n_chains, D]."""
        return self.state()

    @positions.setter
    def positions(self, x) -> None:
        """[n_chains, D] of the handle's dtype: a numpy array, or a contiguous torch tensor on the handle's device (copied on
        torch's current stream, like run(to="torch"))."""
        self._set_state(x)

    def run_scheduled(self, step_sizes, n_leapfrogs, n_collect: int, to: str = "numpy", accept_counts: bool = True):
        """Transition k of the run uses (step_sizes[k], n_leapfrogs[k]); the first len - n_collect transitions are discarded.
        Bit for bit the loop `step_size = eps_k; n_leapfrog = L_k; step()`, keeping the last n_collect states, in one call (one
        launch on the default kernels of the fixed-dimension targets).  step_size / n_leapfrog are unchanged afterwards.
        Returns the sample [n_chains, n_collect, dim] like run()."""
        eps = np.ascontiguousarray(step_sizes, dtype=np.float64).reshape(-1)
        nl = np.ascontiguousarray(n_leapfrogs, dtype=np.int32).reshape(-1)
        if eps.shape != nl.shape:
            raise ValueError("step_sizes and n_leapfrogs differ in length")
        n_collect = int(n_collect)
        if not 0 <= n_collect <= eps.size:
            raise ValueError(f"n_collect {n_collect} outside [0, {eps.size}]")
        n_discard = eps.size - n_collect
        epsp = eps.ctypes.data_as(C.POINTER(C.c_double))
        nlp = nl.ctypes.data_as(C.POINTER(C.c_int32))
        acc = np.zeros(self.n_chains, dtype=np.uint64) if accept_counts else None
        accp = acc.ctypes.data_as(C.POINTER(C.c_uint64)) if accept_counts else None
        fn = L.lib().mmcmc_hmc_run_scheduled
        if to == "torch":
            import torch

            tdt = torch.float32 if self.dtype == np.float32 else torch.float64
            dev = torch.device("cuda", self.device)
            out = torch.empty((self.n_chains, n_collect, self.dim), dtype=tdt, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(fn(self._h, n_collect, n_discard, epsp, nlp, C.c_void_p(out.data_ptr()), 1, accp, C.c_void_p(stream)),
                    "mmcmc_hmc_run_scheduled")
        else:
            out = np.empty((self.n_chains, n_collect, self.dim), dtype=self.dtype)
            L.check(fn(self._h, n_collect, n_discard, epsp, nlp, out.ctypes.data, 0, accp, None), "mmcmc_hmc_run_scheduled")
            L.check(L.lib().mmcmc_hmc_sync(self._h), "mmcmc_hmc_sync")
        self.accept_counts = acc
        return out


def jitter_schedule(n_blocks: int, block: int, eps_range, leapfrog_range, schedule_seed: int = 7):
    """Per-transition (step_sizes [n_blocks * block] float64, n_leapfrogs int32) holding one (eps_k, L_k) per block of `block`
    transitions, eps_k ~ U(eps_range), L_k ~ U{leapfrog_range}, drawn from numpy's PCG64(schedule_seed) in run_chain_of_handles'
    order (eps, then L, per block): block = its n_per_launch gives its sequence of (eps, L)."""
    rng = np.random.default_rng(schedule_seed)
    eps = np.empty(n_blocks, dtype=np.float64)
    nl = np.empty(n_blocks, dtype=np.int32)
    for k in range(n_blocks):
        eps[k] = float(rng.uniform(eps_range[0], eps_range[1]))
        nl[k] = int(rng.integers(leapfrog_range[0], leapfrog_range[1] + 1))
    return np.repeat(eps, block), np.repeat(nl, block)


def run_jittered(target: Target, initial_positions, eps_range, leapfrog_range, block: int, burn_blocks: int, keep_blocks: int,
                 seed: int = 42, schedule_seed: int = 7, device: int = 0):
    """run_chain_of_handles' workload on ONE handle: the same (eps_k, L_k) per block of `block` transitions (jitter_schedule),
    one run_scheduled call -- no host round trip of the state between blocks.  Each transition leaves the target invariant, so
    does the sequence; the noise stream is the handle's (seed), not run_chain_of_handles' seed + k per launch.  Returns
    (sample [n_chains, keep_blocks * block, dim] as a torch tensor on the device, info) with run_chain_of_handles' info keys and
    wall_ms (the call, synchronised, host clock).  accept_rate is over all transitions, the burned blocks included."""
    import time

    import torch

    eps, nl = jitter_schedule(burn_blocks + keep_blocks, block, eps_range, leapfrog_range, schedule_seed)
    h = HMC(target, initial_positions, float(eps[0]), int(nl[0]), device=device).set_seed(seed)
    n_chains = h.n_chains
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    t = h.run_scheduled(eps, nl, keep_blocks * block, to="torch")
    torch.cuda.synchronize(device)
    wall_ms = (time.perf_counter() - t0) * 1e3
    kernel_ms = float(h.timing()["kernel_ms"])
    info = {"kernel_ms": kernel_ms, "launches": int(h.timing()["n_launches"]), "leapfrogs": float(n_chains) * float(nl.astype(np.float64).sum()),
            "accept_rate": float(h.accept_counts.mean()) / len(eps) if len(eps) else 0.0,
            "schedule_head": [(float(eps[k * block]), int(nl[k * block])) for k in range(min(4, burn_blocks + keep_blocks))],
            "wall_ms": wall_ms}
    h.close()
    return t, info


def run_chain_of_handles(target: Target, initial_positions, eps_range, leapfrog_range, n_per_launch: int, burn_launches: int,
                         keep_launches: int, seed: int = 42, schedule_seed: int = 7, device: int = 0):
    """A converged sample from the REFERENCE's sampler on a target where one fixed (step_size, n_leapfrog) does not mix
    (RosenbrockND(3): profiles/r5b_, r6m_converged_probe.jsonl, r6s_converged_hmc_robustness.jsonl).  `HMC` has no jitter (hmc.rs:87-121, 304-431), but its
    constructor takes any initial positions: launch k is `HMC::new(target, positions of launch k - 1, eps_k, L_k)` followed
    by `run(n_per_launch, 0)` (hmc.rs:137-158), with eps_k ~ U(eps_range), L_k ~ U{leapfrog_range} drawn on the host from
    numpy's PCG64(schedule_seed) -- every launch IS the reference's sampler, each leaves the target invariant, so does their
    sequence.  Handle k is seeded `seed + k` (a handle's stream starts at iteration 0).  The first `burn_launches` launches are
    discarded.  Returns (sample [n_chains, keep_launches * n_per_launch, dim] as a torch tensor on the device, info)."""
    import torch

    rng = np.random.default_rng(schedule_seed)
    state = np.ascontiguousarray(initial_positions)
    n_chains, dim = state.shape
    keep = torch.empty((n_chains, keep_launches * n_per_launch, dim), dtype=torch.float32 if state.dtype == np.float32 else torch.float64,
                       device=torch.device("cuda", device))
    kernel_ms, accepts, leapfrogs, schedule = 0.0, 0.0, 0.0, []
    for k in range(burn_launches + keep_launches):
        eps = float(rng.uniform(eps_range[0], eps_range[1]))
        n_leap = int(rng.integers(leapfrog_range[0], leapfrog_range[1] + 1))
        h = HMC(target, state, eps, n_leap, device=device).set_seed(seed + k)
        t = h.run(n_per_launch, 0, to="torch")
        torch.cuda.synchronize(device)
        kernel_ms += float(h.timing()["kernel_ms"])
        leapfrogs += float(n_chains) * n_per_launch * n_leap
        if k >= burn_launches:
            keep[:, (k - burn_launches) * n_per_launch:(k - burn_launches + 1) * n_per_launch] = t
            accepts += float(h.accept_counts.mean())
        schedule.append((eps, n_leap))
        state = h.state()
        h.close()
        del t
    info = {"kernel_ms": kernel_ms, "launches": burn_launches + keep_launches, "leapfrogs": leapfrogs,
            "accept_rate": accepts / (keep_launches * n_per_launch), "schedule_head": schedule[:4]}
    return keep, info

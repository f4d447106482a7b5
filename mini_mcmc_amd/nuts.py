"""`NUTS` -- host-side mirror of src/nuts.rs:123-170, 194-353 over the GPU engine."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import checkpoint as K
from .distributions import IsotropicGaussian, Target


# mmcmc_nuts_draw as a numpy structured dtype: [n_chains, n_rows] records indexed like the sample's first two axes
DRAW_DTYPE = np.dtype([("accept_stat", np.float32), ("step_size", np.float32), ("energy", np.float32), ("tree", np.uint32)])


def unpack_tree(tree):
    """The packed `tree` field of per-draw records -> (n_leapfrog, depth, divergent, depth_cap, transition): integer arrays for
    the first two, boolean ones for the flags; `transition` is False for a row no transition produced (row 0 of a run without
    burn-in, the initial position)."""
    t = np.asarray(tree, dtype=np.uint32)
    return (t & np.uint32(0xFFFF)).astype(np.int64), ((t >> np.uint32(16)) & np.uint32(15)).astype(np.int64), \
        ((t >> np.uint32(24)) & np.uint32(1)).astype(bool), ((t >> np.uint32(25)) & np.uint32(1)).astype(bool), (t >> np.uint32(31)) == 0


class NUTS(K.Checkpointable):
    """NUTS::new(target, initial_positions, target_accept_p) (nuts.rs:123-129).

    mode 0: f32 tensors + f64 scalars (the reference's `NUTS<f64, Autodiff<NdArray>, _>`), 1: f32 + f32,
    2: f64 + f64.  `run(n_collect, n_discard)` keeps the reference's N-1-steps semantics; `run_progress` takes all
    N steps and returns (sample, RunStats) like nuts.rs:194-338 (without the terminal UI)."""

    _cprefix = _ckpt_sampler = "nuts"

    def __init__(self, target: Target, initial_positions, target_accept_p: float, mode: int = 0, device: int = 0):
        init = np.ascontiguousarray(initial_positions, dtype=np.float64)
        if init.ndim == 1:
            init = init[None, :]
        self.n_chains, self.dim = init.shape
        self.mode, self.device = mode, device
        self.dtype = np.float64 if mode == 2 else np.float32
        if target.dim != self.dim:
            if type(target).__name__ in ("RosenbrockND", "StandardNormal"):
                target = type(target)(self.dim)
            elif isinstance(target, IsotropicGaussian):
                target = IsotropicGaussian(target.std, self.dim)
            else:
                raise ValueError(f"target dim {target.dim} != state dim {self.dim}")
        self.target = target
        self._h = C.c_void_p()
        d = target.desc()
        st = L.lib().mmcmc_nuts_create(C.byref(self._h), C.byref(d), init.ctypes.data_as(C.POINTER(C.c_double)),
                                       self.n_chains, float(target_accept_p), mode, device)
        L.check(st, "mmcmc_nuts_create")

    def set_seed(self, seed: int) -> "NUTS":
        """nuts.rs:347-353"""
        L.check(L.lib().mmcmc_nuts_seed(self._h, int(seed)), "mmcmc_nuts_seed")
        return self

    def set_chain_offset(self, first_global_chain: int) -> "NUTS":
        L.check(L.lib().mmcmc_nuts_set_chain_offset(self._h, int(first_global_chain)), "set_chain_offset")
        return self

    def set_max_depth(self, max_depth: int) -> "NUTS":
        L.check(L.lib().mmcmc_nuts_set_max_depth(self._h, int(max_depth)), "mmcmc_nuts_set_max_depth")
        return self

    def set_kernel_variant(self, variant: int) -> "NUTS":
        """One chain per lane: 0 = the lanes of a wave take their transitions in step, 4 = every lane advances on its
        own, one leaf per tick (default for dim <= 8; same results as 0).  1 = lane-group / MFMA mapping in one launch;
        2 / 3 = the same with tree-depth compaction by one launch per level / by a persistent scheduler (1..3: mode 2,
        GaussianND, dim 16 or 32, where 3 is the default; all three give bit-identical samples).  6 = run-time dimension
        (the N-dimensional built-in targets at any dim; the default where no compiled instance exists; same results as 0)."""
        L.check(L.lib().mmcmc_nuts_set_kernel_variant(self._h, int(variant)), "mmcmc_nuts_set_kernel_variant")
        return self

    def set_compaction(self, first_level: int = 5, n_groups: int = 0) -> "NUTS":
        """variants 2, 3: doublings below `first_level` run before the first re-packing; variant 2: `n_groups` chain groups
        with their own launch sequences (0 = one per 16 384 chains).  Neither changes a result."""
        L.check(L.lib().mmcmc_nuts_set_compaction(self._h, int(first_level), int(n_groups)), "mmcmc_nuts_set_compaction")
        return self

    @property
    def kernel_variant(self) -> int:
        return int(L.lib().mmcmc_nuts_kernel_variant(self._h))

    def _run(self, n_collect, n_discard, progress, to):
        if to == "torch":
            import torch

            dev = torch.device("cuda", self.device)
            out = torch.empty((self.n_chains, n_collect, self.dim), device=dev,
                              dtype=torch.float64 if self.mode == 2 else torch.float32)
            stream = torch.cuda.current_stream(dev).cuda_stream
            st = L.lib().mmcmc_nuts_run(self._h, n_collect, n_discard, out.data_ptr(), 1, int(progress), C.c_void_p(stream))
            L.check(st, "mmcmc_nuts_run")
            return out
        out = np.empty((self.n_chains, n_collect, self.dim), dtype=self.dtype)
        st = L.lib().mmcmc_nuts_run(self._h, n_collect, n_discard, out.ctypes.data, 0, int(progress), None)
        L.check(st, "mmcmc_nuts_run")
        L.check(L.lib().mmcmc_nuts_sync(self._h), "mmcmc_nuts_sync")
        return out

    def run(self, n_collect: int, n_discard: int, to: str = "numpy"):
        """NUTS::run (nuts.rs:163-170): sample [n_chains, n_collect, dim]."""
        return self._run(n_collect, n_discard, False, to)

    def run_progress(self, n_collect: int, n_discard: int, to: str = "numpy", every: int = 0, callback=None):
        """NUTS::run_progress (nuts.rs:172-345): (sample, RunStats); per-chain ChainTrackers fed the initial position and
        all n_discard + n_collect states (nuts.rs:486-506) end up in `self.tracker` (mmcmc_nuts_run_progress)."""
        from .core import _run_progress_c

        return _run_progress_c(self, L.lib().mmcmc_nuts_run_progress, n_collect, n_discard, every, callback, to, self.dtype)

    def positions(self) -> np.ndarray:
        out = np.empty((self.n_chains, self.dim), dtype=self.dtype)
        L.check(L.lib().mmcmc_nuts_state(self._h, out.ctypes.data), "mmcmc_nuts_state")
        return out

    def adapt_state(self) -> dict:
        out = np.empty((self.n_chains, 4), dtype=np.float64)
        L.check(L.lib().mmcmc_nuts_adapt_state(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "adapt_state")
        return dict(epsilon=out[:, 0], epsilon_bar=out[:, 1], h_bar=out[:, 2], mu=out[:, 3])

    # NUTSChain's public state (nuts.rs:361-386: pub position and the adaptation fields): from the next run on; seed, chain
    # offset and iteration (self.m) untouched.
    def set_positions(self, x) -> "NUTS":
        """[n_chains, D] of the mode's tensor type (float32 for modes 0 / 1, float64 for mode 2): a numpy array, or a
        contiguous torch tensor on the handle's device (copied on torch's current stream)."""
        if type(x).__module__.startswith("torch"):
            import torch

            tdt = torch.float64 if self.mode == 2 else torch.float32
            if (x.dtype != tdt or tuple(x.shape) != (self.n_chains, self.dim) or not x.is_contiguous() or x.device.type != "cuda"
                    or x.device.index != self.device):
                raise ValueError(f"positions: a contiguous {tdt} tensor [{self.n_chains}, {self.dim}] on cuda:{self.device}")
            stream = torch.cuda.current_stream(x.device).cuda_stream
            L.check(L.lib().mmcmc_nuts_set_state(self._h, C.c_void_p(x.data_ptr()), 1, C.c_void_p(stream)), "mmcmc_nuts_set_state")
            return self
        a = np.asarray(x)
        if a.shape != (self.n_chains, self.dim):
            raise ValueError(f"positions: shape {a.shape} != ({self.n_chains}, {self.dim})")
        a = np.ascontiguousarray(a, dtype=self.dtype)
        L.check(L.lib().mmcmc_nuts_set_state(self._h, a.ctypes.data, 0, None), "mmcmc_nuts_set_state")
        return self

    def set_adapt_state(self, adapt) -> "NUTS":
        """The inverse of adapt_state(): its dict, or [n_chains, 4] = epsilon, epsilon_bar, h_bar, mu.  Finite values,
        epsilon > 0 or the sentinel -1 (not yet searched)."""
        if isinstance(adapt, dict):
            adapt = np.stack([np.asarray(adapt[k], dtype=np.float64) for k in ("epsilon", "epsilon_bar", "h_bar", "mu")], axis=1)
        K.set_adapt_array(self, adapt)
        return self

    @property
    def metric(self):
        """The diagonal metric: scales [dim] float64 (M = diag(1 / s_i^2); the leapfrog steps coordinate i by epsilon * s_i), or
        None when none is set.  Setting it (finite scales > 0, or None to clear) applies from the next run on; seed, iteration
        and adaptation records are untouched -- set epsilon to the sentinel -1 (set_adapt_state) to have the next run search
        the step size under the new metric, as warmup.warmup_nuts does.  Up to dim 32; the first use compiles the target's
        metric unit (seconds); kernel_variant is 7 while a metric is set."""
        return K.get_metric(self)

    @metric.setter
    def metric(self, scale) -> None:
        K.set_metric(self, scale)

    @property
    def metric_chol(self):
        """The dense metric: a lower-triangular factor L [dim, dim] float64 with positive diagonal (Sigma = L L^T stands for the
        posterior covariance; the leapfrog drifts by epsilon * (L p) and kicks by (epsilon / 2) * (L^T g), the stop criterion
        takes L^-1 (x+ - x-)), or None when none is set; the getter returns exactly what was set.  A handle has one
        metric: setting this replaces a diagonal `metric` and the other way round, None to either removes whichever is
        set.  Seed, iteration and adaptation records are untouched (warmup.warmup_nuts(..., dense=True) resets epsilon to
        the sentinel).  Up to dim 32; the first use compiles the target's dense-metric unit (seconds)."""
        return K.get_metric_chol(self)

    @metric_chol.setter
    def metric_chol(self, chol) -> None:
        K.set_metric_chol(self, chol)

    def set_draw_stats(self, on: bool = True) -> "NUTS":
        """Record one `DRAW_DTYPE` entry per chain and sample row from the next run on (accept_stat, step_size, energy, and the
        packed tree: leapfrogs, depth, divergent, depth cap; `unpack_tree`).  No result changes; the handle runs its target's stats
        unit (compiled on the first use, seconds; kernel_variant 7) until recording is switched off, which frees the records.
        The buffer is n_chains * n_rows * 16 bytes on the device."""
        L.check(L.lib().mmcmc_nuts_set_draw_stats(self._h, 1 if on else 0), "mmcmc_nuts_set_draw_stats")
        return self

    @property
    def draw_stats_enabled(self) -> bool:
        return L.lib().mmcmc_nuts_draw_stats_enabled(self._h) == 1

    def draw_stats(self, to: str = "numpy"):
        """The records of the last run: numpy [n_chains, n_rows] of `DRAW_DTYPE`, or with to="torch" a uint8 tensor
        [n_chains, n_rows, 16] on the handle's device (the same bytes; stats.nuts_summary takes either)."""
        n = C.c_size_t()
        L.check(L.lib().mmcmc_nuts_draw_stats(self._h, None, 0, C.byref(n)), "mmcmc_nuts_draw_stats")
        if to == "torch":
            import torch

            out = torch.empty((self.n_chains, n.value, 16), device=torch.device("cuda", self.device), dtype=torch.uint8)
            L.check(L.lib().mmcmc_nuts_draw_stats(self._h, C.c_void_p(out.data_ptr()), 1, None), "mmcmc_nuts_draw_stats")
            return out
        out = np.empty((self.n_chains, n.value), dtype=DRAW_DTYPE)
        L.check(L.lib().mmcmc_nuts_draw_stats(self._h, out.ctypes.data, 0, None), "mmcmc_nuts_draw_stats")
        return out

    def _params(self):
        p, d = C.c_double(), C.c_int()
        L.check(L.lib().mmcmc_nuts_params(self._h, C.byref(p), C.byref(d)), "mmcmc_nuts_params")
        return p.value, d.value

    @property
    def target_accept_p(self) -> float:
        return self._params()[0]

    def set_target_accept_p(self, p: float) -> "NUTS":
        L.check(L.lib().mmcmc_nuts_set_target_accept_p(self._h, float(p)), "mmcmc_nuts_set_target_accept_p")
        return self

    @property
    def max_depth(self) -> int:
        return self._params()[1]

    def leapfrog_counts(self) -> np.ndarray:
        out = np.zeros(self.n_chains, dtype=np.uint64)
        L.check(L.lib().mmcmc_nuts_leapfrog_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "leapfrog_counts")
        return out

    def depth_histogram(self) -> np.ndarray:
        out = np.zeros(13, dtype=np.uint32)
        L.check(L.lib().mmcmc_nuts_depth_histogram(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))), "depth_histogram")
        return out

    def timing(self) -> dict:
        t = L.Timing()
        L.check(L.lib().mmcmc_nuts_timing(self._h, C.byref(t)), "mmcmc_nuts_timing")
        return dict(kernel_ms=t.kernel_ms, n_launches=t.n_launches, out_bytes=t.out_bytes, state_bytes=t.state_bytes)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            L.lib().mmcmc_nuts_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

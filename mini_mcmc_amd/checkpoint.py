"""Checkpoint and resume (include/mmcmc.h: "chain state and stream position").

The engine's noise is a function of (seed, global chain id, iteration) alone.  A handle's whole future is therefore fixed
by its positions, seed, chain offset, iteration counter and sampler fields, plus NUTS's per-chain adaptation records; a
checkpoint holds exactly these, and a handle restored from one continues bit for bit as the original would -- in another
process, or as a device group with another number of shards (a group's checkpoint has a single handle's layout).  The
reference marks this as a TODO (nuts.rs:524: "Somehow save state of the chains and enable continuing runs").

A checkpoint stores the target's KIND, not its parameters and not the data of a kind that carries data (`UserTarget(...,
data=)`): restoring onto a handle created over another array continues from the stored state under the new density, which is
the caller's business.  Created over the same array, the handle continues bit for bit.

A diagonal metric (`HMC.metric`, `NUTS.metric`) is part of a checkpoint: "metric", the scales as set, present only while one
is set.  A checkpoint without the key -- every checkpoint written before metrics existed -- restores as "no metric".
A dense metric (`HMC.metric_chol`, `NUTS.metric_chol`) is stored as "metric_chol", the factor as set, present only while a
dense metric is set (a handle has one metric: "metric" is then absent).

Not in a checkpoint: accept counts (per run), NUTS's cumulative leapfrog counts and depth histogram, tracker state
(`MultiChainTracker`), the kernel variant and iters_per_launch (none of them changes a result).

    ckpt = a.checkpoint()            # a dict of scalars (int / float / str) and numpy arrays
    save("run.npz", ckpt)            # numpy .npz, no pickle
    b.restore(load("run.npz"))       # b: same sampler kind, chain count, dimension, dtype / mode, target kind
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

FORMAT = 1
_U64 = C.c_uint64
_MAX_DEPTH = 12  # MM_NUTS_JMAX


def _fn(obj, name):
    return getattr(L.lib(), f"mmcmc_{obj._cprefix}_{name}")


def _is_group(obj) -> bool:
    return obj._cprefix.endswith("_group")


class Checkpointable:
    """Stream position, iteration counter, checkpoint() and restore() of a handle or device group.  A class using it sets
    `_cprefix` (the C ABI prefix: "mh", "hmc_group", ...) and `_ckpt_sampler` ("mh", "hmc", "nuts", "mh_discrete",
    "gibbs_mixture") and has n_chains / dim / dtype (NUTS: mode) and a target kind."""

    _cprefix = ""
    _ckpt_sampler = ""

    def stream_position(self):
        """(seed, first global chain, iteration): what keys the next transition's noise besides the positions (NUTS: the
        iteration is self.m, which the adaptation also reads against n_discard)."""
        seed, off, it = _U64(), _U64(), _U64()
        L.check(_fn(self, "stream_position")(self._h, C.byref(seed), C.byref(off), C.byref(it)),
                f"mmcmc_{self._cprefix}_stream_position")
        return int(seed.value), int(off.value), int(it.value)

    def set_iteration(self, iteration: int):
        """The next transition's iteration index (< 2^32); nothing else changes."""
        it = int(iteration)
        if not 0 <= it < 2 ** 32:
            raise ValueError(f"iteration {it} outside [0, 2^32)")
        L.check(_fn(self, "set_iteration")(self._h, it), f"mmcmc_{self._cprefix}_set_iteration")
        return self

    def checkpoint(self) -> dict:
        return take(self)

    def restore(self, ckpt: dict):
        apply(self, ckpt)
        return self


def _target_kind(obj) -> int:
    if obj._ckpt_sampler == "mh_discrete":
        return int(obj.model.kind)
    if obj._ckpt_sampler == "gibbs_mixture":
        return -1  # the built-in mixture conditional: no target registry
    return int(obj.target.kind)


def _positions(obj) -> np.ndarray:
    if obj._ckpt_sampler == "nuts" and not _is_group(obj):
        return obj.positions()
    return obj.state()


def _dims(obj):
    """(dim, dtype name) as a checkpoint records them"""
    if obj._ckpt_sampler == "mh_discrete":
        return 1, "int32"
    if obj._ckpt_sampler == "gibbs_mixture":
        return 2, "float64"
    return int(obj.dim), np.dtype(obj.dtype).name


def _fields(obj) -> dict:
    s = obj._ckpt_sampler
    if s == "mh":
        std = C.c_double()
        L.check(_fn(obj, "params")(obj._h, C.byref(std)), f"mmcmc_{obj._cprefix}_params")
        return {"proposal_std": std.value}
    if s == "hmc":
        eps, n = C.c_double(), C.c_int()
        L.check(_fn(obj, "params")(obj._h, C.byref(eps), C.byref(n)), f"mmcmc_{obj._cprefix}_params")
        return {"step_size": eps.value, "n_leapfrog": n.value}
    if s == "nuts":
        p, d = C.c_double(), C.c_int()
        L.check(_fn(obj, "params")(obj._h, C.byref(p), C.byref(d)), f"mmcmc_{obj._cprefix}_params")
        return {"target_accept_p": p.value, "max_depth": d.value}
    return {}


def adapt_array(obj) -> np.ndarray:
    """NUTS adaptation records [n_chains, 4] float64 = epsilon, epsilon_bar, h_bar, mu"""
    out = np.empty((obj.n_chains, 4), dtype=np.float64)
    L.check(_fn(obj, "adapt_state")(obj._h, out.ctypes.data_as(C.POINTER(C.c_double))), f"mmcmc_{obj._cprefix}_adapt_state")
    return out


def check_adapt(adapt, n_chains: int, mode: int) -> np.ndarray:
    """[n_chains, 4] float64, every value finite (also in the mode's scalar type), epsilon > 0 or exactly -1"""
    a = np.ascontiguousarray(adapt, dtype=np.float64)
    if a.shape != (n_chains, 4):
        raise ValueError(f"adaptation state: shape {a.shape} != ({n_chains}, 4)")
    with np.errstate(over="ignore"):
        v = a.astype(np.float32).astype(np.float64) if mode == 1 else a
    if not np.all(np.isfinite(a)) or not np.all(np.isfinite(v)):
        raise ValueError("adaptation state: every value must be finite")
    if not np.all((v[:, 0] > 0) | (a[:, 0] == -1.0)):
        raise ValueError("adaptation state: epsilon must be > 0 or the sentinel -1")
    return a


def set_adapt_array(obj, adapt) -> None:
    a = check_adapt(adapt, obj.n_chains, obj.mode)
    L.check(_fn(obj, "set_adapt_state")(obj._h, a.ctypes.data_as(C.POINTER(C.c_double))), f"mmcmc_{obj._cprefix}_set_adapt_state")


def set_positions_host(obj, x) -> None:
    """positions from a host array of the checkpoint's shape and exactly the handle's dtype"""
    dim, dt = _dims(obj)
    shape = (obj.n_chains,) if obj._ckpt_sampler == "mh_discrete" else (obj.n_chains, dim)
    a = np.asarray(x)
    if a.shape != shape or a.dtype != np.dtype(dt):
        raise ValueError(f"positions: {a.dtype} {a.shape}, the handle holds {dt} {shape}")
    a = np.ascontiguousarray(a)
    fn, name = _fn(obj, "set_state"), f"mmcmc_{obj._cprefix}_set_state"
    if obj._ckpt_sampler == "mh_discrete":
        L.check(fn(obj._h, a.ctypes.data_as(C.POINTER(C.c_int32))), name)
    elif obj._ckpt_sampler == "gibbs_mixture":
        L.check(fn(obj._h, a.ctypes.data_as(C.POINTER(C.c_double))), name)
    elif _is_group(obj):
        L.check(fn(obj._h, a.ctypes.data), name)
    else:
        L.check(fn(obj._h, a.ctypes.data, 0, None), name)


def get_metric(obj):
    """The diagonal metric of an HMC / NUTS handle: its scales [dim] float64 as set, or None when none is set."""
    out = np.empty(int(obj.dim), dtype=np.float64)
    st = _fn(obj, "metric")(obj._h, out.ctypes.data_as(C.POINTER(C.c_double)))
    if st < 0:
        L.check(st, f"mmcmc_{obj._cprefix}_metric")
    return out if st == 1 else None  # 2: a dense metric is set (get_metric_chol), not a diagonal one


def get_metric_chol(obj):
    """The dense metric of an HMC / NUTS handle: its factor [dim, dim] float64 exactly as set, or None when none is set."""
    d = int(obj.dim)
    out = np.empty((d, d), dtype=np.float64)
    st = _fn(obj, "metric_dense")(obj._h, out.ctypes.data_as(C.POINTER(C.c_double)))
    if st < 0:
        L.check(st, f"mmcmc_{obj._cprefix}_metric_dense")
    return out if st == 1 else None


def check_metric_chol(chol, dim: int) -> np.ndarray:
    """[dim, dim] float64, finite, lower triangular with positive diagonal (the library checks the handle's type too)"""
    a = np.ascontiguousarray(chol, dtype=np.float64)
    if a.shape != (dim, dim):
        raise ValueError(f"metric_chol: shape {a.shape} != ({dim}, {dim})")
    if not np.all(np.isfinite(a)) or np.any(np.triu(a, 1) != 0) or not np.all(np.diag(a) > 0):
        raise ValueError("metric_chol: a finite lower-triangular factor with positive diagonal is required")
    return a


def set_metric_chol(obj, chol) -> None:
    """chol [dim, dim] lower triangular, or None to remove whichever metric is set; from the next transition on"""
    name = f"mmcmc_{obj._cprefix}_set_metric_dense"
    if chol is None:
        L.check(_fn(obj, "set_metric_dense")(obj._h, None), name)
        return
    a = check_metric_chol(chol, int(obj.dim))
    L.check(_fn(obj, "set_metric_dense")(obj._h, a.ctypes.data_as(C.POINTER(C.c_double))), name)


def check_metric(scale, dim: int) -> np.ndarray:
    """[dim] float64, every value finite and > 0 (the library checks the handle's element type too)"""
    a = np.ascontiguousarray(scale, dtype=np.float64)
    if a.shape != (dim,):
        raise ValueError(f"metric: shape {a.shape} != ({dim},)")
    if not np.all(np.isfinite(a)) or not np.all(a > 0):
        raise ValueError("metric: every scale must be finite and > 0")
    return a


def set_metric(obj, scale) -> None:
    """scale [dim] (finite, > 0), or None for the identity; from the next transition on"""
    name = f"mmcmc_{obj._cprefix}_set_metric"
    if scale is None:
        L.check(_fn(obj, "set_metric")(obj._h, None), name)
        return
    a = check_metric(scale, int(obj.dim))
    L.check(_fn(obj, "set_metric")(obj._h, a.ctypes.data_as(C.POINTER(C.c_double))), name)


def _has_metric(obj) -> bool:
    return obj._ckpt_sampler in ("hmc", "nuts") and not _is_group(obj)


def take(obj) -> dict:
    """The handle's (or group's) checkpoint: a dict of int / float / str scalars and numpy arrays."""
    dim, dt = _dims(obj)
    seed, first, it = obj.stream_position()
    ck = {"format": FORMAT, "sampler": obj._ckpt_sampler, "n_chains": int(obj.n_chains), "dim": dim, "dtype": dt,
          "mode": int(obj.mode) if obj._ckpt_sampler == "nuts" else -1, "target_kind": _target_kind(obj),
          "seed": seed, "first_global_chain": first, "iteration": it}
    ck.update(_fields(obj))
    ck["positions"] = _positions(obj)
    if obj._ckpt_sampler == "nuts":
        ck["adapt"] = adapt_array(obj)
    if _has_metric(obj):
        m = get_metric(obj)
        if m is not None:
            ck["metric"] = m
        m = get_metric_chol(obj)
        if m is not None:
            ck["metric_chol"] = m
    return ck


def apply(obj, ck: dict) -> None:
    """Restore `ck` into obj.  Refuses (ValueError, obj unchanged) a different sampler kind, chain count, dimension, dtype,
    NUTS mode or target kind, and any value a setter would refuse; then sets seed, chain offset, iteration, fields,
    positions and (NUTS) the adaptation records."""
    dim, dt = _dims(obj)
    want = {"format": FORMAT, "sampler": obj._ckpt_sampler, "n_chains": int(obj.n_chains), "dim": dim, "dtype": dt,
            "mode": int(obj.mode) if obj._ckpt_sampler == "nuts" else -1, "target_kind": _target_kind(obj)}
    for k, v in want.items():
        if k not in ck:
            raise ValueError(f"checkpoint: no '{k}'")
        if ck[k] != v:
            raise ValueError(f"checkpoint: {k} = {ck[k]!r}, this handle has {v!r}")
    # every value is checked before anything is set
    seed, first, it = int(ck["seed"]), int(ck["first_global_chain"]), int(ck["iteration"])
    if not (0 <= seed < 2 ** 64 and 0 <= first < 2 ** 64 and 0 <= it < 2 ** 32):
        raise ValueError("checkpoint: seed, first_global_chain or iteration out of range")
    s = obj._ckpt_sampler
    if s == "mh":
        std = float(ck["proposal_std"])
        if not (np.isfinite(std) and std > 0):
            raise ValueError(f"checkpoint: proposal_std {std}")
    elif s == "hmc":
        eps, nl = float(ck["step_size"]), int(ck["n_leapfrog"])
        if not (np.isfinite(eps) and eps > 0) or nl < 0:
            raise ValueError(f"checkpoint: step_size {eps}, n_leapfrog {nl}")
    elif s == "nuts":
        tap, md = float(ck["target_accept_p"]), int(ck["max_depth"])
        if not (0 < tap < 1) or not 1 <= md <= _MAX_DEPTH:
            raise ValueError(f"checkpoint: target_accept_p {tap}, max_depth {md}")
        adapt = check_adapt(ck["adapt"], obj.n_chains, obj.mode)
    metric = None
    if "metric" in ck:
        if not _has_metric(obj):
            raise ValueError("checkpoint: it holds a metric, this handle cannot take one")
        metric = check_metric(ck["metric"], dim)  # a wrong length is refused before anything is set
    metric_chol = None
    if "metric_chol" in ck:
        if not _has_metric(obj) or metric is not None:
            raise ValueError("checkpoint: it holds a dense metric, this handle cannot take it (or a diagonal one is stored too)")
        metric_chol = check_metric_chol(ck["metric_chol"], dim)
    pos = np.asarray(ck["positions"])
    shape = (obj.n_chains,) if s == "mh_discrete" else (obj.n_chains, dim)
    if pos.shape != shape or pos.dtype != np.dtype(dt):
        raise ValueError(f"checkpoint: positions {pos.dtype} {pos.shape}, the handle holds {dt} {shape}")

    L.check(_fn(obj, "seed")(obj._h, seed), f"mmcmc_{obj._cprefix}_seed")
    L.check(_fn(obj, "set_chain_offset")(obj._h, first), f"mmcmc_{obj._cprefix}_set_chain_offset")
    obj.set_iteration(it)
    if s == "mh":
        L.check(_fn(obj, "set_proposal_std")(obj._h, std), f"mmcmc_{obj._cprefix}_set_proposal_std")
    elif s == "hmc":
        L.check(_fn(obj, "set_step_size")(obj._h, eps), f"mmcmc_{obj._cprefix}_set_step_size")
        L.check(_fn(obj, "set_n_leapfrog")(obj._h, nl), f"mmcmc_{obj._cprefix}_set_n_leapfrog")
    elif s == "nuts":
        L.check(_fn(obj, "set_target_accept_p")(obj._h, tap), f"mmcmc_{obj._cprefix}_set_target_accept_p")
        L.check(_fn(obj, "set_max_depth")(obj._h, md), f"mmcmc_{obj._cprefix}_set_max_depth")
    set_positions_host(obj, pos)
    if s == "nuts":
        set_adapt_array(obj, adapt)
    if _has_metric(obj):
        if metric_chol is not None:
            set_metric_chol(obj, metric_chol)
        else:
            set_metric(obj, metric)  # None (a checkpoint without one): no metric


def save(path, ckpt: dict) -> None:
    """A checkpoint as a numpy .npz file: scalars become 0-d arrays (uint64 / int64 / float64 / unicode), no pickle."""
    arrays = {}
    for k, v in ckpt.items():
        if isinstance(v, np.ndarray):
            if v.dtype == object:
                raise TypeError(f"checkpoint: '{k}' is an object array")
            arrays[k] = v
        elif isinstance(v, (bool, np.bool_)):
            raise TypeError(f"checkpoint: '{k}' is a bool")
        elif isinstance(v, (int, np.integer)):
            arrays[k] = np.array(int(v), dtype=np.uint64 if int(v) >= 0 else np.int64)
        elif isinstance(v, (float, np.floating)):
            arrays[k] = np.array(float(v), dtype=np.float64)
        elif isinstance(v, str):
            arrays[k] = np.array(v)
        else:
            raise TypeError(f"checkpoint: '{k}' has type {type(v).__name__}")
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load(path) -> dict:
    """The inverse of save(): 0-d arrays come back as int / float / str, arrays with their dtype."""
    out = {}
    with np.load(path, allow_pickle=False) as z:
        for k in z.files:
            a = z[k]
            if a.ndim == 0:
                v = a.item()
                out[k] = int(v) if a.dtype.kind in "ui" else float(v) if a.dtype.kind == "f" else str(v)
            else:
                out[k] = a
    return out

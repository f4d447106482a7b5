"""Plain numpy reference of the running-diagnostics tracker (csrc/mm_tracker.hip), for tests/test_tracker_edges.py.

A helper module, not a conftest; it imports nothing from the package under test.

  per chain   the f32 recurrences of MultiChainTracker::step (stats.rs:244-249) and ChainTracker::step (stats.rs:109-123)
              on np.float32 arrays, vectorised over the chains, one row after the other, written unfused:
              mean = (mean * (n - 1) + x) / n, mean_sq = x^2 at n == 1 and (mean_sq * (n - 1) + x^2) / n after it, last = x.
              Every numpy operation on float32 is the correctly rounded IEEE operation, so this is exact.
  p_accept    the sequential f32 fold p <- (1 - 0.01) p + 0.01 flag over the WHOLE flag history, step-major and chain-minor,
              from 0 (stats.rs:252-258) -- and `certificate`, which tells without a device which branch
              tracker_paccept_kernel takes for a call and therefore whether its number has to be that fold's bit for bit.
  aggregates  the formulas of tracker_rhat_kernel and tracker_chain_stats_kernel with every f64 block sum replaced by the
              exact sum (math.fsum), rounded where the kernel rounds, the remaining f32 operations as written.  A device
              block sum, once rounded to f32, may sit one f32 ulp off the correctly rounded exact sum (f64 accumulation
              order), so every output is also evaluated for each combination of -1 / 0 / +1 ulp on its rounded sums:
              an interval [lo, hi] per output.
  float64     mean and mean of squares of the first n states from np.cumsum in f64 and R-hat from those: what the f32
              recurrence itself costs.
"""
import math

import numpy as np

F32 = np.float32
ALPHA = F32(0.01)                # stats.rs:13
ONE_MINUS_ALPHA = F32(1.0) - ALPHA  # evaluated in f32, as `1.0 - ALPHA` is in the reference
TAIL = 16384                     # flags tracker_paccept_kernel replays at most (kTail)
PER_LANE = 256                   # its flags per lane
CERT_LANES = 16                  # lanes (of 256 flags) its certificate replays


def to_f32(x):
    """to_f32 (stats.rs:66-71): f64 input is rounded to f32 before anything else"""
    return np.ascontiguousarray(np.asarray(x).astype(np.float32))


def fold(p, flags):
    """p <- fl(fl((1 - a) p) + a f) over flags in order, in f32"""
    p, zero = F32(p), F32(0.0)
    for f in np.asarray(flags).ravel().tolist():
        p = ONE_MINUS_ALPHA * p + (ALPHA if f else zero)
    return p


def certificate(call_flags):
    """What tracker_paccept_kernel does with the flags [k, C] of one call (it never sees earlier ones).

    It looks at the last len = min(k C, 16384) of them, 256 per lane, and first replays the last 16 occupied lanes from
    p = 0 and from p = 1; where the two meet that number is the result.  Otherwise it replays all len flags from the stored
    value (k C <= 16384: the fold simply continues, exact) or, when flags were cut off (`restart`), from 0.5.
    class: 'certificate' | 'carry' | 'restart'; the first two must reproduce the sequential fold bit for bit."""
    fl = np.asarray(call_flags, dtype=np.uint8).ravel()
    need = fl.size
    ln = min(need, TAIL)
    tail = fl[need - ln:]
    last_lane = (ln - 1) // PER_LANE
    l0 = max(0, last_lane + 1 - CERT_LANES)
    window = tail[l0 * PER_LANE:]
    lo, hi = fold(0.0, window), fold(1.0, window)
    w4096 = tail[ln - min(ln, 4096):]
    lo2, hi2 = fold(0.0, w4096), fold(1.0, w4096)
    meets = bool(lo == hi)
    return dict(first=need - ln, len=ln, restart=need > TAIL, meets=meets, value=lo, window=int(window.size),
                meets_last_4096=bool(lo2 == hi2), value_last_4096=lo2,
                cls="certificate" if meets else ("carry" if need <= TAIL else "restart"))


class Tracker:
    """The per-chain state of mmcmc_tracker after create / init_last / steps, and the global p_accept."""

    def __init__(self, n_chains, dim, init=None):
        self.C, self.D, self.n = int(n_chains), int(dim), 0
        self.mean = np.zeros((self.C, self.D), dtype=np.float32)
        self.mean_sq = np.zeros((self.C, self.D), dtype=np.float32)
        self.last = np.zeros((self.C, self.D), dtype=np.float32) if init is None else to_f32(init).reshape(self.C, self.D).copy()
        self.p_chain = np.full(self.C, -1.0, dtype=np.float32)  # ChainTracker::new (stats.rs:76)
        self.p = F32(0.0)                                        # MultiChainTracker::new (stats.rs:216-228)

    def steps(self, rows):
        """consume rows [C, k, D] in order; returns the flags [k, C] of these rows"""
        x = to_f32(rows)
        assert x.ndim == 3 and x.shape[0] == self.C and x.shape[2] == self.D
        k = x.shape[1]
        flags = np.empty((k, self.C), dtype=np.uint8)
        one = F32(1.0)
        for t in range(k):
            self.n += 1
            n = F32(self.n)
            xt = x[:, t, :]
            self.mean = (self.mean * (n - one) + xt) / n
            sq = xt * xt
            self.mean_sq = sq.copy() if self.n == 1 else (self.mean_sq * (n - one) + sq) / n
            dif = xt != self.last
            ne = dif.any(axis=1)
            # the first step starts the per-chain average from the comparison of coordinate 0 alone (quirk Q12)
            p_start = np.where(self.p_chain >= F32(0.0), self.p_chain, dif[:, 0].astype(np.float32))
            self.p_chain = (ONE_MINUS_ALPHA * p_start + ALPHA * ne.astype(np.float32)).astype(np.float32)
            self.last = xt.copy()
            flags[t] = ne
        self.p = fold(self.p, flags)
        return flags

    def snapshot(self):
        return dict(mean=self.mean.copy(), mean_sq=self.mean_sq.copy(), last=self.last.copy(), p_chain=self.p_chain.copy(),
                    p=F32(self.p), n=self.n)


# ---------------------------------------------------------------- aggregates


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def _ulps(v):
    v = F32(v)
    return (np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf)))


def _interval(vals):
    """(exact-sum value, lo, hi, whether some combination is NaN) of the 27 (or 3) evaluations; the centre comes first"""
    a = np.array(vals, dtype=np.float32)
    fin = a[~np.isnan(a)]
    lo = fin.min() if fin.size else F32(np.nan)
    hi = fin.max() if fin.size else F32(np.nan)
    return a[0], lo, hi, bool(np.isnan(a).any())


def _centre_first(seq):
    seq = list(seq)
    return [seq[1], seq[0], seq[2]]


def _sm2(mean_d, mean_sq_d, n):
    return (mean_sq_d - mean_d * mean_d) * n / (n - F32(1.0))


def rhat_stats(mean, mean_sq, n_i):
    """tracker_rhat_kernel (within_and_var, stats.rs:288-306): dict of (value, lo, hi, nan) arrays over the parameters"""
    C, D = mean.shape
    n, nch, one = F32(n_i), F32(C), F32(1.0)
    out = []
    with np.errstate(all="ignore"):
        for d in range(D):
            mc, vals = mean[:, d], []
            mean_chain0 = F32(_fsum(mc) / float(nch))
            within0 = F32(_fsum(_sm2(mc, mean_sq[:, d], n)) / float(nch))
            for mean_chain in _centre_first(_ulps(mean_chain0)):
                df = mc - mean_chain
                for bsum in _centre_first(_ulps(F32(_fsum(df * df)))):
                    between = bsum * (n / (nch - one))
                    for within in _centre_first(_ulps(within0)):
                        var = within * ((n - one) / n) + between * (one / n)
                        vals.append(np.sqrt(var / within))
            out.append(_interval(vals))
    return _columns(out)


def chain_stats(mean, mean_sq, p_chain, n_i):
    """tracker_chain_stats_kernel (collect_rhat, stats.rs:150-178, between / (C D - 1): quirk Q9; core.rs:268-281):
    dict rhat / within / var -> (value, lo, hi, nan) arrays over the parameters, p -> the same for the mean per-chain p"""
    C, D = mean.shape
    n, nch, one = F32(n_i), F32(C), F32(1.0)
    r, w, v = [], [], []
    with np.errstate(all="ignore"):
        for d in range(D):
            mc, rv, wv, vv = mean[:, d], [], [], []
            gm0 = F32(_fsum(mc) / float(nch))
            within0 = F32(_fsum(_sm2(mc, mean_sq[:, d], n)) / float(nch))
            for gm in _centre_first(_ulps(gm0)):
                df = mc - gm
                for ss in _centre_first(_ulps(F32(_fsum(df * df)))):
                    between = ss / F32(C * D - 1)
                    for within in _centre_first(_ulps(within0)):
                        var = between + within * ((n - one) / n)
                        rv.append(np.sqrt(var / within))
                        wv.append(within)
                        vv.append(var)
            r.append(_interval(rv))
            w.append(_interval(wv))
            v.append(_interval(vv))
        p = _interval(_centre_first(_ulps(F32(_fsum(p_chain) / float(C)))))
    return dict(rhat=_columns(r), within=_columns(w), var=_columns(v), p=p)


def _columns(rows):
    a = list(zip(*rows))
    return (np.array(a[0], dtype=np.float32), np.array(a[1], dtype=np.float32), np.array(a[2], dtype=np.float32),
            np.array(a[3], dtype=bool))


def inside(value, interval):
    """value (scalar or array) lies in the interval of `rhat_stats` / `chain_stats`; a NaN only where some combination of
    the rounded sums gives one"""
    _, lo, hi, nan = interval
    value = np.asarray(value, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(value), nan, (lo <= value) & (value <= hi))


def max_interval(interval):
    """[max lo, max hi]: where each R-hat lies in its interval, their maximum lies in this one"""
    c, lo, hi, nan = interval
    return (F32(np.max(c)), F32(np.max(lo)), F32(np.max(hi)), bool(np.any(nan)))


# ---------------------------------------------------------------- the float64 statement


def float64_statement(rows):
    """rows [C, n, D] as the tracker consumed them (already rounded to f32): f64 mean and mean of squares of the first
    1 .. n states of every chain, [C, n, D] each"""
    x = to_f32(rows).astype(np.float64)
    cnt = np.arange(1, x.shape[1] + 1, dtype=np.float64)[None, :, None]
    return np.cumsum(x, axis=1) / cnt, np.cumsum(x * x, axis=1) / cnt


def rhat_f64(mean, mean_sq, n_i):
    """(within_and_var's R-hat, collect_rhat's R-hat) in float64 from per-chain means [C, D]"""
    mean, mean_sq = np.asarray(mean, dtype=np.float64), np.asarray(mean_sq, dtype=np.float64)
    C, D = mean.shape
    n = float(n_i)
    with np.errstate(all="ignore"):
        within = ((mean_sq - mean * mean) * n / (n - 1.0)).mean(axis=0)
        ss = ((mean - mean.mean(axis=0)) ** 2).sum(axis=0)
        var_a = within * ((n - 1.0) / n) + ss * (n / (C - 1.0)) * (1.0 / n)
        var_b = ss / (C * D - 1.0) + within * ((n - 1.0) / n)
        return np.sqrt(var_a / within), np.sqrt(var_b / within)

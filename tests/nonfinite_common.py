"""Shared by tests/test_nonfinite_gpu.py: inputs on which energies and log-ratios are inf or NaN, and a classifier of every
transition that does not use the code under test.

The target is StandardNormal(dim): logp = -1/2 s, s = sum x_i^2 formed in the element type T, so logp is -inf exactly where
s overflows T, while the gradient -x stays finite.  With R = sqrt(largest finite value of T), starts lie at |x| = 0.5 R to 3 R
(s overflows from 1 R on), every seventh chain at N(0, 1) / 4 (ordinary accepts and rejects), and three chains have a NaN, +inf
and -inf coordinate.

The classifier works in numpy.longdouble (x87 extended: 64-bit mantissa, 15-bit exponent -- float64 itself overflows where
f64 does) from the host twin's previous row and the engine's noise: it forms the proposal, s of both ends (HMC: the kinetic
sums too) and calls a quantity `overflowed in T` when it exceeds T's largest finite value.  No row of the twin may lie
within 1 % of that edge -- a condition on the inputs, asserted -- and a proposal that does is left unclassified, so rounding
cannot move a transition between classes:

    escape    current energy +inf, proposed finite     ratio +inf   must accept
    stuck     both +inf                                ratio NaN    must reject
    fall      current finite, proposed +inf            ratio -inf   must reject
    accept / reject   both finite, by what the row did
"""
import numpy as np

LD = np.longdouble
EDGE = 0.01
SEED = 29
FIRST = (24, 4)  # n_collect, n_discard of the first run()
SECOND = 12  # n_collect of the continued run(); 40 transitions in all
N_TRANS = FIRST[0] + FIRST[1] + SECOND
N_GOOD = 130  # two waves and two lanes; with the three bad chains 133 = 8 groups of 16 and 5
BAD_AT = (5, 70, 132)  # where the NaN, +inf and -inf chains sit in the handle
CLASSES = ("escape", "stuck", "fall", "accept", "reject")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def tmax(dtype):
    return LD(np.finfo(dtype).max)


def insert_bad(good, bad_at=BAD_AT):
    """good [n, dim] -> (rows [n + 3, dim], isbad [n + 3]): chains with NaN, +inf, -inf in one coordinate at `bad_at`"""
    n, dim = good.shape
    rows = np.empty((n + len(bad_at), dim), dtype=good.dtype)
    isbad = np.zeros(n + len(bad_at), dtype=bool)
    isbad[list(bad_at)] = True
    rows[~isbad] = good
    for k, (c, v) in enumerate(zip(bad_at, (np.nan, np.inf, -np.inf))):
        rows[c] = np.linspace(-0.5, 0.5, dim).astype(good.dtype)
        rows[c, (k * 3 + 1) % dim] = v
    return rows, isbad


RADII = (0.0, 0.5, 1.15, 0.8, 1.3, 1.7, 3.0)  # of chain c % 7, in units of the edge R = sqrt(largest finite value); 0: N(0, 1) / 4


def edge_radius(dtype):
    return float(np.sqrt(tmax(dtype)))


def mh_std(dtype, dim):
    """proposal steps of about 0.6 R: from just outside the edge a good part of the proposals lands inside"""
    return 0.6 * edge_radius(dtype) / np.sqrt(dim)


def starts(O, dtype, dim, n_good=N_GOOD, bad_at=BAD_AT):
    """(rows [n_good + 3, dim], isbad): directions from init_with_seed, |x| = RADII[c % 7] * R * (1 +- 3 %)"""
    g = O.init_with_seed(n_good, dim, 7, np.float64)
    u = g / np.sqrt((g * g).sum(axis=1, keepdims=True))
    r = np.asarray(RADII)[np.arange(n_good) % len(RADII)] * (1.0 + 0.03 * np.cos(1.7 * np.arange(n_good)))
    x = u * (r * edge_radius(dtype))[:, None]
    x[r == 0.0] = 0.25 * g[r == 0.0]
    return insert_bad(x.astype(dtype), bad_at)


def stretches(isbad):
    """[(lo, hi)] of the runs of consecutive finite-start chains"""
    out, c, n = [], 0, len(isbad)
    while c < n:
        if isbad[c]:
            c += 1
            continue
        e = c
        while e < n and not isbad[e]:
            e += 1
        out.append((c, e))
        c = e
    return out


def ssq(x):
    with np.errstate(all="ignore"):
        return (x.astype(LD) ** 2).sum(axis=-1)


def quad(x, matrix=None):
    """x^T A x in long double (A = identity: the sum of squares): the sum whose overflow makes a Gaussian's logp -inf"""
    if matrix is None:
        return ssq(x)
    with np.errstate(all="ignore"):
        xl = x.astype(LD)
        return ((xl @ np.asarray(matrix).astype(LD)) * xl).sum(axis=-1)


def _classify(cur, prop, moved, dtype, what):
    """cur / prop: lists of the non-negative sums whose overflow makes the current / proposed energy +inf in T [C]"""
    mx = tmax(dtype)
    near = lambda q: np.isfinite(q) & (q > (1 - EDGE) * mx) & (q < (1 + EDGE) * mx)
    with np.errstate(all="ignore"):
        for q in cur:  # rows of the twin: none may lie at the edge
            assert not near(q).any(), (what, "a row within 1 % of the largest finite value", np.flatnonzero(near(q)))
        edge = np.any([near(q) for q in prop], axis=0)  # a proposal there is left unclassified (-1) and counts for nothing
        ci = np.any([q > mx for q in cur], axis=0)
        pi = np.any([q > mx for q in prop], axis=0)
    cls = np.where(ci & ~pi, 0, np.where(ci & pi, 1, np.where(~ci & pi, 2, np.where(moved, 3, 4))))
    cls[edge] = -1
    assert moved[cls == 0].all(), (what, "ratio +inf not accepted", np.flatnonzero((cls == 0) & ~moved))
    assert not moved[cls == 1].any(), (what, "ratio NaN accepted", np.flatnonzero((cls == 1) & moved))
    assert not moved[cls == 2].any(), (what, "ratio -inf accepted", np.flatnonzero((cls == 2) & moved))
    return cls


def count(cls):
    return {name: int((cls == k).sum()) for k, name in enumerate(CLASSES)}


def mh_classes(O, dtype, rows, isbad, std, seed=SEED, offset=0):
    """rows [C, T + 1, dim]: the start and every row of the twin.  -> class of every transition of the finite-start chains
    [C_good, T].  MH: x' = x + std z; the ratio is logp(x') - logp(x)."""
    C, T1, dim = rows.shape
    good = ~isbad
    out = np.empty((int(good.sum()), T1 - 1), dtype=np.int64)
    sd = LD(dtype(std))
    for t in range(T1 - 1):
        z, _ = O.engine_host_noise(seed, offset, t, C, dim, dtype, sampler="mh")
        prev = rows[good, t]
        with np.errstate(all="ignore"):
            prop = prev.astype(LD) + sd * z[good].astype(LD)
        moved = (bits(rows[good, t + 1]) != bits(prev)).any(axis=1)
        out[:, t] = _classify([ssq(prev)], [ssq(prop)], moved, dtype, ("mh", dtype.__name__, dim, t))
    return out


def hmc_classes(O, dtype, rows, isbad, eps, n_leapfrog, seed=SEED, offset=0, iter0=0, scale=None, matrix=None):
    """The same for HMC on StandardNormal (matrix = A: on GaussianND, logp = -1/2 x^T A x, gradient -A x): H = 1/2 p.p - logp; the current energy is +inf iff s(x) overflows (p.p of N(0, 1)
    momenta does not), the proposed one iff s(x') or p'.p' does.  eps, n_leapfrog: scalars or one per transition; scale: the
    diagonal metric's (step of coordinate i = eps * scale_i)."""
    C, T1, dim = rows.shape
    good = ~isbad
    out = np.empty((int(good.sum()), T1 - 1), dtype=np.int64)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (T1 - 1,))
    nl = np.broadcast_to(np.asarray(n_leapfrog), (T1 - 1,))
    sc = np.ones(dim, dtype=LD) if scale is None else np.asarray(scale, dtype=dtype).astype(LD)
    A = None if matrix is None else np.asarray(matrix).astype(dtype).astype(LD)
    ax = (lambda v: v) if A is None else (lambda v: v @ A)  # A is symmetric
    for t in range(T1 - 1):
        z, _ = O.engine_host_noise(seed, offset, iter0 + t, C, dim, dtype)
        prev = rows[good, t]
        e = LD(dtype(eps[t])) * sc
        with np.errstate(all="ignore"):
            x, p = prev.astype(LD), z[good].astype(LD)
            if nl[t] > 0:
                p = p - e / 2 * ax(x)
                for l in range(int(nl[t])):
                    x = x + e * p
                    p = p - (e / 2 if l + 1 == nl[t] else e) * ax(x)
        moved = (bits(rows[good, t + 1]) != bits(prev)).any(axis=1)
        out[:, t] = _classify([quad(prev, A)], [quad(x, A), ssq(p)], moved, dtype, ("hmc", dtype.__name__, dim, t))
    return out


def device_invariants(dtype, start, isbad, sample_rows, accept, what, matrix=None):
    """From the device's output alone.  sample_rows [C, T + 1, dim]: the start and EVERY row (a run without discard);
    accept [C]: its accept counts; matrix: A of a GaussianND (the sum that overflows is then x^T A x)."""
    good = ~isbad
    b = bits(sample_rows)
    moved = (b[:, 1:] != b[:, :-1]).any(axis=2)
    assert np.array_equal(moved.sum(axis=1), accept.astype(np.int64)), (what, "rows that changed != accept counts")
    assert np.isfinite(sample_rows[good]).all(), (what, "NaN or inf in a chain that started finite")
    assert (b[isbad] == bits(start)[isbad][:, None, :]).all() and (accept[isbad] == 0).all(), (what, "a bad chain moved")
    s = quad(sample_rows[good], None if matrix is None else np.asarray(matrix).astype(dtype))
    acc = moved[good]
    assert not (s[:, 1:][acc] > (1 + EDGE) * tmax(dtype)).any(), (what, "accepted a row whose log-density overflows")

"""HMC with one chain per workgroup (csrc/mm_wide.hip, kernel variant 8) at every compiled instantiation and edge dimension.

The kernel is compiled for K = 4, 8, 16, 32 coordinates per thread in f32 and f64.  Coordinate for coordinate a transition
is the arithmetic of the run-time-D path (csrc/mm_generic.h); only the order of the three reduced sums (kinetic energy
before and after, log-density of the end point) differs, and those feed nothing but the accept decision.  So wherever the
accept decisions agree, samples, final states and accept counts equal the host build of mm_generic.h
(O.engine_host_run("hmc_generic", ...)) BIT FOR BIT.  This file holds

  1. `_transition`: one HMC transition (leapfrog with merged half-kicks, hmc.rs:304-431) in plain numpy on the whole
     [chains, D] array, for RosenbrockND, IsotropicGaussian(sigma) and StandardNormal.  In float64 with long-double sums it is
     the truth for both dtypes; in the case's dtype with strictly sequential sums (the host twin's order) it measures how far
     rounding moves the energy difference.  It is fed the engine's own noise (O.engine_host_noise, pinned bit for bit
     against the device in tests/test_generic_dim.py), cast up.
  2. a CPU test that every (chain, transition) of every case has an accept margin
         m = (K0 / 2 - lp0) - (K1 / 2 - lp1) - ln u,      |m| > tau,
     recomputed in float64 from the twin's previous row, and that the twin's decision is `m >= 0`; tau = 4 x the largest
     |dH_seq - dH_f64| of the case.  With such inputs the wide kernel and the twin cannot legitimately disagree, so
  3. the GPU tests compare every chain of every case bit for bit, with no exclusions, and the first transition's proposal
     against the float64 reference within  c * L * eps_machine * max(1, |x|, eps |grad|)  (|x|, |grad|: the largest over the
     chain's trajectory); c is stated below per dtype and the CPU test holds the twin to a quarter of it.

Measured on the CPU, per dtype, target and D (the largest over the chains and transitions of the cases there; tau = 4 x the
first column, and beside it the smallest |m| of those cases; `c/4`: the twin's largest deviation from the float64 proposal
in units of L eps_machine max(1, |x|, eps |grad|); the overflow case has no finite entry).  c = 4 x the largest c/4 of a
dtype, rounded up: 1.2 in float32 (4 x 0.28), 1.5 in float64 (4 x 0.36).  The test takes tau case by case; the row of
D = 1000 pools L = 0, 1, 2, 12, and its smallest |m| is the L = 0 case's, where the proposal is the state and tau is 0.

    dtype    target                 D   max |dH_seq - dH_f64|         tau   smallest |m|    c/4
    float32  RosenbrockND           4                6.57e-06    2.63e-05         0.0482   0.02
    float32  RosenbrockND           5                1.88e-06    7.52e-06         0.0193   0.02
    float32  RosenbrockND           7                8.06e-06    3.23e-05          0.045   0.01
    float32  RosenbrockND         128                6.92e-02    2.77e-01           12.1   0.02
    float32  RosenbrockND         255                1.84e-03    7.38e-03         0.0379   0.02
    float32  RosenbrockND         256                1.39e-03    5.55e-03          0.091   0.02
    float32  RosenbrockND         258                2.10e-03    8.39e-03         0.0647   0.02
    float32  RosenbrockND         259                1.84e-03    7.37e-03         0.0653   0.02
    float32  RosenbrockND        1000                3.51e-02    1.40e-01         0.0465   0.06
    float32  RosenbrockND        4096                1.72e-01    6.87e-01           16.7   0.05
    float32  RosenbrockND        4097                1.46e-01    5.85e-01           17.6   0.04
    float32  RosenbrockND        8192                6.40e-01    2.56e+00             23   0.06
    float32  RosenbrockND        8193                3.28e-01    1.31e+00           23.3   0.06
    float32  RosenbrockND       16384                1.11e+00    4.46e+00           25.7   0.08
    float32  RosenbrockND       16385                1.10e+00    4.38e+00           24.8   0.09
    float32  RosenbrockND       32768                2.91e+00    1.16e+01           34.7   0.08
    float32  IsotropicGaussian    259                1.65e-04    6.59e-04          0.377   0.14
    float32  StandardNormal      4096                1.20e-02    4.81e-02          0.756   0.18
    float32  IsotropicGaussian   4097                7.44e-03    2.98e-02          0.771   0.20
    float32  StandardNormal      8192                2.41e-02    9.64e-02           1.64   0.26
    float32  StandardNormal      8193                2.80e-02    1.12e-01            1.2   0.20
    float32  IsotropicGaussian  16384                5.41e-02    2.16e-01           2.42   0.23
    float32  StandardNormal     16385                5.50e-02    2.20e-01           1.79   0.22
    float32  IsotropicGaussian  32768                9.84e-02    3.93e-01           4.65   0.28
    float64  RosenbrockND           4                7.11e-15    2.84e-14        0.00709   0.01
    float64  RosenbrockND           5                1.78e-15    7.11e-15          0.005   0.01
    float64  RosenbrockND           7                2.84e-14    1.14e-13        0.00603   0.02
    float64  RosenbrockND         128                3.18e-12    1.27e-11       0.000242   0.08
    float64  RosenbrockND         255                5.46e-12    2.18e-11          0.136   0.03
    float64  RosenbrockND         256                6.37e-12    2.55e-11          0.114   0.02
    float64  RosenbrockND         258                5.00e-12    2.00e-11          0.106   0.02
    float64  RosenbrockND         259                5.46e-12    2.18e-11          0.119   0.02
    float64  RosenbrockND        1000                3.27e-11    1.31e-10          0.016   0.12
    float64  RosenbrockND        4096                3.64e-10    1.46e-09         0.0461   0.04
    float64  RosenbrockND        4097                3.78e-10    1.51e-09          0.157   0.03
    float64  RosenbrockND        8192                5.38e-10    2.15e-09          0.137   0.04
    float64  RosenbrockND        8193                1.08e-09    4.31e-09          0.133   0.04
    float64  RosenbrockND       16384                2.97e-09    1.19e-08          0.106   0.04
    float64  RosenbrockND       16385                3.00e-09    1.20e-08          0.101   0.04
    float64  RosenbrockND       32768                7.22e-09    2.89e-08         0.0508   0.08
    float64  IsotropicGaussian    259                3.41e-13    1.36e-12          0.161   0.27
    float64  StandardNormal      4096                1.82e-11    7.28e-11         0.0946   0.28
    float64  IsotropicGaussian   4097                1.27e-11    5.09e-11          0.219   0.33
    float64  StandardNormal      8192                4.00e-11    1.60e-10           0.12   0.36
    float64  StandardNormal      8193                7.46e-11    2.98e-10          0.169   0.25
    float64  IsotropicGaussian  16384                1.46e-10    5.82e-10         0.0775   0.14
    float64  StandardNormal     16385                1.67e-10    6.69e-10         0.0557   0.29
    float64  IsotropicGaussian  32768                6.55e-10    2.62e-09        0.00201   0.26
"""
import functools

import numpy as np
import pytest

ROS, ISO, STD = "RosenbrockND", "IsotropicGaussian", "StandardNormal"
SIGMA = 1.7
N_COLLECT, N_DISCARD = 3, 1
N_TRANS = N_COLLECT + N_DISCARD
# the stated multiple c of the proposal tolerance, per dtype: 4 x the largest `c/4` of the table, rounded up
PROPOSAL_C = {np.float32: 1.2, np.float64: 1.5}


class Case:
    """One row of the matrix.  `f32` overrides eps / scale / pattern for float32: at a large D the rounding of a float32
    energy (tau) reaches the size of an ordinary margin, so the float32 inputs use hotter or colder starts and longer steps,
    which move every margin away from zero; the float64 inputs keep starts whose decisions go both ways within a chain."""

    def __init__(self, kind, dim, L=3, chains=3, eps=None, scale=None, seed=11, offset=0, force=False, overflow=False, pattern=None,
                 f32=None):
        self.kind, self.dim, self.L, self.chains, self.offset, self.force, self.overflow = kind, dim, L, chains, offset, force, overflow
        self.seed = seed
        # start = init_with_seed * scale * pattern[chain % len]: RosenbrockND from 0.3 N(0, 1) descends (accepts), from a
        # tenth of that it sits near its ridge and decides either way; a Gaussian started hotter than its target accepts,
        # colder rejects (the leapfrog's shadow energy), at the target's own scale either
        v = {"eps": eps, "scale": scale if scale is not None else {ROS: 0.3, ISO: SIGMA, STD: 1.0}[kind],
             "pattern": pattern if pattern is not None else ((1.0, 0.1) if kind == ROS else (1.3, 1.0, 0.75))}
        self._v = {np.float64: v, np.float32: dict(v, **(f32 or {}))}
        self.id = f"{kind}-D{dim}-L{L}-C{chains}" + ("-overflow" if overflow else "")

    def step(self, dtype):
        return self._v[dtype]["eps"]

    def start(self, O, dtype):
        v = self._v[dtype]
        rows = np.resize(np.asarray(v["pattern"], dtype=dtype), self.chains)[:, None] * dtype(v["scale"])
        return O.init_with_seed(self.chains, self.dim, 5, dtype) * rows

    @property
    def K(self):
        k = 4
        while (self.dim + k - 1) // k > 1024:
            k *= 2
        return k


def _build_cases():
    c = []
    hot = {"pattern": (1.0,)}
    # RosenbrockND on every row of the matrix; the step shrinks with the dimension, as the energy error grows with it
    for d in (4, 5, 7):
        c.append(Case(ROS, d, chains=2, eps=0.03, force=True))  # one active thread, partially filled K
    for d in (255, 256, 258, 259):
        c.append(Case(ROS, d, eps=0.012))  # D mod 4 = 3, 0, 2, 3 around the wave-0 | wave-1 halo (coordinates 255 | 256)
    c.append(Case(ROS, 4096, chains=4, eps=0.006, f32=hot))  # 1024 threads, 16 waves, no padding
    c.append(Case(ROS, 4097, eps=0.006, f32=hot))  # first K = 8 shape
    c.append(Case(ROS, 8192, eps=0.005, f32=hot))  # full block at K = 8
    c.append(Case(ROS, 8193, eps=0.005, f32=hot))  # first K = 16 shape
    c.append(Case(ROS, 16384, eps=0.004, f32=hot))
    c.append(Case(ROS, 16385, eps=0.004, f32=hot))  # first K = 32 shape
    c.append(Case(ROS, 32768, chains=4, eps=0.0035, f32=hot))  # MM_WIDE_MAX_DIM
    for L in (0, 1, 2, 12):
        c.append(Case(ROS, 1000, L=L, eps=0.008, f32=hot))  # lpn = lp; the only step is also the last (kk = h); ...
    # grid indexing, c * D offsets, a chain index above 2^32
    c.append(Case(ROS, 128, chains=1025, eps=0.015, offset=(1 << 33) + 5, force=True, f32={"pattern": (1.0,), "scale": 1.0, "eps": 0.006}))
    c.append(Case(ROS, 1000, eps=0.5, scale=0.3 * 50, overflow=True))  # inf / NaN trajectories: every proposal rejected
    # the separable targets (no halo): one row per K
    sep32 = (1.3, 0.75, 1.15)
    for d in (259, 4097, 16384, 32768):
        c.append(Case(ISO, d, eps=1.6 * SIGMA * d ** -0.25, f32={"pattern": sep32, "eps": 2.2 * SIGMA * d ** -0.25}))
    for d in (4096, 8192, 8193, 16385):
        c.append(Case(STD, d, eps=1.6 * d ** -0.25, f32={"pattern": sep32, "eps": 2.2 * d ** -0.25}))
    return c


CASES = _build_cases()
DTYPES = [np.float32, np.float64]


def _sum(v, seq):
    """Row sums of v [C, n]: strictly sequential in v's own dtype, or in long double."""
    if seq:
        return np.add.accumulate(v, axis=1, dtype=v.dtype)[:, -1] if v.shape[1] else np.zeros(v.shape[0], v.dtype)
    return v.astype(np.longdouble).sum(axis=1).astype(np.float64)


def _logp_grad(kind, x, inv_var, seq):
    dt = x.dtype.type
    if kind == ROS:
        a, b = x[:, :-1], x[:, 1:]
        t = b - a * a
        u = dt(1) - a
        g = np.zeros_like(x)
        g[:, :-1] = dt(400) * a * t + dt(2) * u
        g[:, 1:] -= dt(200) * t
        terms = np.stack([dt(100) * t * t, u * u], axis=2).reshape(x.shape[0], -1)  # the engine adds them in this order
        return -_sum(terms, seq), g
    iv = dt(inv_var)
    return dt(-0.5) * (_sum(x * x, seq) * iv), -(x * iv)


def _transition(kind, x0, z, eps, L, sigma=SIGMA, dtype=np.float64, seq=False):
    """One HMC transition of every row of x0 [C, D] with momentum z: (proposal, dH = H0 - H1, largest |x|, largest |grad|).
    Accept iff dH >= ln u.  dtype float64, seq False: the reference.  dtype the engine's, seq True: the twin's order of sums."""
    with np.errstate(all="ignore"):
        x, p = x0.astype(dtype), z.astype(dtype)
        eps = dtype(eps)
        h = eps * dtype(0.5)
        inv_var = 1.0 / (float(dtype(sigma)) ** 2) if kind == ISO else 1.0
        lp0, g = _logp_grad(kind, x, inv_var, seq)
        k0 = _sum(p * p, seq)
        xmax, gmax = np.abs(x).max(axis=1), np.abs(g).max(axis=1)
        lp1 = lp0
        if L > 0:
            p = p + h * g
            for l in range(L):
                x = x + eps * p
                lp1, g = _logp_grad(kind, x, inv_var, seq)
                xmax, gmax = np.maximum(xmax, np.abs(x).max(axis=1)), np.maximum(gmax, np.abs(g).max(axis=1))
                p = p + (h if l + 1 == L else eps) * g
        k1 = _sum(p * p, seq)
        dH = (k0 * dtype(0.5) - lp0) - (k1 * dtype(0.5) - lp1)
        return x, dH.astype(np.float64), xmax.astype(np.float64), gmax.astype(np.float64)


def _okind(O, kind):
    return {ROS: (O.ROSENBROCK_ND, []), ISO: (O.ISOTROPIC_GAUSSIAN, [SIGMA]), STD: (O.STANDARD_NORMAL, [])}[kind]


def _ln_u(O, u, dtype):
    return (O.engine_host_lnu_f32(u) if dtype == np.float32 else O.engine_host_log_f64(u)).astype(np.float64)


class Analysis:
    """Everything the CPU says about one (case, dtype): the twin's run, the float64 margins, tau, the proposal deviation."""


@functools.lru_cache(maxsize=None)
def _analyse(O, case, dtype):
    a = Analysis()
    kind, params = _okind(O, case.kind)
    eps, seed = case.step(dtype), case.seed
    a.init = case.start(O, dtype)
    run = lambda nc, nd: O.engine_host_run("hmc_generic", kind, case.dim, params, a.init, eps, nc, nd, seed=seed,
                                           chain_offset=case.offset, n_leapfrog=case.L, dtype=dtype)
    a.out, a.state, a.acc = run(N_COLLECT, N_DISCARD)
    rows, st4, acc4 = run(N_TRANS, 0)  # every row, the discarded one included
    assert np.array_equal(rows[:, N_DISCARD:], a.out) and np.array_equal(st4, a.state) and np.array_equal(acc4, a.acc)
    a.rows = rows
    eps_t = float(dtype(eps))  # the step the engine uses is an input: the reference takes it as rounded to the dtype
    mach = float(np.finfo(dtype).eps)
    a.m = np.empty((case.chains, N_TRANS))
    a.m_seq = np.empty((case.chains, N_TRANS))
    a.dh_err = np.zeros((case.chains, N_TRANS))
    a.accepted = np.empty((case.chains, N_TRANS), dtype=bool)
    prev = a.init
    for t in range(N_TRANS):
        z, u = O.engine_host_noise(seed, case.offset, t, case.chains, case.dim, dtype)
        ln_u = _ln_u(O, u, dtype)
        prop, dh, xmax, gmax = _transition(case.kind, prev, z, eps_t, case.L)
        _, dh_seq, _, _ = _transition(case.kind, prev, z, eps_t, case.L, dtype=dtype, seq=True)
        a.m[:, t] = dh - ln_u
        a.m_seq[:, t] = dh_seq - ln_u
        with np.errstate(all="ignore"):
            a.dh_err[:, t] = np.abs(dh_seq - dh)
        a.accepted[:, t] = (rows[:, t] != prev).any(axis=1)
        if t == 0:
            a.proposal = prop
            a.tol_unit = max(case.L, 1) * mach * np.maximum(1.0, np.maximum(xmax, eps_t * gmax))  # per chain
        prev = rows[:, t]
    fin = np.isfinite(a.dh_err)
    a.dh_err_max = float(a.dh_err[fin].max()) if fin.any() else 0.0
    a.tau = 4.0 * a.dh_err_max
    return a


def _first_diff(got, want):
    """Where two arrays first differ, for the assertion message."""
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(bad):
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at (chain, transition, coordinate) = {i}: {got[i]!r} != {want[i]!r}"


# ------------------------------------------------------------------ CPU: the inputs are margin-safe


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_matrix_inputs_are_margin_safe(O, dtype):
    """Every (chain, transition) of every case: |m| > tau in float64 from the twin's previous row, and the twin's decision
    is m >= 0; no chain is excluded.  The twin's first proposal lies within a quarter of the stated proposal tolerance of
    the float64 reference.  Over the cases together both branches of the accept are taken."""
    total = accepted = 0
    for case in CASES:
        a = _analyse(O, case, dtype)
        name = f"{case.id} {dtype.__name__}"
        fin = np.isfinite(a.m_seq)
        if case.overflow:
            # non-finite in the engine's dtype: safe when the float64 reference is non-finite or below -tau as well
            assert not (np.isfinite(a.m) & (a.m >= -a.tau)).any(), (name, a.m, a.tau)
            assert not a.accepted.any() and a.acc.sum() == 0 and np.array_equal(a.state, a.init), name
            if dtype == np.float32:
                assert not fin.any(), (name, a.m_seq)
        else:
            assert fin.all() and np.isfinite(a.m).all(), name
            assert (np.abs(a.m) > a.tau).all(), (name, "smallest |m|", np.abs(a.m).min(), "tau", a.tau)
            if case.L == 0:  # the proposal is the state: always accepted (ln u <= 0), and no row changes
                assert (a.m >= 0).all() and (a.acc == N_TRANS).all() and not a.accepted.any(), name
            else:
                assert np.array_equal(a.accepted, a.m >= 0), (name, a.m)
                assert np.array_equal(a.accepted.sum(axis=1), a.acc.astype(np.int64)), name
                assert a.accepted[:, 0].any(), (name, "no chain accepts its first transition: nothing to compare the proposal with")
                ok = a.accepted[:, 0]
                dev = np.abs(a.rows[ok, 0].astype(np.float64) - a.proposal[ok]).max(axis=1) / a.tol_unit[ok]
                assert dev.max() <= PROPOSAL_C[dtype] / 4, (name, dev.max())
        total += N_TRANS * case.chains
        accepted += int(a.acc.sum())
    assert 0 < accepted < total, (accepted, total)


def test_every_instantiation_is_in_the_matrix():
    """K = 4, 8, 16, 32 each appear with RosenbrockND and with a separable target; the K switches sit where the launch puts them."""
    assert {c.K for c in CASES if c.kind == ROS} == {4, 8, 16, 32}
    assert {c.K for c in CASES if c.kind != ROS} == {4, 8, 16, 32}
    assert [Case(ROS, d).K for d in (4, 4096, 4097, 8192, 8193, 16384, 16385, 32768)] == [4, 4, 8, 8, 16, 16, 32, 32]


# ------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def M():
    import mini_mcmc_amd
    from mini_mcmc_amd import core, distributions, hmc

    mini_mcmc_amd.lib()

    class NS:
        pass

    ns = NS()
    ns.core, ns.dist, ns.hmc = core, distributions, hmc
    return ns


def _handle(M, case, dtype, init):
    tgt = {ROS: lambda: M.dist.RosenbrockND(case.dim), ISO: lambda: M.dist.IsotropicGaussian(SIGMA, case.dim),
           STD: lambda: M.dist.StandardNormal(case.dim)}[case.kind]()
    s = M.hmc.HMC(tgt, init, case.step(dtype), case.L).set_seed(case.seed)
    if case.offset:
        s.set_chain_offset(case.offset)
    if case.force:
        s.set_kernel_variant(8)
    assert s.kernel_variant == 8, case.id  # by default wherever D >= 128 and fewer than 1024 chains
    return s


_gpu_accepts = {}


def _gpu_case(M, O, case, dtype):
    a = _analyse(O, case, dtype)
    name = f"{case.id} {dtype.__name__} K={case.K}"
    s = _handle(M, case, dtype, a.init)
    out = s.run(N_COLLECT, N_DISCARD)
    acc = s.accept_counts.copy()
    assert np.array_equal(out, a.out, equal_nan=True), (name, "samples", _first_diff(out, a.out))
    assert np.array_equal(s.state(), a.state, equal_nan=True), (name, "state", _first_diff(s.state()[:, None], a.state[:, None]))
    assert np.array_equal(acc, a.acc), (name, "accept counts", acc, a.acc)
    # a continued handle: the stream is keyed by (chain, iteration), the state carries over
    c = _handle(M, case, dtype, a.init)
    first = c.run(1, N_DISCARD)
    acc_c = c.accept_counts.copy()
    parts = np.concatenate([first, c.run(N_COLLECT - 1, 0)], axis=1)
    assert np.array_equal(parts, out, equal_nan=True), (name, "continued", _first_diff(parts, out))
    assert np.array_equal(c.state(), a.state, equal_nan=True) and np.array_equal(acc_c + c.accept_counts, acc), name
    # the first transition's proposal against float64, wherever it was accepted (the row then IS the proposal)
    p = _handle(M, case, dtype, a.init)
    row = p.run(1, 0)[:, 0]
    assert np.array_equal(row, a.rows[:, 0], equal_nan=True), (name, "first row", _first_diff(row[:, None], a.rows[:, :1]))
    ok = a.accepted[:, 0]
    if case.overflow:
        assert acc.sum() == 0 and np.array_equal(row, a.init) and np.array_equal(s.state(), a.init), name
    elif case.L > 0:
        assert ok.any(), name
        err = np.abs(row[ok].astype(np.float64) - a.proposal[ok])
        tol = PROPOSAL_C[dtype] * a.tol_unit[ok]
        assert (err <= tol[:, None]).all(), (name, "proposal vs float64: largest error / tolerance", (err / tol[:, None]).max())
    else:
        assert np.array_equal(row, a.init), name
    _gpu_accepts[(case.id, dtype)] = int(acc.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_wide_hmc_bit_equal_to_host_twin(M, O, case, dtype):
    """Variant 8 against the host build of mm_generic.h: samples, final state and accept counts of every chain bit for
    bit; a continued handle equals the single run; the first proposal within the stated tolerance of the float64 reference."""
    _gpu_case(M, O, case, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_wide_hmc_matrix_takes_both_accept_branches(M, O, dtype):
    """Over the cases of a dtype together, on the device: some transitions accepted, some rejected."""
    for case in CASES:
        if (case.id, dtype) not in _gpu_accepts:
            _gpu_case(M, O, case, dtype)
    accepted = sum(_gpu_accepts[(case.id, dtype)] for case in CASES)
    total = sum(N_TRANS * case.chains for case in CASES)
    assert 0 < accepted < total, (accepted, total)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_wide_hmc_refuses_what_it_is_not_built_for(M, dtype):
    """D = 32769 (one past MM_WIDE_MAX_DIM) and D = 3 (below the minimum of 4) neither select variant 8 nor accept it."""
    for dim in (32769, 3):
        s = M.hmc.HMC(M.dist.RosenbrockND(dim), M.core.init_with_seed(2, dim, 5, dtype) * dtype(0.3), 0.002, 3).set_seed(1)
        assert s.kernel_variant != 8, dim
        with pytest.raises(Exception):
            s.set_kernel_variant(8)
        assert s.kernel_variant != 8, dim

"""Forward-mode automatic differentiation (csrc/mm_autodiff.h) on the host: tests/cpp/autodiff_host.cpp, a stand-alone
program built with the compiler and flags of the host twin (oracle/Makefile: engine_host.cpp), evaluates mm_ad_logp_grad on
log-density bodies written once over a scalar type (tests/cpp/autodiff_cases/) -- RosenbrockND at dims 2, 3, 8, 9, 17, 32
(one pass, two, three, four), the banana of test_user_target.py, one body per overload -- in f32 and f64 on a fixed grid of
257 points with |x| <= 2.  The device must reproduce that file bit for bit (tests/test_autodiff_gpu.py).

Checked here, without a GPU:
 (a) the value returned next to the gradient is bit-equal to logp<T>;
 (b) in f64, on the grid's points that are multiples of 1/8, where every operation of the polynomial densities is exact,
     the gradient equals the hand-written analytic gradient bit for bit (mm_targets.h RosenbrockND, the banana of
     test_user_target.py);
 (c) everywhere, f32 and f64: |g - g_ref| <= k u sum|summands|, for the derived and the hand-written gradients alike.  g_ref is
     the numpy gradient evaluated in extended precision (np.longdouble: 64-bit significand, unit roundoff 2^-64), because a
     float64 reference carries as much rounding as the f64 gradients under test; its own error, a few 2^-64 sum|summands|,
     is 2^-11 of the f64 bound's unit and nothing is added for it.

The bound of (c).  u = 2^-24 (f32) / 2^-53 (f64) is the unit roundoff; sum|summands| is the gradient component expanded
into the terms its formula adds (each a product / quotient of positive-condition factors), absolute values summed, in
float64; k is the number of ROUNDED operations on the longest path from an input to the result through the formulas of
mm_autodiff.h, counted with the numbers printed there after each formula (an operation whose exact result is representable
-- a product with a seed 0 or 1, a sum with an exact 0 -- rounds nothing and is not counted; the scaling by -1/2, 2 and
the sign are exact).  Every term then carries a factor (1 + d)^j, |d| <= u, j <= k.  The counts:

  RosenbrockND, g_j = 400 x_j t_j + 2 (1 - x_j) - 200 t_(j-1), t_i = x_(i+1) - x_i^2, expanded into the six monomials
      200 |x_j| + 200 x_(j-1)^2 + 400 |x_j x_(j+1)| + 400 |x_j|^3 + 2 + 2 |x_j|:
    autodiff, k = 7: iteration j-1 leaves fl(100 t + fl(100 t)) in the tangent (t: 1, 100 t: 2, the sum: 3); iteration j
      passes it through both nested mm_fma of acc = mm_fma(100 t, t, acc) (4, 5) and of acc = mm_fma(u, u, acc) (6, 7); the
      terms that enter in iteration j are shorter (fl(-200 x_j) t: 3, +2 nested; u: 1, +2); later iterations add exact zeros.
    hand-written (mm_targets.h), k = 4: t (1), 400 x_j (1), mm_fma(400 x_j, t, 2 u) (1), mm_fma(-200, t_(j-1), .) (1).
  banana, g_0 = -x_0 / s^2 + 2 b x_0 (x_1 - b x_0^2) -> |x_0| / s^2 + 2 |b x_0 x_1| + 2 b^2 |x_0|^3;  g_1 = -(x_1 - b x_0^2):
    autodiff, k = 8: r = x_1 - (b x_0) x_0 has value path 3 and tangent path 2; (r r)' = mm_fma(r', r, r r') is
      2 + 3 + 1 + 1 = 7; the sum with (x_0^2 / s^2)' one more.
    hand-written, k = 7: r (3), 2 b (1), . x_0 (1), . r (1), sum (1).
  div  (g_0 = -1 / (1 + x_1^2), g_1 = 2 x_0 x_1 / (1 + x_1^2)^2; one term each), k = 9: q = x_0 / den (den: 2, q: 3);
      q' = mm_fma(-q, den', x_0') / den = 3 + 2 + 1, then den (2) and the division (1).
  log  (g_0 = -2 x_0 / (1 + x_0^2), g_1 = -x_1), k = 7: (1 + x_0^2)' 3, value 2, the division 1, the final difference 1.
  exp  (g_0 = -exp(x_0 / 2) / 2, g_1 = -2 x_1), k = 2: x_0 / 2, its tangent 1/2 and the product (1/2) e are scalings by a power
      of two and the difference subtracts an exact 0 -- all exact; what is left is mm_expT itself, whose error mm_math.h
      states as about 1 ulp = 2 u.  g_1: mm_fma(1, x_1, x_1) = 2 x_1 is exact.
  sqrt (g_i = -x_i / sqrt(1 + x_0^2 + x_1^2)), k = 9: the radicand's value 3 and tangent 4, the root 1, the division 1.
  abs  (g = -sign, -2 sign; sign(0) = +1: the right-hand derivative) and
  branch (g_0 = (x_0 < 0 ? -2 x_0 : -4 x_0) + (x_0 < 1/2 ? 1 : 0) -> both terms; g_1 = -(x_1^2 > x_1 ? 2 x_1 : 1)):
      k = 2 and 5 (tangent of x_0^2: 2, the scaling 1, two sums); in fact every operation is exact.
None of the counts was adjusted after seeing the program's output."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import autodiff_common as A

ROOT = A.ROOT
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
ROS_DIMS = (2, 3, 8, 9, 17, 32)


def _rosenbrock(x):
    n, d = x.shape
    t = x[:, 1:] - x[:, :-1] ** 2
    g = np.zeros_like(x)
    s = np.zeros_like(x)
    g[:, :-1] += 400 * x[:, :-1] * t + 2 * (1 - x[:, :-1])
    s[:, :-1] += 400 * np.abs(x[:, :-1] * x[:, 1:]) + 400 * np.abs(x[:, :-1]) ** 3 + 2 + 2 * np.abs(x[:, :-1])
    g[:, 1:] += -200 * t
    s[:, 1:] += 200 * np.abs(x[:, 1:]) + 200 * x[:, :-1] ** 2
    return g, s


def _banana(x):
    sd, b = A.BANANA_PARAMS
    x0, x1 = x[:, 0], x[:, 1]
    r = x1 - b * x0 ** 2
    g = np.stack([-x0 / sd ** 2 + 2 * b * x0 * r, -r], axis=1)
    s = np.stack([np.abs(x0) / sd ** 2 + 2 * np.abs(b * x0 * x1) + 2 * b * b * np.abs(x0) ** 3, np.abs(x1) + b * x0 ** 2], axis=1)
    return g, s


def _div(x):
    den = 1 + x[:, 1] ** 2
    g = np.stack([-1 / den, 2 * x[:, 0] * x[:, 1] / den ** 2], axis=1)
    return g, np.abs(g)


def _log(x):
    g = np.stack([-2 * x[:, 0] / (1 + x[:, 0] ** 2), -x[:, 1]], axis=1)
    return g, np.abs(g)


def _exp(x):
    g = np.stack([-0.5 * np.exp(0.5 * x[:, 0]), -2 * x[:, 1]], axis=1)
    return g, np.abs(g)


def _sqrt(x):
    g = -x / np.sqrt(1 + x[:, 0] ** 2 + x[:, 1] ** 2)[:, None]
    return g, np.abs(g)


def _abs(x):
    sign = np.where(x < 0, -1.0, 1.0).astype(x.dtype)
    g = np.stack([-sign[:, 0], -2 * sign[:, 1]], axis=1)
    return g, np.abs(g)


def _branch(x):
    x0, x1 = x[:, 0], x[:, 1]
    a, n = np.where(x0 < 0, -2 * x0, -4 * x0), np.where(x0 < 0.5, 1.0, 0.0)
    g = np.stack([a + n, -np.where(x1 * x1 > x1, 2 * x1, 1.0)], axis=1)
    return g, np.stack([np.abs(a) + n, np.abs(g[:, 1])], axis=1)


# case -> (numpy gradient and sum|summands|, k of the autodiff gradient, k of the hand-written one or None)
CASES = {f"rosenbrock{d}": (_rosenbrock, 7, 4) for d in ROS_DIMS}
CASES.update({"banana": (_banana, 8, 7), "div": (_div, 9, None), "log": (_log, 7, None), "exp": (_exp, 2, None),
              "sqrt": (_sqrt, 9, None), "abs": (_abs, 2, None), "branch": (_branch, 5, None)})


def test_the_program_covers_every_case_in_both_types():
    res = A.host_results()
    assert set(res) == {(c, t) for c in CASES for t in ("f32", "f64")}
    for (case, ty), r in res.items():
        assert r["x"].shape[0] == 257 and np.abs(r["x"]).max() <= 2.0
        assert np.array_equal(r["x"].astype(np.float64), res[(case, "f64")]["x"])  # the same points, exact in f32
        assert ("grad_hand" in r) == bool(CASES[case][2])


@pytest.mark.parametrize("ty", ["f32", "f64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_value_next_to_the_gradient_is_logp_bit_for_bit(case, ty):
    r = A.host_results()[(case, ty)]
    assert np.array_equal(A.bits(r["value"]), A.bits(r["value_plain"]))
    if "value_hand" in r and case.startswith("rosenbrock"):  # the restatement of the built-in density: the same operations
        assert np.array_equal(A.bits(r["value"]), A.bits(r["value_hand"]))


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c][2]])
def test_f64_gradient_equals_the_analytic_one_where_the_arithmetic_is_exact(case):
    r = A.host_results()[(case, "f64")]
    exact = np.all(r["x"] * 8 == np.rint(r["x"] * 8), axis=1)
    assert exact.sum() >= 129
    g, h = r["grad"][exact], r["grad_hand"][exact]
    assert np.array_equal(A.bits(g), A.bits(h))  # bit for bit, the sign of a zero included
    if case.startswith("rosenbrock"):  # float64 holds every intermediate of these points: numpy's gradient is exact too
        assert np.array_equal(g, CASES[case][0](r["x"][exact])[0])
    # (the banana divides by s^2 = 2.25: one correctly rounded quotient, the same in both gradients)


@pytest.mark.parametrize("ty", ["f32", "f64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_gradient_is_within_the_forward_error_bound_of_an_extended_precision_gradient(case, ty):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not the 80-bit extended type here"
    r = A.host_results()[(case, ty)]
    ref_fn, k_ad, k_hand = CASES[case]
    ref, _ = ref_fn(r["x"].astype(np.longdouble))
    _, summands = ref_fn(r["x"].astype(np.float64))  # sum|summands| in float64
    assert ref.dtype == np.longdouble and summands.dtype == np.float64
    for what, k in (("grad", k_ad), ("grad_hand", k_hand)):
        if k is None:
            continue
        err = np.abs(r[what].astype(np.longdouble) - ref)
        tol = (k * U[ty]) * summands.astype(np.longdouble)
        worst = np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)))
        print(f"{case} {ty} {what}: k = {k}, worst error / bound = {float(worst):.3f}")
        assert np.all(err <= tol), (case, ty, what, float(worst))


def test_host_program_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    exe = A.build_host(str(tmp_path), sanitize=True)
    san = A.run_host(exe, str(tmp_path))  # asserts exit status 0 (-fno-sanitize-recover: any report aborts)
    ref = A.host_results()
    for key, r in ref.items():
        for name, arr in r.items():
            assert np.array_equal(A.bits(arr), A.bits(san[key][name])), (key, name)


@pytest.mark.parametrize("dim", [3, 8])
def test_batch_gradient_kernel_uses_no_scratch_memory(dim):
    """Offline code generation (tools/autodiff_codegen.py: `hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off`, the
    RosenbrockND body, a stand-alone batch kernel): the dual numbers stay in registers -- .private_segment_fixed_size of the
    code object's metadata note is 0 in f32 and f64.  Register counts are recorded in DESIGN.md 5.11, not asserted."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import autodiff_codegen

    if autodiff_codegen.tools() is None:
        # a machine without ROCm cannot build the library either; where ROCm is installed the check must run
        assert not os.path.isdir("/opt/rocm"), "ROCm is installed but hipcc or llvm-readelf was not found"
        pytest.skip("no ROCm installation: neither hipcc nor llvm-readelf")
    md = autodiff_codegen.kernel_metadata(dim)
    assert set(md) == {"ad_logp_grad_f32", "ad_logp_grad_f64"}
    for name, fields in md.items():
        print(dim, name, fields)
        assert fields[".private_segment_fixed_size"] == 0, (dim, name, fields)


def test_register_logp_source_status_codes_without_a_device():
    import torch

    import mini_mcmc_amd
    from mini_mcmc_amd import _lib as L

    lib = mini_mcmc_amd.lib()
    src, _ = A.case_source("banana")
    kind = C.c_int()
    reg = lib.mmcmc_target_register_logp_source
    assert reg(None, 2, src.encode(), C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert reg(b"b", 2, None, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert reg(b"b", 2, src.encode(), None, None, 0) == L.ERR_INVALID_ARG
    for dim in (0, -1, 33):
        assert reg(b"b", dim, src.encode(), C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert lib.mmcmc_version() == 102
    if not torch.cuda.is_available():
        log = C.create_string_buffer(256)
        assert reg(b"b", 2, src.encode(), C.byref(kind), log, 256) == L.ERR_NO_DEVICE
        from mini_mcmc_amd.distributions import AutodiffTarget

        with pytest.raises(L.MmcmcError) as e:
            AutodiffTarget("banana", 2, src, params=A.BANANA_PARAMS)
        assert e.value.status == L.ERR_NO_DEVICE


def test_header_travels_to_run_time_compilation():
    mk = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "Makefile")).read()
    hdrs = [ln for ln in mk.splitlines() if ln.startswith("RTC_HDRS")][0].split()
    assert "mm_autodiff.h" in hdrs and hdrs.index("mm_autodiff.h") > hdrs.index("mm_nuts.h")

"""Targets that carry data, on the host: tests/cpp/data_host.cpp, a stand-alone program built with the compiler and flags of
the host twin (oracle/Makefile), evaluates the two models of tests/data_common.py -- each from its log-density alone (forward
mode, csrc/mm_autodiff.h) and with a hand-written gradient -- through the row helper of csrc/mm_data.h on 257 points with
|x| <= 2, and mm_softplusT / mm_sigmoidT on a lattice over [-110, 100].  The device must reproduce that file bit for bit
(tests/test_data_target_gpu.py).  No GPU is needed here.

Bounds.  u = 2^-24 (f32) / 2^-53 (f64).  csrc/mm_math.h states about 1 ulp for mm_expT and mm_logT.  One softplus
m + log(1 + e), e = exp(-|a|) <= 1: e carries at most 1 ulp(e) <= u absolute (e < 1; e = 1 is exact), which log(1 + e) passes
on divided by 1 + e >= 1; rounding 1 + e in [1, 2] is u relative, u in the logarithm; log(1 + e) <= ln 2 < 1 carries 1 ulp <= u;
the final sum rounds by u |value|: at most 4 u max(1, |value|).  The models' bounds propagate that through their sums and
are derived next to the assertions, to first order in u; a factor 1.01 covers the higher orders (n u <= 2^-18).  The
reference is numpy float64: against the f64 results it carries rounding of its own of the same kind (the same sums, no more
roundings per term), so the f64 comparison allows the bound twice; against the f32 results (u 2^29 times larger) its error
is nothing."""
import numpy as np
import pytest

import autodiff_common as A
import data_common as D

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
SLACK = {"f32": 1.01, "f64": 2.02}  # higher-order terms; the float64 reference's own rounding (see above)


def _softplus(a):
    return np.logaddexp(0.0, a)


def _sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1 / (1 + e), e / (1 + e))


def test_the_program_covers_every_case_in_both_types():
    res = D.host_results()
    assert set(res) == {(c, t) for c in ("linreg3", "logit9", "softplus", "softplus_composed", "sigmoid") for t in ("f32", "f64")}
    for (case, ty), r in res.items():
        assert r["x"].shape[0] == 257
        assert np.array_equal(r["x"].astype(np.float64), res[(case, "f64")]["x"])  # the same points, exact in f32
        assert ("grad_hand" in r) == (case in D.MODELS)
        assert np.array_equal(A.bits(r["value"]), A.bits(r["value_plain"]))  # the value next to the gradient is logp<T>
    assert D.LINREG3.size == 28 > 3 * 3 and D.LOGIT9.size == 50 < 9 * 9
    for a in (D.LINREG3, D.LOGIT9):
        assert np.all(a[:, :-1] != 0) and np.array_equal(a.astype(np.float32).astype(np.float64), a)
        assert not np.any(np.all(a[:-1] == a[-1], axis=1)) and a[-1, -1] not in a[:-1, -1]


@pytest.mark.parametrize("ty", ["f32", "f64"])
def test_softplus_on_the_lattice_is_within_four_units_of_logaddexp(ty):
    r = D.host_results()[("softplus", ty)]
    a = r["x"][:, 0].astype(np.float64)
    assert a.min() == -110.0 and a.max() == 100.0 and np.sum(a == 0) == 2 and np.signbit(a[a == 0]).tolist() == [False, True]
    ref = _softplus(a)
    err = np.abs(r["value"].astype(np.float64) - ref)
    tol = 4 * U[ty] * np.maximum(1.0, np.abs(ref))  # the docstring's count; numpy's own ulp is inside "about 1 ulp" of each step
    print(f"softplus {ty}: worst error / bound = {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    # the tangent is a' sigmoid(a): e (1 ulp <= 2 u relative), 1 + e (u), the quotient (u), the product with a' = 1 exact
    g, s = r["grad"][:, 0].astype(np.float64), _sigmoid(a)
    assert np.all(np.abs(g - s) <= 4 * U[ty] * s * SLACK[ty] + (2.0 ** -149 if ty == "f32" else 0))  # f32: e may underflow to a denormal
    sg = D.host_results()[("sigmoid", ty)]
    assert np.array_equal(A.bits(sg["value"]), A.bits(r["grad"][:, 0]))  # one formula, one order
    e = np.exp(-np.abs(a))
    w = e / (1 + e) ** 2  # s (1 - s) without the cancellation of 1 - s
    assert np.all(np.abs(sg["grad"][:, 0].astype(np.float64) - w) <= 8 * U[ty] * w * SLACK[ty] + (2.0 ** -149 if ty == "f32" else 0))


@pytest.mark.parametrize("ty", ["f32", "f64"])
def test_softplus_tangent_at_zero_is_one_half_and_the_composed_spelling_gets_the_sign_wrong(ty):
    res = D.host_results()
    prim, comp = res[("softplus", ty)], res[("softplus_composed", ty)]
    zero = prim["x"][:, 0] == 0
    assert zero.sum() == 2  # +0 and -0
    assert np.all(prim["grad"][zero, 0] == 0.5)  # exactly a' / 2, a' = 1
    # max(a, 0) at the tie takes the constant's tangent, |a| at 0 takes +a': 0 + (-a' e / (1 + e)) = -a' / 2.  Why the primitive exists.
    assert np.all(comp["grad"][zero, 0] == -0.5)
    assert np.array_equal(A.bits(prim["value"]), A.bits(comp["value"]))  # the same value everywhere
    # away from the kink both are the derivative (sigmoid <= 1), each within 4 u of it: the composed one as 1 - e / (1 + e) for a > 0
    away = ~zero
    assert np.all(np.abs(prim["grad"][away].astype(np.float64) - comp["grad"][away].astype(np.float64)) <= 8 * U[ty])


def _linreg3_ref(b):
    """value, gradient and the magnitudes the bound is made of, in float64"""
    x, y = D.LINREG3[:, :3], D.LINREG3[:, 3]
    p0, p1 = D.LINREG3_PARAMS
    res = y[None, :] - b @ x.T  # [n, rows]
    big_r = np.abs(y)[None, :] + np.abs(b) @ np.abs(x).T  # |y| + sum |x b|: what rounding of res scales with
    pr = np.sum(b * b, axis=1)
    sq = np.sum(res * res, axis=1)
    value = -0.5 * (p0 * sq + p1 * pr)
    grad = p0 * res @ x - p1 * b
    n_rows = x.shape[0]
    # value: res_r by 3 fma: 3 u R_r, into res^2 as 2 |res| 3 u R; the 7 fma of the sum: 7 u sum res^2; the prior's 3 fma: 3 u pr;
    # p0 *, p1 *, their sum: 2 u on each term (-1/2 is exact)
    b_val = 0.5 * p0 * (6 * np.sum(np.abs(res) * big_r, axis=1) + n_rows * sq) + 1.5 * p1 * pr + 2 * (0.5 * p0 * sq + 0.5 * p1 * pr)
    # gradient: -1/2 (p0 ga + p1 2 b_k), ga = sum_r 2 (-x_rk res_r) by two fma per row: the error of res enters as 2 |x_rk| 3 u R_r,
    # the 2 x 7 fma as 14 u sum 2 |x_rk res_r|; p0 *, the (exact) 2 b_k, p1 *, the sum: 3 u on the magnitudes
    xr = np.abs(res) @ np.abs(x)  # sum_r |x_rk res_r|
    b_grad = 0.5 * p0 * (6 * big_r @ np.abs(x) + 2 * n_rows * 2 * xr) + 3 * (p0 * xr + p1 * np.abs(b))
    return value, grad, b_val, b_grad


def _logit9_ref(b):
    x, y = D.LOGIT9[:, :9], D.LOGIT9[:, 9]
    eta = b @ x.T  # [n, rows]
    a_r = np.abs(b) @ np.abs(x).T  # sum |x b|: the 9 fma of eta err by 9 u A_r
    sp, s = _softplus(eta), _sigmoid(eta)
    pr = np.sum(b * b, axis=1)
    terms = y[None, :] * eta - sp
    value = np.sum(terms, axis=1) - 0.5 * pr
    grad = (y[None, :] - s) @ x - b
    n_rows = x.shape[0]
    ay = np.abs(y)[None, :]
    # value, per row: eta's error through y eta (|y| 9 u A) and through the 1-Lipschitz softplus (9 u A); the softplus itself
    # 4 u max(1, sp); the product y eta u |y eta|; the difference u (|y eta| + sp).  The 5 additions of the sum: 5 u sum (|y eta| + sp);
    # the prior's 9 fma: 9 u pr / 2; the last difference: u (sum (|y eta| + sp) + pr / 2)
    mag = ay * np.abs(eta) + sp
    b_val = (np.sum(9 * a_r * (1 + ay) + 4 * np.maximum(1.0, sp) + 2 * ay * np.abs(eta) + sp, axis=1) + (n_rows + 1) * np.sum(mag, axis=1) + 5 * pr)
    # gradient, per row and coordinate, |x_rk| times: y x (u |y|); sigmoid: e 2 u, 1 + e u (through e / q: twice), the quotient u -> 5 u s, and
    # its slope <= 1/4 on eta's error: 9/4 u A; the product x s (u s); the difference u (|y| + s).  The 5 additions: 5 u sum |x| (|y| + s);
    # 1/2 (b_k + b_k) is exact; the last difference u (sum |x| (|y| + s) + |b_k|)
    b_grad = (2 * ay + 7 * s + 2.25 * a_r) @ np.abs(x) + (n_rows + 1) * ((ay + s) @ np.abs(x)) + np.abs(b)
    return value, grad, b_val, b_grad


@pytest.mark.parametrize("ty", ["f32", "f64"])
@pytest.mark.parametrize("model", ["linreg3", "logit9"])
def test_value_and_gradient_agree_with_numpy_float64(model, ty):
    r = D.host_results()[(model, ty)]
    value, grad, b_val, b_grad = (_linreg3_ref if model == "linreg3" else _logit9_ref)(r["x"].astype(np.float64))
    for what, got, ref, bound in (("value", r["value"], value, b_val), ("grad", r["grad"], grad, b_grad),
                                  ("value_hand", r["value_hand"], value, b_val), ("grad_hand", r["grad_hand"], grad, b_grad)):
        err, tol = np.abs(got.astype(np.float64) - ref), SLACK[ty] * U[ty] * bound
        print(f"{model} {ty} {what}: worst error / bound = {np.max(err / tol):.3f}")
        assert np.all(err <= tol), (model, ty, what)


@pytest.mark.parametrize("ty", ["f32", "f64"])
@pytest.mark.parametrize("model", ["linreg3", "logit9"])
def test_autodiff_and_hand_written_gradient_are_equal_bit_for_bit(model, ty):
    """linreg3 by construction (the hand-written gradient follows the derivative's operation order); logit9 too, which lets the
    GPU tests run it under HMC and NUTS"""
    r = D.host_results()[(model, ty)]
    assert np.array_equal(A.bits(r["grad"]), A.bits(r["grad_hand"]))
    assert np.array_equal(A.bits(r["value"]), A.bits(r["value_hand"]))


def test_the_posterior_bands_of_the_gpu_test_tell_the_full_model_from_one_without_its_last_row():
    """tests/test_data_target_gpu.py asserts |mean - mu| <= 5 sd / sqrt(4096) and |var / sd^2 - 1| <= 5 sqrt(2 / 4096): not vacuous --
    the posterior of the first six rows alone lies outside both, so an upload that loses the last row fails there"""
    mu, cov = D.linreg3_posterior()
    sd = np.sqrt(np.diag(cov))
    assert np.all(sd > 1 / 3) and np.all(sd < 3) and np.all(np.abs(mu) < 2 * sd + 1)  # a standard-normal start is not in the tail
    mu6, cov6 = D.linreg3_posterior(D.LINREG3[:-1])
    assert np.all(np.abs(mu6 - mu) > 5 * sd / 64)
    assert np.all(np.abs(np.diag(cov6) / sd ** 2 - 1) > 5 * np.sqrt(2 / 4096))
    # the gradient of the log-density vanishes at mu: the closed form and the sources describe the same model
    _, grad, _, _ = _linreg3_ref(mu[None, :])
    assert np.all(np.abs(grad) < 1e-13)


def test_host_program_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main, linked with the sanitizers' runtimes: the bound arrays hold exactly data_len elements,
    so a row helper that reads one too many is a report (-fno-sanitize-recover: any report fails the run)"""
    exe = D.build_host(str(tmp_path), sanitize=True)
    san = D.run_host(exe, str(tmp_path))
    for key, r in D.host_results().items():
        for name, arr in r.items():
            assert np.array_equal(A.bits(arr), A.bits(san[key][name])), (key, name)


def test_header_travels_to_run_time_compilation():
    import os

    mk = open(os.path.join(D.ROOT, "mini_mcmc_amd", "csrc", "Makefile")).read()
    hdrs = [ln for ln in mk.splitlines() if ln.startswith("RTC_HDRS")][0].split()
    assert "mm_data.h" in hdrs and "mm_autodiff.h" in hdrs

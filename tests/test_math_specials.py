"""The engine's scalar math at its edges, on the device (tests/hip/math_specials.hip) and in the host build.

mm_expf_sel / mm_exp_sel (csrc/mm_math.h) are device-only text that claims the bits of mm_expf / mm_exp; mm_accept_stat
(csrc/mm_nuts.h) takes them on the device and the plain forms on the host; mm_logf / mm_log, the two sin / cos (2 pi u) and the
Box-Muller transform define the noise.  One fixed input list (`inputs`) covers, for the exponentials and mm_accept_stat:
both thresholds of each exponential with the 64 representable values on each side, the whole range where the result is
subnormal (f32: every 1/64 from -104 to -87, f64: from -746 to -708), +-0, +-inf, NaN, the largest and smallest normal
values, 2^-24, 2^-53, 1, and 100 000 seeded ordinary values; for the logarithms, sin / cos and Box-Muller the ends of their
domains, 2^-24, 2^-53, 1 and 100 000 seeded values each.

Asserted: `_sel` = the plain form bit for bit on the device; the device = the host build (g++, -ffp-contract=off, the flags of
the `mmath` fixture of tests/test_engine_stream.py) bit for bit, every function; the host build within the bounds that file
states against float64 libm wherever the result is normal (3e-7 relative in f32, 5e-16 in f64; sin / cos 3e-7 and 2e-15
absolute); and where the exponential's result is subnormal, within SUBNORMAL_ULPS units of the subnormal spacing (2^-149,
2^-1074) of float64 (f32) / numpy.longdouble (f64) exp.

Measured on the CPU over the subnormal-result inputs of the list (1910 in f32, 2416 in f64): the largest error is 0.7206
units in f32 and 0.6936 units in f64 (a correctly rounded result would stay within 0.5; the polynomial's own rounding is
scaled down with the result); the bound is the next whole unit, 1.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_mcmc_amd", "csrc")
SUBNORMAL_ULPS = {np.float32: 1.0, np.float64: 1.0}
THRESHOLDS = {np.float32: (np.float32(88.72283905206835), np.float32(-103.97208)),
              np.float64: (np.float64(709.782712893384), np.float64(-745.1332191019411))}
N_ORDINARY = 100_000


def _around(v, n=64):
    dt = type(v)
    out, lo, hi = [v], v, v
    for _ in range(n):
        lo, hi = np.nextafter(lo, dt(-np.inf)), np.nextafter(hi, dt(np.inf))
        out += [lo, hi]
    return np.array(out, dtype=dt)


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(20)
    d = {}
    for dt, key, (lo, hi), span in ((np.float32, "32", (-104, -87), (-90.0, 88.0)), (np.float64, "64", (-746, -708), (-700.0, 700.0))):
        fi = np.finfo(dt)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -53,
                            -(2.0 ** -53), 1.0, -1.0], dtype=dt)
        d["e" + key] = np.concatenate([_around(THRESHOLDS[dt][0]), _around(THRESHOLDS[dt][1]),
                                       (np.arange(lo * 64, hi * 64 + 1) / 64.0).astype(dt), special,
                                       rng.uniform(span[0], span[1], N_ORDINARY // 2).astype(dt),
                                       rng.normal(0.0, 3.0, N_ORDINARY // 2).astype(dt)])
        d["l" + key] = np.concatenate([np.array([fi.tiny, fi.max, 1.0, 2.0 ** -24, 2.0 ** -53, 0.5, 0.70710678, 1.4142135623730951, 2.0], dtype=dt),
                                       rng.random(N_ORDINARY // 2).astype(dt) + dt(fi.tiny),
                                       (2.0 ** rng.uniform(-60, 60, N_ORDINARY // 2)).astype(dt)])
        d["u" + key] = np.concatenate([np.array([0.0, 1.0, 2.0 ** -24, 2.0 ** -53, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0 - 2.0 ** -24],
                                                dtype=dt), rng.random(N_ORDINARY).astype(dt)])
    u1 = np.concatenate([[2.0 ** -53, 1.0, 2.0 ** -24, 0.5], 1.0 - rng.random(N_ORDINARY)])  # (0, 1]: mm_u53 never gives 0
    u2 = np.concatenate([[1.0, 2.0 ** -53, 0.25, 0.75], 1.0 - rng.random(N_ORDINARY)])
    d["b64"] = np.stack([u1, u2], axis=1).astype(np.float64)
    return d


HOST_SRC = r'''
#include "mm_nuts.h"
#define W1(NAME, T, EXPR) extern "C" void NAME(const T *x, size_t n, T *o) { for (size_t i = 0; i < n; ++i) o[i] = EXPR; }
W1(h_expf, float, mm_expf(x[i]))
W1(h_accept32, float, mm_accept_stat<float>(x[i]))
W1(h_logf, float, mm_logf(x[i]))
W1(h_exp, double, mm_exp(x[i]))
W1(h_accept64, double, mm_accept_stat<double>(x[i]))
W1(h_log, double, mm_log(x[i]))
extern "C" void h_sincos32(const float *x, size_t n, float *o) { for (size_t i = 0; i < n; ++i) mm_sincos2pif(x[i], &o[2 * i], &o[2 * i + 1]); }
extern "C" void h_sincos64(const double *x, size_t n, double *o) { for (size_t i = 0; i < n; ++i) mm_sincos2pi(x[i], &o[2 * i], &o[2 * i + 1]); }
extern "C" void h_boxmuller(const double *x, size_t n, double *o)
{
    for (size_t i = 0; i < n; ++i) mm_box_muller_f64(x[2 * i], x[2 * i + 1], &o[2 * i], &o[2 * i + 1]);
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory, inputs):
    """every function over the input list in the host build: {name: array}, names as the device program prints them"""
    d = tmp_path_factory.mktemp("math_specials_host")
    src, so = d / "h.cpp", d / "h.so"
    src.write_text(HOST_SRC)
    subprocess.run(["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(src), "-o",
                    str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))

    def call(fn, x, n_out=1):
        x = np.ascontiguousarray(x)
        n = x.size // (x.shape[1] if x.ndim == 2 else 1)
        o = np.empty(n * n_out, dtype=x.dtype)
        f = getattr(lib, fn)
        f.restype, f.argtypes = None, [C.c_void_p, C.c_size_t, C.c_void_p]
        f(x.ctypes.data, n, o.ctypes.data)
        return o

    return {"expf": call("h_expf", inputs["e32"]), "accept32": call("h_accept32", inputs["e32"]), "exp": call("h_exp", inputs["e64"]),
            "accept64": call("h_accept64", inputs["e64"]), "logf": call("h_logf", inputs["l32"]), "log": call("h_log", inputs["l64"]),
            "sincos32": call("h_sincos32", inputs["u32"], 2), "sincos64": call("h_sincos64", inputs["u64"], 2),
            "boxmuller": call("h_boxmuller", inputs["b64"], 2)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def subnormal_error_units(x, got):
    """largest |got - exp(x)| in units of the subnormal spacing, over the inputs whose exact result is below the smallest
    normal value and above half the smallest subnormal; reference float64 for f32, longdouble for f64"""
    dt = got.dtype.type
    fi = np.finfo(dt)
    wide = np.float64 if dt == np.float32 else np.longdouble
    with np.errstate(all="ignore"):
        ref = np.exp(x.astype(wide))
        spacing = wide(fi.smallest_subnormal)
        sel = np.isfinite(x) & (ref < wide(fi.tiny)) & (ref > spacing / 2)
        return float(np.max(np.abs(got[sel].astype(wide) - ref[sel]) / spacing)), int(sel.sum())


@pytest.mark.parametrize("dt,key", [(np.float32, "32"), (np.float64, "64")], ids=["f32", "f64"])
def test_host_build_against_libm(inputs, host, dt, key):
    fi = np.finfo(dt)
    wide = np.float64 if dt == np.float32 else np.longdouble
    rel = 3e-7 if dt == np.float32 else 5e-16
    x = inputs["e" + key]
    got = host["expf" if dt == np.float32 else "exp"]
    hi, lo = THRESHOLDS[dt]
    with np.errstate(all="ignore"):
        ref = np.exp(x.astype(wide))
        # the edges: NaN stays NaN (payload and sign kept), above the upper threshold +inf, below the lower one +0
        nan = np.isnan(x)
        assert np.array_equal(_bits(got[nan]), _bits(x[nan]))
        assert np.isposinf(got[x > hi]).all() and np.isfinite(got[ref < wide(fi.max) * (1 - rel)]).all()
        assert np.isposinf(got[ref > wide(fi.max) * (1 + rel)]).all()
        assert (_bits(got[x < lo]) == 0).all()
        assert (got[(x == 0)] == 1).all()
        # normal results
        normal = ~nan & (ref <= wide(fi.max) * (1 - rel)) & (ref >= wide(fi.tiny))
        err = np.abs(got[normal].astype(wide) - ref[normal]) / ref[normal]
        assert normal.sum() > N_ORDINARY // 2 and float(err.max()) < rel, float(err.max())
    # subnormal results, in units of their spacing
    units, n = subnormal_error_units(x, got)
    print(f"{dt.__name__}: subnormal results: {n} inputs, largest error {units:.4f} units of {fi.smallest_subnormal}")
    assert n > 500 and units <= SUBNORMAL_ULPS[dt], units
    # the acceptance statistic is min(1, exp(d)) on the same bits, 1 for a NaN
    acc = host["accept" + key]
    with np.errstate(all="ignore"):
        want = np.where(x < 0, got, dt(1))
    assert np.array_equal(_bits(acc), _bits(want.astype(dt)))
    # logarithm, sin / cos
    xl = inputs["l" + key]
    gl = host["logf" if dt == np.float32 else "log"]
    refl = np.log(xl.astype(wide))
    errl = np.abs(gl.astype(wide) - refl) / np.maximum(np.abs(refl), wide(1e-6 if dt == np.float32 else 1e-12))
    assert float(errl.max()) < rel, float(errl.max())
    assert gl[xl == 1][0] == 0
    u = inputs["u" + key]
    sc = host["sincos" + key].reshape(-1, 2).astype(wide)
    ang = 2 * wide(np.pi) * u.astype(wide) if wide is np.float64 else 2 * np.longdouble("3.14159265358979323846264338327950288") * u.astype(wide)
    errs = max(float(np.abs(sc[:, 0] - np.sin(ang)).max()), float(np.abs(sc[:, 1] - np.cos(ang)).max()))
    assert errs < (3e-7 if dt == np.float32 else 2e-15), errs


def _run_device(tmp_path, inputs):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "math_specials")
    src = os.path.join(ROOT, "tests", "hip", "math_specials.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + CSRC, src, "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    path = tmp_path / "in.bin"
    order = ["e32", "e64", "l32", "l64", "u32", "u64", "b64"]
    with open(path, "wb") as f:
        f.write(np.array([len(inputs[k]) for k in order], dtype=np.uint64).tobytes())
        for k in order:
            f.write(np.ascontiguousarray(inputs[k]).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, n, words = line.split(" ")
        f32 = name in ("expf", "expf_sel", "accept32", "logf", "sincos32")
        raw = bytes.fromhex(words)
        out[name] = np.frombuffer(raw, dtype=">u4" if f32 else ">u8").astype(np.uint32 if f32 else np.uint64)
        assert out[name].size == int(n)
    return out


@pytest.mark.gpu
def test_device_math_equals_host_build_bit_for_bit(tmp_path, inputs, host):
    dev = _run_device(tmp_path, inputs)
    assert set(dev) == set(host) | {"expf_sel", "exp_sel"}
    # the branch-free forms are the plain forms, on the device
    for sel, plain, key in (("expf_sel", "expf", "e32"), ("exp_sel", "exp", "e64")):
        bad = np.flatnonzero(dev[sel] != dev[plain])
        assert bad.size == 0, (sel, bad.size, inputs[key][bad[:5]], dev[sel][bad[:5]], dev[plain][bad[:5]])
    # the device is the host build
    arg = {"expf": "e32", "accept32": "e32", "exp": "e64", "accept64": "e64", "logf": "l32", "log": "l64", "sincos32": "u32",
           "sincos64": "u64", "boxmuller": "b64"}
    for name, h in host.items():
        hb = _bits(h)
        assert dev[name].shape == hb.shape, name
        bad = np.flatnonzero(dev[name] != hb)
        per = 2 if name in ("sincos32", "sincos64", "boxmuller") else 1
        assert bad.size == 0, (name, bad.size, "first inputs", inputs[arg[name]][bad[:5] // per], "device", dev[name][bad[:5]], "host", hb[bad[:5]])

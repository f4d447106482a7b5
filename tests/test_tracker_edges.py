"""The tracker kernels (csrc/mm_tracker.hip) checked exactly, per chain and per flag, at the edges of every path.

The C ABI shows only aggregates of the tracker (R-hat per parameter, one p_accept, the mean of the per-chain averages),
which tests/test_tracker.py compares with the oracle at 2e-5 / 1e-6: one wrong chain of 300, one wrong flag byte outside
the last 4096, or two opposite errors pass there.  Here tests/hip/tracker_probe.hip -- a stand-alone program that
includes the unit and so sees `struct mmcmc_tracker` -- copies back the per-chain mean, mean of squares, last state and
acceptance average, the flag bytes and p_accept after EVERY mmcmc_tracker_steps call, and they are compared bit for bit
with the plain numpy reference of tests/tracker_ref.py, which the CPU tests below tie to the pinned oracle.

Paths of mm_tracker.hip (mmcmc_tracker_steps sends the first k - k % 16 rows of a call through a tile kernel where one
exists and the remainder through the generic kernel):
  generic   tracker_step_kernel<T>: k < 16, the remainder of k % 16 rows, every row for D > 8 (f32) / D > 4 (f64)
  tiled     tracker_step_tiled_kernel<T, 1>: D = 1 (and D > 1 in the -DMMCMC_TUNING build with MMCMC_TRACKER_ONE_WAVE)
  dims      tracker_step_dims_kernel<T, D>: D 2..8 (f32), 2..4 (f64); per workgroup of 64 chains the 16 x 64 flags of a
            tile leave `packed` (one 16-byte store per lane) when the workgroup is full and C % 16 == 0, else `bytes`
  paccept   tracker_paccept_kernel: 16-flags-per-load (`vector`) or byte loads per lane, certificate / carry / restart
The table CASES names, for every case, the path it is there for.
"""
import dataclasses
import functools
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import tracker_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_mcmc_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "tracker_probe.hip")
# csrc/Makefile's HIPFLAGS without -fPIC and the warning switches (test_probe_is_compiled_like_the_library)
PROBE_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]
ERR_STATE = -5  # include/mmcmc.h: the aggregates before the second step (n / (n - 1))
# The child does well under a second of GPU work (69 cases, the largest 45 000 states) after the start-up of the runtime
# and the load of one code object: a few seconds in all.
PROBE_RUN_TIMEOUT_S = 60
PROBE_BUILD_TIMEOUT_S = 900

# Largest deviation of the f32 recurrence (tracker_ref.Tracker) from the float64 statement over CASES, measured on the
# reference on the CPU (test_f32_recurrence_stays_close_to_float64 prints the three figures):
#   mean, relative to the root mean square of the chain's states so far   MEASURED_DEV["mean"]
#   mean of squares, relative                                             MEASURED_DEV["mean_sq"]
#   R-hat (within_and_var's and collect_rhat's), relative, where finite   MEASURED_DEV["rhat"]
# asserted with a margin of 4x.
# Measured: mean 3.9e-7 (chains-f32-D3-C300), mean of squares 1.08e-6 (pacc-carry-12x64, 192 rows), R-hat 1.0e-7
# (packed-f64-C256-k16): a few f32 ulps, growing slowly with the number of rows.
MEASURED_DEV = {"mean": 3.9e-7, "mean_sq": 1.08e-6, "rhat": 1.0e-7}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    C: int
    D: int
    dtype: str                      # "f32" | "f64"
    calls: tuple                    # ((t0, k, states_is_device), ...)
    path: str                       # what the case is there for
    n_rows: int = 0                 # rows per chain of the buffer (0: exactly the rows the calls consume)
    init: bool = False              # mmcmc_tracker_init_last first
    data: str = "normal"            # "normal" | "ones" (no state repeats) | "const" (no state ever changes)
    restart_class: bool = False     # one of the two designated cases whose p_accept is held to 1e-6
    states_of: str = ""             # takes the states of that case (the same states fed in another way)

    @property
    def rows(self):
        return max(t0 + k for t0, k, _ in self.calls) if not self.n_rows else self.n_rows

    @property
    def consumed(self):
        return [t for t0, k, _ in self.calls for t in range(t0, t0 + k)]

    @property
    def one_wave(self):
        """has rows that tracker_step_dims_kernel takes -- and tracker_step_tiled_kernel<T, D> in the tuning build"""
        return self.D > 1 and self.D * (4 if self.dtype == "f32" else 8) <= 32 and any(k >= 16 for _, k, _ in self.calls)


def _one(k, dev=0, t0=0):
    return ((t0, k, dev),)


def _blocks(sizes, dev):
    out, t = [], 0
    for k in sizes:
        out.append((t, k, dev))
        t += k
    return tuple(out)


UNEVEN = (1, 5, 16, 3, 33, 12)  # 70 rows: generic, generic, one tile, generic, two tiles + 1, the rest


def _cases():
    c = []

    def add(name, C, D, dtype, calls, path, **kw):
        c.append(Case(name, C, D, dtype, calls, path, **kw))

    # ---- kernel dispatch: f32 and f64 at D in {1, 2, 3, 4, 5, 8, 9, 64}
    add("disp-f32-D1", 65, 1, "f32", _one(33), "tiled<f32,1> 2 tiles + generic 1 row, ragged 2nd block of 1 chain")
    add("disp-f32-D2", 80, 2, "f32", _one(48, 1), "dims<f32,2> 3 tiles (difs buffers wrap), block 0 packed, block 1 n_valid=16 bytes")
    add("disp-f32-D3", 128, 3, "f32", _one(32), "dims<f32,3> 2 tiles, every block packed")
    add("disp-f32-D4", 144, 4, "f32", _one(17, 1), "dims<f32,4> 1 tile + generic 1 row, C%16==0 with n_valid=16 last block")
    add("disp-f32-D5", 64, 5, "f32", _one(33), "dims<f32,5> 2 tiles + 1, one full packed block")
    add("disp-f32-D8", 300, 8, "f32", _one(16, 1), "dims<f32,8> single tile, no prefetch, C%16!=0: bytes everywhere")
    add("disp-f32-D9", 63, 9, "f32", _one(17), "generic<f32> only (D > 8), below one wave")
    add("disp-f32-D64", 65, 64, "f32", _one(16, 1), "generic<f32> only, kMaxDim")
    add("disp-f64-D1", 64, 1, "f64", _one(48, 1), "tiled<f64,1> 3 tiles")
    add("disp-f64-D2", 128, 2, "f64", _one(33), "dims<f64,2> 2 tiles + 1, packed")
    add("disp-f64-D3", 80, 3, "f64", _one(32, 1), "dims<f64,3> 2 tiles, packed block + n_valid=16 bytes block")
    add("disp-f64-D4", 63, 4, "f64", _one(48), "dims<f64,4> 3 tiles, n_valid=63 bytes")
    add("disp-f64-D5", 144, 5, "f64", _one(33, 1), "generic<f64> only (D > 4 for f64)")
    add("disp-f64-D8", 2, 8, "f64", _one(17), "generic<f64> only, the minimum chain count")
    add("disp-f64-D9", 300, 9, "f64", _one(15, 1), "generic<f64> only, two blocks of 256")
    add("disp-f64-D64", 2, 64, "f64", _one(32), "generic<f64> only, kMaxDim")
    # ---- chain counts through the dims kernel
    add("chains-f32-D3-C2", 2, 3, "f32", _one(16), "dims n_valid=2, single tile")
    add("chains-f32-D3-C63", 63, 3, "f32", _one(32, 1), "dims n_valid=63 bytes")
    add("chains-f32-D3-C64", 64, 3, "f32", _one(48), "dims one packed block, 3 tiles")
    add("chains-f32-D3-C65", 65, 3, "f32", _one(33, 1), "dims C%16!=0: full block 0 still bytes, block 1 one chain")
    add("chains-f32-D3-C80", 80, 3, "f32", _one(17), "dims block 0 packed, block 1 n_valid=16 bytes, + generic row")
    add("chains-f32-D3-C144", 144, 3, "f32", _one(32, 1), "dims blocks 0,1 packed, block 2 n_valid=16 bytes")
    add("chains-f32-D3-C300", 300, 3, "f32", _one(33), "dims ragged, bytes everywhere, generic row over 2 blocks of 256")
    add("chains-f64-D2-C64", 64, 2, "f64", _one(16, 1), "dims<f64,2> one packed block, single tile")
    add("chains-f64-D2-C144", 144, 2, "f64", _one(48), "dims<f64,2> packed + n_valid=16, 3 tiles")
    add("chains-f64-D2-C300", 300, 2, "f64", _one(17, 1), "dims<f64,2> ragged + generic row")
    # ---- rows per call at a packed shape (k = 32: disp-f32-D3)
    for k, what in ((1, "generic only, one row"), (15, "generic only, no tile"), (16, "single tile, no prefetch"),
                    (17, "tile + generic remainder of 1"), (33, "2 tiles + 1"), (48, "3 tiles: difs buffers wrap")):
        add(f"rows-f32-D3-k{k}", 128, 3, "f32", _one(k, k & 1), "dims packed, " + what)
    add("rows-f32-D1-k15", 65, 1, "f32", _one(15, 1), "D=1 below a tile: generic only")
    add("rows-f32-D1-k16", 65, 1, "f32", _one(16), "tiled<f32,1> single tile, no prefetch")
    # ---- addressing: odd n_rows > t0 + k, so the 16-byte pieces of a chain's run are only element-aligned
    for dt in ("f32", "f64"):
        for t0 in (0, 1, 9):
            add(f"addr-{dt}-D3-t{t0}", 80, 3, dt, _one(33, t0 & 1, t0), f"dims<{dt},3> pieces at element alignment, t0={t0}",
                n_rows=t0 + 33 + (2 if (t0 + 33) % 2 else 3))
    # ---- the same 70 states fed in four ways
    for dt, C, D in (("f32", 144, 3), ("f64", 80, 2)):
        add(f"multi-{dt}-one", C, D, dt, _one(70), "one call: 4 tiles + 6")
        add(f"multi-{dt}-rows", C, D, dt, _blocks((1,) * 70, 1), "70 calls of one row (generic), device memory",
            states_of=f"multi-{dt}-one")
        add(f"multi-{dt}-uneven-host", C, D, dt, _blocks(UNEVEN, 0), "blocks 1, 5, 16, 3, 33, 12 from host memory",
            states_of=f"multi-{dt}-one")
        add(f"multi-{dt}-uneven-dev", C, D, dt, _blocks(UNEVEN, 1), "blocks 1, 5, 16, 3, 33, 12 from device memory",
            states_of=f"multi-{dt}-one")
    add("init-f32", 80, 2, "f32", _blocks(UNEVEN, 1), "init_last, then uneven blocks", init=True)
    add("init-f64", 65, 4, "f64", _blocks(UNEVEN, 0), "init_last (f64 rounded to f32), then uneven blocks", init=True)
    # ---- packed flags seen end to end: the last 4096 flags are all tile output, p_accept exact
    add("packed-C64-k64", 64, 3, "f32", _one(64, 1), "dims packed, 4 tiles; need=4096")
    add("packed-C256-k16", 256, 3, "f32", _one(16), "dims packed, 4 blocks; need=4096")
    add("packed-C1024-k16", 1024, 3, "f32", _one(16, 1), "dims packed, 16 blocks; need=16384, certificate over the last 4 rows")
    add("packed-f64-C256-k16", 256, 2, "f64", _one(16), "dims<f64,2> packed; need=4096")
    # ---- tracker_paccept_kernel: need = k C at the edges of its lanes (256 flags) and of its tail (16384).  need = 1 cannot
    # be reached: mmcmc_tracker_create refuses fewer than two chains, so 2 is the minimum.
    add("pacc-2", 2, 1, "f32", _one(1), "need=2: one partial lane, byte loads, carry")
    add("pacc-255", 85, 1, "f32", _one(3, 1), "need=255: lane 0 one short of full, byte loads")
    add("pacc-256", 16, 1, "f32", _one(16), "need=256: lane 0 full, vector loads")
    add("pacc-257", 257, 1, "f32", _one(1, 1), "need=257: lane 0 vector, lane 1 one flag by bytes")
    add("pacc-4095", 65, 1, "f32", _one(63), "need=4095: 15 vector lanes + partial; the certificate covers everything")
    add("pacc-4096", 128, 1, "f32", _one(32, 1), "need=4096: 16 full lanes")
    add("pacc-4097", 241, 1, "f32", _one(17), "need=4097: 17 lanes, the certificate skips lane 0")
    add("pacc-16383", 381, 1, "f32", _one(43, 1), "need=16383: last lane one short")
    add("pacc-16384", 512, 1, "f32", _one(32), "need=16384: every lane full, first=0, no restart")
    add("pacc-16385", 565, 1, "f32", _one(29, 1), "need=16385: first=1 unaligned (byte loads in every lane), restart set")
    add("pacc-16391x1", 16391, 1, "f32", _one(1), "first=7 unaligned, restart set (init_last: one row of mixed flags)", init=True)
    add("pacc-20000x1", 20000, 1, "f32", _one(1, 1), "first=3616 aligned: vector loads at an offset, restart set (init_last)",
        init=True)
    add("pacc-carry-12x64", 4, 1, "f32", _blocks((16,) * 12, 1), "twelve calls of 64 flags: the certificate never meets, p is carried")
    add("pacc-ones-5000x9", 5000, 2, "f32", _one(9), "every flag 1: no meeting, restart from 0.5 over 16384 flags",
        data="ones", restart_class=True)
    add("pacc-zeros-5000x4", 5000, 2, "f32", _one(4, 1), "every flag 0 (constant states after init_last): restart from 0.5",
        data="const", init=True, restart_class=True)
    return tuple(c)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ONE_WAVE_CASES = tuple(c for c in CASES if c.one_wave)
_ids = [c.name for c in CASES]


def _np_dtype(case):
    return np.float32 if case.dtype == "f32" else np.float64


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(init [C, D] or None, states [C, n_rows, D]) of a case; read-only"""
    case = BY_NAME[name]
    C, D, rows, dt = case.C, case.D, case.rows, _np_dtype(case)
    if case.states_of:
        assert (case.C, case.D, case.dtype, case.consumed, case.init) == (
            BY_NAME[case.states_of].C, BY_NAME[case.states_of].D, BY_NAME[case.states_of].dtype,
            BY_NAME[case.states_of].consumed, BY_NAME[case.states_of].init)
        return inputs(case.states_of)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    init = rng.standard_normal((C, D)).astype(dt) if case.init else None
    if case.data == "const":
        # constants with few mantissa bits: every recurrence is exact, within = 0 and R-hat = +inf on every side
        init = (np.round(rng.standard_normal((C, D)) * 8.0) / 8.0).astype(dt)
        x = np.repeat(init[:, None, :], rows, axis=1)
    else:
        x = rng.standard_normal((C, rows, D)).astype(dt)  # f64: not representable in f32, the rounding matters
    if case.data == "normal":
        keep = rng.random((C, rows)) < 0.35  # a rejected step repeats the state before it
        for t in range(1, rows):
            x[:, t][keep[:, t]] = x[:, t - 1][keep[:, t]]
        o = case.consumed
        base = init if case.init else np.zeros((C, D), dtype=dt)
        if case.init:                             # a rejected first step repeats the initial state
            keep0 = rng.random(C) < 0.35
            x[keep0, o[0], :] = init[keep0]
        x[0, o[0], :] = base[0]                   # the first state equals `last`: flag 0 (all zeros without init_last)
        if len(o) > 2:
            x[0, o[1], :] = dt(-0.0)              # -0.0 ...
            x[0, o[2], :] = dt(0.0)               # ... then +0.0: equal, flag 0, but `last` changes its sign bit
        if D > 1:
            x[1, o[0], :] = base[1] + dt(1.0)     # first comparison: coordinate 0 unchanged, the others moved (Q12)
            x[1, o[0], 0] = base[1, 0]
            if len(o) > 2:
                x[1, o[2], :] = x[1, o[1], :]     # a row where only the last coordinate changes
                x[1, o[2], D - 1] += dt(1.0)
    x.setflags(write=False)
    if init is not None:
        init.setflags(write=False)
    return init, x


@functools.lru_cache(maxsize=None)
def reference(name):
    """tracker_ref run over the calls of a case: snapshots and flags per call, certificate per call, aggregates; computed
    once and shared by every test below"""
    case = BY_NAME[name]
    init, x = inputs(name)
    tr = R.Tracker(case.C, case.D, init)
    snaps, flags, certs = [], [], []
    for t0, k, _ in case.calls:
        f = tr.steps(x[:, t0:t0 + k, :])
        flags.append(f)
        certs.append(R.certificate(f))
        snaps.append(tr.snapshot())
    out = dict(snaps=snaps, flags=flags, certs=certs, n=tr.n, rows=R.to_f32(x[:, case.consumed, :]))
    if tr.n >= 2:
        out["rhat"] = R.rhat_stats(tr.mean, tr.mean_sq, tr.n)
        out["cs"] = R.chain_stats(tr.mean, tr.mean_sq, tr.p_chain, tr.n)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ================================================================ CPU: the reference against the oracle


@functools.lru_cache(maxsize=None)
def oracle_values(name):
    import oracle as O

    case = BY_NAME[name]
    init, _ = inputs(name)
    rows = reference(name)["rows"]
    i0 = np.zeros((case.C, case.D), dtype=np.float32) if init is None else R.to_f32(init)
    with np.errstate(all="ignore"):
        rhat_cs, p_chain = O.chain_trackers_rhat(i0, rows)
        rhat_mc, p = O.multichain_tracker_rhat(np.ascontiguousarray(rows.transpose(1, 0, 2)))
    return dict(rhat_cs=rhat_cs, p_chain=p_chain, rhat_mc=rhat_mc, p=p)


def test_case_table_covers_what_it_claims():
    """every chain count, row count, dimension and call form of the plan is there, about 60 cases"""
    assert 55 <= len(CASES) <= 75
    assert {2, 63, 64, 65, 80, 128, 144, 300} <= {c.C for c in CASES if c.one_wave}
    assert {1, 15, 16, 17, 32, 33, 48} <= {k for c in CASES if c.C == 128 and c.D == 3 for _, k, _ in c.calls}
    for dt in ("f32", "f64"):
        assert {1, 2, 3, 4, 5, 8, 9, 64} <= {c.D for c in CASES if c.dtype == dt}
        assert {0, 1, 9} <= {c.calls[0][0] for c in CASES if c.name.startswith("addr-" + dt)}
    for c in CASES:
        if c.name.startswith("addr-"):
            assert c.rows % 2 == 1 and c.rows > c.calls[0][0] + c.calls[0][1]
    needs = {c.calls[0][1] * c.C for c in CASES if c.name.startswith("pacc-") and len(c.calls) == 1}
    assert {2, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 16391, 20000, 45000} <= needs
    assert sum(c.restart_class for c in CASES) == 2
    # the tuning binary gets every case that has rows for the dims kernel, and only those
    assert all(c.D in (2, 3, 4, 5, 8) for c in ONE_WAVE_CASES) and len(ONE_WAVE_CASES) >= 30


@pytest.mark.parametrize("name", _ids)
def test_reference_per_chain_p_accept_equals_the_oracle(O, name):
    """tracker_ref's per-chain acceptance average = ChainTracker's (O.chain_trackers_rhat), bit for bit"""
    assert np.array_equal(bits(reference(name)["snaps"][-1]["p_chain"]), bits(oracle_values(name)["p_chain"]))


@pytest.mark.parametrize("name", _ids)
def test_reference_p_accept_equals_the_oracle(O, name):
    """tracker_ref's sequential fold = MultiChainTracker's p_accept (O.multichain_tracker_rhat), bit for bit.  The oracle
    starts from an all-zero `last`; for the cases that call init_last the reference is run once more that way over the
    same states (their own first row of flags is tied to the oracle through the per-chain averages above)."""
    case = BY_NAME[name]
    if case.init:
        tr = R.Tracker(case.C, case.D)
        tr.steps(reference(name)["rows"])
        p = tr.p
    else:
        p = reference(name)["snaps"][-1]["p"]
    assert bits(p) == bits(oracle_values(name)["p"])


@pytest.mark.parametrize("name", _ids)
def test_reference_rhat_is_the_oracles(O, name):
    """the exact-sum R-hat of tracker_ref within the suite's 2e-5 of both oracle functions"""
    ref, o = reference(name), oracle_values(name)
    if ref["n"] < 2:
        assert "rhat" not in ref  # n / (n - 1): the library answers MMCMC_ERR_STATE
        return
    np.testing.assert_allclose(ref["rhat"][0], o["rhat_mc"], rtol=2e-5)
    np.testing.assert_allclose(ref["cs"]["rhat"][0], o["rhat_cs"], rtol=2e-5)
    for iv in (ref["rhat"], ref["cs"]["rhat"], ref["cs"]["within"], ref["cs"]["var"]):
        assert np.all(R.inside(iv[0], iv))


@pytest.mark.parametrize("name", _ids)
def test_certificate_class_of_every_call(name):
    """Only the two designated cases may be held to 1e-6; everywhere else the device's p_accept has to be the sequential
    fold's bit for bit: the certificate meets (and then gives the fold's number -- checked here on the reference), or the
    call has at most 16 384 flags and the kernel continues from the stored value."""
    case, ref = BY_NAME[name], reference(name)
    for i, (cert, snap) in enumerate(zip(ref["certs"], ref["snaps"])):
        if case.restart_class:
            assert cert["cls"] == "restart" and len(case.calls) == 1 and cert["len"] == R.TAIL
            assert len(set(ref["flags"][i].ravel().tolist())) == 1  # all flags 1, or all flags 0
        else:
            assert cert["cls"] in ("certificate", "carry"), (i, cert)
        if cert["meets"]:
            assert bits(cert["value"]) == bits(snap["p"]), (i, cert)
        # the kernel's window (the last 16 occupied lanes: 3841 .. 4096 flags) decides like the last min(len, 4096) flags
        assert cert["meets"] == cert["meets_last_4096"] and cert["window"] >= min(cert["len"], 3841)
        if cert["meets_last_4096"]:
            assert bits(cert["value_last_4096"]) == bits(snap["p"])
    if name == "pacc-carry-12x64":
        assert [c["cls"] for c in ref["certs"]] == ["carry"] * 12
    if name in ("pacc-16385", "pacc-16391x1", "pacc-20000x1", "packed-C1024-k16"):
        assert ref["certs"][0]["cls"] == "certificate"
    if name.startswith("pacc-163") or name == "pacc-20000x1":
        assert ref["certs"][0]["first"] == {"pacc-16383": 0, "pacc-16384": 0, "pacc-16385": 1, "pacc-16391x1": 7,
                                            "pacc-20000x1": 3616}[name]


def _deviations(name):
    ref = reference(name)
    rows, n = ref["rows"], ref["n"]
    m64, q64 = R.float64_statement(rows)
    dev = {"mean": 0.0, "mean_sq": 0.0, "rhat": 0.0}
    tr = R.Tracker(rows.shape[0], rows.shape[2])
    for t in range(n):  # after every row
        tr.steps(rows[:, t:t + 1, :])
        scale = np.sqrt(q64[:, t, :])
        ok = scale > 0
        if ok.any():
            dev["mean"] = max(dev["mean"], float(np.max(np.abs(tr.mean.astype(np.float64) - m64[:, t, :])[ok] / scale[ok])))
            dev["mean_sq"] = max(dev["mean_sq"], float(np.max(np.abs(tr.mean_sq.astype(np.float64) - q64[:, t, :])[ok] / q64[:, t, :][ok])))
    if n >= 2:
        for mine, f64 in zip((ref["rhat"][0], ref["cs"]["rhat"][0]), R.rhat_f64(m64[:, -1, :], q64[:, -1, :], n)):
            ok = np.isfinite(f64) & np.isfinite(mine)
            if ok.any():
                dev["rhat"] = max(dev["rhat"], float(np.max(np.abs(mine.astype(np.float64) - f64)[ok] / f64[ok])))
            assert np.array_equal(np.isfinite(f64), np.isfinite(mine))
    return dev


def test_f32_recurrence_stays_close_to_float64():
    """What the reference's f32 recurrence costs against float64 running means: a property of the reference, measured on
    the reference (MEASURED_DEV above), held with a margin of 4x."""
    worst = {"mean": (0.0, ""), "mean_sq": (0.0, ""), "rhat": (0.0, "")}
    for c in CASES:
        if c.states_of:
            continue
        for key, v in _deviations(c.name).items():
            if v > worst[key][0]:
                worst[key] = (v, c.name)
    print("f32 recurrence vs float64:", worst)
    for key, (v, where) in worst.items():
        assert v <= 4.0 * MEASURED_DEV[key], (key, v, where)
        assert v >= MEASURED_DEV[key] / 4.0, (key, v, where)  # the recorded figure is the measured one, not a loose cap


def makefile_hipflags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    line = re.search(r"^HIPFLAGS\s*\?=\s*(.+)$", text, re.M).group(1)
    return line.replace("$(ARCH)", arch).split(), text


def test_probe_is_compiled_like_the_library():
    """the kernels the probe recompiles are the shipped ones: same --offload-arch, -O, -ffp-contract and -std as
    csrc/Makefile's HIPFLAGS, which no rule changes for mm_tracker.o; the tuning build adds -DMMCMC_TUNING as the Makefile does"""
    flags, text = makefile_hipflags()

    def pick(fl):
        return sorted(f for f in fl if f.startswith(("--offload-arch", "-O", "-ffp-contract", "-std", "-f", "-m", "-D"))
                      and f not in ("-fPIC",))

    assert pick(flags) == pick(PROBE_FLAGS)
    assert len([f for f in PROBE_FLAGS if f.startswith(("--offload-arch", "-O", "-ffp-contract", "-std"))]) == 4
    assert not re.search(r"mm_tracker\.o\s*:\s*HIPFLAGS", text)
    assert re.search(r"^ifdef TUNING\nHIPFLAGS \+= -DMMCMC_TUNING$", text, re.M)
    assert '#include "../../mini_mcmc_amd/csrc/mm_tracker.hip"' in open(PROBE_SRC).read()  # the unit itself, not the library


# ================================================================ GPU: the probe


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x504B5254, len(cases)))
        for c in cases:
            init, x = inputs(c.name)
            nm = c.name.encode()
            f.write(struct.pack("<I", len(nm)) + nm)
            f.write(struct.pack("<QQQIII", c.C, c.D, c.rows, 0 if c.dtype == "f32" else 1, 1 if c.init else 0, len(c.calls)))
            for t0, k, dev in c.calls:
                f.write(struct.pack("<QQI", t0, k, dev))
            if c.init:
                f.write(np.ascontiguousarray(init).astype("<" + ("f4" if c.dtype == "f32" else "f8")).tobytes())
            f.write(np.ascontiguousarray(x).astype("<" + ("f4" if c.dtype == "f32" else "f8")).tobytes())


def read_results(path, cases):
    buf = open(path, "rb").read()
    pos = 0

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=pos)
        pos += a.nbytes
        return a

    out = {}
    for c in cases:
        cd, calls = c.C * c.D, []
        for _, k, _ in c.calls:
            calls.append(dict(mean=take("<f4", cd).reshape(c.C, c.D), mean_sq=take("<f4", cd).reshape(c.C, c.D),
                              last=take("<f4", cd).reshape(c.C, c.D), p_chain=take("<f4", c.C),
                              flags=take("u1", k * c.C).reshape(k, c.C), p=take("<f4", 1)[0]))
        r = dict(calls=calls)
        st = int(take("<i4", 1)[0])
        r["stats"] = dict(status=st, rhat=take("<f4", c.D), max_rhat=take("<f4", 1)[0], p=take("<f4", 1)[0])
        st = int(take("<i4", 1)[0])
        r["cs"] = dict(status=st, rhat=take("<f4", c.D), max_rhat=take("<f4", 1)[0], p=take("<f4", 1)[0])
        st = int(take("<i4", 1)[0])
        r["wv"] = dict(status=st, within=take("<f4", c.D), var=take("<f4", c.D))
        r["n"] = int(take("<u8", 1)[0])
        out[c.name] = r
    assert pos == len(buf), "the probe wrote more than the cases account for"
    return out


@pytest.fixture(scope="module")
def probe_binaries(tmp_path_factory):
    """tests/hip/tracker_probe.hip compiled twice, side by side: as the library is, and with -DMMCMC_TUNING"""
    d = tmp_path_factory.mktemp("tracker_probe")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exes = {"default": str(d / "tracker_probe"), "tuning": str(d / "tracker_probe_tuning")}
    procs = {}
    for which, exe in exes.items():
        cmd = [hipcc] + PROBE_FLAGS + (["-DMMCMC_TUNING"] if which == "tuning" else []) + [PROBE_SRC, "-o", exe]
        procs[which] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    logs = {}
    for which, p in procs.items():
        try:
            logs[which] = (p.returncode, p.communicate(timeout=PROBE_BUILD_TIMEOUT_S)[0])
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
    for which, p in procs.items():
        assert p.returncode == 0, (which, logs[which][1][-3000:])
    return d, exes


def _run_probe(d, exe, tag, cases, extra_env):
    """one child process under its own time limit; any failure raises, and pytest then fails every test that depends on
    the (module-scoped) fixture without running it again"""
    cases_bin, out_bin = str(d / f"cases_{tag}.bin"), str(d / f"out_{tag}.bin")
    write_cases(cases_bin, cases)
    env = dict(os.environ)
    env.pop("MMCMC_TRACKER_ONE_WAVE", None)
    env.update(extra_env)
    r = subprocess.run([exe, cases_bin, out_bin], capture_output=True, text=True, timeout=PROBE_RUN_TIMEOUT_S, env=env)
    assert r.returncode == 0, f"tracker_probe ({tag}) ended with {r.returncode}: {r.stdout[-1000:]} {r.stderr[-3000:]}"
    return read_results(out_bin, cases)


@pytest.fixture(scope="module")
def probe(probe_binaries):
    d, exes = probe_binaries
    return _run_probe(d, exes["default"], "default", CASES, {})


@pytest.fixture(scope="module")
def probe_one_wave(probe_binaries, probe):
    """the -DMMCMC_TUNING build with MMCMC_TRACKER_ONE_WAVE=1 in the child's environment only; depends on `probe`, so it
    does not start after that one failed"""
    d, exes = probe_binaries
    return _run_probe(d, exes["tuning"], "one_wave", ONE_WAVE_CASES, {"MMCMC_TRACKER_ONE_WAVE": "1"})


def _assert_per_chain_state(got_calls, ref, what):
    assert len(got_calls) == len(ref["snaps"])
    for i, (got, snap, flags) in enumerate(zip(got_calls, ref["snaps"], ref["flags"])):
        for key in ("mean", "mean_sq", "last", "p_chain"):
            g, e = bits(got[key]), bits(snap[key])
            if not np.array_equal(g, e):
                bad = np.argwhere(g != e)
                raise AssertionError(f"{what}: {key} after call {i}: {len(bad)} of {e.size} differ, first at {bad[0].tolist()}: "
                                     f"{got[key][tuple(bad[0])]!r} != {snap[key][tuple(bad[0])]!r}")
        if not np.array_equal(got["flags"], flags):
            bad = np.argwhere(got["flags"] != flags)
            raise AssertionError(f"{what}: flags of call {i}: {len(bad)} of {flags.size} bytes differ, first at (row, chain) "
                                 f"{bad[0].tolist()}: {got['flags'][tuple(bad[0])]} != {flags[tuple(bad[0])]}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids)
def test_per_chain_state_and_flags_are_exact(probe, name):
    """(a) after every steps call: mean, mean of squares, last state and acceptance average of EVERY chain equal the
    reference's as bit patterns, and so do all k x C flag bytes of the call"""
    _assert_per_chain_state(probe[name]["calls"], reference(name), name)
    assert probe[name]["n"] == reference(name)["n"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids)
def test_p_accept_after_every_call(probe, name):
    """(b) p_accept equals the sequential fold over the whole history bit for bit after every call; in the two cases of
    the restart class (test_certificate_class_of_every_call) it is held to the 1e-6 of
    test_tracker_p_accept_when_the_certificate_fails"""
    case, ref = BY_NAME[name], reference(name)
    for i, (got, snap) in enumerate(zip(probe[name]["calls"], ref["snaps"])):
        print(name, i, ref["certs"][i]["cls"], repr(got["p"]), repr(snap["p"]))
        if case.restart_class:
            assert abs(float(got["p"]) - float(snap["p"])) < 1e-6, i
        else:
            assert bits(got["p"]) == bits(snap["p"]), (i, got["p"], snap["p"], ref["certs"][i])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids)
def test_aggregates_lie_in_the_reference_interval(probe, O, name):
    """(c) every R-hat, max_rhat, mean per-chain p_accept, within and var lies in the interval that one ulp on each
    rounded block sum spans around the exact-sum value -- and R-hat within the suite's 2e-5 of the oracle's, as in
    tests/test_tracker.py"""
    got, ref = probe[name], reference(name)
    if ref["n"] < 2:
        assert got["stats"]["status"] == got["cs"]["status"] == got["wv"]["status"] == ERR_STATE
        return
    assert got["stats"]["status"] == got["cs"]["status"] == got["wv"]["status"] == 0
    cs = ref["cs"]
    checks = [("rhat", got["stats"]["rhat"], ref["rhat"]), ("max_rhat", got["stats"]["max_rhat"], R.max_interval(ref["rhat"])),
              ("chain rhat", got["cs"]["rhat"], cs["rhat"]), ("chain max_rhat", got["cs"]["max_rhat"], R.max_interval(cs["rhat"])),
              ("mean p_chain", got["cs"]["p"], cs["p"]), ("within", got["wv"]["within"], cs["within"]), ("var", got["wv"]["var"], cs["var"])]
    for what, value, iv in checks:
        print(name, what, value, iv[1], iv[2])
        assert np.all(R.inside(value, iv)), (what, value, iv)
    assert bits(got["stats"]["p"]) == bits(got["calls"][-1]["p"])
    o = oracle_values(name)
    np.testing.assert_allclose(got["stats"]["rhat"], o["rhat_mc"], rtol=2e-5)
    np.testing.assert_allclose(got["cs"]["rhat"], o["rhat_cs"], rtol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ids)
def test_shipped_library_gives_the_probes_numbers(probe, name):
    """(d) the same calls through mini_mcmc_amd.stats.MultiChainTracker -- the loaded libmmcmc.so -- give rhat(), p_accept,
    chain_stats() and within_var() bit-equal to the probe's: the recompiled kernels are the shipped ones"""
    import torch

    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd import stats as S

    case, got = BY_NAME[name], probe[name]
    init, x = inputs(name)
    tr = S.MultiChainTracker(case.C, case.D)
    if case.init:
        tr.init_last(np.array(init))
    xh = np.array(x)
    xd = torch.as_tensor(xh, device="cuda") if any(dev for _, _, dev in case.calls) else None
    for t0, k, dev in case.calls:
        tr.step(xd if dev else xh, t0=t0, k=k)
    assert tr.n == got["n"]
    if got["n"] < 2:
        for fn in (tr.rhat, tr.chain_stats, tr.within_var):
            with pytest.raises(L.MmcmcError) as e:
                fn()
            assert e.value.status == L.ERR_STATE
        return
    rhat, mx, p = tr._stats()
    assert np.array_equal(bits(rhat), bits(got["stats"]["rhat"])) and bits(mx) == bits(got["stats"]["max_rhat"])
    assert bits(p) == bits(got["stats"]["p"]) and bits(tr.p_accept) == bits(p)
    rhat, mx, p = tr.chain_stats()
    assert np.array_equal(bits(rhat), bits(got["cs"]["rhat"])) and bits(mx) == bits(got["cs"]["max_rhat"])
    assert bits(p) == bits(got["cs"]["p"])
    w, v = tr.within_var()
    assert np.array_equal(bits(w), bits(got["wv"]["within"])) and np.array_equal(bits(v), bits(got["wv"]["var"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in ONE_WAVE_CASES])
def test_one_wave_kernel_gives_the_same_state(probe, probe_one_wave, name):
    """(e) tracker_step_tiled_kernel<T, D> for D > 1 (the tuning build's MMCMC_TRACKER_ONE_WAVE form): per-chain state and
    flags after every call equal the default binary's -- and the reference's -- bit for bit"""
    a, b = probe[name], probe_one_wave[name]
    for i, (ca, cb) in enumerate(zip(a["calls"], b["calls"])):
        for key in ("mean", "mean_sq", "last", "p_chain", "p"):
            assert np.array_equal(bits(ca[key]), bits(cb[key])), (key, i)
        assert np.array_equal(ca["flags"], cb["flags"]), i
    _assert_per_chain_state(b["calls"], reference(name), name + " (one wave)")


@pytest.mark.gpu
def test_same_states_fed_four_ways_end_in_the_same_state(probe):
    """one call, rows one at a time, uneven blocks from host memory, the same from device memory: identical per-chain state
    and p_accept after the last call"""
    for dt in ("f32", "f64"):
        ends = [probe[f"multi-{dt}-{how}"]["calls"][-1] for how in ("one", "rows", "uneven-host", "uneven-dev")]
        for other in ends[1:]:
            for key in ("mean", "mean_sq", "last", "p_chain", "p"):
                assert np.array_equal(bits(ends[0][key]), bits(other[key])), (dt, key)
        stats = [probe[f"multi-{dt}-{how}"] for how in ("one", "rows", "uneven-host", "uneven-dev")]
        for other in stats[1:]:
            assert np.array_equal(bits(stats[0]["stats"]["rhat"]), bits(other["stats"]["rhat"]))
            assert np.array_equal(bits(stats[0]["wv"]["var"]), bits(other["wv"]["var"]))

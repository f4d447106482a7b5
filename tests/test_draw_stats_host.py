"""NUTS's per-draw statistics without a GPU (include/mmcmc.h: "Per-draw sampler statistics").

  * tests/cpp/draw_stats_twin.cpp -- the host build of the kernels' own headers -- checks that the recording policy changes
    nothing, that every field of every record is what the tree holds, and divergence forced and absent (its head comment),
    as built and once more under the address and undefined-behaviour sanitizers (a stand-alone program: no preload involved);
  * the ABI: the new symbols are exported, bound and in the Rust -sys source, the two structs have the C compiler's layout
    in ctypes and in numpy, the version is 102, and every entry point answers a NULL handle and a machine without a device
    as the header says;
  * nuts.unpack_tree and the float64 restatement on hand-made records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import autodiff_common as A
import draw_stats_common as DS

NEW = ("mmcmc_nuts_set_draw_stats", "mmcmc_nuts_draw_stats_enabled", "mmcmc_nuts_draw_stats", "mmcmc_nuts_draw_summary",
       "mmcmc_nuts_group_set_draw_stats")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_twin_recorder_changes_nothing_records_are_right_divergence_forced_and_absent(tmp_path_factory, sanitize):
    exe = DS.build_twin(tmp_path_factory, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"checks (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    checks, failed = map(int, m.groups())
    assert failed == 0
    # not vacuous.  Per (type mode, metric): 7 checks on each of 240 transitions of a checked run; per n_discard two walks, each
    # one checked run + 2 checks (+ 8 rows 0 without burn-in), then 2 checks; one more checked run under a depth cap of 2 + 1
    per_run = 7 * 240
    per_case = (2 * (per_run + 2 + 8) + 2) + (2 * (per_run + 2) + 2) + (per_run + 1)
    assert checks == 3 * 3 * per_case + 3 * 5


def test_twin_dump_is_what_its_checks_saw(tmp_path_factory):
    """the reference the GPU tests read: shapes, the no-transition row, and the integer fields against the run's own totals"""
    for mode in (0, 1, 2):
        s, x, ad, nlf, hist, rec = DS.twin_nuts(tmp_path_factory, mode, 96, 10, 0, False, 13)
        assert rec.shape == (96, 10) and np.all(rec["tree"][:, 0] == DS.NONE) and np.all(np.isnan(rec["energy"][:, 0]))
        assert np.all(rec["step_size"][:, 0] > 0) and np.all(rec["tree"][:, 1:] >> np.uint32(31) == 0)
        assert np.array_equal((rec["tree"][:, 1:] & np.uint32(0xFFFF)).sum(axis=1).astype(np.uint64), nlf)
        depth = (rec["tree"][:, 1:] >> np.uint32(16)) & np.uint32(15)
        assert np.array_equal(np.bincount(depth.ravel(), minlength=13).astype(np.uint32), hist)
    forced = DS.twin_gauss(tmp_path_factory, 0, 96, 20, 64.0, 7)
    absent = DS.twin_gauss(tmp_path_factory, 0, 96, 20, 0.1, 7)
    assert np.all(forced[5]["tree"][:, 1:] == np.uint32((1 << 24) | (1 << 16) | 1)) and np.all(forced[0] == forced[0][:, :1])
    assert np.all((absent[5]["tree"] & DS.DIVERGENT) == 0) and not np.all(absent[0] == absent[0][:, :1])


def test_new_symbols_are_exported_bound_and_in_the_rust_sys_source():
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    sys_rs = open(os.path.join(DS.ROOT, "rust", "mini-mcmc-hip-sys", "src", "lib.rs")).read()
    header = open(os.path.join(DS.ROOT, "include", "mmcmc.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), name
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    for struct in ("mmcmc_nuts_draw", "mmcmc_nuts_chain_summary"):
        assert "pub struct %s " % struct in sys_rs and "size_of::<%s>()" % struct in sys_rs
    assert lib.mmcmc_version() == 102 and "#define MMCMC_VERSION 102" in header


def test_struct_layouts_are_the_c_compilers(tmp_path):
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.nuts import DRAW_DTYPE

    fields = {"mmcmc_nuts_draw": [f for f, _ in L.NutsDraw._fields_], "mmcmc_nuts_chain_summary": [f for f, _ in L.NutsChainSummary._fields_]}
    src = ['#include <stddef.h>\n#include <stdio.h>\n#include "mmcmc.h"\nint main(void) {']
    for s, fs in fields.items():
        src.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f in fs:
            src.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(DS.ROOT, "include"), str(c), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["mmcmc_nuts_draw"]) == 16 == C.sizeof(L.NutsDraw) == DRAW_DTYPE.itemsize == DS.DRAW.itemsize
    assert int(got["mmcmc_nuts_chain_summary"]) == C.sizeof(L.NutsChainSummary) == 48
    for s, cls in (("mmcmc_nuts_draw", L.NutsDraw), ("mmcmc_nuts_chain_summary", L.NutsChainSummary)):
        for f in fields[s]:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    for f in fields["mmcmc_nuts_draw"]:
        assert DRAW_DTYPE.fields[f][1] == int(got[f"mmcmc_nuts_draw.{f}"])


def test_entry_points_without_a_handle_and_without_a_device():
    import torch

    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    n = C.c_size_t(0)
    rec = np.zeros((2, 3), dtype=DS.DRAW)
    out = (L.NutsChainSummary * 2)()
    assert lib.mmcmc_nuts_set_draw_stats(None, 1) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_draw_stats_enabled(None) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_draw_stats(None, None, 0, C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_group_set_draw_stats(None, 1) == L.ERR_INVALID_ARG
    p = C.c_void_p(rec.ctypes.data)
    assert lib.mmcmc_nuts_draw_summary(p, 0, 2, 3, 0, None) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_draw_summary(None, 0, 2, 3, 0, out) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_draw_summary(p, 0, 0, 3, 0, out) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_draw_summary(C.c_void_p(rec.ctypes.data + 4), 1, 2, 3, 0, out) == L.ERR_INVALID_ARG  # a device pointer off 16 bytes
    if not torch.cuda.is_available():
        assert lib.mmcmc_nuts_draw_summary(p, 0, 2, 3, 0, out) == L.ERR_NO_DEVICE  # no CPU fallback


def test_unpack_tree_and_the_float64_restatement_on_hand_made_records():
    from mini_mcmc_amd.nuts import DRAW_DTYPE, unpack_tree

    tree = np.array([[1 << 31, 7 | (3 << 16), 1 | (1 << 16) | (1 << 24)], [4095 | (12 << 16) | (1 << 25), 3 | (2 << 16), 15 | (4 << 16)]], dtype=np.uint32)
    n_lf, depth, div, cap, tr = unpack_tree(tree)
    assert n_lf.tolist() == [[0, 7, 1], [4095, 3, 15]] and depth.tolist() == [[0, 3, 1], [12, 2, 4]]
    assert div.tolist() == [[False, False, True], [False, False, False]] and cap.tolist() == [[False, False, False], [True, False, False]]
    assert tr.tolist() == [[False, True, True], [True, True, True]]
    rec = np.zeros((2, 3), dtype=DRAW_DTYPE)
    rec["tree"] = tree
    rec["energy"] = [[np.nan, 1.0, 3.0], [2.0, 2.0, 5.0]]
    rec["accept_stat"] = [[np.nan, 0.5, 1.0], [0.25, 0.5, 0.75]]
    rec["step_size"] = 0.5
    s = DS.summary_f64(rec)
    assert s["n_transitions"].tolist() == [2, 3] and s["n_divergent"].tolist() == [1, 0] and s["n_depth_cap"].tolist() == [0, 1]
    assert s["max_depth_seen"].tolist() == [3, 12] and s["n_leapfrog"].tolist() == [8, 4113]
    assert s["mean_accept"].tolist() == [0.75, 0.5] and s["mean_step"].tolist() == [0.5, 0.5]
    assert s["ebfmi"].tolist() == [4.0 / 2.0, 9.0 / 6.0]  # (3 - 1)^2 / (1 + 1); (0 + 9) / (1 + 1 + 4)

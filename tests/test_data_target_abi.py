"""The C ABI of targets that carry data (include/mmcmc.h: mmcmc_target_register_data_source, mmcmc_target_data_len), as far as it
goes without a GPU: the symbols are declared, exported and bound, the version and the description's layout are what they were,
the argument checks and the data length of kinds that have none."""
import ctypes as C
import os
import re

import pytest

import data_common as D

NEW = ("mmcmc_target_register_data_source", "mmcmc_target_data_len")


@pytest.fixture(scope="module")
def lib():
    import mini_mcmc_amd

    return mini_mcmc_amd.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from mini_mcmc_amd import _lib as L

    header = open(os.path.join(D.ROOT, "include", "mmcmc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert re.search(r"#define\s+MMCMC_SOURCE_LOGP_GRAD\s+0\b", code) and re.search(r"#define\s+MMCMC_SOURCE_LOGP\s+1\b", code)
    assert "beyond data_len is the caller's fault" in header
    assert lib.mmcmc_version() == 102  # additive entry points do not bump it
    assert C.sizeof(L.TargetDesc) == 80
    for binding in ("include/mmcmc.hpp", "rust/mini-mcmc-hip-sys/src/lib.rs", "rust/mini-mcmc-hip/src/lib.rs"):
        text = open(os.path.join(D.ROOT, binding)).read()
        assert "mmcmc_target_register_data_source" in text, binding


def test_data_len_of_kinds_without_data(lib):
    from mini_mcmc_amd import _lib as L

    n = C.c_size_t(123)
    for kind in range(0, L.GAUSSIAN_ND + 1):  # every built-in kind: 0
        n.value = 123
        assert lib.mmcmc_target_data_len(kind, C.byref(n)) == L.OK and n.value == 0
    for kind in (-1, L.GAUSSIAN_ND + 1, 999, 1000 + (1 << 20)):  # nobody registered these
        n.value = 123
        assert lib.mmcmc_target_data_len(kind, C.byref(n)) == L.ERR_INVALID_ARG and n.value == 0
    assert lib.mmcmc_target_data_len(0, None) == L.ERR_INVALID_ARG


def test_registration_status_codes(lib):
    import torch

    from mini_mcmc_amd import _lib as L

    reg = lib.mmcmc_target_register_data_source
    src = D.source("linreg3", "logp").encode()
    kind = C.c_int()
    assert reg(None, 3, 28, 1, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert reg(b"d", 3, 28, 1, None, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert reg(b"d", 3, 28, 1, src, None, None, 0) == L.ERR_INVALID_ARG
    for dim in (0, -1, 33):
        assert reg(b"d", dim, 28, 1, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    assert reg(b"d", 3, 0, 1, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG  # no data
    for flavour in (-1, 2):
        assert reg(b"d", 3, 28, flavour, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    for huge in ((1 << 61), (1 << 64) - 1):  # 8 * data_len does not fit size_t
        assert reg(b"d", 3, huge, 1, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG
    if not torch.cuda.is_available():
        # without a device: what mmcmc_target_register_source returns on this machine
        log = C.create_string_buffer(256)
        plain = lib.mmcmc_target_register_source(b"p", 3, D.source("linreg3", "hand").encode(), C.byref(kind), log, 256)
        assert plain == L.ERR_NO_DEVICE
        for flavour, which in ((0, "hand"), (1, "logp")):
            assert reg(b"d", 3, 28, flavour, D.source("linreg3", which).encode(), C.byref(kind), log, 256) == plain
        from mini_mcmc_amd.distributions import AutodiffTarget

        with pytest.raises(L.MmcmcError) as e:
            AutodiffTarget("linreg3", 3, D.source("linreg3", "logp"), params=D.LINREG3_PARAMS, data=D.LINREG3)
        assert e.value.status == plain


def test_matrix_and_data_together_are_refused_before_anything_is_compiled():
    import numpy as np

    from mini_mcmc_amd.distributions import AutodiffTarget, UserTarget

    for cls, which in ((UserTarget, "hand"), (AutodiffTarget, "logp")):
        with pytest.raises(ValueError):
            cls("both", 3, D.source("linreg3", which), matrix=np.eye(3), data=D.LINREG3)

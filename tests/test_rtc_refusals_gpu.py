"""What the run-time compiled unit kinds refuse (csrc/mm_rtc.hip, the predicates of csrc/mm_rtc_units.h), by status: a model, and
a unit the library built for itself, carries no functor source to compile a proposal with; a proposal's dimension is its
target's; an internal unit has no data length to report and is not a kind a description may name.  The units are made from
the banana of tests/test_user_target.py (dim 2) and one 64-chain HMC handle over it, whose first metric builds the metric unit."""
import ctypes as C

import numpy as np
import pytest

import autodiff_common as A
import test_user_proposal as TP
import test_user_target as TU


def _top_kind(lib, first):
    """the last kind handed out: kinds are consecutive, and mmcmc_rtc_unit_compiler knows exactly the registered ones"""
    k = first
    while lib.mmcmc_rtc_unit_compiler(k + 1) > 0:
        k += 1
    return k


@pytest.mark.gpu
def test_unit_kinds_refuse_what_they_are_not():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import UserProposal, UserTarget
    from mini_mcmc_amd.hmc import HMC

    lib = L.lib()
    banana = UserTarget("refusal_banana", 2, TU.BANANA, params=A.BANANA_PARAMS)
    model = UserProposal("refusal_model", banana, TP.ISOTROPIC, 1.0)
    init = init_with_seed(64, 2, 7, np.float32)
    hmc = HMC(banana, init, 0.1, 3)
    before = _top_kind(lib, banana.kind)
    hmc.metric = [1.0, 2.0]  # the first metric of this kind: builds and registers its metric unit
    metric_unit = _top_kind(lib, before)
    assert metric_unit > before >= model.kind > banana.kind

    kind, src = C.c_int(-7), TP.ISOTROPIC.encode()

    def register_proposal(target_kind, dim):
        return lib.mmcmc_proposal_register_source(b"refused", target_kind, dim, src, C.byref(kind), None, 0)

    assert register_proposal(model.kind, 2) == L.ERR_UNSUPPORTED
    assert register_proposal(metric_unit, 2) == L.ERR_UNSUPPORTED
    assert register_proposal(banana.kind, 3) == L.ERR_SHAPE
    assert kind.value == -7  # nothing was handed out
    n = C.c_size_t(99)
    assert lib.mmcmc_target_data_len(metric_unit, C.byref(n)) == L.ERR_INVALID_ARG and n.value == 0
    assert lib.mmcmc_target_data_len(model.kind, C.byref(n)) == L.OK and n.value == 0
    d = banana.desc()
    d.kind = metric_unit
    h = C.c_void_p()
    st = lib.mmcmc_hmc_create(C.byref(h), C.byref(d), init.ctypes.data, 64, 0.1, 3, L.F32, 0)
    assert st == L.ERR_UNSUPPORTED and not h.value  # a unit the library built for itself is not a kind a caller may name

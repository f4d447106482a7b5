"""Offline code generation for log-densities that read a bound array (csrc/mm_data.h), no GPU needed: with
`hipcc --genco -O3 -ffp-contract=off --offload-arch=gfx950` (tools/autodiff_codegen.py) the batch-gradient kernel around the
autodiff bodies of logit9 and linreg3 (tests/cpp/data_cases/) keeps its dual numbers in registers in f32 and f64 -- the
code object's metadata says .private_segment_fixed_size 0 and no spilled register -- although the loop over the observations
is rolled and only the loops over the coordinates are unrolled: the combination a likelihood over data has."""
import os
import sys

import pytest

import data_common as D


@pytest.mark.parametrize("model", ["logit9", "linreg3"])
def test_batch_gradient_kernel_over_a_bound_array_uses_no_scratch_memory(model):
    sys.path.insert(0, os.path.join(D.ROOT, "tools"))
    import autodiff_codegen

    if autodiff_codegen.tools() is None:
        # a machine without ROCm cannot build the library either; where ROCm is installed the check must run
        assert not os.path.isdir("/opt/rocm"), "ROCm is installed but hipcc or llvm-readelf was not found"
        pytest.skip("no ROCm installation: neither hipcc nor llvm-readelf")
    dim = D.MODELS[model][0]
    body = os.path.join(D.CASES, model + "_logp.inc")
    text = open(body).read()
    assert "for (int r = 0; r < rows; ++r)" in text and "MM_UNROLL\n        for (int r" not in text  # the rows' loop is rolled
    md = autodiff_codegen.kernel_metadata(dim, body=body, header="mm_data.h")
    assert set(md) == {"ad_logp_grad_f32", "ad_logp_grad_f64"}
    for name, fields in md.items():
        print(model, name, fields)
        assert fields[".private_segment_fixed_size"] == 0, (model, name, fields)
        assert fields[".vgpr_spill_count"] == 0 and fields[".sgpr_spill_count"] == 0, (model, name, fields)

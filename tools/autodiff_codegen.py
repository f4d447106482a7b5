"""Register use of the forward-mode gradient (csrc/mm_autodiff.h) from a code object's metadata, no GPU needed:
    python tools/autodiff_codegen.py [dim ...]        (default: 3 8 9 32)
compiles, with `hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off`, a stand-alone batch log-density / gradient kernel
(the one mm_rtc.hip generates for a registered target) around the RosenbrockND log-density written over a scalar type
(tests/cpp/autodiff_cases/rosenbrock.inc), for f32 and f64, and prints one JSON line per kernel with the fields of the
metadata note: .private_segment_fixed_size (scratch bytes per lane: 0 = the dual numbers stay in registers),
.vgpr_count, .sgpr_count, .vgpr_spill_count.  tests/test_autodiff_host.py asserts the first at dims 3 and 8."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_mcmc_amd", "csrc")
BODY = os.path.join(ROOT, "tests", "cpp", "autodiff_cases", "rosenbrock.inc")

KERNEL = r"""
#include <hip/hip_runtime.h>
#include "%(header)s"
%(body)s
template <class T> __device__ __forceinline__ void batch(const mm_tparams<T> &P, const T *x, T *logp, T *grad, unsigned long long n)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T xv[MM_USER_DIM], gv[MM_USER_DIM];
    for (int k = 0; k < MM_USER_DIM; ++k) xv[k] = x[i * MM_USER_DIM + k];
    logp[i] = mm_ad_logp_grad<T, mmcmc_user_logp<T>>(P, xv, gv);
    for (int k = 0; k < MM_USER_DIM; ++k) grad[i * MM_USER_DIM + k] = gv[k];
}
extern "C" __global__ void ad_logp_grad_f32(const mm_tparams<float> P, const float *x, float *logp, float *grad, unsigned long long n) { batch<float>(P, x, logp, grad, n); }
extern "C" __global__ void ad_logp_grad_f64(const mm_tparams<double> P, const double *x, double *logp, double *grad, unsigned long long n) { batch<double>(P, x, logp, grad, n); }
"""

FIELDS = (".private_segment_fixed_size", ".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count")


def tools():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    readelf = os.path.join(os.path.dirname(isa_mix.OBJDUMP), "llvm-readelf")
    return (hipcc, readelf) if os.path.exists(hipcc) and os.path.exists(readelf) else None


def kernel_metadata(dim: int, body: str = BODY, header: str = "mm_autodiff.h") -> dict:
    """{kernel name: {field: int}} for the batch kernels at `dim` around the log-density in the file `body` (default: RosenbrockND;
    a body that reads a bound array needs header="mm_data.h": tests/test_data_target_codegen.py)."""
    hipcc, readelf = tools()
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "unit.hip"), os.path.join(d, "unit.hsaco")
        with open(src, "w") as f:
            f.write(KERNEL % {"body": open(body).read(), "header": header})
        subprocess.run([hipcc, "--genco", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", f"-DMM_USER_DIM={dim}",
                        "-Wno-pass-failed", "-I" + CSRC, "-o", out, src], check=True, capture_output=True, text=True)
        notes = ""
        for n, co in enumerate(isa_mix.code_objects(out)):  # --genco writes an offload bundle: unwrap the gfx950 code object
            elf = os.path.join(d, f"unit{n}.co")
            with open(elf, "wb") as f:
                f.write(co)
            notes += subprocess.run([readelf, "--notes", elf], check=True, capture_output=True, text=True).stdout
    res = {}
    # one map per kernel under amdhsa.kernels; every map names its kernel descriptor once (.symbol: <name>.kd), so the text between
    # two list items that holds a .symbol is one kernel's map, whatever the order of its keys
    for entry in re.split(r"(?m)^\s*- (?=\.\w+:)", notes):
        m = re.search(r"\.symbol:\s+'?(\w+)\.kd", entry)
        if m:
            res[m.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in FIELDS}
    assert sorted(res) == ["ad_logp_grad_f32", "ad_logp_grad_f64"], sorted(res)
    return res


if __name__ == "__main__":
    for dim in [int(a) for a in sys.argv[1:]] or [3, 8, 9, 32]:
        for name, md in sorted(kernel_metadata(dim).items()):
            print(json.dumps({"dim": dim, "kernel": name, **md}))

"""Shared by tests/test_rtc_units_host.py and the recorder tools/experiments/rtc_record_units.py: the functor texts the unit
texts of tests/golden/rtc_unit_texts.json are made from, and how a directory of unit texts is summarised (byte length, sha256,
the ordered extern "C" kernel names).  The texts are the ones the GPU tests register."""
import hashlib
import os
import re

import autodiff_common as A
import data_common as D
import test_user_proposal as TP
import test_user_target as TU

ROOT = A.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "rtc_unit_texts.json")
LINREG3_DATA_LEN = D.LINREG3.size  # 28


def functors():
    """file name -> text, as the callers hand them to the mmcmc_*_register_* entry points"""
    return {
        "banana": TU.BANANA,                            # hand gradient, dim 2
        "banana_logp": A.case_source("banana")[0],      # log-density alone, dim 2
        "linreg3_hand": D.source("linreg3", "hand"),    # data kind, MMCMC_SOURCE_LOGP_GRAD, dim 3
        "linreg3_logp": D.source("linreg3", "logp"),    # data kind, MMCMC_SOURCE_LOGP
        "isotropic": TP.ISOTROPIC,                      # a proposal
        "poisson_reflect": TP.POISSON_REFLECT,          # an integer-state model
    }


def write_functors(out_dir):
    for name, text in functors().items():
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write(text)


def summarise(unit_dir):
    """{case: {"bytes", "sha256", "kernels"}} of every <case>.hip in unit_dir"""
    res = {}
    for fn in sorted(os.listdir(unit_dir)):
        if fn.endswith(".hip"):
            raw = open(os.path.join(unit_dir, fn), "rb").read()
            res[fn[:-4]] = {"bytes": len(raw), "sha256": hashlib.sha256(raw).hexdigest(),
                            "kernels": re.findall(r'extern "C" __global__ (?:__launch_bounds__\(\d+\) )?void (\w+)\(', raw.decode())}
    return res

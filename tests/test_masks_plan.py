"""CPU: the per-stripe plan of ecamd_rs_decode_masks (csrc/hip/ecamd_masks_plan.hpp -- the very text
masks_plan_kernel runs on the device) through the stand-alone tests/c/masks_plan.cpp, built with g++
-fsanitize=address,undefined together with the host planning sources.  The record must equal what
ecamd_rs_decode_map returns for the ascending list of the mask -- inputs, outputs, coefficients -- for both
values of rebuild_parity: every pattern of (10,4) and (4,2); for (20,8) every pattern of at most two lost,
both C5 patterns and 2000 seeded patterns of 3-8 lost; 500 seeded patterns of (24,8); and a mask with a bit
>= k+m or more than m bits must read unrecoverable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liberasurecode_amd", "csrc")
HOST_SRC = ["gf16.cpp", "tables.cpp", "xor_plan.cpp", "crc.cpp", "bitslice.cpp", "host_api.cpp", "copy_pool.cpp"]


# compiled in the build container only, as test_tune_rules: nothing is compiled inside a GPU run
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="compiles: build container only")
def test_masks_plan(tmp_path):
    exe = str(tmp_path / "masks_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"),
                    "-I" + os.path.join(CSRC, "hip"), "-o", exe, os.path.join(ROOT, "tests", "c", "masks_plan.cpp"),
                    *[os.path.join(CSRC, "host", s) for s in HOST_SRC], "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "masks_plan: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

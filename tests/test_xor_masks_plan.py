"""CPU: the decode table of ecamd_xor_decode_masks (ecamd_xor_decode_masks_plan in host_api.cpp, and the entry
and rank of csrc/hip/ecamd_xor_masks_plan.hpp -- the very text xor_decode_masks_kernel runs on the device)
through the stand-alone tests/c/xor_masks_plan.cpp, built with g++ -fsanitize=address,undefined together
with the host planning sources.  For all 38 codes: the entry count is the sum of C(k+m, t) over t < hd; the
rank is a bijection of the recoverable masks onto [0, count); every entry is ecamd_xor_plan's decode_parity
1 plan with the lost bits dropped, its data rows the decode_parity 0 plan unchanged; every list of exactly
hd fragments is refused by the plan, and every mask of hd or more bits or with a bit >= k+m ranks
unrecoverable.  24229 patterns in all."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liberasurecode_amd", "csrc")
HOST_SRC = ["gf16.cpp", "tables.cpp", "xor_plan.cpp", "crc.cpp", "bitslice.cpp", "host_api.cpp", "copy_pool.cpp"]


# compiled in the build container only, as test_masks_plan: nothing is compiled inside a GPU run
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="compiles: build container only")
def test_xor_masks_plan(tmp_path):
    exe = str(tmp_path / "xor_masks_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"),
                    "-I" + os.path.join(CSRC, "hip"), "-o", exe, os.path.join(ROOT, "tests", "c", "xor_masks_plan.cpp"),
                    *[os.path.join(CSRC, "host", s) for s in HOST_SRC], "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "xor_masks_plan: ok (38 codes, 24229 patterns" in r.stdout, (r.stdout + r.stderr)[-3000:]

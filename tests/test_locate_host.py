"""CPU: ecamd_rs_locate_map (include/ecamd_host.h) through the stand-alone tests/c/locate_map_test.cpp,
compiled together with the host planning sources, plain and with -fsanitize=address,undefined: the
planner writes exactly the buffers the header promises, and its ratios single out every corrupted
fragment."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liberasurecode_amd", "csrc")
HOST_SRC = ["gf16.cpp", "tables.cpp", "xor_plan.cpp", "crc.cpp", "bitslice.cpp", "host_api.cpp", "copy_pool.cpp"]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_locate_map(tmp_path, flags):
    exe = str(tmp_path / "locate_map_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", *flags,
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"),
                    "-I" + os.path.join(CSRC, "hip"), "-o", exe,
                    os.path.join(ROOT, "tests", "c", "locate_map_test.cpp"),
                    *[os.path.join(CSRC, "host", s) for s in HOST_SRC], "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "locate_map: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

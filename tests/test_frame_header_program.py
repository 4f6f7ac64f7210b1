"""CPU: the shared header text (csrc/hip/ecamd_frame_header.hpp -- the very text crc_finalize_kernel and the
stamp kernel of ecamd_frame_reconstruct_masks run on the device) through the stand-alone
tests/c/frame_header.cpp, built with g++ -fsanitize=address,undefined together with the host planning
sources.  Every header (both backends, both checksum machines, checksum types 1/2/3, small and > 4 GiB
objects) equals one packed field by field from the wire format with a bit-by-bit CRC; the helper that picks
item j's fragment from a stripe's mask equals a bit-by-bit walk for every j over every 16-bit mask and a
sweep of wide ones, bits at and past k + m included."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "liberasurecode_amd", "csrc")
HOST_SRC = ["gf16.cpp", "tables.cpp", "xor_plan.cpp", "crc.cpp", "bitslice.cpp", "host_api.cpp", "copy_pool.cpp"]


# compiled in the build container only, as test_xor_masks_plan: nothing is compiled inside a GPU run
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="compiles: build container only")
def test_frame_header_program(tmp_path):
    exe = str(tmp_path / "frame_header")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "host"),
                    "-I" + os.path.join(CSRC, "hip"), "-o", exe, os.path.join(ROOT, "tests", "c", "frame_header.cpp"),
                    *[os.path.join(CSRC, "host", s) for s in HOST_SRC], "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "frame_header: ok (2304 headers, " in r.stdout, (r.stdout + r.stderr)[-3000:]

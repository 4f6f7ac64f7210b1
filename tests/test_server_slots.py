"""CPU: the resident small server's slot decision (csrc/hip/ecamd_server_slots.hpp: which of its two cached
argument slots a request takes, and whether the block -- and with it the staged coefficient tables -- is
rewritten) through the stand-alone tests/c/server_slots_test.cpp, built plain and with
-fsanitize=address,undefined.  This is the deterministic check that a map is identified by its serial and not
by its tables' device address: it does not depend on what the device allocator hands back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_server_slots(tmp_path, flags):
    exe = str(tmp_path / "server_slots_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I" + os.path.join(ROOT, "liberasurecode_amd", "csrc", "hip"), "-o", exe,
                    os.path.join(ROOT, "tests", "c", "server_slots_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "server_slots: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

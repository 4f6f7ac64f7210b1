"""CPU: every ecamd_tune() knob's default and normalising rule (csrc/host/tune_knobs.def, the table in
host/tune.cpp) against tests/golden/tune_rules.json, through the stand-alone tests/c/tune_rules.cpp built with
-fsanitize=address,undefined; also the table's integrity and the $ECAMD_TUNE parser.

Every knob setting gives bit-identical output, so no GPU test can see a wrong rule or default: it would only
falsify the next A/B.  The fixture was recorded once from the hand-written setter chain the table replaced (its
`struct Tuning` and `ecamd_tune` text compiled stand-alone): per knob, starting from a freshly constructed
state, 45 values from INT_MIN to INT_MAX applied in order, with the return code and the stored value after each.
A new knob, or a default or rule changed on purpose, updates the fixture in the same commit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liberasurecode_amd", "csrc", "host")


# compiled in the build container only, as conftest's _built: nothing is compiled inside a GPU run
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="compiles: build container only")
def test_tune_rules(tmp_path):
    exe = str(tmp_path / "tune_rules")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-I" + HOST, "-o", exe,
                    os.path.join(ROOT, "tests", "c", "tune_rules.cpp"), os.path.join(HOST, "tune.cpp")], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "tune_rules.json")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0 and "tune_rules: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

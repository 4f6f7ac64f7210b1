"""GPU: EVERY bitsliced code object build() ships in lib/jit/ executes and is byte-checked against the
reference codec -- all 1,470 1- to 4-loss decodes of RS(10,4), every single-loss decode and reconstruct
of (10,4), (4,2) and (20,8), and the benched maps (liberasurecode_amd/prebuild.py all_ops(full=True)).

Each case runs tests/shipped_objects_run.py on one slice of the op list in a FRESH process with an empty
$ECAMD_JIT_CACHE and the default knob (bitslice 1: never waits for a compile), so whatever runs bitsliced
was loaded from lib/jit/ under the run time's own key.  Per op: ecamd_rs_kernel_form answers BITSLICED
(TABLES for the maps that take the LDS tables by shape), the launch counter rises, the outputs' SHA-256
equals the digest the reference produced (tests/golden/rs_shipped.json) and no other fragment changes.
Fragments are two tiles and a 48-byte tail in 3 stripes.  Then 16 patterns at a time go interleaved
through one rs_decode_multi call, and slices longer than the 256-entry kernel cache run their first ops
again after eviction."""
import json
import os
import subprocess
import sys

import pytest

import shipped_ops as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLICES = ["A", "loss2", "loss3", "loss4_0", "loss4_1", "loss4_2"]


@pytest.mark.parametrize("name", SLICES)
def test_every_shipped_object_runs_and_matches_the_reference(tmp_path, name):
    ops = so.ops()
    indices = so.slices(ops)[name]
    cache = tmp_path / "jitcache"
    cache.mkdir(mode=0o700)
    env = dict(os.environ, ECAMD_JIT_CACHE=str(cache))
    env.pop("LIBERASURECODE_AMD_LIBDIR", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "shipped_objects_run.py"), name], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(name, {k: v for k, v in out.items() if k != "mismatches"})
    assert out["mismatches"] == [], out["mismatches"]
    expected = sum(so.expected_bitsliced(ops[i]) for i in indices)
    assert out["ops"] == len(indices) and out["bitsliced"] == expected == out["expected_bitsliced"], out
    decodes = sum(so.is_decode_10_4(ops[i]) for i in indices)
    assert out["multi_runs"] == decodes // 16, out
    assert out["entries"] <= 256, out
    if len(indices) > 256:
        assert out["rerun"] == 8 and out["rerun_bitsliced"] == 8, out
    if name != "A":  # nothing but (10,4) decodes: every op bitsliced
        assert expected == len(indices)


def test_slices_cover_every_shipped_op():
    ops = so.ops()
    part = so.slices(ops)
    assert sorted(part) == sorted(SLICES)
    assert sum(len(v) for v in part.values()) == len(ops)
    expected = [i for i in range(len(ops)) if so.expected_bitsliced(ops[i])]
    assert len(expected) >= 1470 + 14 + 56
    assert sum(so.is_decode_10_4(ops[i]) for i in expected) == 1470

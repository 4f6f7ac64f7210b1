"""CPU: the option bits of the plain one-wave bitsliced kernel (csrc/host/bitslice.cpp, BitsliceStyle::opts:
write-through output stores, the timeline form) -- their compile requests, their cache names and what the
compiler makes of their source for the C3 encode and decode {0,1,2,3} maps.

A request without option bits must stay what it was before they existed: its text, and with it the name of
its code object (tests/golden/launch_forms.json holds both, recorded from the commit before them), so
shipped and cached objects of every other form keep being found.

The golden names hash the generator's fingerprint (the source it emits for a set of tiny maps, hip/ecamd_jit.hip
generator_fingerprint), so a change that alters any form's emitted source on purpose renames every object and
fails the name comparison here while the cache works as designed.  Then check that the REQUEST texts still
match (they do not depend on the generator), rebuild, and record the names anew with
`PYTHONPATH=. python3 tests/test_bitslice_launch_forms.py > tests/golden/launch_forms.json` (repository root)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import shipped_ops as so
from liberasurecode_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_forms.json")
HIPCC = "/opt/rocm/bin/hipcc"
CAPS = (96, 64, 40, 16)  # kCaps, hip/ecamd_jit.hip
THROUGH, TIMELINE = 1, 2  # kBsOpt*, host/bitslice.hpp
MAPS = {"encode": (10, 4, None, -1, 1), "decode0123": (10, 4, [0, 1, 2, 3], -1, 1)}


def coeff_of(name):
    inputs, rows = so.plan(MAPS[name])
    return [c for row in rows for c in row], len(rows), len(inputs)


def request(coeff, R, K, cap, opts):
    h = _lib.host()
    n = h.ecamd_bitslice_wave_request(_lib.ints(coeff), R, K, cap, opts, None, 0)
    assert n > 0
    buf = C.create_string_buffer(n + 1)
    h.ecamd_bitslice_wave_request(_lib.ints(coeff), R, K, cap, opts, buf, n + 1)
    return buf.value


def source(req):
    h = _lib.host()
    n = h.ecamd_bitslice_request_source(req, None, 0)
    assert n > 0
    buf = C.create_string_buffer(n + 1)
    h.ecamd_bitslice_request_source(req, buf, n + 1)
    return buf.value.decode()


def object_name(req):
    buf = C.create_string_buffer(64)
    assert _lib.dev().ecamd_bitslice_object_name(req, b"gfx950", buf, 64) > 0
    return buf.value.decode()


def compiled(tmp_path, tag, src):
    """(VGPRs, scratch bytes, assembly) of ecamd_bs_kernel built from src for gfx950."""
    hip = tmp_path / f"{tag}.hip"
    hip.write_text("#include <hip/hip_runtime.h>\n" + src)
    asm = tmp_path / f"{tag}.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", str(asm),
                        str(hip)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    text = asm.read_text()
    vgprs = int(re.search(r"; NumVgprs: (\d+)", text).group(1))
    scratch = int(re.search(r"; ScratchSize: (\d+)", text).group(1))
    return vgprs, scratch, text


@pytest.mark.parametrize("name", sorted(MAPS))
def test_request_round_trip_and_old_requests_unchanged(name):
    coeff, R, K = coeff_of(name)
    h = _lib.host()
    with open(GOLDEN) as f:
        gold = json.load(f)[name]
    plain = request(coeff, R, K, 96, 0)
    assert plain.decode() == gold["request"]
    assert object_name(plain) == gold["object"]
    assert h.ecamd_bitslice_request_opts(plain) == 0
    assert b"opts" not in plain
    names = {object_name(plain)}
    for bits in (THROUGH, TIMELINE, THROUGH | TIMELINE):
        req = request(coeff, R, K, 96, bits)
        assert h.ecamd_bitslice_request_opts(req) == bits
        assert req == plain + b"opts %d\n" % bits
        names.add(object_name(req))
    assert len(names) == 4
    # the word belongs to the plain one-wave register form alone, with bits that exist, and ends the request
    head, rest = plain.split(b"\n", 2)[1], plain.split(b"\n", 2)[2]
    R_, K_, cap_, depth_, flags = (int(x) for x in head.split())
    for bad in (plain + b"opts 0\n", plain + b"opts 4\n", plain + b"opts\n", plain + b"opts 1\ncheck\n",
                plain + b"check\nopts 1\n",
                b"ecamd-bitslice-request 2\n%d %d %d 0 %d\n" % (R_, K_, cap_, flags & ~64) + rest + b"opts 1\n",
                b"ecamd-bitslice-request 2\n%d %d %d 2 %d\n" % (R_, K_, cap_, flags) + rest + b"opts 1\n"):
        assert h.ecamd_bitslice_request_opts(bad) == -1, bad[-40:]


def test_source_without_option_bits_is_the_plain_form():
    coeff, R, K = coeff_of("encode")
    src = source(request(coeff, R, K, 96, 0))
    for word in ("tl_records", "s_memrealtime", "s_getreg"):
        assert word not in src, word
    assert src.count(", 0, 2);") > 0 and ", 0, 19);" not in src


@pytest.mark.skipif(not shutil.which(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(MAPS))
def test_option_forms_compile_in_the_plain_forms_registers(tmp_path, name):
    """Each form at the cap the plain form ships at (the first without scratch): no scratch, at most 4 VGPRs
    more; every output store write-through exactly when asked; the timeline record written by two 16-byte
    vector stores."""
    coeff, R, K = coeff_of(name)
    for cap in CAPS:
        base_v, base_s, _ = compiled(tmp_path, f"plain{cap}", source(request(coeff, R, K, cap, 0)))
        if base_s == 0:
            break
    assert base_s == 0
    for bits in (THROUGH, TIMELINE, THROUGH | TIMELINE):
        v, s, asm = compiled(tmp_path, f"form{bits}", source(request(coeff, R, K, cap, bits)))
        print(name, "cap", cap, "opts", bits, "VGPRs", v, "plain", base_v, "scratch", s)
        assert s == 0, (bits, s)
        assert v <= base_v + 4, (bits, v, base_v)
        records = sum(1 for ln in asm.splitlines() if ln.strip().startswith("global_store_dwordx4"))
        assert records == (2 if bits & TIMELINE else 0), (bits, records)
        outs = [ln.rstrip() for ln in asm.splitlines() if ln.strip().startswith("buffer_store_dwordx4")]
        assert len(outs) == 4 * R
        assert all(ln.endswith("sc0 nt sc1") if bits & THROUGH else ln.endswith(" nt") and " sc0" not in ln for ln in outs), bits


if __name__ == "__main__":  # the golden file, from the libraries as built (see the module docstring)
    gold = {}
    for name_ in sorted(MAPS):
        coeff_, R_, K_ = coeff_of(name_)
        req_ = request(coeff_, R_, K_, 96, 0)
        gold[name_] = {"request": req_.decode(), "object": object_name(req_)}
    print(json.dumps(gold, indent=1))

"""CPU: planning of the stripe consistency check (ecamd_rs_check_map, include/ecamd_host.h), its
syndrome network [A | I] through the bitsliced generator (ecamd_bitslice_eval), and the build-time
compile of the fused check kernels (ecamd_check_prebuild).  Expected values come from the reference
codec (oracle_lib) and plain numpy GF(2^16) (gfnp), never from the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gfnp
import oracle_lib as orc
import shipped_ops
from ecdata import stripe_fragments
from liberasurecode_amd import _lib, prebuild

CODES = [(10, 4), (4, 2), (20, 8)]
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def patterns(k, m):
    """(missing, expected ncheck or None for -1)."""
    n = k + m
    return [([], m), ([0], m - 1), ([n - 1], m - 1), ([2, 7] if n > 7 else [2, 5], m - 2),
            (list(range(m)), 0), (list(range(m + 1)), None)]


def check_map(k, m, missing):
    h = _lib.host()
    G = _lib.ints(orc.generator(k, m))
    inputs = (C.c_int * k)()
    checked = (C.c_int * (k + m))()
    coeff = (C.c_int * ((k + m) * k))()
    n = C.c_int(-7)
    rc = h.ecamd_rs_check_map(G, k, m, _lib.ints(list(missing) + [-1]), inputs, checked, coeff, C.byref(n))
    if rc != 0:
        return rc, None, None, None
    R = n.value
    return rc, list(inputs), list(checked[:R]), [[coeff[r * k + j] for j in range(k)] for r in range(R)]


def stripe(k, m, bs, seed):
    data = stripe_fragments(seed, k, bs)
    return np.concatenate([data, orc.encode(k, m, data)])


@pytest.mark.parametrize("k,m", CODES)
def test_check_map_inputs_checked_and_rows(k, m):
    full = stripe(k, m, 256, 40 + k)
    for missing, ncheck in patterns(k, m):
        rc, inputs, checked, rows = check_map(k, m, missing)
        if ncheck is None:
            assert rc == -1, missing
            continue
        assert rc == 0
        avail = [f for f in range(k + m) if f not in missing]
        assert inputs == avail[:k]
        assert checked == avail[k:] and len(checked) == ncheck
        if not checked:
            continue
        # each row applied to the reference-encoded inputs reproduces the stored fragment
        got = gfnp.apply_map(rows, [full[i] for i in inputs])
        for f, g in zip(checked, got):
            assert (g == full[f]).all(), (missing, f)
    # nothing missing: the rows are the generator's parity rows, the encode map
    G = orc.generator(k, m)
    assert check_map(k, m, [])[3] == [G[(k + p) * k:(k + p + 1) * k] for p in range(m)]


def syndrome(k, rows, words, cap=64):
    """ecamd_bitslice_eval of [A | I] on (K + R) x 32 words -> (R x 32 words, ops)."""
    R = len(rows)
    syn = [list(rows[r]) + [1 if i == r else 0 for i in range(R)] for r in range(R)]
    flat = _lib.ints([c for row in syn for c in row])
    inp = np.ascontiguousarray(words, dtype=np.uint16)
    out = np.zeros((R, 32), dtype=np.uint16)
    ops = C.c_int()
    assert _lib.host().ecamd_bitslice_eval(flat, R, k + R, cap, inp.ctypes.data, out.ctypes.data, C.byref(ops)) == 0
    return out, ops.value


@pytest.mark.parametrize("k,m", CODES)
def test_syndrome_network_zero_on_consistent_and_lit_where_the_oracle_says(k, m):
    full = stripe(k, m, 64, 70 + k)  # 32 words per fragment: one lane's share of a tile
    for missing, ncheck in patterns(k, m):
        if not ncheck:
            continue
        _, inputs, checked, rows = check_map(k, m, missing)
        for R0 in range(0, len(checked), 8):  # row groups of 8, as the kernel takes them
            grp, grows = checked[R0:R0 + 8], rows[R0:R0 + 8]
            words = np.stack([full[f].view("<u2") for f in inputs + grp])
            out, _ = syndrome(k, grows, words)
            assert not out.any(), (missing, "consistent words must give zero syndromes")
            for victim in (inputs[min(3, k - 1)], grp[-1]):
                bad = full.copy()
                bad[victim, 17] ^= 0x10
                held = bad.copy()
                for f in missing:
                    held[f] = 0x5A
                want = []
                for f in grp:  # the oracle: stored fragment f against the reference's reconstruct of f
                    frags = [np.ascontiguousarray(x) for x in held]
                    assert orc.reconstruct(k, m, frags, list(missing), f) == 0
                    want.append(bool((frags[f] != bad[f]).any()))
                words = np.stack([bad[f].view("<u2") for f in inputs + grp])
                out, _ = syndrome(k, grows, words)
                assert [bool(o.any()) for o in out] == want, (missing, victim)
                assert any(want)


def test_check_rows_cost_16_ops_each_over_encode():
    k, m = 10, 4
    rows = check_map(k, m, [])[3]
    full = stripe(k, m, 64, 3)
    words = np.stack([full[f].view("<u2") for f in range(k + m)])
    _, ops_check = syndrome(k, rows, words, cap=64)
    enc = np.zeros((m, 32), dtype=np.uint16)
    ops = C.c_int()
    flat = _lib.ints([c for row in rows for c in row])
    assert _lib.host().ecamd_bitslice_eval(flat, m, k, 64, np.ascontiguousarray(words[:k]).ctypes.data,
                                           enc.ctypes.data, C.byref(ops)) == 0
    assert ops_check == ops.value + 16 * m


def _ints_ptr(v):
    arr = _lib.ints(list(v) + [-1])
    return arr, C.cast(arr, C.c_void_p)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/libhiprtc.so"), reason="needs hiprtc")
def test_check_prebuild_objects(tmp_path):
    d = _lib.dev()
    out = tmp_path / "jit"
    out.mkdir()
    keep, p = _ints_ptr([])
    assert d.ecamd_check_prebuild(10, 4, p, b"gfx950", str(out).encode()) >= 1
    cos = [n for n in os.listdir(out) if n.endswith(".co")]
    assert len(cos) == 1
    notes = subprocess.run([READELF, "--notes", str(out / cos[0])], capture_output=True, text=True).stdout
    assert ".private_segment_fixed_size: 0" in notes  # no scratch: the network did not spill
    assert ".group_segment_fixed_size: 0" in notes
    # (4,2): 2 rows over 6 fragments take no bitsliced form
    assert d.ecamd_check_prebuild(4, 2, p, b"gfx950", str(out).encode()) == 0
    assert len([n for n in os.listdir(out) if n.endswith(".co")]) == 1
    keep, p = _ints_ptr([0, 1, 2, 3, 4])
    assert d.ecamd_check_prebuild(10, 4, p, b"gfx950", str(out).encode()) < 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/libhiprtc.so"), reason="needs hiprtc")
def test_check_request_is_a_form_of_its_own(tmp_path):
    """The trailing `check` word makes the read-only kernel: an atomic OR, no fragment store; the same
    request without it stays the plain map; the word is refused on copy-through requests."""
    jitc = os.path.join(_lib.LIBDIR, "ecamd_jitc")
    rows = check_map(10, 4, [])[3]
    body = "\n".join(" ".join(map(str, list(r) + [int(i == j) for j in range(4)])) for i, r in enumerate(rows)) + "\n"
    head = f"ecamd-bitslice-request 2\n4 14 40 0 {64 | (2 << 11) | (2 << 15) | (1 << 19)}\n"
    env = dict(os.environ, ECAMD_JIT_KEEP_SOURCE="1")
    for name, tail in (("chk", "check\n"), ("plain", "")):
        req = tmp_path / f"{name}.req"
        req.write_text(head + body + tail)
        r = subprocess.run([jitc, str(req), str(tmp_path / f"{name}.co")], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
    chk, plain = (tmp_path / "chk.hip").read_text(), (tmp_path / "plain.hip").read_text()
    assert "__hip_atomic_fetch_or(a.status + s" in chk and "raw_buffer_store" not in chk
    assert "u8 status_bit[8];" in chk
    assert "atomic" not in plain and "status" not in plain and "raw_buffer_store_b128" in plain
    bad = tmp_path / "bad.req"
    bad.write_text(f"ecamd-bitslice-request 2\n4 14 40 0 1\n" + body + "check\n")
    assert subprocess.run([jitc, str(bad), str(tmp_path / "bad.co")], capture_output=True).returncode == 2
    bad.write_text(head + body + "chekc\n")
    assert subprocess.run([jitc, str(bad), str(tmp_path / "bad.co")], capture_output=True).returncode == 2


def test_shipped_op_list_unchanged_and_check_ops_separate():
    ops = [(k, m, list(miss) if miss is not None else None, dest, rebuild)
           for k, m, miss, dest, rebuild in prebuild.all_ops(full=True)]
    shipped_ops.golden_for(ops)  # rs_shipped.json still describes exactly all_ops(full=True)
    want = [(10, 4, []), (4, 2, []), (20, 8, [])] + [(10, 4, [f]) for f in range(14)]
    assert [(k, m, list(miss)) for k, m, miss in prebuild.CHECK_OPS] == want

"""CPU: planning of locate (ecamd_rs_locate_map, include/ecamd_host.h), the candidate rule it serves, the
second-stage network of the fused kernel (ecamd_bitslice_eval of the ratio matrix) and the build-time
compile of the locate kernels (ecamd_locate_prebuild).  Expected values come from the reference codec
(oracle_lib) and plain numpy GF(2^16) (gfnp), never from the code under test."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import gfnp
import oracle_lib as orc
from liberasurecode_amd import _lib, prebuild
from test_check_planning import CODES, READELF, _ints_ptr, check_map, patterns, stripe

def gf_mul(a, b):
    return int(gfnp.mul_vec(a, np.array([b], dtype=np.uint16))[0])


def gf_inv(a):
    """a^(2^16 - 2) by square and multiply on gfnp products."""
    assert a
    r, p, e = 1, a, 65534
    while e:
        if e & 1:
            r = gf_mul(r, p)
        p = gf_mul(p, p)
        e >>= 1
    return r


def locate_map(k, m, missing):
    h = _lib.host()
    G = _lib.ints(orc.generator(k, m))
    inputs = (C.c_int * k)()
    checked = (C.c_int * (k + m))()
    coeff = (C.c_int * ((k + m) * k))()
    ratio = (C.c_int * ((k + m) * k))()
    n = C.c_int(-7)
    rc = h.ecamd_rs_locate_map(G, k, m, _lib.ints(list(missing) + [-1]), inputs, checked, coeff, C.byref(n), ratio)
    if rc != 0:
        return rc, None, None, None, None
    R = n.value
    return (rc, list(inputs), list(checked[:R]), [[coeff[r * k + j] for j in range(k)] for r in range(R)],
            [[ratio[r * k + j] for j in range(k)] for r in range(max(R - 1, 0))])


@pytest.mark.parametrize("k,m", CODES)
def test_locate_map_is_the_check_map_with_ratios(k, m):
    for missing, ncheck in patterns(k, m):
        rc, inputs, checked, rows, ratio = locate_map(k, m, missing)
        if ncheck is None:
            assert rc == -1, missing
            continue
        assert (rc, inputs, checked, rows) == check_map(k, m, missing)
        assert len(ratio) == max(ncheck - 1, 0)
        assert all(c != 0 for row in rows for c in row), (missing, "every entry of A is non-zero")
        for r in range(1, ncheck):
            for j in range(k):
                assert ratio[r - 1][j] == gf_mul(rows[r][j], gf_inv(rows[0][j])), (missing, r, j)
                assert gf_mul(ratio[r - 1][j], rows[0][j]) == rows[r][j]


def candidates(rows, ratio, S):
    """The rule on syndrome words S (R x W uint16): the set of participants (inputs 0..K-1, then the
    checked rows K..K+R-1) that explain every word."""
    R, K = len(rows), len(rows[0])
    out = set()
    for j in range(K):
        if all((gfnp.mul_vec(ratio[r - 1][j], S[0]) == S[r]).all() for r in range(1, R)):
            out.add(j)
    for c in range(R):
        if all(not S[r].any() for r in range(R) if r != c):
            out.add(K + c)
    return out


def syndromes(rows, words):
    """S_r = stored_r ^ sum_j A[r][j] in_j on (K + R) x W words."""
    R, K = len(rows), len(rows[0])
    S = []
    for r in range(R):
        acc = words[K + r].copy()
        for j in range(K):
            acc ^= gfnp.mul_vec(rows[r][j], words[j])
        S.append(acc)
    return np.stack(S)


@pytest.mark.parametrize("k,m", CODES)
def test_rule_locates_every_single_fragment_and_no_pair(k, m):
    full = stripe(k, m, 64, 90 + k)
    for missing, ncheck in patterns(k, m):
        if not ncheck or ncheck < 2:
            continue
        _, inputs, checked, rows, ratio = locate_map(k, m, missing)
        part = inputs + checked
        words = np.stack([full[f].view("<u2") for f in part]).copy()
        assert not syndromes(rows, words).any()
        for c in range(len(part)):  # two flipped bytes in one fragment
            bad = words.copy()
            bad[c, 3] ^= 0x0110
            bad[c, 20] ^= 0x8000
            assert candidates(rows, ratio, syndromes(rows, bad)) == {c}, (missing, c)
        if ncheck >= 3:  # any two fragments corrupted in the same word: nobody explains it alone
            for a, b in itertools.combinations(range(len(part)), 2):
                bad = words.copy()
                bad[a, 5] ^= 0x0004
                bad[b, 5] ^= 0x0300
                assert candidates(rows, ratio, syndromes(rows, bad)) == set(), (missing, a, b)


@pytest.mark.parametrize("k,m", CODES)
def test_second_stage_network_equals_gf_products(k, m):
    """The stage-2 network is the bitsliced network of the (R - 1) x K ratio matrix with each column
    applied to the SAME planes (S_0): ecamd_bitslice_eval with every input set to the same words."""
    rng = np.random.default_rng(5 + k)
    for missing, ncheck in patterns(k, m):
        if not ncheck or ncheck < 2 or ncheck > 8:
            continue
        ratio = locate_map(k, m, missing)[4]
        R1 = ncheck - 1
        flat = _lib.ints([c for row in ratio for c in row])
        s0 = rng.integers(0, 65536, size=32, dtype=np.uint16)
        for j in range(k):  # column j alone: S_0 on input j, zero elsewhere
            inp = np.zeros((k, 32), dtype=np.uint16)
            inp[j] = s0
            out = np.zeros((R1, 32), dtype=np.uint16)
            assert _lib.host().ecamd_bitslice_eval(flat, R1, k, 8, inp.ctypes.data, out.ctypes.data, None) == 0
            for r in range(R1):
                assert (out[r] == gfnp.mul_vec(ratio[r][j], s0)).all(), (missing, r, j)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/libhiprtc.so"), reason="needs hiprtc")
def test_locate_prebuild_objects(tmp_path):
    d = _lib.dev()
    out = tmp_path / "jit"
    out.mkdir()
    keep, p = _ints_ptr([])
    assert d.ecamd_locate_prebuild(10, 4, p, b"gfx950", str(out).encode()) == 1
    cos = [n for n in os.listdir(out) if n.endswith(".co")]
    assert len(cos) == 1
    notes = subprocess.run([READELF, "--notes", str(out / cos[0])], capture_output=True, text=True).stdout
    assert ".private_segment_fixed_size: 0" in notes  # no scratch
    assert ".group_segment_fixed_size: 0" in notes
    # its name differs from the check kernel's of the same map
    assert d.ecamd_check_prebuild(10, 4, p, b"gfx950", str(out).encode()) == 1
    assert len([n for n in os.listdir(out) if n.endswith(".co")]) == 2
    # (4,2): 2 rows over 6 fragments take no bitsliced form
    assert d.ecamd_locate_prebuild(4, 2, p, b"gfx950", str(out).encode()) == 0
    # one checked fragment: no locate kernel at all
    keep, p = _ints_ptr([0, 1, 2])
    assert d.ecamd_locate_prebuild(10, 4, p, b"gfx950", str(out).encode()) == 0
    assert len([n for n in os.listdir(out) if n.endswith(".co")]) == 2
    keep, p = _ints_ptr([0, 1, 2, 3, 4])
    assert d.ecamd_locate_prebuild(10, 4, p, b"gfx950", str(out).encode()) < 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/libhiprtc.so"), reason="needs hiprtc")
def test_locate_request_is_a_form_of_its_own(tmp_path):
    """The trailing `locate` word makes the check kernel with the second stage: an atomic AND on the
    suspects, still no fragment store; the same request with `check` knows nothing of suspects."""
    jitc = os.path.join(_lib.LIBDIR, "ecamd_jitc")
    rows = check_map(10, 4, [])[3]
    body = "\n".join(" ".join(map(str, list(r) + [int(i == j) for j in range(4)])) for i, r in enumerate(rows)) + "\n"
    head = f"ecamd-bitslice-request 2\n4 14 40 0 {64 | (2 << 11) | (2 << 15) | (1 << 19)}\n"
    env = dict(os.environ, ECAMD_JIT_KEEP_SOURCE="1")
    for name, tail in (("loc", "locate\n"), ("chk", "check\n")):
        req = tmp_path / f"{name}.req"
        req.write_text(head + body + tail)
        r = subprocess.run([jitc, str(req), str(tmp_path / f"{name}.co")], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
    loc, chk = (tmp_path / "loc.hip").read_text(), (tmp_path / "chk.hip").read_text()
    assert "__hip_atomic_fetch_and(a.suspects" in loc and "raw_buffer_store" not in loc
    assert "__hip_atomic_fetch_or(a.status + s" in loc and "u8 frag_bit[32];" in loc
    assert "suspects" not in chk and "fetch_and" not in chk and "frag_bit" not in chk
    bad = tmp_path / "bad.req"
    bad.write_text("ecamd-bitslice-request 2\n4 14 40 0 1\n" + body + "locate\n")  # copy-through: refused
    assert subprocess.run([jitc, str(bad), str(tmp_path / "bad.co")], capture_output=True).returncode == 2
    one_row = " ".join(map(str, list(rows[0]) + [1])) + "\n"  # a single row has nothing to compare
    bad.write_text(f"ecamd-bitslice-request 2\n1 11 40 0 {64 | (2 << 11) | (2 << 15)}\n" + one_row + "locate\n")
    assert subprocess.run([jitc, str(bad), str(tmp_path / "bad.co")], capture_output=True).returncode == 2


def test_locate_ops_are_a_list_of_their_own():
    want = [(10, 4, []), (4, 2, []), (20, 8, [])] + [(10, 4, [f]) for f in range(14)]
    assert [(k, m, list(miss)) for k, m, miss in prebuild.LOCATE_OPS] == want
    assert [(k, m, list(miss)) for k, m, miss in prebuild.CHECK_OPS] == want

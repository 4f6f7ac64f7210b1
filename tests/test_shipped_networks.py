"""CPU: the XOR network the generator (csrc/host/bitslice.cpp) builds for EVERY shipped map -- each of
the 1,470 1- to 4-loss decode matrices of RS(10,4), the single-loss maps of (10,4) and (20,8) and the
benched maps -- evaluated on the host (ecamd_bitslice_eval) against the oracle codec on the same 64-byte
fragments.  A shipped object is the network at the first cap whose compile does not spill (kCaps 96,
64, 40, 16 in hip/ecamd_jit.hip): cap 96 is checked for every op, the lower caps for every 14th.

Measured on one core of the build machine: 0.11-0.16 s per (10,4) network; the cap-96 pass over all
ops about 235 s in all, split into chunks of at most 100 ops so that no case runs longer than ~25 s."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import shipped_ops as so
from liberasurecode_amd import _lib

OPS = so.ops()
CHUNK = 100
LOWER_CAPS = (64, 40, 16)
EVERY = 14


def _chunks():
    """Op indices grouped by (code, kind, losses, leading index), each group cut into pieces of CHUNK."""
    groups = {}
    for i, (k, m, miss, dest, _) in enumerate(OPS):
        key = (k, m, so.kind(OPS[i]), len(miss or ()), (miss or [-1])[0] if (k, m) == (10, 4) and dest < 0 else -1)
        groups.setdefault(key, []).append(i)
    out = []
    for key, idx in groups.items():
        for p in range(0, len(idx), CHUNK):
            name = "rs%d_%d-%s-loss%d-lead%d-part%d" % (key + (p // CHUNK,))
            out.append(pytest.param(idx[p:p + CHUNK], id=name))
    return out


def evaluate(coeff, R, K, cap, words):
    out = np.zeros((R, 32), np.uint16)
    ops = C.c_int()
    assert _lib.host().ecamd_bitslice_eval(_lib.ints(coeff), R, K, cap, words.ctypes.data, out.ctypes.data,
                                           C.byref(ops)) == 0
    return out


def check_network(i, cap):
    """True if op i is expected bitsliced and was checked; raises on a mismatch."""
    op = OPS[i]
    if not so.expected_bitsliced(op):
        return False
    k, m, miss, dest, rebuild = op
    inputs, rows = so.plan(op)
    R, K = len(rows), len(inputs)
    assert R <= 8  # one row group of 8 covers every shipped map
    rng = np.random.default_rng(7000 + i)
    frags = rng.integers(0, 256, (k + m, 64), dtype=np.uint8)  # fragments outside `inputs` must not matter
    words = np.ascontiguousarray(frags[inputs]).view(np.uint16).reshape(K, 32)
    got = evaluate([c for row in rows for c in row], R, K, cap, words).view(np.uint8).reshape(R, 64)
    want = so.run_host(op, frags[None].copy(), orc)[0]
    for r, f in enumerate(so.outputs(op)):
        assert (got[r] == want[f]).all(), (op, cap, "output fragment", f)
    return True


@pytest.mark.parametrize("indices", _chunks())
def test_network_of_every_shipped_map_at_first_cap(indices):
    assert sum(check_network(i, 96) for i in indices) > 0 or all(OPS[i][0] == 4 for i in indices)


@pytest.mark.parametrize("cap", LOWER_CAPS)
@pytest.mark.parametrize("half", [0, 1])
def test_network_of_every_14th_map_at_the_retry_caps(cap, half):
    idx = list(range(0, len(OPS), EVERY))
    mid = len(idx) // 2
    assert sum(check_network(i, cap) for i in (idx[:mid] if half == 0 else idx[mid:])) >= mid - 4


def test_every_expected_op_is_covered():
    covered = sorted(i for p in _chunks() for i in p.values[0])
    assert covered == list(range(len(OPS)))
    assert sum(so.expected_bitsliced(op) for op in OPS) >= 1470 + 14 + 56

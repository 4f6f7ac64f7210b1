"""CPU: tests/golden/rs_shipped.json (digests from the reference codec, make_shipped_golden.py) against
the restated oracle on every operation whose bitsliced kernel ships -- all 1,470 1- to 4-loss patterns
of RS(10,4), the single-loss maps of (10,4), (4,2) and (20,8) and the benched maps.  The GPU test
(test_gpu_shipped_objects.py) checks the kernels against the same digests and uses the oracle for its
diagnostics; this ties the two together."""
import os

import pytest

import oracle_lib as orc
import shipped_ops as so

OPS = so.ops()
GOLD = so.golden_for(OPS)
CHUNK = 200
MAX_GOLDEN_BYTES = 194520  # tests/golden/xor_codes.json, the largest golden committed before this one


def test_op_list_and_golden_file():
    so.check_ops(OPS)
    assert len(OPS) == len(GOLD)
    assert sum(so.expected_bitsliced(op) for op in OPS) >= 1470 + 14 + 56
    for op, (_, bs, _) in zip(OPS, GOLD):
        assert bs == so.blocksize(op), op
    assert os.path.getsize(so.GOLDEN) <= MAX_GOLDEN_BYTES
    part = so.slices(OPS)
    assert all(len(part[f"loss4_{p}"]) in (333, 334) for p in range(3))


@pytest.mark.parametrize("start", range(0, len(OPS), CHUNK))
def test_oracle_reproduces_reference_digests(start):
    bad = []
    for i in range(start, min(start + CHUNK, len(OPS))):
        op = OPS[i]
        full, erased = so.op_inputs(i, op, orc.encode)
        got = so.run_host(op, erased, orc)
        if so.digest(op, got) != GOLD[i][2]:
            bad.append(op)
        # consistent stripes: what the operation rebuilds is what was erased
        assert all((got[:, f] == full[:, f]).all() for f in so.outputs(op)), op
    assert not bad, bad


def test_digest_sees_one_byte_in_the_second_tile():
    i = next(j for j, op in enumerate(OPS) if op[2] == [0, 5, 10, 13] and op[3] < 0)
    op = OPS[i]
    _, erased = so.op_inputs(i, op, orc.encode)
    assert so.digest(op, so.run_host(op, erased, orc)) == GOLD[i][2]
    survivor = 1
    assert survivor not in op[2]
    erased[1, survivor, so.TILE_WAVE + 1234] ^= 0x01  # inside the second 4 KiB tile of stripe 1
    assert so.digest(op, so.run_host(op, erased, orc)) != GOLD[i][2]

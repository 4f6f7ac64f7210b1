"""CPU: ecamd_frame_header (libecamd_host.so) -- the header text of csrc/hip/ecamd_frame_header.hpp that
crc_finalize_kernel and the stamp kernel of ecamd_frame_reconstruct_masks run on the device -- against
the framing restatement of tests/ec_api.py (pinned to the reference's known-answer headers)."""
import ctypes as C
import zlib

import pytest

import ec_api

PAYLOAD = bytes(range(251)) * 3


def _header(idx, bs, obj_size, backend, ct, crc, legacy):
    from liberasurecode_amd import _lib
    out = (C.c_uint8 * 80)()
    assert _lib.host().ecamd_frame_header(idx, bs, obj_size, backend, ct, crc, int(legacy), out) == 0
    return bytes(out)


@pytest.mark.parametrize("legacy", [False, True], ids=["zlib", "legacy"])
@pytest.mark.parametrize("ct", [ec_api.CHKSUM_NONE, ec_api.CHKSUM_CRC32, ec_api.CHKSUM_MD5])
@pytest.mark.parametrize("backend,k,m", [(ec_api.EC_BACKEND_LIBERASURECODE_RS_VAND, 10, 4),
                                         (ec_api.EC_BACKEND_FLAT_XOR_HD, 10, 6)], ids=["rs_vand", "flat_xor_hd"])
def test_frame_header_matches_restated_reference(backend, k, m, ct, legacy):
    crc = ec_api.crc32_legacy(PAYLOAD) if legacy else zlib.crc32(PAYLOAD)
    for idx in (0, k + m - 1):
        for obj_size in (1, (1 << 32) + 5):
            bs = len(PAYLOAD)
            want = ec_api.expected_header(idx, bs, obj_size, backend, ct, PAYLOAD, legacy=legacy)
            got = _header(idx, bs, obj_size, backend, ct, crc, legacy)
            assert got == want, (idx, obj_size, got.hex(), want.hex())
            # the CRC word is stored for CRC32 only: another value changes nothing for the other types
            other = _header(idx, bs, obj_size, backend, ct, crc ^ 0x5A5A5A5A, legacy)
            assert (other == want) == (ct != ec_api.CHKSUM_CRC32)


def test_frame_header_rejects():
    from liberasurecode_amd import _lib
    out = (C.c_uint8 * 80)()
    assert _lib.host().ecamd_frame_header(0, 16, 16, 6, 2, 0, 0, None) == -1
    assert _lib.host().ecamd_frame_header(-1, 16, 16, 6, 2, 0, 0, out) == -1
    assert bytes(out) == bytes(80)

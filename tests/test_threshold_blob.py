"""The partial-decryption blob ("SHPD", api_internal.h) through the host-only helpers
shelfi_partial_blob_pack / shelfi_partial_blob_info: no device needed.  The header fields and the
lead / main mark round-trip; a wrong magic, a wrong length and a length off by one word are refused."""
import struct

import numpy as np
import pytest

import SHELFI_FHE as m
from SHELFI_FHE import _lib

K, L, N = 3, 2, 2048
SCALE, PARAMS_ID, KEY_ID, BATCH = 2.0 ** 104, 0x1122334455667788, 0xA1B2C3D4E5F60718, 1024


def _blob(lead, K=K):
    r = np.arange(K * L * N, dtype=np.uint64).reshape(K, L, N) * np.uint64(977)
    return r, m.partial_blob_pack(r, lead, SCALE, PARAMS_ID, KEY_ID, BATCH, depth=2)


@pytest.mark.parametrize("lead", [True, False])
def test_header_and_payload_round_trip(lead):
    r, b = _blob(lead)
    assert len(b) == 64 + K * L * N * 8 and b[:4] == b"SHPD"
    inf = m.partial_blob_info(b)
    assert inf == {"num_cts": K, "towers": L, "lead": lead, "scale": SCALE, "key_id": KEY_ID}
    # the ciphertext blob's 64-byte header, field by field
    magic, ver, hb, logN, towers, k, depth, level, scale, pid, kid, batch, enc = struct.unpack("<4sHHIIQIIdQQII",
                                                                                               b[:64])
    assert (ver, hb, logN, towers, k, depth, level) == (1, 64, 11, L, K, 2, int(lead))
    assert (scale, pid, kid, batch, enc) == (SCALE, PARAMS_ID, KEY_ID, BATCH, 4)
    assert np.array_equal(np.frombuffer(b, np.uint64, offset=64).reshape(K, L, N), r)


def test_empty_batch():
    _, b = _blob(True, K=0)
    assert len(b) == 64 and m.partial_blob_info(b)["num_cts"] == 0


def _refused(b):
    with pytest.raises(m.ShelfiError) as ei:
        m.partial_blob_info(bytes(b))
    assert ei.value.code == _lib.SHELFI_ERR_FORMAT


def test_malformed_blobs_are_refused():
    _, b = _blob(True)
    _refused(b"SHCT" + b[4:])  # a ciphertext blob's magic
    _refused(b"XXXX" + b[4:])
    _refused(b[:-8])           # one word short
    _refused(b + b"\0" * 8)    # one word long
    _refused(b[:-1])
    _refused(b[:63])
    _refused(b"")
    bad = bytearray(b)
    bad[28:32] = struct.pack("<I", 2)  # the role word: only 0 (main) and 1 (lead)
    _refused(bad)
    bad = bytearray(b)
    bad[16:24] = struct.pack("<Q", K + 1)  # K against the payload
    _refused(bad)
    bad = bytearray(b)
    bad[16:24] = struct.pack("<Q", 2 ** 63)  # K * bytes wraps
    _refused(bad)
    # and a ciphertext-blob reader does not take a partial for a ciphertext
    with pytest.raises(m.ShelfiError):
        m.blob_info(b)


def test_pack_refuses_bad_shapes():
    r = np.zeros((1, 2, 1000), np.uint64)  # ring dimension not a power of two
    with pytest.raises(ValueError):
        m.partial_blob_pack(r, True, SCALE, PARAMS_ID, KEY_ID, BATCH)
    with pytest.raises(ValueError):
        m.partial_blob_pack(np.zeros((1, 17, 2048), np.uint64), True, SCALE, PARAMS_ID, KEY_ID, BATCH)

"""Range GETs of stored SSE-S3 blobs through sse_read_range_kernel: plaintext [from, from + want) of
the blob [nonce][ciphertext][tag] into a registered buffer with out % 16 == from % 16, exact against
OpenSSL, with guard bytes around the range. The counter proves which route ran."""
import functools

import numpy as np
import pytest

from rust_hadoop_generated_by_llm_amd import native as _native

pytestmark = pytest.mark.gpu

GUARD = 0xA5
KEY = bytes(range(201, 233))
NONCE = bytes(range(50, 62))
TILE, GRID = _native.lib.sse_read_tile_bytes, _native.lib.sse_read_max_grid
OK, NOT_FOUND, CORRUPT, AUTH_FAILED, IO_ERROR = range(5)
N1, TWO_STEPS = TILE + 5, 2 * GRID * TILE - 28 + 7
# The range TILE - 19, +30 ends at TILE + 11, behind N1's plaintext, where the store answers IO_ERROR
# (test_sse_range_fastpath.py): it runs on a blob of N2 bytes, just long enough to hold it with the
# end unaligned, and cut to the plaintext's end on N1.
N2 = TILE + 13
CASES = [
    (N1, 5, 3),  # head and tail in one AES block
    (N1, 16, 16),  # exactly one aligned block
    (N2, TILE - 12 - 7, 30),  # across the tile edge and lane 63's funnel, both ends unaligned
    (N1, TILE - 12 - 7, 24),  # the same up to the plaintext's last byte
    (N1, TILE + 4, 1),  # the last byte, in the ragged final block
    (500, 1, 499),  # a blob of one short slice
    ((1 << 20) + 3, (1 << 18) + 9, 3 * TILE + 1),  # whole inside tiles between two edge tiles
    (TWO_STEPS, GRID * TILE - 12 - 40, 100),  # across the grid-stride step boundary
    (TWO_STEPS, GRID * TILE + 100, TILE + 33),  # wholly in the second step
]


@pytest.fixture(scope="module")
def gstore(native, tmp_path_factory):
    s = native.ChunkStore(str(tmp_path_factory.mktemp("sse_read_range")), "", 0, 256 << 20, 0, 100, 2, 1, False)
    assert s.gpu
    floor = native.sse_read_fused_min_bytes()
    native.set_sse_read_fused(True, 0)
    yield s
    native.set_sse_read_fused(True, floor)


@functools.lru_cache(maxsize=None)
def reference(n):
    """Plaintext of n bytes and the blob the gateway stores for it: nonce, OpenSSL's ciphertext, tag."""
    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    return pt, NONCE + _native.lib.aes256gcm_encrypt(KEY, NONCE, pt.tobytes(), b"")


def read(gstore, native, block_id, start, want, key=KEY, register=True, skew=0):
    """sse_read of the range into a buffer at address % 16 == (start + skew) % 16, 16 guard bytes on
    both sides. Returns (status, n or bad slice, the range's bytes, whether the guards held, counter moved)."""
    buf = native.pinned_array(48 + want + 16) if register else np.empty(48 + want + 16, dtype=np.uint8)
    buf[:] = GUARD
    at = 16 + (start + skew - (buf.ctypes.data + 16)) % 16
    if register:
        assert gstore.register_host(buf)
    try:
        before = gstore.stats()["sse_fused_range_reads"]
        st, got = gstore.sse_read(block_id, key, buf[at:at + want], offset=start, length=want)
        moved = gstore.stats()["sse_fused_range_reads"] - before
        held = bool((buf[:at] == GUARD).all() and (buf[at + want:] == GUARD).all())
        return st, got, buf[at:at + want].copy(), held, moved
    finally:
        if register:
            gstore.unregister_host(buf)


@pytest.mark.parametrize("n,start,want", CASES)
def test_kernel_range_matches_openssl(gstore, native, n, start, want):
    pt, blob = reference(n)
    assert gstore.write(f"rng-{n}", blob, 0)[0]
    st, got, out, held, moved = read(gstore, native, f"rng-{n}", start, want)
    assert (st, got, moved) == (OK, want, 1) and held
    assert (out == pt[start:start + want]).all()


@pytest.mark.parametrize("why", ["corrupt-slice", "wrong-tag", "wrong-key"])
def test_a_fault_outside_the_range_zeroes_it(gstore, native, why):
    """The slice is named by the CRC; the store checksums what it is given, so only the GHASH catches the other two."""
    _, blob = reference(N1)
    assert gstore.write(f"rng-{why}", blob[:-1] + bytes([blob[-1] ^ 1]) if why == "wrong-tag" else blob, 0)[0]
    assert why != "corrupt-slice" or gstore.debug_corrupt(f"rng-{why}", 12 + 5000)
    st, bad, out, held, moved = read(gstore, native, f"rng-{why}", 100, 64, bytes(32) if why == "wrong-key" else KEY)
    assert (st, moved) == (CORRUPT if why == "corrupt-slice" else AUTH_FAILED, 1)
    assert why != "corrupt-slice" or bad == (12 + 5000) // 512
    assert held and not out.any()


@pytest.mark.parametrize("why", ["misaligned", "unregistered", "switched-off"])
def test_staged_route_gives_the_same_bytes(gstore, native, why):
    pt, blob = reference(N2)
    assert gstore.write(f"rng-staged-{why}", blob, 0)[0]
    native.set_sse_read_fused(why != "switched-off")
    try:
        st, got, out, held, moved = read(gstore, native, f"rng-staged-{why}", TILE - 19, 30,
                                         register=why != "unregistered", skew=why == "misaligned")
    finally:
        native.set_sse_read_fused(True, 0)
    assert (st, got, moved) == (OK, 30, 0) and held
    assert (out == pt[TILE - 19:TILE - 19 + 30]).all()

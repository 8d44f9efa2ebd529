"""CopyObjects of stored SSE-S3 blobs through sse_rekey_kernel: OpenSSL's blob under (KEY_A, NONCE_A),
written to the store, becomes a new block that must equal OpenSSL's blob of the same plaintext under
(KEY_B, NONCE_B), byte for byte, with zlib's CRC and write()'s .meta. The counters prove which route ran."""
import functools
import os
import zlib

import numpy as np
import pytest

from rust_hadoop_generated_by_llm_amd import native as _native

pytestmark = pytest.mark.gpu

KEY_A, NONCE_A = bytes(range(201, 233)), bytes(range(50, 62))
KEY_B, NONCE_B = bytes(range(7, 39)), bytes(range(90, 102))
TILE, GRID = _native.lib.sse_read_tile_bytes, _native.lib.sse_read_max_grid
OK, NOT_FOUND, CORRUPT, AUTH_FAILED, IO_ERROR = range(5)
# sub-block and block edges; the tag across a slice edge; the blob filling its tile; the tag across and
# behind the tile edge; every workgroup of the capped grid takes a second grid-stride step
LENGTHS = [1, 16, 17, 492, 500, TILE - 28, TILE - 20, TILE - 12, TILE + 5, 2 * GRID * TILE - 28 + 7]
TWO_TILES = TILE + 5


@pytest.fixture(scope="module")
def gstore(native, tmp_path_factory):
    from rust_hadoop_generated_by_llm_amd import native as n

    assert n.gpu_count() > 0, "GPU tests need a HIP device"
    s = native.ChunkStore(str(tmp_path_factory.mktemp("sse_copy")), "", 0, 256 << 20, 0, 100, 2, 1, False)
    assert s.gpu
    floor = native.sse_copy_fused_min_bytes()
    native.set_sse_copy_fused(True, 0)
    yield s
    native.set_sse_copy_fused(True, floor)
    del s


@functools.lru_cache(maxsize=None)
def reference(n):
    """The source's blob of a seeded plaintext of n bytes, and the blob its copy must be."""
    from rust_hadoop_generated_by_llm_amd import native

    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    return (NONCE_A + native.lib.aes256gcm_encrypt(KEY_A, NONCE_A, pt, b""),
            NONCE_B + native.lib.aes256gcm_encrypt(KEY_B, NONCE_B, pt, b""))


def stored(gstore, block_id, size):
    st, total, data, partial, _bad, err = gstore.read(block_id, 0, size)
    assert (st, total, partial) == (OK, size, False), err
    return data


def copy(gstore, src, dst, key=KEY_A):
    """sse_copy of src to dst. Returns (status, crc or bad slice, sse_fused_copies moved, launches moved)."""
    before = gstore.stats()
    st, val, _err = gstore.sse_copy(src, dst, key, KEY_B, NONCE_B)
    after = gstore.stats()
    return (st, val, after["sse_fused_copies"] - before["sse_fused_copies"],
            after["gpu_kernel_launches"] - before["gpu_kernel_launches"])


@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_copy_matches_openssl(gstore, n):
    old, new = reference(n)
    src, dst = f"c-src-{n}", f"c-dst-{n}"
    assert gstore.write(src, old, 0)[0]
    st, crc, moved, launches = copy(gstore, src, dst)
    assert (st, moved, launches) == (OK, 1, 1)
    assert stored(gstore, dst, n + 28) == new
    assert crc == zlib.crc32(new) == gstore.crc(dst)
    assert gstore.write(f"c-ref-{n}", new, 0)[0]
    assert gstore.meta(dst) == gstore.meta(f"c-ref-{n}")
    gstore.drop_resident()
    assert stored(gstore, dst, n + 28) == new  # from the durable copy
    assert stored(gstore, src, n + 28) == old
    for bid in (src, dst, f"c-ref-{n}"):
        assert gstore.remove(bid)


@pytest.mark.parametrize("why", ["corrupt-slice", "wrong-source-key", "missing-source"])
def test_refusals_leave_no_destination(gstore, why):
    old, _ = reference(TWO_TILES)
    src, dst = f"c-bad-{why}", f"c-never-{why}"
    if why != "missing-source":
        assert gstore.write(src, old, 0)[0]
    if why == "corrupt-slice":
        assert gstore.debug_corrupt(src, 12 + 5000)
    used = gstore.stats()["hbm_used"]
    st, val, _, _ = copy(gstore, src, dst, bytes(32) if why == "wrong-source-key" else KEY_A)
    want = {"corrupt-slice": CORRUPT, "wrong-source-key": AUTH_FAILED, "missing-source": NOT_FOUND}[why]
    assert st == want and (why != "corrupt-slice" or val == (12 + 5000) // 512)
    assert not gstore.exists(dst)
    assert gstore.stats()["hbm_used"] == used


@pytest.mark.parametrize("why", ["switched-off", "below-the-floor", "source-not-resident"])
def test_staged_route_stores_the_same_blob(gstore, native, why):
    old, new = reference(TWO_TILES)
    src, dst = f"c-staged-{why}", f"c-staged-dst-{why}"
    assert gstore.write(src, old, 0)[0]
    if why == "source-not-resident":
        gstore.drop_resident()
    native.set_sse_copy_fused(why != "switched-off", TWO_TILES + 1 if why == "below-the-floor" else 0)
    try:
        st, crc, moved, _ = copy(gstore, src, dst)
    finally:
        native.set_sse_copy_fused(True, 0)
    assert (st, moved) == (OK, 0)
    assert stored(gstore, dst, TWO_TILES + 28) == new and crc == zlib.crc32(new) == gstore.crc(dst)


def test_fast_path_op(gstore, native):
    """Fast-path op 14 re-keys a resident blob into a new block with no slot and moves the counter."""
    from rust_hadoop_generated_by_llm_amd.utils import fastpath as fp

    n = TILE + 17
    old, new = reference(n)
    assert gstore.write("c-fp-src", old, 0)[0]
    srv = native.FastPathServer(gstore, f"dfs_fp_ssec_{os.getpid()}")
    ok, err = srv.start()
    assert ok, err
    cli = fp.FastPathClient(srv.name)
    try:
        st, replicas, crc = cli.sse_copy("c-fp-src", "c-fp-dst", KEY_A, KEY_B, NONCE_B, 0)
        assert (st, replicas, crc) == (fp.OK, 1, zlib.crc32(new))
        assert stored(gstore, "c-fp-dst", n + 28) == new
        assert srv.stats()["fp_sse_copies"] == 1
    finally:
        cli.close()
        srv.stop()

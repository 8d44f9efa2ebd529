"""PUTs of SSE-S3 objects through sse_write_kernel: the plaintext in a registered slot becomes the
blob [nonce][ciphertext][tag] there and in the store, exact against OpenSSL and zlib, with guard
bytes around the slot. The counters prove which route ran."""
import functools
import os
import zlib

import numpy as np
import pytest

from rust_hadoop_generated_by_llm_amd import native as _native

pytestmark = pytest.mark.gpu

GUARD = 0xA5
KEY = bytes(range(201, 233))
NONCE = bytes(range(50, 62))
TILE, GRID = _native.lib.sse_read_tile_bytes, _native.lib.sse_read_max_grid
OK = 0
# sub-block and block edges; the tag across a slice edge; the blob one vector past a slice; the blob
# filling its tile; the tag across the tile edge; the tag alone in tile 2; a tile of a few bytes;
# every workgroup of the capped grid takes a second grid-stride step
LENGTHS = [1, 16, 17, 492, 500, TILE - 28, TILE - 20, TILE - 12, TILE + 5, 2 * GRID * TILE - 28 + 7]
STAGED = TILE - 20


@pytest.fixture(scope="module")
def gstore(native, tmp_path_factory):
    from rust_hadoop_generated_by_llm_amd import native as n

    assert n.gpu_count() > 0, "GPU tests need a HIP device"
    s = native.ChunkStore(str(tmp_path_factory.mktemp("sse_write")), "", 0, 256 << 20, 0, 100, 2, 1, False)
    assert s.gpu
    floor = native.sse_read_fused_min_bytes()
    native.set_sse_write_fused(True, 0)
    native.set_sse_read_fused(True, 0)
    yield s
    native.reset_sse_write_fused()
    native.set_sse_read_fused(True, floor)
    del s


@functools.lru_cache(maxsize=None)
def reference(n):
    """Plaintext of n bytes and the blob a PUT stores for it: nonce, OpenSSL's ciphertext, tag."""
    from rust_hadoop_generated_by_llm_amd import native

    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    return pt, NONCE + native.lib.aes256gcm_encrypt(KEY, NONCE, pt.tobytes(), b"")


def put(gstore, native, block_id, n, start=16, register=True):
    """sse_write of block_id from a slot at buf[start:] with guards on both sides, the plaintext at + 12
    and junk where nonce and tag go. Asserts ok; returns (crc, the slot's bytes, guards held,
    sse_fused_writes moved, gpu_kernel_launches moved)."""
    pt, _ = reference(n)
    size = start + n + 28 + 16
    buf = native.pinned_array(size) if register else np.empty(size, dtype=np.uint8)
    buf[:] = GUARD
    slot = buf[start:start + n + 28]
    slot[:12] = 0x3C
    slot[12:12 + n] = pt
    slot[12 + n:] = 0xC3
    if register:
        assert gstore.register_host(buf)
    try:
        before = gstore.stats()
        ok, crc, err = gstore.sse_write(block_id, KEY, NONCE, slot)
        after = gstore.stats()
        assert ok, err
        held = bool((buf[:start] == GUARD).all() and (buf[start + n + 28:] == GUARD).all())
        return (crc, slot.tobytes(), held, after["sse_fused_writes"] - before["sse_fused_writes"],
                after["gpu_kernel_launches"] - before["gpu_kernel_launches"])
    finally:
        if register:
            gstore.unregister_host(buf)


def stored(gstore, block_id, size):
    st, total, data, partial, _bad, err = gstore.read(block_id, 0, size)
    assert (st, total, partial) == (OK, size, False), err
    return data


@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_write_matches_openssl(gstore, native, n):
    pt, blob = reference(n)
    bid = f"w-{n}"
    crc, slot, held, moved, launches = put(gstore, native, bid, n)
    assert slot == blob and held
    assert (moved, launches) == (1, 1)
    assert crc == zlib.crc32(blob) == gstore.crc(bid)
    assert gstore.write(f"ref-{n}", blob, 0)[0]
    assert gstore.meta(bid) == gstore.meta(f"ref-{n}")
    assert stored(gstore, bid, n + 28) == blob
    gstore.drop_resident()
    assert stored(gstore, bid, n + 28) == blob  # from the durable copy
    out = native.pinned_array(n + 28)
    assert gstore.sse_read(bid, KEY, out) == (OK, n) and (out[:n] == pt).all()
    assert gstore.remove(bid) and gstore.remove(f"ref-{n}")


@pytest.mark.parametrize("why", ["misaligned", "unregistered", "switched-off", "below-the-floor"])
def test_staged_route_stores_the_same_blob(gstore, native, why):
    _, blob = reference(STAGED)
    native.set_sse_write_fused(why != "switched-off", STAGED + 1 if why == "below-the-floor" else 0)
    try:
        crc, slot, held, moved, _ = put(gstore, native, f"w-{why}", STAGED, 17 if why == "misaligned" else 16,
                                        why != "unregistered")
    finally:
        native.set_sse_write_fused(True, 0)
    assert slot == blob and held and moved == 0
    assert crc == zlib.crc32(blob) == gstore.crc(f"w-{why}")
    assert stored(gstore, f"w-{why}", STAGED + 28) == blob


def test_fast_path_op(gstore, native, can_pin_existing_memory):
    """A client slot through fast-path op 13 is stored as OpenSSL's blob and moves the counters. Where
    the host cannot pin a client's arena the kernel cannot reach the slot: the op declines and leaves
    the bytes alone, and the client encrypts and writes its own way."""
    from rust_hadoop_generated_by_llm_amd.utils import fastpath as fp
    from rust_hadoop_generated_by_llm_amd.utils.shm import ShmArena

    n = TILE + 17
    pt, blob = reference(n)
    srv = native.FastPathServer(gstore, f"dfs_fp_ssew_{os.getpid()}")
    ok, err = srv.start()
    assert ok, err
    arena = ShmArena(size=1 << 20, slot=1 << 19)
    cli = fp.FastPathClient(srv.name)
    try:
        slot = arena.acquire(n + 28)
        before = bytes(12) + pt.tobytes() + bytes(16)
        arena.view[slot:slot + n + 28] = before
        st, replicas, crc = cli.sse_write("w-fp", arena.path, slot, n + 28, KEY, NONCE, 0)
        if can_pin_existing_memory:
            assert (st, replicas, crc) == (fp.OK, 1, zlib.crc32(blob))
            assert bytes(arena.view[slot:slot + n + 28]) == blob == stored(gstore, "w-fp", n + 28)
            assert srv.stats()["fp_sse_writes"] == 1
        else:
            assert st == fp.UNSUPPORTED and bytes(arena.view[slot:slot + n + 28]) == before
            assert srv.stats()["fp_sse_writes"] == 0 and not gstore.exists("w-fp")
    finally:
        cli.close()
        arena.close()
        srv.stop()

"""SSE-S3 bodies through sse_gcm_kernel: AES-256-GCM in place on a registered buffer against
OpenSSL's ciphertext and tag, exact, with guard bytes where the nonce and the tag would lie.
The counter proves which path ran."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5
KEY = bytes(range(201, 233))
NONCE = bytes(range(50, 62))
LANE, WAVE, TILE, GRID = 64, 4 << 10, 16 << 10, 512
# every workgroup of the capped grid folds two tiles and some fold three; an odd tail
BIG = 2 * GRID * TILE + 3 * TILE + 5


@pytest.fixture(scope="module")
def gstore(native, tmp_path_factory):
    from rust_hadoop_generated_by_llm_amd import native as n

    assert n.gpu_count() > 0, "GPU tests need a HIP device"
    s = native.ChunkStore(str(tmp_path_factory.mktemp("sse")), "", 0, 256 << 20, 0, 100, 2, 1, False)
    assert s.gpu
    floor = native.sse_fused_min_bytes()
    native.set_sse_fused(True, 0)  # the kernel at every size; the store's own floor is a fallback case below
    yield s
    native.set_sse_fused(True, floor)
    del s


@functools.lru_cache(maxsize=None)
def reference(n):
    """Plaintext of n bytes and OpenSSL's ciphertext || tag for it."""
    from rust_hadoop_generated_by_llm_amd import native

    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    return pt, native.lib.aes256gcm_encrypt(KEY, NONCE, pt.tobytes(), b"")


def crypt(gstore, native, start, n, register=True):
    """Encrypts n bytes in place at buf[start:], checks bytes, tag and guards against OpenSSL, then
    decrypts: with the tag, with a flipped ciphertext byte, with a flipped tag bit. Returns by how
    much sse_fused_crypts moved during the encryption."""
    pt, sealed = reference(n)
    size = start + n + 48
    buf = native.pinned_array(size) if register else np.empty(size, dtype=np.uint8)
    buf[:] = GUARD
    body = buf[start:start + n]
    body[:] = pt
    if register:
        assert gstore.register_host(buf)
    try:
        before = gstore.stats()["sse_fused_crypts"]
        tag = gstore.sse_crypt(body, KEY, NONCE, True)
        moved = gstore.stats()["sse_fused_crypts"] - before
        assert body.tobytes() + tag == sealed
        assert (buf[:start] == GUARD).all() and (buf[start + n:] == GUARD).all()
        assert gstore.sse_crypt(body, KEY, NONCE, False, tag) == tag
        assert (body == pt).all()
        assert (buf[:start] == GUARD).all() and (buf[start + n:] == GUARD).all()
        body[:] = np.frombuffer(sealed[:n], dtype=np.uint8)
        body[n // 2] ^= 0x10
        with pytest.raises(RuntimeError, match="authentication failed"):
            gstore.sse_crypt(body, KEY, NONCE, False, tag)
        body[:] = np.frombuffer(sealed[:n], dtype=np.uint8)
        with pytest.raises(RuntimeError, match="authentication failed"):
            gstore.sse_crypt(body, KEY, NONCE, False, bytes([tag[0] ^ 1]) + tag[1:])
    finally:
        if register:
            gstore.unregister_host(buf)
    return moved


LENGTHS = [1, 15, 16, 17, LANE - 1, LANE, LANE + 1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, BIG]


@pytest.mark.parametrize("a,n", [(12, n) for n in LENGTHS] +  # where a slot's body lies: behind a 12-byte nonce
                         [(a, n) for a in (0, 4, 8) for n in (17, WAVE + 1, TILE + 1, BIG)])
def test_kernel_matches_openssl(gstore, native, a, n):
    assert crypt(gstore, native, 16 + a, n) == 1


@pytest.mark.parametrize("why", ["unregistered", "misaligned", "switched-off", "below-the-floor"])
def test_fallbacks_give_the_same_bytes(gstore, native, why):
    native.set_sse_fused(why != "switched-off", TILE + 18 if why == "below-the-floor" else 0)
    try:
        assert crypt(gstore, native, 16 + (1 if why == "misaligned" else 12), TILE + 17, why != "unregistered") == 0
    finally:
        native.set_sse_fused(True, 0)


def test_fast_path_op(gstore, native, can_pin_existing_memory):
    """A client slot through fast-path op 10 gives OpenSSL's bytes and moves the counters. Where the
    host cannot pin a client's arena the kernel cannot reach the slot: the op declines and leaves
    the bytes alone, and the client encrypts on its own CPU."""
    import os

    from rust_hadoop_generated_by_llm_amd.utils import fastpath as fp
    from rust_hadoop_generated_by_llm_amd.utils.shm import ShmArena

    n = TILE + 17
    pt, sealed = reference(n)
    srv = native.FastPathServer(gstore, f"dfs_fp_sse_{os.getpid()}")
    ok, err = srv.start()
    assert ok, err
    arena = ShmArena(size=1 << 20, slot=1 << 19)
    cli = fp.FastPathClient(srv.name)
    try:
        slot = arena.acquire(n + 28)
        arena.view[slot + 12:slot + 12 + n] = pt.tobytes()
        before = gstore.stats()["sse_fused_crypts"]
        st, tag = cli.sse_crypt(arena.path, slot + 12, n, KEY, NONCE, True)
        if can_pin_existing_memory:
            assert st == fp.OK and bytes(arena.view[slot + 12:slot + 12 + n]) + tag == sealed
            assert gstore.stats()["sse_fused_crypts"] - before == 1 and srv.stats()["fp_sse_crypts"] == 1
            bad = bytes([tag[0] ^ 1]) + tag[1:]
            assert cli.sse_crypt(arena.path, slot + 12, n, KEY, NONCE, False, bad)[0] == fp.AUTH_FAILED
        else:
            assert st == fp.UNSUPPORTED and bytes(arena.view[slot + 12:slot + 12 + n]) == pt.tobytes()
            assert gstore.stats()["sse_fused_crypts"] == before and srv.stats()["fp_sse_crypts"] == 0
        assert cli.sse_crypt(arena.path, (1 << 63) + 12, n, KEY, NONCE, True)[0] == fp.BAD_REQUEST
    finally:
        cli.close()
        arena.close()
        srv.stop()

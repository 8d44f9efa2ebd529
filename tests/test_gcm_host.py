"""The host half of the SSE kernel (gcm_host): GHASH through the kernel's tile cut, its log tree
and the fold of its workgroup partials, against OpenSSL's AES-256-GCM tags, exact."""
import numpy as np
import pytest

TILE = 16 << 10  # 1024 blocks of 16 B
KEY = bytes(range(7, 39))
NONCE = bytes(range(100, 112))


@pytest.mark.parametrize("grid", [0, 2], ids=["grid", "two-workgroups"])
@pytest.mark.parametrize("n", [0, 1, 16, 17, TILE - 1, TILE, TILE + 1, 5 * TILE + 333])
def test_ghash_closes_openssl_tag(native, n, grid):
    """tag = E_K(J0) xor GHASH(ct); E_K(J0) is the tag of the empty message. With a grid of two
    the 5-tile message makes each workgroup fold several tiles (the jump power)."""
    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    sealed = native.aes256gcm_encrypt(KEY, NONCE, pt, b"")
    ct, tag = sealed[:n], sealed[n:]
    tag0 = native.aes256gcm_encrypt(KEY, NONCE, b"", b"")
    ghash = native.gcm_ghash(KEY, ct, grid)
    assert tag == bytes(a ^ b for a, b in zip(tag0, ghash))

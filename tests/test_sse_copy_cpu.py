"""CopyObject of SSE-S3 objects without a GPU: ChunkStore.sse_copy on a host store takes the staged
route and must store OpenSSL's blob under the new key; and a native gateway with the offload on,
whose chunkserver declines fast-path op 14 here, must fall through to the copy it always made."""
import zlib

import numpy as np
import pytest
import requests

from rust_hadoop_generated_by_llm_amd.cluster.launcher import ROOT, LocalCluster
from rust_hadoop_generated_by_llm_amd.native import lib as native

KEY_A, NONCE_A = bytes(range(201, 233)), bytes(range(50, 62))
KEY_B, NONCE_B = bytes(range(7, 39)), bytes(range(90, 102))
OK, NOT_FOUND = 0, 1


@pytest.mark.parametrize("n", [17, (16 << 10) + 5])
def test_host_store_copy_matches_openssl(tmp_path, n):
    s = native.ChunkStore(str(tmp_path / "data"), "", -1, 0, 0, 100, 2, 1, False)
    assert not s.gpu
    pt = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    old = NONCE_A + native.aes256gcm_encrypt(KEY_A, NONCE_A, pt, b"")
    new = NONCE_B + native.aes256gcm_encrypt(KEY_B, NONCE_B, pt, b"")
    assert s.write("src", old, 0)[0]
    st, crc, err = s.sse_copy("src", "dst", KEY_A, KEY_B, NONCE_B)
    assert (st, crc) == (OK, zlib.crc32(new)), err
    assert s.read("dst", 0, n + 28)[2] == new and s.read("src", 0, n + 28)[2] == old
    assert s.stats()["sse_fused_copies"] == 0 and not s.sse_copy_fusable("src", "dst2")
    assert s.sse_copy("nope", "dst3", KEY_A, KEY_B, NONCE_B)[0] == NOT_FOUND and not s.exists("dst3")


def test_gateway_copy_falls_through_when_the_op_declines():
    if not (ROOT / "build" / "native" / "dfs_s3_gateway").exists():
        pytest.fail("dfs_s3_gateway is not built (python build_native.py)")
    with LocalCluster(n_chunkservers=1, fsync=False) as cluster:
        u = cluster.start_s3({"SSE_MASTER_KEY": "ab" * 32, "AUDIT_LOG_ENABLED": "false", "DFS_SSE_OFFLOAD": "1",
                              "LOCAL_CHUNKSERVER": cluster.cs_addrs[0]}, name="s3copy")
        data = np.random.default_rng(5).integers(0, 256, 300_001, dtype=np.uint8).tobytes()
        assert requests.put(f"{u}/cp").status_code == 200
        put = requests.put(f"{u}/cp/obj", data=data)
        assert put.status_code == 200
        r = requests.put(f"{u}/cp/copy", headers={"x-amz-copy-source": "/cp/obj"})
        assert r.status_code == 200 and put.headers["ETag"] in r.text
        got = requests.get(f"{u}/cp/copy")
        assert got.content == data and got.headers["ETag"] == put.headers["ETag"]
        c = cluster.client()
        deks = [c.get_file_info(p).attributes["x-amz-sse-encrypted-dek"] for p in ("/cp/obj", "/cp/copy")]
        assert deks[0] != deks[1]

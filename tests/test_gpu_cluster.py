"""End-to-end on a real MI355X: a ChunkServer bound to GPU 0 (HBM chunk store, HIP CRC /
range-verify kernels) behind a master, driven through the client, the CLI benchmark and
the S3 gateway. CPU-only twins of these paths live in test_cluster.py / test_s3_gateway.py.
"""
import json
import os
import time
import urllib.request

import pytest
import requests

from rust_hadoop_generated_by_llm_amd.cli import dfs_cli
from rust_hadoop_generated_by_llm_amd.cluster.launcher import LocalCluster

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_cluster():
    from rust_hadoop_generated_by_llm_amd import native

    if native.gpu_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    with LocalCluster(gpus=[0], fsync=True, hbm_capacity="4G", env={"DFS_DEBUG_ENDPOINTS": "1"}) as c:
        yield c


def stats(c):
    return json.load(urllib.request.urlopen(f"{c.cs_http[0]}/stats"))


def test_gpu_put_get_range_and_scrub(gpu_cluster):
    c = gpu_cluster.client()
    data = os.urandom((3 << 20) + 777)
    c.create_file_from_buffer(data, "/gpu/a")
    assert c.get_file_content("/gpu/a") == data
    assert c.read_file_range("/gpu/a", 1_000_001, 123_457) == data[1_000_001:1_123_458]
    st = stats(gpu_cluster)
    assert st["hbm_capacity"] > 0 and st["hbm_resident_blocks"] >= 1 and st["gpu_kernel_launches"] > 0
    blk = c.get_file_info("/gpu/a").blocks[0]
    # flip a byte in HBM + disk: the fused range-verify kernel must flag the slice
    r = json.load(urllib.request.urlopen(f"{gpu_cluster.cs_http[0]}/debug/corrupt?block={blk.block_id}&offset=2000000"))
    assert r["corrupted"]
    bad = json.load(urllib.request.urlopen(f"{gpu_cluster.cs_http[0]}/debug/scrub"))["bad"]
    assert bad == [blk.block_id]
    c.close()


def test_gpu_fused_reads_local_and_remote(can_pin_existing_memory, gpu_cluster):
    """Reads land through the fused K3 verify+copy kernel: into the co-located client's
    registered shm slot, and into the native gRPC server's registered reply buffers for a
    client that is not co-located (every RPC over gRPC/TCP)."""
    if not can_pin_existing_memory:
        pytest.skip("the GPU runtime here cannot pin memory a process already has (hipHostRegister refused)")  # the co-located client's arena is another process's shared memory
    data = os.urandom((2 << 20) + 333)
    c = gpu_cluster.client(local_chunkserver=gpu_cluster.cs_addrs[0])
    c.create_file_from_buffer(data, "/gpu/fz")
    # the fast path pins a client's shm arena on a background thread (no lock held on the
    # data path); until that lands, reads take the staged verify + DMA path
    f_init = stats(gpu_cluster)["fused_reads"]
    deadline = time.time() + 30
    while time.time() < deadline:
        assert c.get_file_content("/gpu/fz") == data
        if stats(gpu_cluster)["fused_reads"] > f_init:
            break  # this client's arena is pinned: every read from now on is fused
        time.sleep(0.05)
    f0 = stats(gpu_cluster)["fused_reads"]
    assert f0 > f_init
    assert c.get_file_content("/gpu/fz") == data
    # ranges land at slot + offset % 16 (client_fast.cpp), so unaligned ones are fused too
    assert c.read_file_range("/gpu/fz", 4096 + 48, 100_000) == data[4144:104_144]
    assert c.read_file_range("/gpu/fz", 777, 100_000) == data[777:100_777]
    assert c.read_file_range("/gpu/fz", (2 << 20) + 300, 1000) == data[(2 << 20) + 300:]
    f1 = stats(gpu_cluster)["fused_reads"]
    assert f1 - f0 >= 4
    rc = gpu_cluster.client(local_chunkserver=None, local_rpc=False)
    for _ in range(3):
        assert rc.get_file_content("/gpu/fz") == data
    assert rc.read_file_range("/gpu/fz", 1_048_577, 5) == data[1_048_577:1_048_582]
    assert stats(gpu_cluster)["fused_reads"] - f1 >= 3
    rc.close()
    c.close()


def test_gpu_remote_writes_land_in_registered_request_buffers(gpu_cluster):
    """A client that is not co-located writes over gRPC/TCP: the native server receives the
    WriteBlock into a registered, page-aligned request buffer and the client's alignment_pad
    puts the payload on a 16-byte boundary, so the block is staged by the fused copy+checksum
    kernel straight from where the socket put it (no bounce copy)."""
    rc = gpu_cluster.client(local_chunkserver=None, local_rpc=False)
    f0 = stats(gpu_cluster)["fused_writes"]
    blobs = {f"/gpu/rw{i}": os.urandom(sz) for i, sz in enumerate([(1 << 20), 300_001, (3 << 20) + 5])}
    for p, d in blobs.items():
        rc.create_file_from_buffer(d, p)
    for p, d in blobs.items():
        assert rc.get_file_content(p) == d
    assert stats(gpu_cluster)["fused_writes"] - f0 >= len(blobs)
    rc.close()


def test_gpu_cli_benchmark(gpu_cluster, capsys):
    m = ["-m", gpu_cluster.master_addrs[0]]
    assert dfs_cli.main([*m, "benchmark", "write", "-c", "20", "-s", "1048576", "-n", "10", "-p", "/gbw",
                         "--json"]) == 0
    w = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert w["ops"] == 20 and w["mb_per_s"] > 0
    assert dfs_cli.main([*m, "benchmark", "read", "-p", "/gbw", "-n", "10", "--json"]) == 0
    r = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert r["ops"] == 20 and r["bytes"] == 20 << 20


def test_gpu_s3_gateway(gpu_cluster):
    url = gpu_cluster.start_s3({"AUDIT_LOG_ENABLED": "false", "SSE_MASTER_KEY": "cd" * 32})
    assert requests.put(url + "/gbkt").status_code == 200
    body = os.urandom(2 << 20)
    assert requests.put(url + "/gbkt/obj", data=body).status_code == 200
    r = requests.get(url + "/gbkt/obj")
    assert r.status_code == 200 and r.content == body
    r = requests.get(url + "/gbkt/obj", headers={"Range": "bytes=100-199"})
    assert r.status_code == 206 and r.content == body[100:200]

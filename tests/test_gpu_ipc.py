"""The device replication transport between PROCESSES on one MI355X ("hipipc",
csrc/p2p_ipc.cpp): four ChunkServer processes share GPU 0, each exports its HBM arena over
HIP IPC, and every replica slice is a one-sided copy into the receiver's posted extent,
checksummed (K1) as it lands. Crossing RF=3 traffic from four co-located clients at
concurrency 10, blocks up to 64 MiB.

Run three ways: the production mode, receiver pull (the sender offers each slice, the
receiver's crc_write_copy_kernel reads it from the sender's arena, stores it and writes the
.meta words in one pass: one kernel per hop); the round-5 push mode (DFS_IPC_PULL=0: the
sender's copy kernel, then a checksum kernel on arrival); and spin mode, the RCCL emulation in which every send and receive is a kernel parked on its
channel stream until the peer shows up (p2p_kernels.hip) — the shape that can couple
unrelated streams through GPU_MAX_HW_QUEUES hardware queues. Reference semantics:
dfs/chunkserver/src/chunkserver.rs:777-829,1039-1077 (replicas_written)."""
import json
import os
import random
import time
import urllib.request
from concurrent.futures import ThreadPoolExecutor

import pytest

from rust_hadoop_generated_by_llm_amd.cluster.launcher import LocalCluster
from rust_hadoop_generated_by_llm_amd.models import proto as pb
from rust_hadoop_generated_by_llm_amd.utils.rpc import ChannelPool

pytestmark = pytest.mark.gpu


def stats(url):
    return json.load(urllib.request.urlopen(f"{url}/stats", timeout=10))


def run_crossing(c: LocalCluster, nfiles: int, sizes, seed: int):
    rng = random.Random(seed)
    clients = [c.client(local_chunkserver=a) for a in c.cs_addrs]
    jobs = [(i, rng.choice(sizes)) for i in range(nfiles)]
    payload = {i: os.urandom(sz) for i, sz in jobs}

    def one(job):
        i, _sz = job
        cl = clients[i % len(clients)]  # heads rotate over the four processes: crossing pairs
        cl.create_file_from_buffer(payload[i], f"/ipc/{seed}/f{i}")
        return i

    t0 = time.time()
    with ThreadPoolExecutor(10) as ex:
        done = list(ex.map(one, jobs))
    elapsed = time.time() - t0
    assert sorted(done) == [i for i, _ in jobs]
    # every replica holds the bytes (read each location directly over gRPC)
    pool = ChannelPool(local=False)
    try:
        for i, _sz in jobs:
            info = clients[0].get_file_info(f"/ipc/{seed}/f{i}")
            blk = info.blocks[0]
            assert len(blk.locations) == 3, blk
            for loc in blk.locations:
                r = pool.call(f"http://{loc}", "ChunkServerService", "ReadBlock",
                              pb.ReadBlockRequest(block_id=blk.block_id), timeout=60)
                assert r.data == payload[i], (i, loc)
    finally:
        pool.close()
        for cl in clients:
            cl.close()
    return elapsed


def totals(c: LocalCluster):
    agg = {}
    for u in c.cs_http:
        s = stats(u)
        for k in ("fp_rccl_forwards", "fp_p2p_fallbacks", "fp_replica_failures", "fp_shm_forwards",
                  "repl_pair_failures", "repl_turn_timeouts", "repl_bytes_recv", "grpc_forwards", "pulled_recvs",
                  "repl_pull_peers"):
            agg[k] = agg.get(k, 0) + s.get(k, 0)
        agg.setdefault("transports", set()).add(s.get("repl_transport"))
        agg.setdefault("pairs_up", 0)
        agg["pairs_up"] += s.get("repl_pairs_up", 0)
    return agg


@pytest.mark.parametrize("mode", ["hipipc", "hipipc-push", "hipipc-spin"])
def test_four_processes_one_gpu_crossing_traffic(mode, request):
    from rust_hadoop_generated_by_llm_amd import native

    if mode == "hipipc-spin" and native.gpu_count() >= 1 and not request.getfixturevalue("can_pin_existing_memory"):
        pytest.skip("the GPU runtime here cannot pin memory a process already has (hipHostRegister refused)")  # the spin kernels poll a shared-memory ring from the device

    if native.gpu_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    env = {"DFS_IPC_SPIN_MS": "4000"}
    transport = "hipipc" if mode == "hipipc-push" else mode
    if mode == "hipipc-push":
        env["DFS_IPC_PULL"] = "0"
    with LocalCluster(gpus=[0, 0, 0, 0], p2p=transport, fsync=False, hbm_capacity="6G", env=env) as c:
        base = totals(c)
        assert base["transports"] == {transport} and base["pairs_up"] == 12, base
        # odd sizes: a short tail slice (700,000 and 3 MiB + 17 B), several slices (64 MiB)
        sizes = [700_000, 1 << 20, 3 * (1 << 20) + 17, 64 << 20]
        elapsed = run_crossing(c, 48, sizes, seed={"hipipc": 7, "hipipc-push": 9}.get(mode, 8))
        t = totals(c)
        writes = 48
        print(f"\n{mode}: {writes} RF=3 writes in {elapsed:.2f}s; {t}")
        assert t["fp_rccl_forwards"] - base["fp_rccl_forwards"] == writes * 2, t
        assert t["fp_p2p_fallbacks"] == 0 and t["fp_replica_failures"] == 0 and t["fp_shm_forwards"] == 0, t
        assert t["repl_pair_failures"] == 0 and t["repl_turn_timeouts"] == 0, t
        # every replica of the pull mode came through the receivers' copy+checksum kernels
        pulled = t["pulled_recvs"] - base["pulled_recvs"]
        assert pulled == (writes * 2 if mode == "hipipc" else 0), t
        assert t["repl_pull_peers"] == (12 if mode == "hipipc" else 0), t
        assert elapsed < 120

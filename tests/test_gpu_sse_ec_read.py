"""GETs of SSE-S3 objects held as RS(k, m) shards through sse_ec_read_kernel: OpenSSL's blob of a seeded
plaintext, cut into data columns with the CPU codec's parity, written as resident blocks, must come
back as that plaintext, byte for byte, between intact guard bytes. The counters prove which route ran."""
import functools
import json
import time
import urllib.request

import numpy as np
import pytest

from rust_hadoop_generated_by_llm_amd import native as _native
from rust_hadoop_generated_by_llm_amd.cluster.launcher import LocalCluster
from rust_hadoop_generated_by_llm_amd.ops import erasure

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes(range(101, 133)), bytes(range(30, 42))
MIN, TILE, GRID = _native.lib.sse_ec_read_min_shard, _native.lib.sse_read_tile_bytes, _native.lib.sse_read_max_grid
OK, NOT_FOUND, CORRUPT, AUTH_FAILED, IO_ERROR = range(5)
GUARD = 0xA5
ODD = MIN + 3


@pytest.fixture(scope="module")
def gstore(native, tmp_path_factory):
    assert _native.gpu_count() > 0, "GPU tests need a HIP device"
    s = native.ChunkStore(str(tmp_path_factory.mktemp("sse_ec_read")), "", 0, 1 << 30, 0, 100, 2, 1, False)
    assert s.gpu
    floor = native.sse_ec_read_fused_min_bytes()
    native.set_sse_ec_read_fused(True, 0)
    yield s
    native.set_sse_ec_read_fused(True, floor)
    del s


@functools.lru_cache(maxsize=None)
def sealed(orig):
    """A seeded plaintext of orig - 28 bytes and OpenSSL's blob of it."""
    pt = np.random.default_rng(orig).integers(0, 256, orig - 28, dtype=np.uint8).tobytes()
    return pt, NONCE + _native.lib.aes256gcm_encrypt(KEY, NONCE, pt, b"")


@functools.lru_cache(maxsize=None)
def reference(k, m, sl, orig):
    """That plaintext and the k + m shards of its blob."""
    pt, blob = sealed(orig)
    assert len(blob) == orig and (orig + k - 1) // k <= sl
    blob += bytes(k * sl - orig)
    shards = [blob[c * sl:(c + 1) * sl] for c in range(k)]
    return pt, shards + list(_native.lib.gf_matmul_cpu(erasure.parity_matrix(k, m), shards, sl))


def read(gstore, k, m, sl, orig, lost, key=KEY, register=True, corrupt=None):
    """sse_ec_read behind 16 guard bytes. Returns (status, n, the n bytes, sse_fused_ec_reads moved,
    launches moved) after checking the guards."""
    pt, shards = reference(k, m, sl, orig)
    n = len(pt)
    ids = ["" if i in lost else f"sec_{k}_{m}_{sl}_{orig}_{i}" for i in range(k + m)]
    buf = _native.lib.pinned_array(16 + n + 64) if register else np.empty(16 + n + 64, dtype=np.uint8)
    buf[:] = GUARD
    for bid, s in zip(ids, shards):
        if bid:
            assert gstore.write(bid, s, _native.lib.crc32(s))[0]
    if corrupt is not None:
        assert gstore.debug_corrupt(ids[corrupt], 777)
    if register:
        assert gstore.register_host(buf)
    try:
        before = gstore.stats()
        st, got, _err = gstore.sse_ec_read(ids, k, m, sl, orig, key, buf[16:16 + n])
        after = gstore.stats()
    finally:
        if register:
            gstore.unregister_host(buf)
        for bid in filter(None, ids):
            gstore.remove(bid)
    assert (buf[:16] == GUARD).all() and (buf[16 + n:] == GUARD).all()
    return (st, got, buf[16:16 + n].tobytes(), after["sse_fused_ec_reads"] - before["sse_fused_ec_reads"],
            after["gpu_kernel_launches"] - before["gpu_kernel_launches"])


@pytest.mark.parametrize("k,m,sl,orig,lost", [
    (4, 2, MIN, 4 * MIN - 3, []),              # every shift 0, no rebuild
    (4, 2, ODD, 4 * ODD - 3, []),              # a shift per column; blocks and threads straddle boundaries
    (4, 2, ODD, 4 * ODD - 3, [0]),             # the nonce rebuilt
    (4, 2, ODD, 4 * ODD - 3, [3]),             # the tag and the zero padding rebuilt
    (4, 2, ODD, 4 * ODD - 3, [1, 2]),          # a boundary with both sides rebuilt
    (10, 4, 65539, 10 * 65539 - 9, [0, 3, 5, 9]),  # four rows, many inputs, parity survivors
    (2, 1, GRID * TILE - 10, 2 * GRID * TILE - 21, [0]),  # every workgroup takes a second step: hjump
    (4, 2, ODD, 4 * ODD, [2]),                 # no padding
], ids=["aligned", "odd", "nonce", "tag", "adjacent", "rows4", "two-steps", "full"])
def test_kernel_matches_plaintext(gstore, k, m, sl, orig, lost):
    pt, _ = reference(k, m, sl, orig)
    st, n, got, moved, launches = read(gstore, k, m, sl, orig, lost)
    assert (st, n, moved, launches) == (OK, len(pt), 1, 1)
    assert got == pt


@pytest.mark.parametrize("why", ["wrong-key", "flipped-shard"])
def test_refusals_leave_zeros(gstore, why):
    """This call does not checksum shards: a byte flipped in HBM must be caught by the tag."""
    st, n, got, moved, _ = read(gstore, 4, 2, ODD, 4 * ODD - 3, [1], key=bytes(32) if why == "wrong-key" else KEY,
                                corrupt=None if why == "wrong-key" else 4)
    assert (st, n, moved) == (AUTH_FAILED, 0, 1)
    assert not any(got)


@pytest.mark.parametrize("why,k,m,sl,lost", [
    ("unregistered", 4, 2, ODD, [1]),
    ("short-shards", 4, 2, MIN - 1, [1]),
    ("five-rows", 5, 5, ODD, [0, 1, 2, 3, 4]),
    ("switched-off", 4, 2, ODD, [1]),
    ("below-the-floor", 4, 2, ODD, [1]),
])
def test_staged_route_gives_the_same_bytes(gstore, native, why, k, m, sl, lost):
    orig = k * sl - (k - 1)
    pt, _ = reference(k, m, sl, orig)
    native.set_sse_ec_read_fused(why != "switched-off", len(pt) + 1 if why == "below-the-floor" else 0)
    try:
        st, n, got, moved, _ = read(gstore, k, m, sl, orig, lost, register=why != "unregistered")
    finally:
        native.set_sse_ec_read_fused(True, 0)
    assert (st, n, moved) == (OK, len(pt), 0)
    assert got == pt


def summed(c, key):
    return sum(json.load(urllib.request.urlopen(f"{u}/stats", timeout=10)).get(key, 0) for u in c.cs_http)


@pytest.fixture(scope="module")
def eccluster(has_gpu):
    if not has_gpu:
        pytest.fail("GPU test selected but no HIP device is visible")
    with LocalCluster(gpus=[0] * 6, p2p="hipipc", fsync=True, hbm_capacity="3G",
                      env={"DFS_DEBUG_ENDPOINTS": "1"}) as c:
        deadline = time.time() + 60  # the 30 pairs come up in the background after start
        while summed(c, "repl_pairs_up") != 30:
            assert time.time() < deadline
            time.sleep(0.2)
        yield c


def test_fast_client_reads_an_ec_file_through_op_15(eccluster, can_pin_existing_memory):
    """An RS(4,2) file holding an SSE blob, one data shard gone from its holder: FastClient.sse_read
    sends op 15, the chunkserver gathers four survivors, and one kernel rebuilds and decrypts. Where
    the host cannot pin a client's arena the kernel cannot reach the slot: the op declines before it
    gathers anything, and the client reads its own way."""
    c = eccluster
    cl = c.client(local_chunkserver=c.cs_addrs[0])
    try:
        pt, blob = sealed((1 << 20) + 333 + 28)
        cl.create_file_from_buffer_ec(blob, "/sseec/cold", 4, 2)
        info = cl.get_file_info("/sseec/cold")
        blk = info.blocks[0]
        lost = next(i for i, loc in enumerate(blk.locations) if i < 4 and loc != c.cs_addrs[0])
        holder = c.cs_http[c.cs_addrs.index(blk.locations[lost])]
        urllib.request.urlopen(f"{holder}/debug/remove?block={blk.block_id}", timeout=10).read()
        gathered = summed(c, "fp_ec_gathered")
        st, got = cl._fast.sse_read(info.SerializeToString(), KEY)
        if can_pin_existing_memory:
            assert st == 0 and got == pt
            assert summed(c, "fp_sse_ec_reads") == 1 and summed(c, "fp_ec_gathered") - gathered == 3
            assert cl._fast.sse_read(info.SerializeToString(), bytes(32)) == (2, None)  # authentication failure is final
            assert summed(c, "fp_sse_ec_reads") == 1
        else:
            assert (st, got) == (1, None)
            assert summed(c, "fp_sse_ec_reads") == 0 and summed(c, "fp_ec_gathered") == gathered
            assert cl.get_file_content("/sseec/cold") == blob
    finally:
        cl.close()

"""FastClient.sse_write_slot (CreateFile, fast-path op 13, CompleteFile) against a real master and a
stub fast-path server that answers op 13 as scripted: which outcomes leave the slot to the caller
(NotHandled, or Failed without `spent`) and which spend it, so that the gateway never sends a second
op 13 over a slot that already holds the blob."""
import hashlib
import mmap
import socket
import struct
import threading
import zlib

import pytest

from rust_hadoop_generated_by_llm_amd.cluster.launcher import LocalCluster
from rust_hadoop_generated_by_llm_amd.native import lib as native

KEY = bytes(range(7, 39))
NONCE = bytes(range(100, 112))
PLAIN = bytes(range(256)) * 5
BLOB = NONCE + native.aes256gcm_encrypt(KEY, NONCE, PLAIN, b"")
UNTOUCHED = bytes(12) + PLAIN + bytes(16)
OK, NOT_HANDLED, FAILED = 0, 1, 2
FP_OK, FP_IO_ERROR, FP_UNSUPPORTED = 0, 4, 6


class StubFastPath:
    """Answers each op 13 with the next entry of `script`: "seal" stores the blob into the client's slot
    and answers Ok with its CRC, after calling `before_reply()`; "drop"
    closes the connection unanswered; a number is answered as that status with the slot untouched."""

    def __init__(self, name):
        self.name, self.script, self.calls, self.before_reply = name, [], 0, None
        self.sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        self.sock.bind("\0" + name)
        self.sock.listen(4)
        threading.Thread(target=self._accept, daemon=True).start()

    def _accept(self):
        while True:
            try:
                conn, _ = self.sock.accept()
            except OSError:
                return
            threading.Thread(target=self._serve, args=(conn,), daemon=True).start()

    def _serve(self, conn):
        def exact(n):
            buf = b""
            while len(buf) < n:
                part = conn.recv(n - len(buf))
                if not part:
                    raise EOFError
                buf += part
            return buf

        try:
            while True:
                (n,) = struct.unpack("<I", exact(4))
                body = exact(n)
                assert body[0] == 13
                self.calls += 1
                _term, off, length = struct.unpack_from("<QQQ", body, 1)
                fields, at = [], 25
                for _ in range(4):  # block id, arena path, key, nonce
                    (ln,) = struct.unpack_from("<H", body, at)
                    fields.append(body[at + 2:at + 2 + ln])
                    at += 2 + ln
                assert fields[2:] == [KEY, NONCE] and length == len(BLOB)
                step = self.script.pop(0)
                if step == "drop":
                    return
                msg = b""
                if step == "seal":
                    with open(fields[1].decode(), "r+b") as f, mmap.mmap(f.fileno(), 0) as m:
                        m[off:off + length] = BLOB
                    if self.before_reply:
                        self.before_reply()
                    step, msg = FP_OK, b"%08x" % zlib.crc32(BLOB)
                conn.sendall(struct.pack("<I", 19 + len(msg)) + struct.pack("<BQQH", step, length, 1, len(msg)) + msg)
        except EOFError:
            pass
        finally:
            conn.close()

    def close(self):
        self.sock.close()


@pytest.fixture(scope="module")
def rig():
    import os

    with LocalCluster(n_chunkservers=1, fsync=False) as cl:
        c = cl.client(local_chunkserver=cl.cs_addrs[0])
        stub = StubFastPath(f"dfs_fp_stub_{os.getpid()}")
        fc = native.FastClient(stub.name, cl.cs_addrs[0], 8 << 20, 1 << 20, 2)
        c.add_native_routing(fc)
        yield c, stub, fc, cl.cs_addrs[0]
        stub.close()
        c.close()


def put(fc, path):
    return fc.sse_write_slot(path, PLAIN, KEY, NONCE, hashlib.md5(PLAIN).hexdigest())


def test_sealed_put_completes_with_the_reply_crc(rig):
    c, stub, fc, _ = rig
    stub.script, stub.before_reply = ["seal"], None
    st, spent, msg, slot = put(fc, "/ssew/ok")
    assert (st, slot) == (OK, BLOB), msg
    info = c.get_file_info("/ssew/ok")
    assert info.size == len(BLOB) and info.etag_md5 == hashlib.md5(PLAIN).hexdigest()


@pytest.mark.parametrize("answer", [FP_UNSUPPORTED, "no-server"])
def test_declined_leaves_the_slot_to_the_caller(rig, answer):
    c, stub, fc, cs_addr = rig
    stub.script = [answer]
    if answer == "no-server":
        fc = native.FastClient("dfs_fp_nonexistent", cs_addr, 8 << 20, 1 << 20, 2)
        c.add_native_routing(fc)
    st, spent, _, slot = put(fc, f"/ssew/declined-{answer}")
    assert (st, spent, slot) == (NOT_HANDLED, False, UNTOUCHED)


@pytest.mark.parametrize("answer", [FP_IO_ERROR, "drop"])
def test_failure_after_the_op_spends_the_slot(rig, answer):
    _, stub, fc, _ = rig
    stub.script = [answer]
    st, spent, _, _ = put(fc, f"/ssew/failed-{answer}")
    assert (st, spent) == (FAILED, True)


def test_existing_key_is_refused_before_the_op(rig):
    """CreateFile refuses the key: the slot still holds the plaintext and remove-and-retry applies."""
    c, stub, fc, _ = rig
    c.create_file_from_buffer(b"old", "/ssew/old")
    stub.script, calls = [], stub.calls
    st, spent, msg, slot = put(fc, "/ssew/old")
    assert (st, spent, slot) == (FAILED, False, UNTOUCHED) and "already exists" in msg
    assert stub.calls == calls


def test_key_created_during_the_op_spends_the_slot(rig):
    """A rival PUT of the key completes while op 13 runs: CompleteFile answers "already exists" with the
    blob already in the slot. `spent` tells the caller not to send op 13 over it again, which would
    apply the same keystream twice and store the plaintext; the rival's object stays."""
    c, stub, fc, _ = rig
    stub.script = ["seal"]
    stub.before_reply = lambda: c.create_file_from_buffer(b"rival", "/ssew/raced")
    st, spent, msg, slot = put(fc, "/ssew/raced")
    assert (st, spent, slot) == (FAILED, True, BLOB) and "already exists" in msg
    assert c.get_file_content("/ssew/raced") == b"rival"

// Native local data path of a ChunkServer ("fast path").
//
// HDFS serves co-located readers through UNIX domain sockets + shared memory
// (short-circuit local reads). This is the same idea for both directions, handled
// entirely in C++: a client on the same host puts a block into its /dev/shm arena slot
// and sends a ~100-byte request over an abstract UNIX socket; the server thread stages
// it into HBM (H2D DMA + CDNA4 CRC kernel), persists it and answers — no Python, no GIL,
// no HTTP/2 framing on the ChunkServer side. Reads DMA the verified range from HBM
// straight into the client's slot.
//
// Scope: WriteBlock (locally, and along same-node RCCL chains) and ReadBlock. Anything
// else — cross-node hops, corruption needing recovery, fenced or malformed requests — is
// answered with a status telling the client to use the regular gRPC service, which keeps
// every semantic of the reference (fencing, recovery, replicas_written) in one place.
//
// Wire format (little endian), one request/response pair at a time per connection:
//   request  = u32 body_len | u8 op | body
//     op 1 WRITE: u64 term | u32 crc | u64 shm_off | u64 len | u16 id_len id | u16 path_len path
//               [| u16 n_next | (u16 len addr)*]      -- replicas, fanned out natively
//     op 2 READ : u64 offset | u64 length | u64 shm_off | u64 shm_cap | u16 id_len id | u16 path_len path
//     op 3 REPL : u64 term | u32 crc | i32 src_rank | u64 gen | i64 seq | u64 size | u64 slice
//               | u16 id_len id | u16 n_next | (u16 len addr)*   -- payload over the P2P transport
//     op 4 REPL_SHM: u64 term | u32 crc | u64 shm_off | u64 len | u16 id_len id | u16 path_len path
//               | u16 n_next | (u16 len addr)*      -- same-host hop without a P2P pair: read the client slot
//     op 5 CTRL : u16 len blob                       -- replication control (pair bring-up / rebuild)
//     op 6 EC   : u16 k | u16 rows | u64 len | u64 in_off | u64 out_off | u16 rows*k matrix | u16 path
//               [| u16 rid]  -- GF(2^8) matrix x shards (RS encode / reconstruct) on this GPU;
//               shards sit in the client's slot at 16-byte-aligned strides, outputs land there
//     op 7 EC_WRITE: u64 term | u16 k | u16 m | u64 shard_len | u64 shm_off | u64 shm_stride | u16 id
//               | u16 path | u16 n | (u16 len addr)* (k + m targets) [| u16 rid]
//               -- device-resident RS write: the k stripes go up once, parity is computed in
//               HBM, every shard is checksummed there and scattered HBM -> HBM over the engine
//     op 8 EC_READ: u64 offset | u64 length | u16 k | u16 m | u64 shard_len | u64 orig | u64 shm_off
//               | u64 shm_cap | u16 id | u16 path | u16 n | (u16 len addr)* ("" = lost) [| u16 rid]
//               -- degraded read: surviving shards gathered into this GPU, missing data decoded
//               there, the requested range DMA'd into the client's slot
//     op 9 PUSH: u16 id | u16 as_id | u16 dst_addr [| u16 rid] -- send local block `id` to the
//               same-node peer `dst_addr` over the engine, stored there as ephemeral `as_id`
//     op 10 SSE_CRYPT: u8 encrypt | u64 shm_off | u64 len | u16 key(32) | u16 nonce(12) | u16 tag(16, or
//               empty to encrypt) | u16 path [| u16 rid]  -- AES-256-GCM of SSE-S3 in place over the body in
//               the client's slot, by sse_gcm_kernel; answers Ok with the tag as 32 hex digits in msg,
//               AuthFailed, or Unsupported when the kernel would not take it (no GPU, slot not pinned,
//               below the store's floor): the client then encrypts on its own CPU
//     op 11 SSE_READ: u64 shm_off | u64 cap | u16 id | u16 key(32) | u16 path [| u16 rid]  -- GET of the stored
//               SSE-S3 blob `id` ([nonce][ciphertext][tag]) by sse_read_kernel: verified, authenticated,
//               decrypted, and only the plaintext stored at the front of the client's slot; answers Ok with
//               total = the blob's size and bytes = n, NotFound, Corrupt, AuthFailed, or Unsupported when
//               ChunkStore::sse_read_fusable says the kernel would not take it: the client then reads and
//               decrypts its own way. The key crosses only this peer-checked abstract socket.
//     op 12 SSE_READ_RANGE: u64 shm_off | u64 cap | u64 from | u64 want | u16 id | u16 key(32) | u16 path [| u16 rid]
//               -- Range GET of the same blob by sse_read_range_kernel: the whole blob verified and
//               authenticated, plaintext [from, from + want) alone decrypted and stored at shm_off + from % 16
//               of the client's slot (cap counts from shm_off); answers as op 11 with bytes = want and
//               total = the blob's size. want == 0 is BadRequest; a range past the plaintext's end IoError.
//     op 13 SSE_WRITE: u64 term | u64 shm_off | u64 len | u16 id | u16 path | u16 key(32) | u16 nonce(12)
//               [| u16 n_next | (u16 len addr)*] [| u16 rid]  -- PUT of an SSE-S3 object by sse_write_kernel: the
//               slot holds [12 free][plaintext len - 28][16 free] at shm_off and afterwards the blob
//               [nonce][ciphertext][tag], stored as block `id`, persisted and fanned out to `next` as op 1
//               does; answers Ok with bytes = replicas written and msg = the blob's CRC-32 as 8 hex digits.
//               Unsupported only while the slot is untouched (ChunkStore::sse_write_fusable says no, a
//               replica off this host, the arena not mapped or pinned): the client then encrypts and writes
//               its own way. Fenced, BadRequest (key or nonce length, len < 29), IoError after the launch.
//     op 14 SSE_COPY: u64 term | u16 src_id | u16 dst_id | u16 path | u16 key_src(32) | u16 key_dst(32) | u16 nonce(12)
//               [| u16 n_next | (u16 len addr)*] [| u16 rid]  -- CopyObject of an SSE-S3 object by sse_rekey_kernel:
//               the stored blob `src_id` verified, authenticated, re-keyed under (key_dst, nonce) and stored,
//               durable, as block `dst_id`, HBM to HBM: no slot is used (`path` only names the client's
//               arena and may be empty), then persisted from device memory and fanned out to `next` from
//               HBM as a mid-chain op 3 forwards (replicate with no shared-memory source: the engine pins
//               the resident block by its id). Answers as op 13, Ok with bytes = replicas written and msg =
//               the new blob's CRC-32 as 8 hex digits, or as op 11 NotFound, Corrupt or AuthFailed, after
//               which `dst_id` does not exist. Unsupported only while nothing has been done:
//               ChunkStore::sse_copy_fusable says no, or some server of `next` has no device P2P pair up
//               (with no slot there is no shared-memory fallback, so that replica would only be counted
//               as failed): the client then copies its own way.
//     op 15 SSE_EC_READ: u16 k | u16 m | u64 shard_len | u64 orig | u64 shm_off | u64 shm_cap | u16 id | u16 key(32)
//               | u16 path | u16 n | (u16 len addr)* ("" = lost) [| u16 rid]  -- GET of an SSE-S3 object held as
//               an RS(k, m) file, whole object only: the surviving shards gathered into this GPU as op 8
//               gathers them, then sse_ec_read_kernel rebuilds the lost columns, authenticates, decrypts and
//               stores only the plaintext at the front of the client's slot. Answers as op 11: Ok with
//               total = orig and bytes = orig - 28, AuthFailed (final), or Unsupported when
//               ChunkStore::sse_ec_read_fusable says no (asked before anything is gathered), the gather is
//               unavailable or ChunkStore::sse_ec_read declines: the client then reads and decrypts its
//               own way.
//   response = u32 body_len | u8 status | u64 total | u64 bytes | u16 msg_len msg
//   (for WRITE/REPL ``bytes`` carries replicas_written; for CTRL ``msg`` is the engine reply)
//
// Replication stays native when every replica is a ChunkServer of this host. The head
// stages the block in HBM (H2D + CRC kernel) and FANS OUT to all replicas at once: over the
// P2P transport (RCCL/xGMI, slices pipelined with the receiver's checksum kernel) where the
// pair is up, else the replica stages straight from the client's shared-memory slot. Each
// path overlaps the local fdatasync. A replica that fails is not counted (replicas_written
// shrinks, like the reference's chain); a replica off this host makes the head answer
// Unsupported and the client redoes the write on the gRPC path.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "chunk_store.h"
#include "io_pool.h"
#include "replication.h"

namespace dfs {

enum class FpStatus : uint8_t {
  Ok = 0,
  NotFound = 1,
  OutOfRange = 2,
  Corrupt = 3,      // use gRPC: the Python service recovers from a replica
  IoError = 4,
  Fenced = 5,       // stale master term
  Unsupported = 6,  // use gRPC
  BadRequest = 7,
  PartialCorrupt = 8,  // data returned; block queued for background recovery
  AuthFailed = 9,      // SSE_CRYPT: the tag does not match (final: no path will decrypt these bytes)
};

struct FpStats {
  uint64_t writes = 0, reads = 0, fenced = 0, punts = 0, connections = 0;
  uint64_t replicas_in = 0, rccl_forwards = 0, shm_forwards = 0, forward_failures = 0;
  uint64_t rejected_peers = 0;  // connections from another uid (SO_PEERCRED)
  uint64_t replica_failures = 0;  // replicas that could not be written (not counted)
  uint64_t p2p_fallbacks = 0;     // replicas moved to shared memory after a P2P failure
  uint64_t ec_ops = 0;            // erasure-coding matrix products run for clients
  uint64_t sse_crypts = 0;        // SSE bodies encrypted or decrypted in clients' slots
  uint64_t sse_reads = 0;         // stored SSE blobs decrypted into clients' slots by one kernel
  uint64_t sse_writes = 0;        // SSE bodies encrypted in clients' slots and stored by one kernel
  uint64_t sse_copies = 0;        // stored SSE blobs re-keyed into new blocks by one kernel
  uint64_t sse_ec_reads = 0;      // SSE blobs held as RS shards gathered, rebuilt and decrypted into clients' slots by one kernel
  uint64_t heals_out = 0, heals_in = 0;  // heal / balancer copies sent / received on the engine
  uint64_t sliced_writes = 0;  // head writes whose replica sends overlapped the staging
  // device-resident erasure coding: EC writes whose shards were encoded and scattered HBM ->
  // HBM, shards forwarded that way, degraded reads / reconstructions gathered into HBM and
  // decoded there, shards pulled for a gather, and requests that had to take the host path
  uint64_t ec_device_writes = 0, ec_shard_forwards = 0, ec_device_reads = 0, ec_device_decodes = 0;
  uint64_t ec_gathered = 0, ec_device_fallbacks = 0;
  // chained head writes (below the sliced size): staging + checksum, then the local persist
  // and replica fan-out together (ns summed); each device forward's descriptor round trip
  // (from its sends being posted to the replica's reply)
  uint64_t chain_writes = 0, chain_stage_ns = 0, chain_forward_ns = 0;
  uint64_t desc_calls = 0, desc_ns = 0;
};

class FastPathServer {
 public:
  FastPathServer(ChunkStore* store, std::string name);
  ~FastPathServer();
  FastPathServer(const FastPathServer&) = delete;
  FastPathServer& operator=(const FastPathServer&) = delete;

  bool start(std::string* err);
  void stop();
  // Abstract-namespace socket name (without the leading NUL), e.g. "dfs_fp_1234_50051".
  const std::string& name() const { return name_; }

  // Epoch fencing shared with the gRPC service: rejects 0 < term < known, adopts higher.
  bool fence(uint64_t term, uint64_t* known);
  void adopt_term(uint64_t term);
  uint64_t term() const { return term_.load(); }

  std::vector<std::string> drain_suspects();  // blocks needing background recovery
  // The request ids of the last few data-path ops served here (newest last): lets tests and
  // operators follow one client request across the head and every replica.
  std::vector<std::string> recent_request_ids();
  FpStats stats();

  // Native replication: this server's engine (RCCL or socket transport) and the fast-path
  // socket of every same-node peer (advertised address -> rank, socket name).
  void set_replication(ReplicationEngine* engine);
  void set_peer(const std::string& addr, int rank, const std::string& fp_name);
  // Control exchange with the fast path of the peer of `rank` (the engine's ControlFn).
  bool control(int rank, const std::string& req, std::string* reply);
  // For the native gRPC service (cs_grpc.cpp): whether every address is a same-host peer
  // this server can replicate to natively; persist a staged block while fanning it out to
  // `next` (the replicas count written downstream); queue a block for background recovery.
  bool all_local(const std::vector<std::string>& next);
  bool p2p_ready(const std::vector<std::string>& next);  // every hop has a P2P pair up
  bool persist_and_replicate(const std::string& id, const uint8_t* host, uint64_t n, uint32_t crc, uint64_t term,
                             const std::vector<std::string>& next, int* downstream, std::string* err);
  void add_suspect(const std::string& id);
  // For the native gRPC chain (dfs_chunkserver): a client's shared-memory slot
  // [off, off+len) (nullptr + *err when it is not mappable here), the replication engine,
  // and one replica pushed to a same-node `addr` over it (replicas written, 0 = failed).
  uint8_t* map_client_shm(const std::string& path, uint64_t off, uint64_t len, std::string* err) {
    return map_shm(path, off, len, err);
  }
  ReplicationEngine* replication() const { return repl_; }
  int replicate_to(const std::string& addr, const std::string& id, uint32_t crc, uint64_t term, const uint8_t* host,
                   uint64_t n, bool heal) {
    return replicate_one(addr, id, crc, term, ShmSrc{}, host, n, heal);
  }
  // Heal / balancer / shuffle copy (master REPLICATE command; reference chunkserver.rs:462-499)
  // of a block held here to same-node `targets`, payload over the replication engine (HBM ->
  // HBM on device transports), descriptor on the peers' fast-path sockets. Returns the
  // replicas written; a target that is not reachable this way counts 0 (the caller falls
  // back to gRPC for it).
  int replicate_block(const std::string& id, const std::vector<std::string>& targets, uint64_t term,
                      std::vector<std::string>* done);
  // Blocks received as heal copies since the last call (reported to the masters as new
  // locations by the heartbeat).
  std::vector<std::string> drain_healed();
  void note_rid(const std::string& rid);  // record a served request id (recent_request_ids)
  // Test hook: the next `n` REPL descriptors are dropped on the way out.
  void debug_drop_descriptors(int n) { drop_descriptors_ += n; }
  void set_self_host(const std::string& host);  // our advertised host: same-host peer detection
  void set_self_addr(const std::string& addr);  // our advertised address (EC targets that are us)

  // Device gather of EC shards into this GPU (degraded reads, RECONSTRUCT_EC_SHARD): each
  // shard held here is pinned in place, each held by a same-node peer is pushed over the
  // replication engine into an ephemeral block here. ptrs[i] = device pointer (nullptr:
  // lost, skipped or unreachable). The destructor unpins and drops what it gathered.
  struct EcGather {
    FastPathServer* fp = nullptr;
    std::vector<const uint8_t*> ptrs;
    std::vector<std::string> pinned, temps;
    int unreachable = 0;  // shards that exist but could not be gathered over the engine
    uint64_t len = 0;     // shard length (given, or the length the gathered shards agree on)
    ~EcGather();
  };
  bool ec_gather(const std::string& id, const std::vector<std::string>& locations, uint64_t shard_len, int skip,
                 int want, EcGather* g, std::string* err);

 private:
  struct Peer {
    int rank = -1;
    std::string name;
    std::mutex mu;
    std::vector<int> idle;  // pooled connections to the peer's fast-path socket
  };
  void accept_loop();
  void serve(int fd);
  // Maps the client arena and checks [off, off+len) lies inside it (overflow-safe).
  uint8_t* map_shm(const std::string& path, uint64_t off, uint64_t len, std::string* err);
  struct ShmSrc {
    std::string path;  // client arena the block came from (empty: HBM-only, e.g. P2P-received)
    uint64_t off = 0, len = 0;
  };
  // Fan block `id` out to every address in `next` (all same-host); *replicas = replicas
  // written downstream. `host` is the block in host memory when there is one (shm slot).
  void replicate(const std::string& id, uint32_t crc, uint64_t term, const std::vector<std::string>& next,
                 const ShmSrc& src, const uint8_t* host, uint64_t n, int* replicas,
                 const StagedSource* staged = nullptr);
  int replicate_one(const std::string& addr, const std::string& id, uint32_t crc, uint64_t term, const ShmSrc& src,
                    const uint8_t* host, uint64_t n, bool heal = false, const StagedSource* staged = nullptr,
                    bool ephemeral = false);
  bool is_self(const std::string& addr) const;
  // op 7 / op 8 / op 9 bodies (answered on fd)
  bool ec_write(int fd, const uint8_t* body, const uint8_t* end);
  bool ec_read(int fd, const uint8_t* body, const uint8_t* end);
  bool sse_ec_read(int fd, const uint8_t* body, const uint8_t* end);
  bool push_block(int fd, const uint8_t* body, const uint8_t* end);
  // Pipelined head write of a large replicated block; false = not applicable (the caller
  // takes the stage-then-forward path), true = answered on `fd` (*sent = write result).
  bool write_sliced(int fd, const std::string& id, const uint8_t* host, uint64_t len, uint32_t crc, uint64_t term,
                    const std::vector<std::string>& next, const ShmSrc& src, bool* sent);
  bool exchange_with(struct Peer* p, const std::vector<uint8_t>& req, std::vector<uint8_t>* resp);
  Peer* local_peer(const std::string& addr);

  ChunkStore* store_;
  std::string name_;
  int lfd_ = -1;
  std::atomic<bool> stop_{false};
  std::atomic<uint64_t> term_{0};
  std::thread acceptor_;
  std::mutex mu_;
  int live_workers_ = 0;  // detached per-connection threads still running (guarded by mu_)
  std::condition_variable workers_cv_;
  std::vector<int> conns_;
  struct Mapping {
    uint8_t* p = nullptr;
    uint64_t size = 0;
    bool registered = false;  // hipHostRegister'ed for direct DMA
  };
  std::unordered_map<std::string, Mapping> maps_;
  int pending_regs_ = 0;  // arena registrations in flight (mu_); stop() waits for them
  std::vector<Mapping> retired_;
  std::vector<std::string> suspects_;
  std::vector<std::string> healed_;  // heal copies received (mu_), drained by the heartbeat
  std::vector<std::string> recent_rids_;  // ring of the last kRecentRids request ids (mu_)
  size_t recent_pos_ = 0;
  FpStats st_;
  IoPool pool_{16, 30000, "fp-fanout"};  // replica fan-out helpers: reused threads, none created per write
  ReplicationEngine* repl_ = nullptr;
  std::atomic<int> drop_descriptors_{0};
  std::mutex peers_mu_;
  std::unordered_map<std::string, std::unique_ptr<Peer>> peers_;
  std::string self_host_;
  std::string self_addr_;
  std::atomic<uint64_t> tmp_seq_{0};
};

}  // namespace dfs

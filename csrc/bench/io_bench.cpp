// io_bench — native ChunkServer I/O + kernel microbenchmark (C45).
//
// Reference: dfs/chunkserver/benches/io_bench.rs (criterion: write+fsync and read of
// 4 KiB / 64 KiB / 1 MiB, plus a 4 KiB partial read at offset 32 KiB of a 64 KiB file).
// Same cases against the HBM chunk store, in both durability modes, plus the data-plane
// kernels the reference runs on the CPU: CRC-32 slice checksums (GPU vs PCLMUL CPU),
// batched scrub, and Reed-Solomon RS(6,3) encode (GPU vs CPU). Run under
// `rocprofv3 --kernel-trace --stats` to get per-kernel device time.
//
//   io_bench [--device N] [--dir PATH] [--iters N] [--no-fsync] [--staged] [--rs-only]   -> one JSON object
//   io_bench --disk-sweep [--dir PATH]   -> aggregate 1 MiB write+fdatasync bandwidth of the
//            storage directory at 1..240 concurrent writers, buffered and O_DIRECT (what bounds
//            nvme-sync replication when every GPU of a node writes RF replicas to one volume)
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "trace.h"
#include "chunk_store.h"
#include "crypto.h"
#include "disk_gate.h"
#include "crc32.h"
#include "gf256.h"
#include "journal.h"
#include "md5_mb.h"

using namespace dfs;
using Clock = std::chrono::steady_clock;

static double secs(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double>(b - a).count();
}

struct Lat {
  std::vector<double> v;
  void add(double s) { v.push_back(s); }
  double pct(double p) {
    if (v.empty()) return 0;
    std::vector<double> s = v;
    std::sort(s.begin(), s.end());
    return s[std::min(s.size() - 1, static_cast<size_t>(p * s.size()))];
  }
  double mean() const {
    double t = 0;
    for (double x : v) t += x;
    return v.empty() ? 0 : t / v.size();
  }
};

static std::vector<uint8_t> random_bytes(size_t n, uint32_t seed) {
  std::vector<uint8_t> b(n);
  std::mt19937_64 g(seed);
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x = g();
    std::memcpy(&b[i], &x, 8);
  }
  for (; i < n; ++i) b[i] = static_cast<uint8_t>(g());
  return b;
}

static void emit_case(bool& first, const char* name, size_t size, Lat& l) {
  std::printf("%s\n    \"%s_%zu\": {\"mean_us\": %.2f, \"p50_us\": %.2f, \"p99_us\": %.2f, \"MBps\": %.1f}",
              first ? "" : ",", name, size, l.mean() * 1e6, l.pct(0.5) * 1e6, l.pct(0.99) * 1e6,
              l.mean() > 0 ? size / l.mean() / (1 << 20) : 0.0);
  first = false;
}

// T threads each write `per` 1 MiB files (+ an 8 KiB sidecar like the .meta) with fdatasync.
static void disk_case(const std::string& dir, int threads, int per, bool direct, int gate_slots, bool first) {
  std::filesystem::create_directories(dir);
  DiskGate gate(dir, gate_slots);
  const size_t n = 1 << 20, meta = 8192;
  std::vector<Lat> lat(threads);
  std::vector<std::thread> ts;
  std::atomic<int> errors{0};
  auto t0 = Clock::now();
  for (int t = 0; t < threads; ++t)
    ts.emplace_back([&, t] {
      void* buf = nullptr;
      if (posix_memalign(&buf, 4096, n) != 0) { ++errors; return; }
      std::memset(buf, t + 1, n);
      for (int i = 0; i < per; ++i) {
        std::string f = dir + "/t" + std::to_string(t) + "_" + std::to_string(i);
        auto a = Clock::now();
        DiskGate::Slot slot = gate.acquire();
        int fd = ::open(f.c_str(), O_CREAT | O_WRONLY | O_TRUNC | (direct ? O_DIRECT : 0), 0644);
        int fm = ::open((f + ".meta").c_str(), O_CREAT | O_WRONLY | O_TRUNC | (direct ? O_DIRECT : 0), 0644);
        if (fd < 0 || fm < 0 || ::pwrite(fd, buf, n, 0) != static_cast<ssize_t>(n) ||
            ::pwrite(fm, buf, meta, 0) != static_cast<ssize_t>(meta) || ::fdatasync(fd) != 0 || ::fdatasync(fm) != 0)
          ++errors;
        if (fd >= 0) ::close(fd);
        if (fm >= 0) ::close(fm);
        slot.release();
        lat[t].add(secs(a, Clock::now()));
      }
      std::free(buf);
    });
  for (auto& th : ts) th.join();
  double el = secs(t0, Clock::now());
  Lat all;
  for (auto& l : lat) all.v.insert(all.v.end(), l.v.begin(), l.v.end());
  std::printf("%s\n    {\"threads\": %d, \"direct\": %s, \"gate\": %d, \"files\": %d, \"GBps\": %.2f, \"p50_ms\": %.3f, \"p99_ms\": %.3f, \"errors\": %d}",
              first ? "" : ",", threads, direct ? "true" : "false", gate_slots, threads * per,
              double(threads) * per * n / el / 1e9, all.pct(0.5) * 1e3, all.pct(0.99) * 1e3, errors.load());
  std::fflush(stdout);
  std::filesystem::remove_all(dir);
}

// Journal variant of disk_case: T threads append 1 MiB records (+ a 4 KiB header/.meta
// frame) to ONE preallocated, already-written segment at reserved offsets; a record is
// durable once a group fdatasync that started after its pwrite completed. mode 0: buffered
// appends, 1: O_DIRECT appends, 2: O_DIRECT|O_DSYNC per append (no group commit).
static void journal_case(const std::string& dir, int threads, int per, int mode, bool first, bool falloc = false,
                         int syncers = 1) {
  std::filesystem::create_directories(dir);
  const size_t n = 1 << 20, hdr = 4096, rec = n + hdr;
  const uint64_t total = uint64_t(threads) * per * rec;
  std::string f = dir + "/journal.seg";
  int fd = ::open(f.c_str(), O_CREAT | O_RDWR | O_TRUNC, 0644);
  if (falloc) {  // unwritten extents: every first write converts them (a metadata change per flush)
    (void)::fallocate(fd, 0, 0, static_cast<off_t>(total));
    ::fsync(fd);
    ::close(fd);
  } else {  // preallocate by writing: later appends overwrite written extents (no metadata change)
    std::vector<uint8_t> z(8 << 20, 0);
    for (uint64_t off = 0; off < total; off += z.size())
      if (::pwrite(fd, z.data(), std::min<uint64_t>(z.size(), total - off), off) < 0) break;
    ::fsync(fd);
    ::close(fd);
  }
  int flags = O_RDWR | (mode >= 1 ? O_DIRECT : 0) | (mode == 2 ? O_DSYNC : 0);
  fd = ::open(f.c_str(), flags);
  std::atomic<uint64_t> tail{0};
  std::mutex mu;
  std::condition_variable cv;
  uint64_t issued = 0, done = 0, rounds = 0, syncing = 0;
  int running = 0;
  // group commit with up to `syncers` rounds in flight: a writer whose ticket no running
  // round covers starts its own (BlockJournal::commit's pipelined mode)
  auto group_sync = [&]() {
    std::unique_lock<std::mutex> lk(mu);
    uint64_t ticket = ++issued;
    while (done < ticket) {
      if (syncing >= ticket || running >= syncers) { cv.wait(lk); continue; }
      ++running;
      uint64_t covers = issued;
      syncing = covers;
      lk.unlock();
      ::fdatasync(fd);
      lk.lock();
      --running;
      done = std::max(done, covers);
      ++rounds;
      cv.notify_all();
    }
  };
  std::vector<Lat> lat(threads);
  std::vector<std::thread> ts;
  std::atomic<int> errors{0};
  auto t0 = Clock::now();
  for (int t = 0; t < threads; ++t)
    ts.emplace_back([&, t] {
      void* buf = nullptr;
      if (posix_memalign(&buf, 4096, rec) != 0) { ++errors; return; }
      std::memset(buf, t + 1, rec);
      for (int i = 0; i < per; ++i) {
        auto a = Clock::now();
        uint64_t off = tail.fetch_add(rec);
        if (::pwrite(fd, buf, rec, off) != static_cast<ssize_t>(rec)) ++errors;
        if (mode != 2) group_sync();
        lat[t].add(secs(a, Clock::now()));
      }
      std::free(buf);
    });
  for (auto& th : ts) th.join();
  double el = secs(t0, Clock::now());
  ::close(fd);
  Lat all;
  for (auto& l : lat) all.v.insert(all.v.end(), l.v.begin(), l.v.end());
  static const char* names[] = {"buffered", "direct", "direct_dsync"};
  std::printf("%s\n    {\"journal\": \"%s%s\", \"syncers\": %d, \"threads\": %d, \"records\": %d, \"GBps\": %.2f, \"p50_ms\": %.3f, \"p99_ms\": %.3f, \"sync_rounds\": %llu, \"errors\": %d}",
              first ? "" : ",", names[mode], falloc ? "_fallocated" : "", syncers, threads, threads * per, double(threads) * per * n / el / 1e9,
              all.pct(0.5) * 1e3, all.pct(0.99) * 1e3, static_cast<unsigned long long>(rounds), errors.load());
  std::fflush(stdout);
  std::filesystem::remove_all(dir);
}

// K journals on one volume (K chunkservers of a node), `per_journal` writers each appending
// 1 MiB records to their journal's pre-written segment. Flush policy:
//   0 per-journal group commit (each journal's leader fdatasyncs its own file),
//   1 node-wide combining, fdatasync: one leader at a time flushes every journal with
//     completed-but-unflushed records (one round covers all K),
//   2 node-wide combining, syncfs: one leader syncfs()es the filesystem per round.
// Threads stand in for processes: flush costs are the kernel's and the device's either way.
static void multi_journal_case(const std::string& dir, int K, int per_journal, int per, int mode, bool first) {
  std::filesystem::create_directories(dir);
  const size_t n = 1 << 20, hdr = 4096, rec = n + hdr;
  const uint64_t total = uint64_t(per_journal) * per * rec;
  std::vector<int> fds(K);
  for (int k = 0; k < K; ++k) {
    std::string f = dir + "/j" + std::to_string(k) + ".seg";
    int fd = ::open(f.c_str(), O_CREAT | O_RDWR | O_TRUNC, 0644);
    std::vector<uint8_t> z(8 << 20, 0);
    for (uint64_t off = 0; off < total; off += z.size())
      if (::pwrite(fd, z.data(), std::min<uint64_t>(z.size(), total - off), off) < 0) break;
    ::fsync(fd);
    fds[k] = fd;
  }
  std::vector<std::atomic<uint64_t>> tails(K);
  for (auto& t : tails) t = 0;
  // per-journal state (mode 0) or one node-wide state (modes 1, 2): ticket counters
  struct G {
    std::mutex mu;
    std::condition_variable cv;
    uint64_t issued = 0, done = 0;
    bool running = false;
  };
  std::vector<G> gs(mode == 0 ? K : 1);
  std::vector<std::atomic<bool>> dirty(K);
  for (auto& d : dirty) d = false;
  std::atomic<uint64_t> rounds{0};
  auto sync_for = [&](int k) {
    G& g = gs[mode == 0 ? k : 0];
    std::unique_lock<std::mutex> lk(g.mu);
    uint64_t ticket = ++g.issued;
    while (g.done < ticket) {
      if (g.running) {
        g.cv.wait(lk);
        continue;
      }
      g.running = true;
      uint64_t covers = g.issued;
      lk.unlock();
      if (mode == 0) {
        ::fdatasync(fds[k]);
      } else if (mode == 1) {
        for (int j = 0; j < K; ++j)
          if (dirty[j].exchange(false)) ::fdatasync(fds[j]);
      } else {
        ::syncfs(fds[0]);
      }
      lk.lock();
      g.running = false;
      g.done = covers;
      rounds++;
      g.cv.notify_all();
    }
  };
  std::vector<Lat> lat(K * per_journal);
  std::vector<std::thread> ts;
  std::atomic<int> errors{0};
  auto t0 = Clock::now();
  for (int k = 0; k < K; ++k)
    for (int w = 0; w < per_journal; ++w)
      ts.emplace_back([&, k, w] {
        std::vector<uint8_t> buf(rec, static_cast<uint8_t>(k * 16 + w + 1));
        for (int i = 0; i < per; ++i) {
          auto a = Clock::now();
          uint64_t off = tails[k].fetch_add(rec);
          if (::pwrite(fds[k], buf.data(), rec, off) != static_cast<ssize_t>(rec)) ++errors;
          dirty[k] = true;
          sync_for(k);
          lat[k * per_journal + w].add(secs(a, Clock::now()));
        }
      });
  for (auto& th : ts) th.join();
  double el = secs(t0, Clock::now());
  for (int fd : fds) ::close(fd);
  Lat all;
  for (auto& l : lat) all.v.insert(all.v.end(), l.v.begin(), l.v.end());
  static const char* names[] = {"per_journal_fdatasync", "node_wide_fdatasync", "node_wide_syncfs"};
  std::printf("%s\n    {\"journals\": %d, \"writers_per_journal\": %d, \"flush\": \"%s\", \"records\": %d, \"GBps\": %.2f, "
              "\"p50_ms\": %.3f, \"p99_ms\": %.3f, \"flush_rounds\": %llu, \"errors\": %d}",
              first ? "" : ",", K, per_journal, names[mode], K * per_journal * per,
              double(K) * per_journal * per * n / el / 1e9, all.pct(0.5) * 1e3, all.pct(0.99) * 1e3,
              static_cast<unsigned long long>(rounds.load()), errors.load());
  std::fflush(stdout);
  std::filesystem::remove_all(dir);
}

// PCIe roofline of the bench path: `threads` concurrent 1 MiB transfers
// host <-> HBM, (a) plain hipMemcpyAsync from pinned memory on one stream per thread (the
// copy engines' rate) and (b) the store's fused kernels (crc_write_copy_kernel: load over
// PCIe + checksum + store into HBM; crc_read_copy_kernel: verify + store over PCIe) from
// registered host memory, as the fast path drives them for co-located clients.
static void pcie_roofline(int device, int threads, int per, size_t n) {
  (void)hipSetDevice(device);
  StoreConfig cfg;
  cfg.storage_dir = "/tmp/io_bench_roofline";
  cfg.device = device;
  cfg.hbm_capacity = 16ull << 30;
  cfg.durability = Durability::HbmAck;
  cfg.sync_writes = false;
  cfg.lanes = std::max(8, threads);
  double h2d = 0, d2h = 0, wr = 0, rd = 0;
  uint64_t fused_w = 0, fused_r = 0;
  {
    ChunkStore store(cfg);
    store.debug_pause_spill(true);  // store only: no NVMe spill competing for the host
    // the writers' buffers as the fast path has them: ordinary pages, registered with the
    // store (hipHostRegister) so the fused kernels reach them over PCIe
    std::vector<uint8_t*> host(threads), dev(threads);
    std::vector<hipStream_t> st(threads);
    for (int t = 0; t < threads; ++t) {
      host[t] = static_cast<uint8_t*>(std::aligned_alloc(4096, (n + 4095) & ~size_t(4095)));
      for (size_t i = 0; i < n; ++i) host[t][i] = static_cast<uint8_t>(i * 131 + t);
      store.register_host(host[t], n);
      (void)hipMalloc(reinterpret_cast<void**>(&dev[t]), n);
      (void)hipStreamCreateWithFlags(&st[t], hipStreamNonBlocking);
    }
    auto run = [&](auto&& body) {
      std::vector<std::thread> ts;
      auto t0 = Clock::now();
      for (int t = 0; t < threads; ++t)
        ts.emplace_back([&, t] {
          for (int i = 0; i < per; ++i) body(t);
        });
      for (auto& th : ts) th.join();
      return double(threads) * per * n / secs(t0, Clock::now()) / 1e9;
    };
    auto h2d_one = [&](int t) {
      (void)hipMemcpyAsync(dev[t], host[t], n, hipMemcpyHostToDevice, st[t]);
      (void)hipStreamSynchronize(st[t]);
    };
    auto d2h_one = [&](int t) {
      (void)hipMemcpyAsync(host[t], dev[t], n, hipMemcpyDeviceToHost, st[t]);
      (void)hipStreamSynchronize(st[t]);
    };
    run(h2d_one);  // warm-up
    h2d = run(h2d_one);
    d2h = run(d2h_one);
    for (int t = 0; t < threads; ++t)  // d2h overwrote them with the device's (random) bytes
      for (size_t i = 0; i < n; ++i) host[t][i] = static_cast<uint8_t>(i * 131 + t);
    std::vector<uint32_t> crcs(threads);
    for (int t = 0; t < threads; ++t) crcs[t] = crc32(host[t], n);
    std::atomic<int> seq{0};
    auto write_one = [&](int t) {
      std::string id = "r" + std::to_string(seq.fetch_add(1));
      if (!store.write(id, host[t], n, crcs[t]).ok) std::fprintf(stderr, "roofline write failed\n");
    };
    run(write_one);  // warm-up, and the blocks the reads use
    wr = run(write_one);
    std::atomic<int> rs{0};
    rd = run([&](int t) {
      std::string id = "r" + std::to_string(rs.fetch_add(1) % (threads * per));
      ReadResult r = store.read_into(id, 0, n, host[t]);
      if (r.status != ReadStatus::Ok) std::fprintf(stderr, "roofline read failed\n");
    });
    StoreStats ss = store.stats();
    fused_w = ss.fused_writes;
    fused_r = ss.fused_reads;
    for (int t = 0; t < threads; ++t) {
      store.unregister_host(host[t]);
      std::free(host[t]);
      (void)hipFree(dev[t]);
      (void)hipStreamDestroy(st[t]);
    }
    store.debug_pause_spill(false);
  }
  std::filesystem::remove_all("/tmp/io_bench_roofline");
  std::printf("{\"pcie_roofline\": {\"threads\": %d, \"bytes\": %zu, \"per_thread\": %d, \"memcpy_h2d_GBps\": %.2f, "
              "\"memcpy_d2h_GBps\": %.2f, \"store_write_fused_GBps\": %.2f, \"store_read_fused_GBps\": %.2f, "
              "\"write_vs_h2d\": %.3f, \"read_vs_d2h\": %.3f, \"fused_writes\": %llu, \"fused_reads\": %llu}}\n",
              threads, n, per, h2d, d2h, wr, rd, h2d > 0 ? wr / h2d : 0.0, d2h > 0 ? rd / d2h : 0.0,
              static_cast<unsigned long long>(fused_w), static_cast<unsigned long long>(fused_r));
}

// --md5: the ETag hash of a 1 MiB write, OpenSSL on one core against the multi-buffer engine
// (md5_mb.cpp): one message alone (latency), and `conc` messages in flight at once, each
// submitter starting its next as soon as its last returns (the benchmark's 10 writers).
static void md5_bench(int conc, int per) {
  const size_t n = 1 << 20;
  std::vector<std::vector<uint8_t>> bufs(conc, std::vector<uint8_t>(n));
  std::mt19937 rng(5);
  for (auto& b : bufs)
    for (auto& x : b) x = static_cast<uint8_t>(rng());
  auto timed = [&](auto&& fn) {
    auto t0 = Clock::now();
    fn();
    return secs(t0, Clock::now());
  };
  // engine: nullptr = OpenSSL on each submitting thread
  auto run = [&](Md5MultiBuffer* mb, double* one_ms, double* p50, double* cpu_cores) {
    double best = 1e9;
    for (int i = 0; i < 10; ++i)
      best = std::min(best, timed([&] {
        if (mb) (void)mb->submit(bufs[0].data(), n).get();
        else (void)md5_hex_scalar(bufs[0].data(), n);
      }));
    *one_ms = 1e3 * best;
    std::vector<double> lat;
    std::mutex mu;
    struct timespec c0, c1;
    ::clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &c0);
    const double wall = timed([&] {
      std::vector<std::thread> ts;
      for (int t = 0; t < conc; ++t)
        ts.emplace_back([&, t] {
          std::vector<double> mine;
          for (int i = 0; i < per; ++i) {
            auto a = Clock::now();
            if (mb) (void)mb->submit(bufs[t].data(), n).get();
            else (void)md5_hex_scalar(bufs[t].data(), n);
            mine.push_back(secs(a, Clock::now()));
          }
          std::lock_guard<std::mutex> g(mu);
          lat.insert(lat.end(), mine.begin(), mine.end());
        });
      for (auto& t : ts) t.join();
    });
    ::clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &c1);
    std::sort(lat.begin(), lat.end());
    *p50 = 1e3 * lat[lat.size() / 2];
    *cpu_cores = ((c1.tv_sec - c0.tv_sec) + 1e-9 * (c1.tv_nsec - c0.tv_nsec)) / wall;
    return conc * per * 1.0 / wall;  // MiB/s
  };
  std::printf("{\"md5\": {\"avx512\": %s, \"concurrent\": %d, \"engines\": [", Md5MultiBuffer::available() ? "true" : "false",
              conc);
  struct E {
    const char* name;
    Md5MultiBuffer::Kind kind;
    int lanes;
  };
  bool first = true;
  for (const E& e : {E{"openssl", Md5MultiBuffer::Kind::None, 0}, E{"scalar-x1", Md5MultiBuffer::Kind::Scalar, 1},
                     E{"scalar-x2", Md5MultiBuffer::Kind::Scalar, 2}, E{"scalar-x3", Md5MultiBuffer::Kind::Scalar, 3},
                     E{"avx512-x16", Md5MultiBuffer::Kind::Avx512, 16}}) {
    if (e.kind == Md5MultiBuffer::Kind::Avx512 && !Md5MultiBuffer::available()) continue;
    std::unique_ptr<Md5MultiBuffer> mb;
    if (e.kind != Md5MultiBuffer::Kind::None) {
      const int lanes = e.kind == Md5MultiBuffer::Kind::Avx512 ? Md5MultiBuffer::kLanes : e.lanes;
      mb = std::make_unique<Md5MultiBuffer>((conc + lanes - 1) / lanes, e.kind, e.lanes);
    }
    double one = 0, p50 = 0, cores = 0;
    const double rate = run(mb.get(), &one, &p50, &cores);
    std::printf("%s\n  {\"engine\": \"%s\", \"one_mib_ms\": %.3f, \"mib_s\": %.0f, \"p50_ms\": %.3f, \"cpu_cores\": %.2f}",
                first ? "" : ",", e.name, one, rate, p50, cores);
    first = false;
  }
  std::printf("\n]}}\n");
}

// --roofline: what the volume gives a chunkserver's journal right now — T writers appending
// 1 MiB block records (header + .meta image + data) to a BlockJournal like the store's
// (8 parts, 256 MiB segments, written out once before the timed appends), each record
// group-committed before the next. bench.py runs it on every rank at once after its timed
// region, so each rank's share of the node's volume is recorded next to its throughput.
static void roofline(const std::string& dir, int threads, int per) {
  std::filesystem::remove_all(dir);
  const uint64_t n = 1 << 20, S = num_slices(n);
  double secs_total = 0, mbps = 0;
  std::vector<double> lat;
  {
    JournalConfig c;
    c.dir = dir;
    c.max_segs = static_cast<int>((uint64_t(threads) * per * (n + 12288)) / (c.seg_bytes * 9 / 10)) + 2;
    BlockJournal j(c);
    (void)j.recover();
    for (int i = 0; i < 6000 && j.stats().parts_unready; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(10));
    std::vector<uint8_t> meta(4 * S, 0);
    std::mutex mu;
    auto t0 = Clock::now();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t)
      ts.emplace_back([&, t] {
        std::vector<uint8_t> buf(n, static_cast<uint8_t>(t + 1));
        std::vector<double> mine;
        for (int i = 0; i < per; ++i) {
          auto a = Clock::now();
          JournalRec r;
          std::string err;
          if (!j.reserve(n, S, &r, &err) || !j.write(r, 0, buf.data(), n) ||
              !j.finish(&r, "roof-" + std::to_string(t) + "-" + std::to_string(i), n, 0, meta.data(), S) ||
              !j.commit(r))
            break;
          mine.push_back(secs(a, Clock::now()));
        }
        std::lock_guard<std::mutex> g(mu);
        lat.insert(lat.end(), mine.begin(), mine.end());
      });
    for (auto& t : ts) t.join();
    secs_total = secs(t0, Clock::now());
    mbps = lat.size() * (n / 1048576.0) / std::max(1e-9, secs_total);
  }
  std::filesystem::remove_all(dir);
  std::sort(lat.begin(), lat.end());
  auto pct = [&](double p) { return lat.empty() ? 0.0 : 1e3 * lat[std::min(lat.size() - 1, size_t(lat.size() * p))]; };
  std::printf("{\"roofline_mb_s\": %.1f, \"threads\": %d, \"records\": %zu, \"seconds\": %.3f, \"p50_ms\": %.3f, "
              "\"p99_ms\": %.3f}\n", mbps, threads, lat.size(), secs_total, pct(0.5), pct(0.99));
}

// --ec-fused: ChunkStore::ec_encode of a stripe in registered memory, the single-kernel path
// against the staged one (copies, K4, one K2 launch per shard), alternating in every repetition.
// One JSON line per (k, m, shard length) cell; times are microseconds per stripe, each the mean
// of `iters` back-to-back encodes (every encode ends in a stream synchronise).
static int ec_fused_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--ec-fused needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/ecf";
  cfg.device = device;
  cfg.hbm_capacity = 2ull << 30;
  ChunkStore s(cfg);
  const int shapes[][2] = {{4, 2}, {6, 3}, {10, 4}};
  int rc = 0;
  for (auto& km : shapes)
    for (uint64_t len : {256ull << 10, 1ull << 20, 16ull << 20}) {
      const int k = km[0], m = km[1];
      uint8_t* buf = nullptr;
      if (hipHostMalloc(reinterpret_cast<void**>(&buf), k * len, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
        return 1;
      const auto data = random_bytes(k * len, static_cast<uint32_t>(k * 131 + len));
      std::memcpy(buf, data.data(), data.size());
      s.register_host(buf, k * len);
      gf::Matrix full = gf::rs_matrix(k, m), parity(full.begin() + k, full.end());
      const int iters = static_cast<int>(std::clamp<uint64_t>((256ull << 20) / (k * len), 3, 100));
      std::vector<uint32_t> crcs[2];
      std::vector<double> us[2];  // [0] staged, [1] fused
      bool ok = true;
      auto run = [&](int fused, int n) {
        set_ec_fused(fused != 0);
        const auto t0 = Clock::now();
        for (int i = 0; i < n && ok; ++i) {
          ChunkStore::EcBuffers enc;
          std::string err;
          ok = s.ec_encode(buf, len, len, k, parity, &enc, &err);
          if (ok) crcs[fused] = enc.crc;
          s.ec_free(&enc);
        }
        return secs(t0, Clock::now()) * 1e6 / n;
      };
      for (int fused = 0; fused < 2; ++fused) run(fused, 2);  // warm-up: code objects, scratch, extents
      const uint64_t before = s.stats().ec_fused_encodes;
      for (int rep = 0; rep < reps; ++rep)
        for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters));
      const uint64_t fused_runs = s.stats().ec_fused_encodes - before;
      auto list = [](const std::vector<double>& v) {
        std::string o;
        for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
        return o;
      };
      const bool match = ok && crcs[0] == crcs[1] && fused_runs == static_cast<uint64_t>(reps) * iters;
      std::printf("{\"ec_fused\": {\"k\": %d, \"m\": %d, \"shard_len\": %llu, \"iters\": %d, \"fused_us\": [%s], "
                  "\"staged_us\": [%s], \"fused_min_us\": %.1f, \"staged_min_us\": %.1f, \"match\": %s}}\n",
                  k, m, static_cast<unsigned long long>(len), iters, list(us[1]).c_str(), list(us[0]).c_str(),
                  *std::min_element(us[1].begin(), us[1].end()), *std::min_element(us[0].begin(), us[0].end()),
                  match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
      s.unregister_host(buf);
      (void)hipHostFree(buf);
    }
  set_ec_fused(true);
  std::filesystem::remove_all(dir);
  return rc;
}

// --ec-convert: the tiering conversion of a resident block (ENCODE_EC) three ways, alternating in
// every repetition: ChunkStore::ec_encode_block on the single kernel, the same call staged (one
// copy per column, K4, one K2 launch per shard), and the host route it replaces (verified read to
// the host, split into padded columns, gf_matmul_gpu, k + m CPU CRCs). Block sizes are a few
// bytes under 1, 16 and 100 MiB so that sl % 16 != 0 and the last column is short. One JSON line
// per (k, m, size) cell; times are microseconds per block, each the mean of `iters` back-to-back
// conversions (every one ends in a stream synchronise).
static int ec_convert_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--ec-convert needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/ecc";
  cfg.device = device;
  cfg.hbm_capacity = 2ull << 30;
  ChunkStore s(cfg);
  const int shapes[][2] = {{6, 3}, {10, 4}};
  int rc = 0;
  for (auto& km : shapes)
    for (uint64_t mib : {1ull, 16ull, 100ull}) {
      const int k = km[0], m = km[1];
      uint64_t n = (mib << 20) - 7;
      while (((n + k - 1) / k) % 16 == 0) --n;
      const uint64_t sl = (n + k - 1) / k;
      const auto data = random_bytes(n, static_cast<uint32_t>(k * 131 + mib));
      const std::string id = "conv";
      if (!s.write(id, data.data(), n, crc32(data.data(), n)).ok) return 1;
      gf::Matrix full = gf::rs_matrix(k, m), parity(full.begin() + k, full.end());
      const int iters = static_cast<int>(std::clamp<uint64_t>((256ull << 20) / n, 2, 50));
      std::vector<uint32_t> crcs[3];
      std::vector<double> us[3];  // [0] host route, [1] staged, [2] fused
      bool ok = true;
      auto host_route = [&] {
        std::vector<uint8_t> blk(n);
        ReadResult r = s.read_into(id, 0, n, blk.data());
        if (r.status != ReadStatus::Ok || r.bytes != n) return false;
        std::vector<std::vector<uint8_t>> sh(k + m, std::vector<uint8_t>(sl, 0));
        for (int c = 0; c < k; ++c)
          if (c * sl < n) std::memcpy(sh[c].data(), blk.data() + c * sl, std::min(sl, n - c * sl));
        std::vector<const uint8_t*> in;
        std::vector<uint8_t*> out;
        for (int c = 0; c < k; ++c) in.push_back(sh[c].data());
        for (int r2 = 0; r2 < m; ++r2) out.push_back(sh[k + r2].data());
        if (!s.gf_matmul_gpu(parity, in, out, sl)) return false;
        crcs[0].clear();
        for (auto& v : sh) crcs[0].push_back(crc32(v.data(), sl));
        return true;
      };
      auto run = [&](int mode, int cnt) {
        set_ec_convert_fused(mode == 2);
        const auto t0 = Clock::now();
        for (int i = 0; i < cnt && ok; ++i) {
          if (mode == 0) {
            ok = host_route();
            continue;
          }
          ChunkStore::EcBuffers enc;
          std::string err;
          ok = s.ec_encode_block(id, k, parity, &enc, &err);
          if (ok) crcs[mode] = enc.crc;
          s.ec_free(&enc);
        }
        return secs(t0, Clock::now()) * 1e6 / cnt;
      };
      for (int mode = 0; mode < 3; ++mode) run(mode, 2);  // warm-up: code objects, scratch, extents
      const uint64_t before = s.stats().ec_fused_converts;
      for (int rep = 0; rep < reps; ++rep)
        for (int mode = 2; mode >= 0; --mode) us[mode].push_back(run(mode, iters));
      const uint64_t fused_runs = s.stats().ec_fused_converts - before;
      auto list = [](const std::vector<double>& v) {
        std::string o;
        for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
        return o;
      };
      auto least = [](const std::vector<double>& v) { return *std::min_element(v.begin(), v.end()); };
      const bool match = ok && crcs[0] == crcs[1] && crcs[1] == crcs[2] && fused_runs == static_cast<uint64_t>(reps) * iters;
      std::printf("{\"ec_convert\": {\"k\": %d, \"m\": %d, \"block_bytes\": %llu, \"shard_len\": %llu, \"iters\": %d, "
                  "\"fused_us\": [%s], \"staged_us\": [%s], \"host_us\": [%s], \"fused_min_us\": %.1f, "
                  "\"staged_min_us\": %.1f, \"host_min_us\": %.1f, \"match\": %s}}\n",
                  k, m, static_cast<unsigned long long>(n), static_cast<unsigned long long>(sl), iters, list(us[2]).c_str(),
                  list(us[1]).c_str(), list(us[0]).c_str(), least(us[2]), least(us[1]), least(us[0]),
                  match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
      s.remove(id);
    }
  set_ec_convert_fused(true);
  std::filesystem::remove_all(dir);
  return rc;
}

// --ec-read: ChunkStore::ec_read_range of a resident RS(6,3) file with 1 and 2 lost data columns
// into a registered buffer: the whole file and a 64 KiB range inside the first lost column, the
// single-kernel path against the staged one (ec_decode into HBM, then one copy per column),
// alternating in every repetition. One JSON line per (shard length, lost, range) cell; times are
// microseconds per read, each the mean of `iters` back-to-back reads.
static int ec_read_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--ec-read needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/ecr";
  cfg.device = device;
  cfg.hbm_capacity = 2ull << 30;
  ChunkStore s(cfg);
  const int k = 6, m = 3;
  int rc = 0;
  for (uint64_t len : {256ull << 10, 1ull << 20, 16ull << 20}) {
    const auto data = random_bytes(k * len, static_cast<uint32_t>(len + 17));
    std::vector<std::vector<uint8_t>> par(m, std::vector<uint8_t>(len));
    std::vector<const uint8_t*> in(k);
    std::vector<uint8_t*> outp(m);
    for (int c = 0; c < k; ++c) in[c] = data.data() + c * len;
    for (int r = 0; r < m; ++r) outp[r] = par[r].data();
    gf::Matrix full = gf::rs_matrix(k, m), parity(full.begin() + k, full.end());
    gf::matmul_cpu(parity, in.data(), outp.data(), len);
    std::vector<std::string> ids;
    std::vector<const uint8_t*> dev(k + m, nullptr);
    bool ok = true;
    for (int i = 0; i < k + m; ++i) {
      const uint8_t* p = i < k ? in[i] : par[i - k].data();
      ids.push_back("ecr_" + std::to_string(len) + "_" + std::to_string(i));
      ok = ok && s.write(ids[i], p, len, crc32(p, len)).ok;
      uint64_t size = 0;
      if (ok) dev[i] = s.pin_device(ids[i], &size);
      ok = ok && dev[i] && size == len;
    }
    uint8_t* buf = nullptr;
    if (!ok || hipHostMalloc(reinterpret_cast<void**>(&buf), k * len, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
      return 1;
    s.register_host(buf, k * len);
    for (int lost = 1; lost <= 2; ++lost)
      for (int whole = 1; whole >= 0; --whole) {
        std::vector<const uint8_t*> shards = dev;
        for (int c = 0; c < lost; ++c) shards[2 * c + 1] = nullptr;  // columns 1 and 3
        const uint64_t from = whole ? 0 : len + len / 2 + 5, want = whole ? k * len : 64ull << 10;
        const int iters = static_cast<int>(std::clamp<uint64_t>((256ull << 20) / (whole ? k * len : len), 3, 100));
        std::vector<double> us[2];  // [0] staged, [1] fused
        bool match = true;
        auto run = [&](int fused, int n) {
          set_ec_read_fused(fused != 0);
          std::memset(buf, 0, want);
          const auto t0 = Clock::now();
          for (int i = 0; i < n && match; ++i) {
            std::string err;
            match = s.ec_read_range(shards, k, m, len, from, want, buf, &err) == ChunkStore::EcRead::Ok;
          }
          const double t = secs(t0, Clock::now()) * 1e6 / n;
          match = match && std::memcmp(buf, data.data() + from, want) == 0;
          return t;
        };
        for (int fused = 0; fused < 2; ++fused) run(fused, 2);  // warm-up: code objects, scratch, extents
        const uint64_t before = s.stats().ec_fused_reads;
        for (int rep = 0; rep < reps; ++rep)
          for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters));
        match = match && s.stats().ec_fused_reads - before == static_cast<uint64_t>(reps) * iters;
        auto list = [](const std::vector<double>& v) {
          std::string o;
          for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
          return o;
        };
        auto median = [](std::vector<double> v) {
          std::sort(v.begin(), v.end());
          return v[v.size() / 2];
        };
        std::printf("{\"ec_read\": {\"k\": %d, \"m\": %d, \"shard_len\": %llu, \"lost\": %d, \"from\": %llu, \"want\": %llu, "
                    "\"iters\": %d, \"fused_us\": [%s], \"staged_us\": [%s], \"fused_median_us\": %.1f, "
                    "\"staged_median_us\": %.1f, \"match\": %s}}\n",
                    k, m, static_cast<unsigned long long>(len), lost, static_cast<unsigned long long>(from),
                    static_cast<unsigned long long>(want), iters, list(us[1]).c_str(), list(us[0]).c_str(), median(us[1]),
                    median(us[0]), match ? "true" : "false");
        std::fflush(stdout);
        if (!match) rc = 1;
      }
    s.unregister_host(buf);
    (void)hipHostFree(buf);
    for (auto& id : ids) {
      s.unpin(id);
      s.remove(id);
    }
  }
  set_ec_read_fused(true);
  std::filesystem::remove_all(dir);
  return rc;
}

// --sse-ec-read: a GET of an SSE-S3 object held as a resident RS(6,3) file, with 0 and 1 lost data
// column, into a registered buffer: [1] ChunkStore::sse_ec_read's one-kernel route against [0] what a
// GET costs without it (ec_read_range of the whole blob into the slot, then sse_crypt where the
// ciphertext lies, under sse_crypt's own floor), alternating in every repetition. One JSON line per
// (size, lost); times are microseconds per call, each the mean of `iters` back-to-back calls, with the
// median and the spread (max - min over the repetitions) of either route. `n` counts plaintext bytes.
static int sse_ec_read_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--sse-ec-read needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/sse_ec_read";
  cfg.device = device;
  cfg.hbm_capacity = 1ull << 30;
  ChunkStore s(cfg);
  uint8_t key[32], nonce[12];
  for (int i = 0; i < 32; ++i) key[i] = static_cast<uint8_t>(3 * i + 1);
  for (int i = 0; i < 12; ++i) nonce[i] = static_cast<uint8_t>(7 * i + 5);
  const int k = 6, m = 3;
  int rc = 0;
  for (uint64_t n : {64ull << 10, 1ull << 20, 4ull << 20, 100ull << 20}) {
    const auto plain = random_bytes(n, static_cast<uint32_t>(n + 37));
    const uint64_t orig = n + 28, len = (orig + k - 1) / k;
    std::vector<uint8_t> blob(k * len, 0);
    std::memcpy(blob.data(), nonce, 12);
    std::memcpy(blob.data() + 12, plain.data(), n);
    crypto::aes256gcm_encrypt_inplace(key, nonce, blob.data() + 12, n, blob.data() + 12 + n);
    std::vector<std::vector<uint8_t>> par(m, std::vector<uint8_t>(len));
    std::vector<const uint8_t*> in(k);
    std::vector<uint8_t*> outp(m);
    for (int c = 0; c < k; ++c) in[c] = blob.data() + c * len;
    for (int r = 0; r < m; ++r) outp[r] = par[r].data();
    gf::Matrix full = gf::rs_matrix(k, m), parity(full.begin() + k, full.end());
    gf::matmul_cpu(parity, in.data(), outp.data(), len);
    std::vector<std::string> ids;
    std::vector<const uint8_t*> dev(k + m, nullptr);
    bool ok = true;
    for (int i = 0; i < k + m; ++i) {
      const uint8_t* p = i < k ? in[i] : par[i - k].data();
      ids.push_back("secr_" + std::to_string(n) + "_" + std::to_string(i));
      ok = ok && s.write(ids[i], p, len, crc32(p, len)).ok;
      uint64_t size = 0;
      if (ok) dev[i] = s.pin_device(ids[i], &size);
      ok = ok && dev[i] && size == len;
    }
    uint8_t* out = nullptr;
    if (!ok || hipHostMalloc(reinterpret_cast<void**>(&out), orig + 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
      return 1;
    s.register_host(out, orig + 64);
    const int iters = static_cast<int>(std::clamp<uint64_t>((64ull << 20) / n, 2, 100));
    for (int lost = 0; lost <= 1; ++lost) {
      std::vector<const uint8_t*> shards = dev;
      if (lost) shards[1] = nullptr;
      std::vector<double> us[2];  // [0] ec_read_range + sse_crypt, [1] the kernel
      bool match = true;
      auto run = [&](int fused, int count) {
        std::memset(out, 0, orig);
        const auto t0 = Clock::now();
        for (int i = 0; i < count && match; ++i) {
          std::string err;
          if (fused) {
            uint64_t got = 0;
            match = s.sse_ec_read(shards, k, m, len, orig, key, out, n, &got, &err, true) == ChunkStore::SseRead::Ok && got == n;
          } else {
            match = s.ec_read_range(shards, k, m, len, 0, orig, out, &err) == ChunkStore::EcRead::Ok &&
                    s.sse_crypt(out + 12, n, key, out, false, out + 12 + n, &err);
          }
        }
        const double t = secs(t0, Clock::now()) * 1e6 / count;
        match = match && std::memcmp(out + (fused ? 0 : 12), plain.data(), n) == 0;
        return t;
      };
      set_sse_ec_read_fused(true, 0);  // every size takes the kernel: the floor is what this measures
      for (int fused = 0; fused < 2; ++fused) run(fused, 2);  // warm-up: code objects, scratch
      const uint64_t before = s.stats().sse_fused_ec_reads;
      for (int rep = 0; rep < reps; ++rep)
        for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters));
      match = match && s.stats().sse_fused_ec_reads - before == static_cast<uint64_t>(reps) * iters;
      auto list = [](const std::vector<double>& v) {
        std::string o;
        for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
        return o;
      };
      auto median = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v[v.size() / 2];
      };
      auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
      std::printf("{\"sse_ec_read\": {\"k\": %d, \"m\": %d, \"n\": %llu, \"shard_len\": %llu, \"lost\": %d, \"iters\": %d, "
                  "\"fused_us\": [%s], \"staged_us\": [%s], \"fused_median_us\": %.1f, \"staged_median_us\": %.1f, "
                  "\"fused_spread_us\": %.1f, \"staged_spread_us\": %.1f, \"match\": %s}}\n",
                  k, m, static_cast<unsigned long long>(n), static_cast<unsigned long long>(len), lost, iters,
                  list(us[1]).c_str(), list(us[0]).c_str(), median(us[1]), median(us[0]), spread(us[1]), spread(us[0]),
                  match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
    }
    s.unregister_host(out);
    (void)hipHostFree(out);
    for (auto& id : ids) {
      s.unpin(id);
      s.remove(id);
    }
  }
  std::filesystem::remove_all(dir);
  return rc;
}

// --sse: ChunkStore::sse_crypt in place on a registered buffer whose body starts 12 bytes into a
// 16 B vector (a slot's [nonce 12][body][tag 16]): the kernel path against OpenSSL on the calling
// thread, alternating in every repetition, encrypt and decrypt. One JSON line per (size, direction)
// cell; times are microseconds per call, each the mean of `iters` back-to-back calls, with the
// median and the spread (max - min over the repetitions) of either path.
static int sse_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--sse needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/sse";
  cfg.device = device;
  cfg.hbm_capacity = 256ull << 20;
  ChunkStore s(cfg);
  uint8_t key[32], nonce[12];
  for (int i = 0; i < 32; ++i) key[i] = static_cast<uint8_t>(3 * i + 1);
  for (int i = 0; i < 12; ++i) nonce[i] = static_cast<uint8_t>(7 * i + 5);
  int rc = 0;
  for (uint64_t n : {64ull << 10, 1ull << 20, 4ull << 20, 16ull << 20, 100ull << 20}) {
    const auto plain = random_bytes(n, static_cast<uint32_t>(n + 29));
    uint8_t* buf = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&buf), n + 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return 1;
    s.register_host(buf, n + 64);
    uint8_t* body = buf + 12;
    std::vector<uint8_t> sealed(plain);
    uint8_t ref_tag[16];
    crypto::aes256gcm_encrypt_inplace(key, nonce, sealed.data(), n, ref_tag);
    for (int encrypt = 1; encrypt >= 0; --encrypt) {
      const int iters = static_cast<int>(std::clamp<uint64_t>((64ull << 20) / n, 2, 100));
      std::vector<double> us[2];  // [0] OpenSSL, [1] kernel
      bool match = true;
      auto run = [&](int fused, int count) {
        set_sse_fused(fused != 0, 0);  // every size takes the kernel: the threshold is what this measures
        double t = 0;
        for (int i = 0; i < count && match; ++i) {
          std::memcpy(body, encrypt ? plain.data() : sealed.data(), n);
          uint8_t tag[16];
          std::memcpy(tag, ref_tag, 16);
          std::string err;
          const auto t0 = Clock::now();
          match = s.sse_crypt(body, n, key, nonce, encrypt != 0, tag, &err);
          t += secs(t0, Clock::now());
          match = match && std::memcmp(tag, ref_tag, 16) == 0 &&
                  std::memcmp(body, encrypt ? sealed.data() : plain.data(), n) == 0;
        }
        return t * 1e6 / count;
      };
      for (int fused = 0; fused < 2; ++fused) run(fused, 2);  // warm-up: code object, scratch, OpenSSL's key setup
      const uint64_t before = s.stats().sse_fused_crypts;
      for (int rep = 0; rep < reps; ++rep)
        for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters));
      match = match && s.stats().sse_fused_crypts - before == static_cast<uint64_t>(reps) * iters;
      auto list = [](const std::vector<double>& v) {
        std::string o;
        for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
        return o;
      };
      auto median = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v[v.size() / 2];
      };
      auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
      std::printf("{\"sse\": {\"bytes\": %llu, \"encrypt\": %s, \"iters\": %d, \"kernel_us\": [%s], \"openssl_us\": [%s], "
                  "\"kernel_median_us\": %.1f, \"openssl_median_us\": %.1f, \"kernel_spread_us\": %.1f, "
                  "\"openssl_spread_us\": %.1f, \"kernel_gbps\": %.2f, \"openssl_gbps\": %.2f, \"match\": %s}}\n",
                  static_cast<unsigned long long>(n), encrypt ? "true" : "false", iters, list(us[1]).c_str(),
                  list(us[0]).c_str(), median(us[1]), median(us[0]), spread(us[1]), spread(us[0]), n / median(us[1]) / 1e3,
                  n / median(us[0]) / 1e3, match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
    }
    s.unregister_host(buf);
    (void)hipHostFree(buf);
  }
  set_sse_fused(true, static_cast<int64_t>(kSseFusedMinBytes));
  std::filesystem::remove_all(dir);
  return rc;
}

// The range rows of --sse-read: plaintext [n / 2 + 5, + want) of a stored blob by three routes that
// alternate inside every repetition. [0] staged, as a gateway without the range kernel serves a
// Range GET: read_into of the whole blob, sse_crypt where it lies, the range sent from where it
// fell. [1] ChunkStore::sse_read with the range: one sse_read_range_kernel launch. [2] for
// reference, sse_read of the whole object: one sse_read_kernel launch. Same clock, warm-ups, median
// and spread as the whole-object rows; `match` compares every call's bytes with the original.
static int sse_read_range_rows(ChunkStore& s, const uint8_t key[32], const uint8_t nonce[12], int reps) {
  int rc = 0;
  for (uint64_t n : {1ull << 20, 16ull << 20, 100ull << 20}) {
    const auto plain = random_bytes(n, static_cast<uint32_t>(n + 47));
    std::vector<uint8_t> blob(n + 28);
    std::memcpy(blob.data(), nonce, 12);
    std::memcpy(blob.data() + 12, plain.data(), n);
    crypto::aes256gcm_encrypt_inplace(key, nonce, blob.data() + 12, n, blob.data() + 12 + n);
    const std::string id = "sse-range-" + std::to_string(n);
    if (!s.write(id, blob.data(), blob.size(), 0).ok) return 1;
    uint8_t* out = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&out), n + 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return 1;
    s.register_host(out, n + 64);
    const int iters = static_cast<int>(std::clamp<uint64_t>((64ull << 20) / n, 2, 100));
    const uint64_t from = n / 2 + 5;
    for (uint64_t want : {64ull << 10, 1ull << 20, 8ull << 20}) {
      if (from + want > n) continue;
      std::vector<double> us[3];
      bool match = true;
      auto run = [&](int route, int count) {
        set_sse_read_fused(route != 0, 0);
        double t = 0;
        for (int i = 0; i < count && match; ++i) {
          std::memset(out, 0, 64);
          std::string err;
          uint64_t got = 0;
          const auto t0 = Clock::now();
          if (route == 0) {
            const ReadResult r = s.read_into(id, 0, n + 28, out);
            const bool ok = r.status == ReadStatus::Ok && s.sse_crypt(out + 12, n, key, out, false, out + 12 + n, &err);
            t += secs(t0, Clock::now());
            match = ok && std::memcmp(out + 12 + from, plain.data() + from, want) == 0;
          } else if (route == 1) {
            const auto st = s.sse_read(id, key, out + from % 16, want, &got, &err, nullptr, true, from, want);
            t += secs(t0, Clock::now());
            match = st == ChunkStore::SseRead::Ok && got == want && std::memcmp(out + from % 16, plain.data() + from, want) == 0;
          } else {
            const auto st = s.sse_read(id, key, out, n, &got, &err, nullptr, true);
            t += secs(t0, Clock::now());
            match = st == ChunkStore::SseRead::Ok && got == n && std::memcmp(out + from, plain.data() + from, want) == 0;
          }
        }
        return t * 1e6 / count;
      };
      for (int route = 0; route < 3; ++route) run(route, 2);
      const uint64_t before = s.stats().sse_fused_range_reads;
      for (int rep = 0; rep < reps; ++rep)
        for (int route = 2; route >= 0; --route) us[route].push_back(run(route, iters));
      match = match && s.stats().sse_fused_range_reads - before == static_cast<uint64_t>(reps) * iters;
      auto median = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v[v.size() / 2];
      };
      auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
      std::printf("{\"sse_read_range\": {\"bytes\": %llu, \"from\": %llu, \"want\": %llu, \"iters\": %d, "
                  "\"range_median_us\": %.1f, \"range_spread_us\": %.1f, \"staged_median_us\": %.1f, "
                  "\"staged_spread_us\": %.1f, \"whole_median_us\": %.1f, \"whole_spread_us\": %.1f, \"match\": %s}}\n",
                  static_cast<unsigned long long>(n), static_cast<unsigned long long>(from),
                  static_cast<unsigned long long>(want), iters, median(us[1]), spread(us[1]), median(us[0]), spread(us[0]),
                  median(us[2]), spread(us[2]), match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
    }
    s.unregister_host(out);
    (void)hipHostFree(out);
    s.remove(id);
  }
  return rc;
}

// --sse-read: ChunkStore::sse_read of a stored blob [nonce 12][ciphertext n][tag 16] into a registered
// buffer: the one-kernel route against what a caller without it does (read_into of the whole blob,
// then sse_crypt where the ciphertext lies, under sse_crypt's own floor, the plaintext left at + 12
// and nothing moved), alternating in every repetition. One JSON line per
// size; times are microseconds per call, each the mean of `iters` back-to-back calls, with the median
// and the spread (max - min over the repetitions) of either route. `n` counts plaintext bytes.
static int sse_read_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--sse-read needs a GPU\n");
    return 1;
  }
  std::filesystem::remove_all(dir);
  StoreConfig cfg;
  cfg.storage_dir = dir + "/sse_read";
  cfg.device = device;
  cfg.hbm_capacity = 512ull << 20;
  ChunkStore s(cfg);
  uint8_t key[32], nonce[12];
  for (int i = 0; i < 32; ++i) key[i] = static_cast<uint8_t>(3 * i + 1);
  for (int i = 0; i < 12; ++i) nonce[i] = static_cast<uint8_t>(7 * i + 5);
  int rc = 0;
  for (uint64_t n : {64ull << 10, 1ull << 20, 4ull << 20, 16ull << 20, 100ull << 20}) {
    const auto plain = random_bytes(n, static_cast<uint32_t>(n + 31));
    std::vector<uint8_t> blob(n + 28);
    std::memcpy(blob.data(), nonce, 12);
    std::memcpy(blob.data() + 12, plain.data(), n);
    crypto::aes256gcm_encrypt_inplace(key, nonce, blob.data() + 12, n, blob.data() + 12 + n);
    const std::string id = "sse-" + std::to_string(n);
    if (!s.write(id, blob.data(), blob.size(), 0).ok) return 1;
    uint8_t* out = nullptr;
    if (hipHostMalloc(reinterpret_cast<void**>(&out), n + 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return 1;
    s.register_host(out, n + 64);
    const int iters = static_cast<int>(std::clamp<uint64_t>((64ull << 20) / n, 2, 100));
    std::vector<double> us[2];  // [0] staged, [1] fused
    bool match = true;
    auto run = [&](int fused, int count) {
      set_sse_read_fused(fused != 0, 0);  // every size takes the kernel: the floor is what this measures
      double t = 0;
      for (int i = 0; i < count && match; ++i) {
        std::memset(out, 0, 64);
        std::string err;
        if (fused) {
          uint64_t got = 0;
          const auto t0 = Clock::now();
          const auto st = s.sse_read(id, key, out, n, &got, &err);
          t += secs(t0, Clock::now());
          match = st == ChunkStore::SseRead::Ok && got == n && std::memcmp(out, plain.data(), n) == 0;
        } else {  // as a caller without sse_read does it: the blob into its slot, decrypted where it lies, sent from + 12
          const auto t0 = Clock::now();
          const ReadResult r = s.read_into(id, 0, n + 28, out);
          const bool ok = r.status == ReadStatus::Ok && s.sse_crypt(out + 12, n, key, out, false, out + 12 + n, &err);
          t += secs(t0, Clock::now());
          match = ok && std::memcmp(out + 12, plain.data(), n) == 0;
        }
      }
      return t * 1e6 / count;
    };
    for (int fused = 0; fused < 2; ++fused) run(fused, 2);  // warm-up: code objects, scratch, residency
    const uint64_t before = s.stats().sse_fused_reads;
    for (int rep = 0; rep < reps; ++rep)
      for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters));
    match = match && s.stats().sse_fused_reads - before == static_cast<uint64_t>(reps) * iters;
    auto list = [](const std::vector<double>& v) {
      std::string o;
      for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
      return o;
    };
    auto median = [](std::vector<double> v) {
      std::sort(v.begin(), v.end());
      return v[v.size() / 2];
    };
    auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
    std::printf("{\"sse_read\": {\"bytes\": %llu, \"iters\": %d, \"fused_us\": [%s], \"staged_us\": [%s], "
                "\"fused_median_us\": %.1f, \"staged_median_us\": %.1f, \"fused_spread_us\": %.1f, "
                "\"staged_spread_us\": %.1f, \"fused_gbps\": %.2f, \"staged_gbps\": %.2f, \"match\": %s}}\n",
                static_cast<unsigned long long>(n), iters, list(us[1]).c_str(), list(us[0]).c_str(), median(us[1]),
                median(us[0]), spread(us[1]), spread(us[0]), n / median(us[1]) / 1e3, n / median(us[0]) / 1e3,
                match ? "true" : "false");
    std::fflush(stdout);
    if (!match) rc = 1;
    s.unregister_host(out);
    (void)hipHostFree(out);
    s.remove(id);
  }
  if (sse_read_range_rows(s, key, nonce, reps) != 0) rc = 1;
  set_sse_read_fused(true, static_cast<int64_t>(kSseReadFusedMinBytes));
  std::filesystem::remove_all(dir);
  return rc;
}

// --sse-write: a PUT of an SSE-S3 object from a registered slot [12 free][plaintext n][16 free]. The
// staged arm is what a PUT does without the kernel: sse_crypt in place (under its own floor), then
// write() from the same slot; the fused arm is ChunkStore::sse_write, one sse_write_kernel launch.
// The arms alternate inside each repetition, in both durability modes; the slot is refilled and the
// block removed outside the timed window. One JSON line per mode and size, in the units of
// --sse-read. `match` requires the slot after every call, and the stored bytes read back after every
// warm-up call and the last call of every timed repetition, to equal OpenSSL's blob, and the counter
// to prove the route.
static int sse_write_bench(int device, const std::string& dir, int reps) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    std::fprintf(stderr, "--sse-write needs a GPU\n");
    return 1;
  }
  uint8_t key[32], nonce[12];
  for (int i = 0; i < 32; ++i) key[i] = static_cast<uint8_t>(3 * i + 1);
  for (int i = 0; i < 12; ++i) nonce[i] = static_cast<uint8_t>(7 * i + 5);
  int rc = 0;
  for (int mode = 0; mode < 2; ++mode) {
    std::filesystem::remove_all(dir);
    StoreConfig cfg;
    cfg.storage_dir = dir + "/sse_write";
    cfg.device = device;
    cfg.hbm_capacity = 512ull << 20;
    cfg.durability = mode == 0 ? Durability::HbmAck : Durability::NvmeSync;
    ChunkStore s(cfg);
    for (uint64_t n : {64ull << 10, 1ull << 20, 4ull << 20, 16ull << 20, 100ull << 20}) {
      const auto plain = random_bytes(n, static_cast<uint32_t>(n + 37));
      std::vector<uint8_t> blob(n + 28), back(n + 28);
      std::memcpy(blob.data(), nonce, 12);
      std::memcpy(blob.data() + 12, plain.data(), n);
      crypto::aes256gcm_encrypt_inplace(key, nonce, blob.data() + 12, n, blob.data() + 12 + n);
      uint8_t* slot = nullptr;
      if (hipHostMalloc(reinterpret_cast<void**>(&slot), n + 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
        std::fprintf(stderr, "--sse-write: no pinned slot of %llu bytes\n", static_cast<unsigned long long>(n + 64));
        rc = 1;
        break;
      }
      s.register_host(slot, n + 64);
      const int iters = static_cast<int>(std::clamp<uint64_t>((64ull << 20) / n, 2, mode == 0 ? 100 : 20));
      std::vector<double> us[2];  // [0] staged, [1] fused
      bool match = true;
      uint64_t seq = 0;
      auto run = [&](int fused, int count, bool check_stored) {
        set_sse_write_fused(fused != 0, 0);  // every size takes the kernel: the floor is what this measures
        double t = 0;
        for (int i = 0; i < count && match; ++i) {
          const std::string id = "ssew-" + std::to_string(n) + "-" + std::to_string(seq++);
          std::memset(slot, 0xEE, 12);
          std::memcpy(slot + 12, plain.data(), n);
          std::memset(slot + 12 + n, 0xEE, 16);
          std::string err;
          bool ok;
          const auto t0 = Clock::now();
          if (fused) {
            ok = s.sse_write(id, key, nonce, slot, n).ok;
          } else {
            std::memcpy(slot, nonce, 12);
            ok = s.sse_crypt(slot + 12, n, key, nonce, true, slot + 12 + n, &err) && s.write(id, slot, n + 28, 0).ok;
          }
          t += secs(t0, Clock::now());
          match = ok && std::memcmp(slot, blob.data(), n + 28) == 0;
          if (match && (check_stored || i == count - 1))  // every warm-up call, and one block of each timed repetition
            match = s.read_into(id, 0, n + 28, back.data()).status == ReadStatus::Ok && back == blob;
          s.remove(id);
        }
        return t * 1e6 / count;
      };
      for (int fused = 0; fused < 2; ++fused) run(fused, 2, true);  // warm-up: code objects, scratch; the stored bytes
      const uint64_t before = s.stats().sse_fused_writes;
      for (int rep = 0; rep < reps; ++rep)
        for (int fused = 1; fused >= 0; --fused) us[fused].push_back(run(fused, iters, false));
      match = match && s.stats().sse_fused_writes - before == static_cast<uint64_t>(reps) * iters;
      auto list = [](const std::vector<double>& v) {
        std::string o;
        for (double x : v) o += (o.empty() ? "" : ", ") + std::to_string(x);
        return o;
      };
      auto median = [](std::vector<double> v) {
        std::sort(v.begin(), v.end());
        return v[v.size() / 2];
      };
      auto spread = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end()); };
      std::printf("{\"sse_write\": {\"durability\": \"%s\", \"bytes\": %llu, \"iters\": %d, \"fused_us\": [%s], "
                  "\"staged_us\": [%s], \"fused_median_us\": %.1f, \"staged_median_us\": %.1f, \"fused_spread_us\": %.1f, "
                  "\"staged_spread_us\": %.1f, \"fused_gbps\": %.2f, \"staged_gbps\": %.2f, \"match\": %s}}\n",
                  mode == 0 ? "hbm-ack" : "nvme-sync", static_cast<unsigned long long>(n), iters, list(us[1]).c_str(),
                  list(us[0]).c_str(), median(us[1]), median(us[0]), spread(us[1]), spread(us[0]), n / median(us[1]) / 1e3,
                  n / median(us[0]) / 1e3, match ? "true" : "false");
      std::fflush(stdout);
      if (!match) rc = 1;
      s.unregister_host(slot);
      (void)hipHostFree(slot);
    }
  }
  reset_sse_write_fused();
  std::filesystem::remove_all(dir);
  return rc;
}

int main(int argc, char** argv) {
  dfs::trace_init();  // before any thread: roctx's first range calls setenv (trace.h)
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--sse-write") {
      std::string dir = "/tmp/io_bench_sse_write";
      int device = 0, reps = 5;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return sse_write_bench(device, dir, std::max(5, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--sse-read") {
      std::string dir = "/tmp/io_bench_sse_read";
      int device = 0, reps = 5;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return sse_read_bench(device, dir, std::max(5, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--sse") {
      std::string dir = "/tmp/io_bench_sse";
      int device = 0, reps = 5;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return sse_bench(device, dir, std::max(5, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--sse-ec-read") {
      std::string dir = "/tmp/io_bench_sse_ec_read";
      int device = 0, reps = 5;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return sse_ec_read_bench(device, dir, std::max(5, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--ec-read") {
      std::string dir = "/tmp/io_bench_ecr";
      int device = 0, reps = 5;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return ec_read_bench(device, dir, std::max(1, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--ec-convert") {
      std::string dir = "/tmp/io_bench_ecc";
      int device = 0, reps = 3;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return ec_convert_bench(device, dir, std::max(1, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--ec-fused") {
      std::string dir = "/tmp/io_bench_ecf";
      int device = 0, reps = 3;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--device") device = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--reps") reps = std::atoi(argv[j + 1]);
      }
      return ec_fused_bench(device, dir, std::max(1, reps));
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--md5") {
      int conc = 10, per = 20;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--conc") conc = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--per") per = std::atoi(argv[j + 1]);
      }
      md5_bench(std::max(1, conc), std::max(1, per));
      return 0;
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--roofline") {
      std::string dir = "/tmp/io_bench_roofline";
      int threads = 10, per = 30;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
        if (std::string(argv[j]) == "--threads") threads = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--per") per = std::atoi(argv[j + 1]);
      }
      roofline(dir, std::max(1, threads), std::max(1, per));
      return 0;
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--multi-journal") {
      std::string dir = "/tmp/io_bench_mj";
      for (int j = 1; j + 1 < argc; ++j)
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
      std::printf("{\"multi_journal\": [");
      bool first = true;
      for (int K : {1, 3, 7})
        for (int mode = 0; mode < 3; ++mode) {
          if (K == 1 && mode == 1) continue;  // same as per-journal
          multi_journal_case(dir, K, K == 1 ? 21 : 3, K == 1 ? 12 : (K == 3 ? 28 : 12), mode, first);
          first = false;
        }
      std::printf("\n]}\n");
      return 0;
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--pcie-roofline") {
      int threads = 10, per = 200;
      size_t n = 1 << 20;
      for (int j = 1; j + 1 < argc; ++j) {
        if (std::string(argv[j]) == "--threads") threads = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--per") per = std::atoi(argv[j + 1]);
        if (std::string(argv[j]) == "--bytes") n = std::strtoull(argv[j + 1], nullptr, 10);
      }
      pcie_roofline(0, threads, per, n);
      return 0;
    }
  int device = 0, iters = 50;
  bool fsync = true;
  bool zero_copy = true;
  bool rs_only = false;  // only the RS(6,3) end-to-end case (pipeline tuning sweeps)
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--journal-sweep") {
      std::string dir = "/tmp/io_bench_journal";
      for (int j = 1; j + 1 < argc; ++j)
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
      std::printf("{\"journal_sweep\": [");
      bool first = true;
      for (int t : {1, 10, 30, 70}) {
        disk_case(dir + "_files", t, std::max(8, 2400 / t / 4), false, 0, first);
        first = false;
        for (int mode = 0; mode < 3; ++mode) journal_case(dir, t, std::max(8, 2400 / t / 4), mode, false);
        journal_case(dir, t, std::max(8, 2400 / t / 4), 0, false, true);
        journal_case(dir, t, std::max(8, 2400 / t / 4), 0, false, false, 4);  // pipelined rounds
        journal_case(dir, t, std::max(8, 2400 / t / 4), 0, false, true, 4);
      }
      std::printf("\n]}\n");
      return 0;
    }
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--disk-sweep") {
      std::string dir = "/tmp/io_bench_disk";
      for (int j = 1; j + 1 < argc; ++j)
        if (std::string(argv[j]) == "--dir") dir = argv[j + 1];
      std::printf("{\"disk_sweep\": [");
      bool first = true;
      for (int j = 1; j + 1 < argc; ++j)  // --cases "threads:gate[:direct],..." in this order
        if (std::string(argv[j]) == "--cases") {
          std::string c = argv[j + 1];
          size_t p = 0;
          while (p < c.size()) {
            size_t e = c.find(',', p);
            if (e == std::string::npos) e = c.size();
            int t = 0, g = 0, d = 0;  // threads:gate[:direct]
            if (std::sscanf(c.substr(p, e - p).c_str(), "%d:%d:%d", &t, &g, &d) >= 2 && t > 0) {
              disk_case(dir, t, std::max(4, 2400 / t / 4), d != 0, g, first);
              first = false;
            }
            p = e + 1;
          }
          std::printf("\n]}\n");
          return 0;
        }
      for (int direct = 0; direct < 2; ++direct)
        for (int t : {1, 10, 30, 60, 120, 240}) {
          disk_case(dir, t, std::max(4, 2400 / t / 4), direct != 0, 0, first);
          first = false;
        }
      // the same overload behind the node-wide gate (what ChunkStore does)
      for (int g : {8, 16, 24, 32})
        for (int t : {60, 240}) disk_case(dir, t, std::max(4, 2400 / t / 4), false, g, false);
      std::printf("\n]}\n");
      return 0;
    }
  std::string dir = "/tmp/io_bench_store";
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--dir" && i + 1 < argc) dir = argv[++i];
    else if (a == "--iters" && i + 1 < argc) iters = std::atoi(argv[++i]);
    else if (a == "--no-fsync") fsync = false;
    else if (a == "--staged") zero_copy = false;
    else if (a == "--rs-only") rs_only = true;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) device = -1;
  std::filesystem::remove_all(dir);

  // zero_copy: the client buffers are registered with the store the way the fast path
  // registers a client's shared-memory arena (one DMA per copy); --staged: pinned bounce
  if (rs_only) std::printf("{\n  \"device\": %d, \"rs_only\": true,\n", device);
  if (!rs_only) {
  std::printf("{\n  \"device\": %d, \"iters\": %d, \"fsync\": %s, \"zero_copy\": %s,\n  \"store\": {", device,
              iters, fsync ? "true" : "false", zero_copy ? "true" : "false");
  bool first = true;
  const size_t sizes[] = {4096, 65536, 1 << 20, 64u << 20};
  for (int mode = 0; mode < 2; ++mode) {
    StoreConfig cfg;
    cfg.storage_dir = dir + (mode == 0 ? "/nvme" : "/hbm");
    cfg.device = device;
    cfg.hbm_capacity = device >= 0 ? (8ull << 30) : 0;
    cfg.durability = mode == 0 ? Durability::NvmeSync : Durability::HbmAck;
    cfg.sync_writes = fsync;
    ChunkStore store(cfg);
    const char* tag = mode == 0 ? "write_nvme_sync" : "write_hbm_ack";
    for (size_t sz : sizes) {
      int n = sz >= (64u << 20) ? std::max(3, iters / 10) : iters;
      auto data = random_bytes(sz, static_cast<uint32_t>(sz + mode));
      uint32_t crc = crc32(data.data(), sz);
      Lat w, r, pr;
      std::vector<uint8_t> out(sz);
      bool reg = zero_copy && store.register_host(data.data(), sz) && store.register_host(out.data(), sz);
      for (int i = 0; i < n; ++i) {
        std::string id = std::string("b") + std::to_string(mode) + "_" + std::to_string(sz) + "_" + std::to_string(i);
        auto t0 = Clock::now();
        WriteResult wr = store.write(id, data.data(), sz, crc);
        auto t1 = Clock::now();
        if (!wr.ok) {
          std::fprintf(stderr, "write failed: %s\n", wr.error.c_str());
          return 1;
        }
        w.add(secs(t0, t1));
        t0 = Clock::now();
        ReadResult rr = store.read_into(id, 0, sz, out.data());
        t1 = Clock::now();
        if (rr.status != ReadStatus::Ok || std::memcmp(out.data(), data.data(), sz) != 0) {
          std::fprintf(stderr, "read mismatch (%s)\n", rr.error.c_str());
          return 1;
        }
        r.add(secs(t0, t1));
        if (sz >= 65536) {
          t0 = Clock::now();
          rr = store.read_into(id, 32768, 4096, out.data());
          t1 = Clock::now();
          if (rr.status != ReadStatus::Ok || std::memcmp(out.data(), data.data() + 32768, 4096) != 0) {
            std::fprintf(stderr, "partial read mismatch\n");
            return 1;
          }
          pr.add(secs(t0, t1));
        }
      }
      if (reg) {
        store.unregister_host(data.data());
        store.unregister_host(out.data());
      }
      emit_case(first, tag, sz, w);
      emit_case(first, mode == 0 ? "read_after_nvme_sync" : "read_after_hbm_ack", sz, r);
      if (sz >= 65536) emit_case(first, mode == 0 ? "partial4k_nvme" : "partial4k_hbm", sz, pr);
    }
    store.flush();
    if (mode == 0) {
      auto t0 = Clock::now();
      auto bad = store.scrub();
      auto t1 = Clock::now();
      StoreStats st = store.stats();
      std::printf(",\n    \"scrub\": {\"blocks\": %llu, \"bytes\": %llu, \"seconds\": %.4f, \"GBps\": %.2f, \"bad\": %zu}",
                  static_cast<unsigned long long>(st.blocks), static_cast<unsigned long long>(st.bytes),
                  secs(t0, t1), st.bytes / std::max(1e-9, secs(t0, t1)) / 1e9, bad.size());
    }
  }
  std::printf("\n  },\n");

  // ---- K1b: batched scrub of HBM-resident blocks (kernel path only; no disk re-read)
  if (device >= 0) {
    StoreConfig cfg;
    cfg.storage_dir = dir + "/scrub";
    cfg.device = device;
    cfg.hbm_capacity = 2ull << 30;
    cfg.durability = Durability::HbmAck;
    cfg.sync_writes = false;
    ChunkStore s(cfg);
    const int nb = 1024;
    auto data = random_bytes((1 << 20) + 100, 11);
    std::vector<std::string> ids;
    for (int i = 0; i < nb; ++i) {
      size_t sz = (i % 4 == 3) ? (1 << 20) + 100 : (1 << 20);  // every 4th block has a short tail slice
      std::string id = "s" + std::to_string(i);
      if (!s.stage(id, data.data(), sz, crc32(data.data(), sz)).ok) return 1;
      ids.push_back(id);
    }
    s.scrub_resident(ids);  // warm-up (allocations, code object)
    auto t0 = Clock::now();
    auto bad = s.scrub_resident(ids);
    auto t1 = Clock::now();
    double bytes = nb * double(1 << 20) + (nb / 4) * 100.0;
    std::printf("  \"scrub_hbm_1024x1MiB\": {\"seconds\": %.6f, \"GBps\": %.1f, \"bad\": %zu},\n", secs(t0, t1),
                bytes / secs(t0, t1) / 1e9, bad.size());
  }

  // ---- CRC: GPU (H2D + K1/K2) vs CPU PCLMUL, 256 MiB
  {
    const size_t n = 256u << 20;
    auto data = random_bytes(n, 7);
    auto t0 = Clock::now();
    uint32_t cpu = crc32(data.data(), n);
    auto t1 = Clock::now();
    double cpu_s = secs(t0, t1);
    double gpu_s = 0;
    uint32_t gpu = cpu;
    if (device >= 0) {
      StoreConfig cfg;
      cfg.storage_dir = dir + "/crc";
      cfg.device = device;
      cfg.hbm_capacity = 1ull << 30;
      ChunkStore s(cfg);
      std::vector<uint32_t> sl;
      s.gpu_crc(data.data(), 1 << 20, &sl);  // warm-up (tables, lanes)
      t0 = Clock::now();
      gpu = s.gpu_crc(data.data(), n, &sl);
      t1 = Clock::now();
      gpu_s = secs(t0, t1);
    }
    std::printf("  \"crc32_256MiB\": {\"cpu_GBps\": %.2f, \"gpu_incl_h2d_GBps\": %.2f, \"match\": %s},\n",
                n / cpu_s / 1e9, gpu_s > 0 ? n / gpu_s / 1e9 : 0.0, cpu == gpu ? "true" : "false");
  }

  }  // !rs_only

  // ---- RS(6,3) encode of 6 x 16 MiB shards: GPU vs CPU
  {
    const int k = 6, m = 3;
    const size_t len = 16u << 20;
    gf::Matrix full = gf::rs_matrix(k, m);
    gf::Matrix parity(full.begin() + k, full.end());
    std::vector<std::vector<uint8_t>> in(k), out_c(m, std::vector<uint8_t>(len)), out_g(m, std::vector<uint8_t>(len));
    std::vector<const uint8_t*> ip;
    std::vector<uint8_t*> oc, og;
    for (int i = 0; i < k; ++i) {
      in[i] = random_bytes(len, 100 + i);
      ip.push_back(in[i].data());
    }
    for (int i = 0; i < m; ++i) {
      oc.push_back(out_c[i].data());
      og.push_back(out_g[i].data());
    }
    auto t0 = Clock::now();
    gf::matmul_cpu(parity, ip.data(), oc.data(), len);
    auto t1 = Clock::now();
    double cpu_s = secs(t0, t1), gpu_s = 0;
    bool match = true;
    if (device >= 0) {
      StoreConfig cfg;
      cfg.storage_dir = dir + "/rs";
      cfg.device = device;
      cfg.hbm_capacity = 1ull << 30;
      ChunkStore s(cfg);
      if (zero_copy) {  // shards in registered memory, as a client's shm slot is
        for (auto* p : ip) s.register_host(p, len);
        for (auto* p : og) s.register_host(p, len);
      }
      s.gf_matmul_gpu(parity, ip, og, 4096);  // warm-up
      gpu_s = 1e9;
      for (int rep = 0; rep < 3; ++rep) {
        t0 = Clock::now();
        s.gf_matmul_gpu(parity, ip, og, len);
        t1 = Clock::now();
        gpu_s = std::min(gpu_s, secs(t0, t1));
      }
      for (int i = 0; i < m; ++i) match = match && out_c[i] == out_g[i];
    }
    std::printf("  \"rs63_encode_96MiB\": {\"cpu_GBps\": %.2f, \"gpu_incl_copies_GBps\": %.2f, \"match\": %s}\n}\n",
                k * len / cpu_s / 1e9, gpu_s > 0 ? k * len / gpu_s / 1e9 : 0.0, match ? "true" : "false");
  }
  std::filesystem::remove_all(dir);
  return 0;
}

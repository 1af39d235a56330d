// modal_amd._core — native runtime core (C++20, pybind11).
//
// The reference ships native client runtimes alongside Python (Go ~19k LoC,
// TypeScript ~11k). This module is the C++ core of the
// MI355X-native runtime's data plane:
//
//  * ShmRing — single-producer/single-consumer byte ring in a mmap'd file:
//    the per-worker payload channel ("per-GPU input/output ring
//    buffers in pinned host memory"). Large input/output frames ride the
//    ring; the Unix socket stays the control/doorbell path. Lock-free
//    (acquire/release atomics), frames length-prefixed, wrap-around via a
//    skip sentinel. memcpy of large frames runs with the GIL released.
//
//  * RingHub / ChunkLane — the native chunk lane (ring.h, lane.h, both free
//    of Python types): futex doorbells on the rings, one waiter thread per
//    process that signals the event loop through an eventfd, and a
//    dispatcher that places map chunks on workers, returns credit on
//    chunk_done and refills, all inside one drain() call.
//
//  * pack_payloads / unpack_payloads — batch pickle-payload framing used by
//    the map fan-out: N buffers <-> one contiguous [u32 len]* blob without
//    per-item Python bytes handling.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "lane.h"
#include "ring.h"

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

namespace py = pybind11;

namespace {

using modal_amd::BellFile;
using modal_amd::Ring;
using modal_amd::RingHub;

// frames this large are copied with the GIL released
constexpr uint64_t kGilReleaseBytes = 64 * 1024;

// producer: returns false when the frame does not fit right now
bool ring_push(Ring& ring, py::buffer buf) {
  py::buffer_info info = buf.request();
  const uint8_t* src = static_cast<const uint8_t*>(info.ptr);
  const uint64_t n = (uint64_t)info.size * (uint64_t)info.itemsize;
  uint8_t* dst = ring.reserve(n);
  if (!dst) return false;
  if (n >= kGilReleaseBytes) {
    py::gil_scoped_release release;
    std::memcpy(dst, src, n);
  } else {
    std::memcpy(dst, src, n);
  }
  ring.commit();
  return true;
}

// consumer: drain up to max_frames frames (0 = all available)
py::list ring_pop_all(Ring& ring, size_t max_frames) {
  py::list out;
  ring.pop(
      [&](const uint8_t* ptr, size_t len) {
        out.append(py::bytes(reinterpret_cast<const char*>(ptr), len));
      },
      max_frames);
  return out;
}

// every frame of every ring of the hub, in ring order: [(slot, bytes)]
py::list hub_drain(RingHub& hub) {
  py::list out;
  hub.drain([&](int slot, const uint8_t* ptr, size_t len) {
    out.append(py::make_tuple(slot, py::bytes(reinterpret_cast<const char*>(ptr), len)));
  });
  return out;
}

using modal_amd::Assignment;
using modal_amd::ChunkDone;
using modal_amd::ChunkLane;
using modal_amd::FrameKind;

py::str sv_str(std::string_view s) { return py::str(s.data(), s.size()); }

// (token, call_id, chunk_id, function_id, count, data, cis)
py::tuple done_tuple(const ChunkDone& d) {
  py::object cis = py::none();
  if (!d.cis_nil) {
    py::list items;
    for (int64_t v : d.cis) items.append(py::int_(v));
    cis = std::move(items);
  }
  return py::make_tuple(sv_str(d.token), sv_str(d.call_id), sv_str(d.chunk_id),
                        sv_str(d.function_id), py::int_(d.count),
                        py::bytes(d.data.data(), d.data.size()), cis);
}

py::list assignment_list(const std::vector<Assignment>& assignments) {
  py::list out;
  for (const auto& a : assignments) out.append(py::make_tuple(a.token, a.worker_slot));
  return out;
}

// the clean tuple, or None for a frame Python has to read itself
py::object parse_chunk_done_py(py::buffer buf) {
  py::buffer_info info = buf.request();
  ChunkDone done;
  FrameKind kind = modal_amd::parse_chunk_done(
      static_cast<const uint8_t*>(info.ptr), (size_t)info.size * (size_t)info.itemsize, &done);
  if (kind != FrameKind::kDoneClean) return py::none();
  return done_tuple(done);
}

int lane_submit(ChunkLane& lane, int fn_slot, const std::string& token, uint64_t count,
                py::buffer frame, bool front) {
  py::buffer_info info = frame.request();
  return lane.submit(fn_slot, token, count, static_cast<const uint8_t*>(info.ptr),
                     (size_t)info.size * (size_t)info.itemsize, front);
}

// (completions[(worker_slot, clean tuple)], raw_frames[(worker_slot, bytes)],
//  assignments[(token, worker_slot)])
py::tuple lane_drain(ChunkLane& lane, RingHub& hub) {
  py::list completions, raw;
  std::vector<Assignment> assignments;
  lane.drain(
      hub,
      [&](int slot, const ChunkDone& done) {
        completions.append(py::make_tuple(slot, done_tuple(done)));
      },
      [&](int slot, const uint8_t* ptr, size_t len) {
        raw.append(py::make_tuple(slot, py::bytes(reinterpret_cast<const char*>(ptr), len)));
      },
      &assignments);
  return py::make_tuple(completions, raw, assignment_list(assignments));
}

py::bytes pack_payloads(const std::vector<py::bytes>& items) {
  uint64_t total = 0;
  std::vector<std::pair<const char*, size_t>> views;
  views.reserve(items.size());
  for (const auto& item : items) {
    char* ptr;
    Py_ssize_t n;
    if (PyBytes_AsStringAndSize(item.ptr(), &ptr, &n) != 0)
      throw std::runtime_error("pack_payloads: not bytes");
    views.emplace_back(ptr, (size_t)n);
    total += 4 + (uint64_t)n;
  }
  std::string out;
  out.resize(total);
  {
    py::gil_scoped_release release;
    char* dst = out.data();
    for (const auto& [ptr, n] : views) {
      uint32_t len32 = (uint32_t)n;
      std::memcpy(dst, &len32, 4);
      std::memcpy(dst + 4, ptr, n);
      dst += 4 + n;
    }
  }
  return py::bytes(out);
}

py::list unpack_payloads(py::buffer buf) {
  py::buffer_info info = buf.request();
  const char* src = static_cast<const char*>(info.ptr);
  size_t n = (size_t)info.size * (size_t)info.itemsize;
  py::list out;
  size_t pos = 0;
  while (pos + 4 <= n) {
    uint32_t len32;
    std::memcpy(&len32, src + pos, 4);
    if (pos + 4 + len32 > n) throw std::runtime_error("unpack_payloads: truncated");
    out.append(py::bytes(src + pos + 4, len32));
    pos += 4 + len32;
  }
  if (pos != n) throw std::runtime_error("unpack_payloads: trailing bytes");
  return out;
}

}  // namespace


// ---------------------------------------------------------------------------
// LZ4 block codec + MALZ41 container (CPU side of ops/csrc/lz4.hip).
//
// The CPU fallback previously ran through a pure-Python codec
// (utils/lz4ref.py, ~tens of MB/s); GPU-less consumers decompressing .z CAS
// entries and image/mount materialization now run at native speed. The
// container format is identical to the HIP kernels': 4 KiB segments, each a
// standard LZ4 block (or stored raw, comp_len 0). Segments compress and
// decompress in parallel across a small thread pool; the GIL is released
// for the whole pass.

static constexpr int kSegSize = 4096;
static constexpr int kMinMatch = 4;
static constexpr int kMFLimit = 12;
static constexpr int kLastLiterals = 5;

static inline uint32_t lz4_hash(uint32_t v) { return (v * 2654435761u) >> (32 - 12); }

// compress one block; returns compressed size or 0 when dst_cap exceeded
static size_t lz4_compress_one(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap) {
  uint16_t table[1 << 12];
  std::memset(table, 0, sizeof(table));
  size_t op = 0, ip = 0, anchor = 0;
  auto emit = [&](size_t lit_start, size_t lit_len, int match_len) -> bool {
    size_t need = 1 + lit_len + (lit_len >= 15 ? 1 + (lit_len - 15) / 255 : 0) +
                  (match_len >= 0 ? 2 + 1 + 16 : 0);
    if (op + need + 8 > dst_cap) return false;
    int ml = match_len >= 0 ? match_len - kMinMatch : 0;
    uint8_t token = (uint8_t)((lit_len < 15 ? lit_len : 15) << 4);
    if (match_len >= 0) token |= (uint8_t)(ml < 15 ? ml : 15);
    dst[op++] = token;
    if (lit_len >= 15) {
      size_t rest = lit_len - 15;
      while (rest >= 255) { dst[op++] = 255; rest -= 255; }
      dst[op++] = (uint8_t)rest;
    }
    std::memcpy(dst + op, src + lit_start, lit_len);
    op += lit_len;
    return true;
  };
  if (n >= (size_t)(kMinMatch + kLastLiterals)) {
    size_t mflimit = n >= kMFLimit ? n - kMFLimit : 0;
    while (ip < mflimit) {
      uint32_t seq;
      std::memcpy(&seq, src + ip, 4);
      uint32_t h = lz4_hash(seq);
      size_t cand = table[h];
      table[h] = (uint16_t)ip;  // n <= 4096 so 16 bits suffice
      uint32_t cseq;
      bool ok = cand < ip && ip - cand <= 0xFFFF;
      if (ok) { std::memcpy(&cseq, src + cand, 4); ok = cseq == seq; }
      if (ok) {
        size_t mlen = kMinMatch;
        size_t maxm = n - kLastLiterals - ip;
        while (mlen < maxm && src[cand + mlen] == src[ip + mlen]) mlen++;
        if (!emit(anchor, ip - anchor, (int)mlen)) return 0;
        size_t off = ip - cand;
        dst[op++] = (uint8_t)(off & 0xFF);
        dst[op++] = (uint8_t)(off >> 8);
        int ml = (int)mlen - kMinMatch;
        if (ml >= 15) {
          int rest = ml - 15;
          while (rest >= 255) { dst[op++] = 255; rest -= 255; }
          dst[op++] = (uint8_t)rest;
        }
        ip += mlen;
        anchor = ip;
      } else {
        ip++;
      }
    }
  }
  if (!emit(anchor, n - anchor, -1)) return 0;
  return op;
}

static bool lz4_decompress_one(const uint8_t* src, size_t comp_len,
                               uint8_t* dst, size_t raw_len) {
  size_t ip = 0, op = 0;
  while (ip < comp_len) {
    uint8_t token = src[ip++];
    size_t lit = token >> 4;
    if (lit == 15) {
      uint8_t b;
      do { if (ip >= comp_len) return false; b = src[ip++]; lit += b; } while (b == 255);
    }
    if (ip + lit > comp_len || op + lit > raw_len) return false;
    std::memcpy(dst + op, src + ip, lit);
    ip += lit; op += lit;
    if (ip >= comp_len) break;  // last literals
    if (ip + 2 > comp_len) return false;
    size_t off = src[ip] | ((size_t)src[ip + 1] << 8);
    ip += 2;
    if (off == 0 || off > op) return false;
    size_t mlen = (token & 0xF) + kMinMatch;
    if ((token & 0xF) == 15) {
      uint8_t b;
      do { if (ip >= comp_len) return false; b = src[ip++]; mlen += b; } while (b == 255);
    }
    if (op + mlen > raw_len) return false;
    // overlapping copy: byte-by-byte when ranges overlap
    if (off >= mlen) {
      std::memcpy(dst + op, dst + op - off, mlen);
    } else {
      for (size_t k = 0; k < mlen; k++) dst[op + k] = dst[op - off + k];
    }
    op += mlen;
  }
  return op == raw_len;
}

static void parallel_for(size_t n, const std::function<void(size_t, size_t)>& body) {
  unsigned hw = std::thread::hardware_concurrency();
  size_t n_threads = std::min<size_t>(std::max(1u, hw / 2), 8);
  if (n < 8 || n_threads <= 1) { body(0, n); return; }
  std::vector<std::thread> threads;
  size_t chunk = (n + n_threads - 1) / n_threads;
  for (size_t t = 0; t < n_threads; t++) {
    size_t lo = t * chunk, hi = std::min(n, lo + chunk);
    if (lo >= hi) break;
    threads.emplace_back([&body, lo, hi] { body(lo, hi); });
  }
  for (auto& th : threads) th.join();
}

// MALZ41 container compress; returns None when incompressible (>= min_gain)
py::object malz_compress(py::bytes data, double min_gain) {
  char* buf; ssize_t n_s;
  if (PyBytes_AsStringAndSize(data.ptr(), &buf, &n_s) != 0) throw py::error_already_set();
  size_t n = (size_t)n_s;
  size_t n_seg = (n + kSegSize - 1) / kSegSize;
  if (n_seg == 0) return py::none();
  std::vector<uint32_t> comp_lens(n_seg, 0);
  std::vector<std::vector<uint8_t>> outs(n_seg);
  const uint8_t* src = (const uint8_t*)buf;
  {
    py::gil_scoped_release release;
    parallel_for(n_seg, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        size_t seg_off = i * kSegSize;
        size_t seg_len = std::min((size_t)kSegSize, n - seg_off);
        outs[i].resize(kSegSize);  // only keep if it SAVES space
        size_t c = lz4_compress_one(src + seg_off, seg_len, outs[i].data(), seg_len > 1 ? seg_len - 1 : 0);
        if (c > 0 && c < seg_len) {
          comp_lens[i] = (uint32_t)c;
          outs[i].resize(c);
        } else {
          comp_lens[i] = 0;
          outs[i].clear();
        }
      }
    });
  }
  size_t total = 0;
  for (size_t i = 0; i < n_seg; i++) {
    size_t seg_len = std::min((size_t)kSegSize, n - i * kSegSize);
    total += comp_lens[i] ? comp_lens[i] : seg_len;
  }
  if ((double)total >= (double)n * min_gain) return py::none();
  size_t header = 6 + 12 + 4 * n_seg;
  py::bytes out_obj(nullptr, (ssize_t)(header + total));
  uint8_t* out = (uint8_t*)PyBytes_AsString(out_obj.ptr());
  std::memcpy(out, "MALZ41", 6);
  uint64_t n64 = n;
  uint32_t ns32 = (uint32_t)n_seg;
  std::memcpy(out + 6, &n64, 8);
  std::memcpy(out + 14, &ns32, 4);
  std::memcpy(out + 18, comp_lens.data(), 4 * n_seg);
  size_t op = header;
  for (size_t i = 0; i < n_seg; i++) {
    size_t seg_off = i * kSegSize;
    size_t seg_len = std::min((size_t)kSegSize, n - seg_off);
    if (comp_lens[i]) {
      std::memcpy(out + op, outs[i].data(), comp_lens[i]);
      op += comp_lens[i];
    } else {
      std::memcpy(out + op, src + seg_off, seg_len);
      op += seg_len;
    }
  }
  return out_obj;
}

py::bytes malz_decompress(py::bytes blob) {
  char* buf; ssize_t bn;
  if (PyBytes_AsStringAndSize(blob.ptr(), &buf, &bn) != 0) throw py::error_already_set();
  if (bn < 18 || std::memcmp(buf, "MALZ41", 6) != 0)
    throw std::runtime_error("not a MALZ41 container");
  uint64_t raw_len;
  uint32_t n_seg;
  std::memcpy(&raw_len, buf + 6, 8);
  std::memcpy(&n_seg, buf + 14, 4);
  size_t header = 6 + 12 + 4 * (size_t)n_seg;
  if ((size_t)bn < header) throw std::runtime_error("truncated container header");
  std::vector<uint32_t> comp_lens(n_seg);
  std::memcpy(comp_lens.data(), buf + 18, 4 * (size_t)n_seg);
  // per-segment payload offsets
  std::vector<size_t> seg_payload_off(n_seg);
  size_t pos = header;
  for (size_t i = 0; i < n_seg; i++) {
    seg_payload_off[i] = pos;
    size_t seg_len = std::min((size_t)kSegSize, (size_t)raw_len - i * kSegSize);
    pos += comp_lens[i] ? comp_lens[i] : seg_len;
  }
  if (pos > (size_t)bn) throw std::runtime_error("truncated container payload");
  py::bytes out_obj(nullptr, (ssize_t)raw_len);
  uint8_t* out = (uint8_t*)PyBytes_AsString(out_obj.ptr());
  const uint8_t* src = (const uint8_t*)buf;
  std::atomic<bool> ok{true};  // written from every worker thread
  {
    py::gil_scoped_release release;
    parallel_for(n_seg, [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) {
        size_t seg_off = i * kSegSize;
        size_t seg_len = std::min((size_t)kSegSize, (size_t)raw_len - seg_off);
        if (comp_lens[i] == 0) {
          std::memcpy(out + seg_off, src + seg_payload_off[i], seg_len);
        } else if (!lz4_decompress_one(src + seg_payload_off[i], comp_lens[i],
                                       out + seg_off, seg_len)) {
          ok.store(false, std::memory_order_relaxed);
        }
      }
    });
  }
  if (!ok.load()) throw std::runtime_error("corrupt LZ4 segment");
  return out_obj;
}




// ---------------------------------------------------------------------------
// Sandbox supervisor: clone3(CLONE_INTO_CGROUP) + execve.
//
// The Python road (asyncio preexec_fn) runs Python between fork and exec in
// a threaded process — both unsafe and racy for cgroup attachment (the child
// runs before the parent can write cgroup.procs). clone3 places the child in
// the target cgroup v2 ATOMICALLY at creation. Parity target: the
// reference's Go sandbox supervisor, done the Linux-native
// way.
// ---------------------------------------------------------------------------
#include <sys/syscall.h>
#include <sys/resource.h>
#include <sched.h>
#include <signal.h>

namespace {

struct clone_args_compat {
  uint64_t flags;
  uint64_t pidfd;
  uint64_t child_tid;
  uint64_t parent_tid;
  uint64_t exit_signal;
  uint64_t stack;
  uint64_t stack_size;
  uint64_t tls;
  uint64_t set_tid;
  uint64_t set_tid_size;
  uint64_t cgroup;
};

#ifndef CLONE_INTO_CGROUP
#define CLONE_INTO_CGROUP 0x200000000ULL
#endif

}  // namespace

// Returns the child pid. Throws on failure. stdio fds are dup2'd onto
// 0/1/2 in the child (pass -1 to inherit). The child setsid()s so the whole
// tree is killable as one process group.
static int64_t spawn_supervised(const std::vector<std::string>& argv,
                                const std::string& cwd,
                                const std::vector<std::string>& env,
                                const std::string& cgroup_dir,
                                int64_t rlimit_as_mib,
                                int stdin_fd, int stdout_fd, int stderr_fd) {
  if (argv.empty()) throw std::runtime_error("empty argv");
  int cg_fd = -1;
  if (!cgroup_dir.empty()) {
    cg_fd = ::open(cgroup_dir.c_str(), O_DIRECTORY | O_RDONLY | O_CLOEXEC);
    if (cg_fd < 0)
      throw std::runtime_error("open cgroup dir: " + std::string(strerror(errno)));
  }

  std::vector<char*> cargv;
  cargv.reserve(argv.size() + 1);
  for (const auto& a : argv) cargv.push_back(const_cast<char*>(a.c_str()));
  cargv.push_back(nullptr);
  std::vector<char*> cenv;
  cenv.reserve(env.size() + 1);
  for (const auto& e : env) cenv.push_back(const_cast<char*>(e.c_str()));
  cenv.push_back(nullptr);

  clone_args_compat ca{};
  ca.exit_signal = SIGCHLD;
  if (cg_fd >= 0) {
    ca.flags = CLONE_INTO_CGROUP;
    ca.cgroup = (uint64_t)cg_fd;
  }

  long pid = syscall(SYS_clone3, &ca, sizeof(ca));
  if (pid < 0 && cg_fd >= 0 && (errno == EINVAL || errno == ENOSYS || errno == EPERM ||
                                errno == EBADF || errno == EOPNOTSUPP)) {
    // kernel/cgroup too old or not delegated: plain clone3; the caller's
    // Python-side attach (child writes cgroup.procs) remains the fallback
    ::close(cg_fd);
    cg_fd = -1;
    throw std::runtime_error("clone3(CLONE_INTO_CGROUP) unavailable: " +
                             std::string(strerror(errno)));
  }
  if (pid < 0) {
    if (cg_fd >= 0) ::close(cg_fd);
    throw std::runtime_error("clone3: " + std::string(strerror(errno)));
  }
  if (pid == 0) {
    // child: async-signal-safe calls only
    ::setsid();
    if (stdin_fd >= 0) ::dup2(stdin_fd, 0);
    if (stdout_fd >= 0) ::dup2(stdout_fd, 1);
    if (stderr_fd >= 0) ::dup2(stderr_fd, 2);
    for (int fd = 3; fd < 1024; ++fd) ::close(fd);
    if (!cwd.empty() && ::chdir(cwd.c_str()) != 0) _exit(126);
    if (rlimit_as_mib > 0) {
      struct rlimit rl;
      rl.rlim_cur = rl.rlim_max = (rlim_t)rlimit_as_mib << 20;
      ::setrlimit(RLIMIT_AS, &rl);
    }
    ::execve(cargv[0], cargv.data(), cenv.data());
    _exit(127);
  }
  if (cg_fd >= 0) ::close(cg_fd);
  return (int64_t)pid;
}


PYBIND11_MODULE(_core, m) {
  m.doc() = "modal_amd native core: shm ring transport + batch framing";
  py::class_<BellFile, std::shared_ptr<BellFile>>(m, "BellFile")
      .def(py::init<const std::string&, bool>(), py::arg("path"), py::arg("create") = false);
  py::class_<Ring, std::shared_ptr<Ring>>(m, "ShmRing")
      .def(py::init<const std::string&, uint64_t, bool>(), py::arg("path"),
           py::arg("capacity") = (uint64_t)64 << 20, py::arg("create") = false)
      .def("push", &ring_push)
      .def("pop_all", &ring_pop_all, py::arg("max_frames") = 0)
      .def("pending_bytes", &Ring::pending_bytes)
      .def("capacity", &Ring::capacity)
      .def("too_large", &Ring::too_large)
      .def("bell_wakes", &Ring::bell_wakes)
      .def("set_shared_bell", &Ring::set_shared_bell);
  py::class_<RingHub>(m, "RingHub")
      .def(py::init<const std::string&, int>(), py::arg("bell_path") = "",
           py::arg("timeout_ms") = 20)
      .def("add_ring", &RingHub::add_ring)
      .def("remove_ring", &RingHub::remove_ring)
      .def("fd", &RingHub::fd)
      .def("drain", &hub_drain)
      // joins the waiter with the GIL held: the waiter never takes it, and a
      // daemon thread that gave it up here could be ended inside this frame
      // by interpreter shutdown
      .def("close", &RingHub::close)
      .def("stats", [](RingHub& hub) {
        py::dict d;
        d["notifies"] = hub.notifies();
        d["waits"] = hub.waits();
        d["drains"] = hub.drains();
        d["producer_wakes"] = hub.producer_wakes();
        d["rings"] = hub.ring_count();
        return d;
      });
  py::class_<ChunkLane>(m, "ChunkLane")
      .def(py::init<>())
      .def("add_worker", &ChunkLane::add_worker)
      .def("remove_worker", &ChunkLane::remove_worker)
      .def("set_eligible", &ChunkLane::set_eligible)
      .def("set_cap", &ChunkLane::set_cap, py::arg("fn_slot"), py::arg("items"),
           py::arg("min_chunks") = 1)
      .def("submit", &lane_submit, py::arg("fn_slot"), py::arg("token"), py::arg("count"),
           py::arg("frame"), py::arg("front") = false)
      .def("kick", [](ChunkLane& lane, int fn_slot) {
        std::vector<Assignment> out;
        lane.kick(fn_slot, &out);
        return assignment_list(out);
      })
      .def("complete", [](ChunkLane& lane, int worker_slot, const std::string& token) {
        std::vector<Assignment> out;
        lane.complete(worker_slot, token, &out);
        return assignment_list(out);
      })
      .def("cancel", &ChunkLane::cancel)
      .def("drop_queue", &ChunkLane::drop_queue)
      .def("drain", &lane_drain)
      .def("queued", &ChunkLane::queued)
      .def("inflight", &ChunkLane::inflight)
      .def("outstanding_items", &ChunkLane::outstanding_items)
      .def("pushed", &ChunkLane::pushed);
  m.def("parse_chunk_done", &parse_chunk_done_py);
  m.def("pack_payloads", &pack_payloads);
  m.def("malz_compress", &malz_compress, py::arg("data"), py::arg("min_gain") = 0.95);
  m.def("malz_decompress", &malz_decompress);
  m.def("unpack_payloads", &unpack_payloads);
  m.def("spawn_supervised", &spawn_supervised, py::arg("argv"), py::arg("cwd"),
        py::arg("env"), py::arg("cgroup_dir") = "", py::arg("rlimit_as_mib") = 0,
        py::arg("stdin_fd") = -1, py::arg("stdout_fd") = -1, py::arg("stderr_fd") = -1,
        "clone3(CLONE_INTO_CGROUP) + execve supervisor (atomic cgroup placement)");
}

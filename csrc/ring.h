// Shared-memory ring, doorbell and hub — the Python-free part of the native
// core, so a stand-alone program (csrc/lane_stress.cpp) can drive it.
//
//  * Ring — single-producer/single-consumer byte ring in a mmap'd file.
//    Frames are length-prefixed; wrap-around uses a skip sentinel. The
//    header carries a Bell: after every push the producer bumps the
//    doorbell word and issues a shared FUTEX_WAKE only when the consumer's
//    "waiting" flag is set.
//
//  * BellFile — one Bell in a file of its own. Every worker that produces
//    into one of the scheduler's inbound rings also bumps this shared bell,
//    so the scheduler needs a single waiter for any number of rings. (The
//    alternative, futex_waitv, is capped at 128 words per call and needs
//    Linux >= 5.16; a shared word has neither limit.)
//
//  * RingHub — one waiter thread for a set of inbound rings. The thread
//    never moves a ring's tail: it only reads the atomics, and when data is
//    pending and the event loop has not been told yet it writes an eventfd
//    the loop has registered a reader for. drain() runs on the loop thread
//    and pops every frame of every ring in one call, so producer and
//    consumer of each ring stay the loop thread of their process (SPSC).

#pragma once

#include <atomic>
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstring>
#include <ctime>
#include <fcntl.h>
#include <linux/futex.h>
#include <memory>
#include <csignal>
#include <pthread.h>
#include <mutex>
#include <stdexcept>
#include <string>
#include <sys/eventfd.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>
#include <utility>
#include <vector>

namespace modal_amd {

struct Bell {
  std::atomic<uint32_t> seq;      // doorbell word (futex)
  std::atomic<uint32_t> waiting;  // consumer is (about to be) asleep on seq
  std::atomic<uint32_t> wakes;    // FUTEX_WAKE syscalls issued by producers
  uint32_t pad;
};

inline void bell_ring(Bell& b) {
  b.seq.fetch_add(1, std::memory_order_seq_cst);
  if (b.waiting.load(std::memory_order_seq_cst)) {
    b.wakes.fetch_add(1, std::memory_order_relaxed);
    ::syscall(SYS_futex, reinterpret_cast<uint32_t*>(&b.seq), FUTEX_WAKE, INT_MAX,
              nullptr, nullptr, 0);
  }
}

// sleep until seq != seen, a wake, or the timeout
inline void bell_wait(Bell& b, uint32_t seen, int timeout_ms) {
  struct timespec ts;
  ts.tv_sec = timeout_ms / 1000;
  ts.tv_nsec = (long)(timeout_ms % 1000) * 1000000L;
  ::syscall(SYS_futex, reinterpret_cast<uint32_t*>(&b.seq), FUTEX_WAIT, seen, &ts,
            nullptr, 0);
}

struct RingHeader {
  alignas(64) std::atomic<uint64_t> head;  // bytes produced
  alignas(64) std::atomic<uint64_t> tail;  // bytes consumed
  alignas(64) uint64_t capacity;
  uint64_t magic;
  Bell bell;
};

constexpr uint64_t kMagic = 0x6d6f64616c616d64ULL;  // "modalamd"
constexpr uint32_t kSkip = 0xFFFFFFFFu;

class BellFile {
 public:
  BellFile(const std::string& path, bool create) {
    int fd = ::open(path.c_str(), create ? (O_RDWR | O_CREAT) : O_RDWR, 0600);
    if (fd < 0) throw std::runtime_error("BellFile: open failed: " + path);
    if (create && ::ftruncate(fd, (off_t)kSize) != 0) {
      ::close(fd);
      throw std::runtime_error("BellFile: ftruncate failed");
    }
    struct stat st;
    if (::fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(Bell)) {
      ::close(fd);
      throw std::runtime_error("BellFile: bad bell file");
    }
    void* mem = ::mmap(nullptr, kSize, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    if (mem == MAP_FAILED) throw std::runtime_error("BellFile: mmap failed");
    bell_ = static_cast<Bell*>(mem);
  }
  ~BellFile() {
    if (bell_) ::munmap(bell_, kSize);
  }
  BellFile(const BellFile&) = delete;
  BellFile& operator=(const BellFile&) = delete;
  Bell* bell() const { return bell_; }

 private:
  static constexpr size_t kSize = 64;
  Bell* bell_ = nullptr;
};

class Ring {
 public:
  Ring(const std::string& path, uint64_t capacity, bool create) {
    int flags = create ? (O_RDWR | O_CREAT) : O_RDWR;
    fd_ = ::open(path.c_str(), flags, 0600);
    if (fd_ < 0) throw std::runtime_error("ShmRing: open failed: " + path);
    uint64_t total = sizeof(RingHeader) + capacity;
    if (create) {
      if (::ftruncate(fd_, (off_t)total) != 0) {
        ::close(fd_);
        throw std::runtime_error("ShmRing: ftruncate failed");
      }
    } else {
      struct stat st;
      if (::fstat(fd_, &st) != 0 || (uint64_t)st.st_size < sizeof(RingHeader)) {
        ::close(fd_);
        throw std::runtime_error("ShmRing: bad ring file");
      }
      total = (uint64_t)st.st_size;
      capacity = total - sizeof(RingHeader);
    }
    void* mem = ::mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, 0);
    if (mem == MAP_FAILED) {
      ::close(fd_);
      throw std::runtime_error("ShmRing: mmap failed");
    }
    base_ = static_cast<uint8_t*>(mem);
    header_ = reinterpret_cast<RingHeader*>(base_);
    data_ = base_ + sizeof(RingHeader);
    total_ = total;
    if (create) {
      header_->head.store(0, std::memory_order_relaxed);
      header_->tail.store(0, std::memory_order_relaxed);
      header_->capacity = capacity;
      header_->bell.seq.store(0, std::memory_order_relaxed);
      header_->bell.waiting.store(0, std::memory_order_relaxed);
      header_->bell.wakes.store(0, std::memory_order_relaxed);
      header_->magic = kMagic;
    } else if (header_->magic != kMagic || header_->capacity != capacity) {
      ::munmap(base_, total_);
      ::close(fd_);
      throw std::runtime_error("ShmRing: magic mismatch");
    }
    capacity_ = capacity;
  }

  ~Ring() {
    if (base_) ::munmap(base_, total_);
    if (fd_ >= 0) ::close(fd_);
  }

  Ring(const Ring&) = delete;
  Ring& operator=(const Ring&) = delete;

  // A frame of n bytes can never be pushed, however empty the ring is.
  bool too_large(uint64_t n) const { return n + 8 > capacity_ || n >= kSkip; }

  // producer, step 1: where a frame of n bytes goes, or nullptr when it
  // does not fit right now. Nothing is visible to the consumer until commit.
  uint8_t* reserve(uint64_t n) {
    if (too_large(n)) throw std::runtime_error("frame larger than ring");
    uint64_t head = header_->head.load(std::memory_order_relaxed);
    uint64_t tail = header_->tail.load(std::memory_order_acquire);
    uint64_t pos = head % capacity_;
    uint64_t to_end = capacity_ - pos;
    uint64_t need = 4 + n;
    // too small for a length, or for the frame: pad to the start
    uint64_t skip = to_end < need ? to_end : 0;
    if (head + skip + need - tail > capacity_) return nullptr;  // full
    if (skip) {
      if (to_end >= 4) {
        uint32_t sentinel = kSkip;
        std::memcpy(data_ + pos, &sentinel, 4);
      }
      pos = 0;
    }
    uint32_t len32 = (uint32_t)n;
    std::memcpy(data_ + pos, &len32, 4);
    pending_commit_ = head + skip + need;
    return data_ + pos + 4;
  }

  // producer, step 2: publish the reserved frame and ring the doorbells
  void commit() {
    header_->head.store(pending_commit_, std::memory_order_release);
    bell_ring(header_->bell);
    if (shared_bell_) bell_ring(*shared_bell_->bell());
  }

  bool push(const uint8_t* src, uint64_t n) {
    uint8_t* dst = reserve(n);
    if (!dst) return false;
    std::memcpy(dst, src, n);
    commit();
    return true;
  }

  // consumer: hand up to max_frames frames (0 = all) to cb(ptr, len); the
  // tail moves once, after the last callback
  template <typename F>
  size_t pop(F&& cb, size_t max_frames = 0) {
    uint64_t tail = header_->tail.load(std::memory_order_relaxed);
    uint64_t head = header_->head.load(std::memory_order_acquire);
    if (tail == head) return 0;
    size_t count = 0;
    while (tail < head) {
      uint64_t pos = tail % capacity_;
      uint64_t to_end = capacity_ - pos;
      if (to_end < 4) {
        tail += to_end;  // padding at end (no room for a length)
        continue;
      }
      uint32_t len32;
      std::memcpy(&len32, data_ + pos, 4);
      if (len32 == kSkip) {
        tail += to_end;
        continue;
      }
      if ((uint64_t)len32 + 4 > to_end || tail + 4 + len32 > head) break;  // corrupt
      cb(static_cast<const uint8_t*>(data_ + pos + 4), (size_t)len32);
      tail += 4 + len32;
      if (max_frames && ++count >= max_frames) break;
    }
    header_->tail.store(tail, std::memory_order_release);
    return count;
  }

  bool has_pending() const {
    return header_->head.load(std::memory_order_acquire) !=
           header_->tail.load(std::memory_order_acquire);
  }

  uint64_t pending_bytes() const {
    return header_->head.load(std::memory_order_acquire) -
           header_->tail.load(std::memory_order_acquire);
  }

  uint64_t capacity() const { return capacity_; }
  Bell* bell() const { return &header_->bell; }
  uint32_t bell_wakes() const { return header_->bell.wakes.load(std::memory_order_relaxed); }

  // producer side: also bump this bell after every push
  void set_shared_bell(std::shared_ptr<BellFile> bell) { shared_bell_ = std::move(bell); }

 private:
  int fd_ = -1;
  uint8_t* base_ = nullptr;
  uint8_t* data_ = nullptr;
  RingHeader* header_ = nullptr;
  uint64_t capacity_ = 0;
  uint64_t total_ = 0;
  uint64_t pending_commit_ = 0;
  std::shared_ptr<BellFile> shared_bell_;
};

class RingHub {
 public:
  // bell_path empty: wait on the header bell of the first ring added (a
  // worker waits on one ring). Otherwise create and wait on the shared bell
  // file every producer bumps (the scheduler waits on all its workers).
  explicit RingHub(const std::string& bell_path = "", int timeout_ms = 20)
      : timeout_ms_(timeout_ms < 1 ? 1 : timeout_ms) {
    if (!bell_path.empty()) {
      bell_file_ = std::make_shared<BellFile>(bell_path, true);
      bell_ = bell_file_->bell();
    }
    efd_ = ::eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
    if (efd_ < 0) throw std::runtime_error("RingHub: eventfd failed");
    thread_ = std::thread([this] { run(); });
  }

  ~RingHub() { close(); }
  RingHub(const RingHub&) = delete;
  RingHub& operator=(const RingHub&) = delete;

  // add/remove/drain are called from the loop thread only
  void add_ring(int slot, std::shared_ptr<Ring> ring) {
    std::lock_guard<std::mutex> lock(mu_);
    for (auto& entry : rings_) {
      if (entry.first == slot) {
        entry.second = std::move(ring);
        return;
      }
    }
    if (!bell_) {
      bell_owner_ = ring;  // keeps the mapping alive while the thread waits on it
      bell_ = ring->bell();
    }
    rings_.emplace_back(slot, std::move(ring));
  }

  void remove_ring(int slot) {
    std::lock_guard<std::mutex> lock(mu_);
    for (size_t i = 0; i < rings_.size(); i++) {
      if (rings_[i].first == slot) {
        rings_.erase(rings_.begin() + (long)i);
        return;
      }
    }
  }

  int fd() const { return efd_; }

  // pop every frame of every ring: cb(slot, ptr, len). Returns frame count.
  template <typename F>
  size_t drain(F&& cb) {
    uint64_t counter;
    if (::read(efd_, &counter, sizeof(counter)) < 0) { /* not signalled */ }
    notified_.store(false, std::memory_order_seq_cst);
    size_t frames = 0;
    for (auto& entry : rings_) {
      int slot = entry.first;
      frames += entry.second->pop(
          [&](const uint8_t* ptr, size_t len) { cb(slot, ptr, len); });
    }
    drains_.fetch_add(1, std::memory_order_relaxed);
    return frames;
  }

  void close() {
    if (stop_.exchange(true)) return;
    Bell* bell;
    {
      std::lock_guard<std::mutex> lock(mu_);
      bell = bell_;
    }
    if (bell) {
      // kick the waiter out of its futex wait
      bell->seq.fetch_add(1, std::memory_order_seq_cst);
      ::syscall(SYS_futex, reinterpret_cast<uint32_t*>(&bell->seq), FUTEX_WAKE, INT_MAX,
                nullptr, nullptr, 0);
    }
    if (thread_.joinable()) thread_.join();
    {
      std::lock_guard<std::mutex> lock(mu_);
      rings_.clear();
    }
    if (efd_ >= 0) ::close(efd_);
    efd_ = -1;
  }

  uint64_t notifies() const { return notifies_.load(std::memory_order_relaxed); }
  uint64_t waits() const { return waits_.load(std::memory_order_relaxed); }
  uint64_t drains() const { return drains_.load(std::memory_order_relaxed); }
  // FUTEX_WAKE syscalls producers made on the bell this hub waits on
  uint64_t producer_wakes() {
    std::lock_guard<std::mutex> lock(mu_);
    return bell_ ? bell_->wakes.load(std::memory_order_relaxed) : 0;
  }
  size_t ring_count() {
    std::lock_guard<std::mutex> lock(mu_);
    return rings_.size();
  }

 private:
  void run() {
    // signals belong to the process's own threads, not to this one
    sigset_t all;
    sigfillset(&all);
    pthread_sigmask(SIG_BLOCK, &all, nullptr);
    while (!stop_.load(std::memory_order_acquire)) {
      Bell* bell;
      bool pending = false;
      uint32_t seen = 0;
      {
        std::lock_guard<std::mutex> lock(mu_);
        bell = bell_;
        if (bell) seen = bell->seq.load(std::memory_order_seq_cst);
        for (auto& entry : rings_) {
          if (entry.second->has_pending()) {
            pending = true;
            break;
          }
        }
      }
      if (!bell) {  // no ring yet
        struct timespec ts = {0, (long)timeout_ms_ * 1000000L};
        ::nanosleep(&ts, nullptr);
        continue;
      }
      if (pending && !notified_.exchange(true, std::memory_order_seq_cst)) {
        uint64_t one = 1;
        if (::write(efd_, &one, sizeof(one)) < 0) { /* counter saturated: still readable */ }
        notifies_.fetch_add(1, std::memory_order_relaxed);
      }
      // Publish the flag, then re-check the word: a producer that bumped it
      // before seeing the flag makes the kernel's compare fail, one that
      // bumps it later sees the flag and wakes us. The timeout bounds any
      // wake this reasoning misses, and shutdown.
      bell->waiting.store(1, std::memory_order_seq_cst);
      if (bell->seq.load(std::memory_order_seq_cst) == seen &&
          !stop_.load(std::memory_order_acquire)) {
        bell_wait(*bell, seen, timeout_ms_);
        waits_.fetch_add(1, std::memory_order_relaxed);
      }
      bell->waiting.store(0, std::memory_order_seq_cst);
    }
  }

  int timeout_ms_;
  int efd_ = -1;
  std::mutex mu_;
  std::vector<std::pair<int, std::shared_ptr<Ring>>> rings_;
  std::shared_ptr<BellFile> bell_file_;
  std::shared_ptr<Ring> bell_owner_;
  Bell* bell_ = nullptr;
  std::atomic<bool> stop_{false};
  std::atomic<bool> notified_{false};
  std::atomic<uint64_t> notifies_{0};
  std::atomic<uint64_t> waits_{0};
  std::atomic<uint64_t> drains_{0};
  std::thread thread_;
};

}  // namespace modal_amd

// Stand-alone stress of ring, hub and lane from two threads (no Python).
//
// The "scheduler" thread owns a ChunkLane and a RingHub over the workers'
// outbound rings; the "worker" thread owns a RingHub over the two inbound
// rings and answers every frame with a clean chunk_done. Rings are 64 KiB
// with 1-4 KiB frames, so they wrap many times. Checked: every chunk
// completes exactly once, frames arrive intact and in submit order per
// worker, and no worker ever holds more than its credit.
//
//   g++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined \
//       csrc/lane_stress.cpp -o lane_stress_asan && ./lane_stress_asan
//   g++ -std=c++20 -O1 -g -pthread -fsanitize=thread \
//       csrc/lane_stress.cpp -o lane_stress_tsan && ./lane_stress_tsan

#include <poll.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "lane.h"
#include "ring.h"

using namespace modal_amd;

namespace {

constexpr int kWorkers = 2;
constexpr int kChunks = 20000;
constexpr uint64_t kRingBytes = 64 * 1024;
constexpr uint64_t kCount = 64;      // items per chunk
constexpr uint64_t kCapItems = 128;  // two chunks of credit per worker
constexpr uint32_t kMinChunks = 2;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
      std::abort();                                                      \
    }                                                                    \
  } while (0)

void put_str(std::string& out, const std::string& s) {
  if (s.size() < 32) {
    out.push_back((char)(0xa0 | s.size()));
  } else {
    out.push_back((char)0xd9);
    out.push_back((char)s.size());
  }
  out += s;
}

// a clean chunk_done, as the worker runtime's msgpack encoder writes it
std::string encode_done(const std::string& token, uint64_t count, const std::string& data) {
  std::string out;
  out.push_back((char)0x88);
  put_str(out, "t");
  put_str(out, "chunk_done");
  put_str(out, "token");
  put_str(out, token);
  put_str(out, "call_id");
  put_str(out, "fc-stress");
  put_str(out, "chunk_id");
  put_str(out, token.substr(2));
  put_str(out, "function_id");
  put_str(out, "fu-stress");
  put_str(out, "count");
  out.push_back((char)count);
  put_str(out, "data");
  out.push_back((char)0xc5);
  out.push_back((char)(data.size() >> 8));
  out.push_back((char)(data.size() & 0xff));
  out += data;
  put_str(out, "cis");
  out.push_back((char)0xc0);
  return out;
}

// frame body: "<seq>:" then filler derived from seq, 1-4 KiB
std::string make_frame(int seq) {
  std::string head = std::to_string(seq) + ":";
  size_t len = 1024 + (size_t)((seq * 2654435761u) % 3072);
  std::string out = head;
  out.resize(len, (char)('a' + seq % 26));
  return out;
}

bool wait_fd(int fd, int timeout_ms) {
  struct pollfd pfd = {fd, POLLIN, 0};
  return ::poll(&pfd, 1, timeout_ms) > 0;
}

}  // namespace

int main() {
  char dir_template[] = "/tmp/lane-stress-XXXXXX";
  CHECK(::mkdtemp(dir_template) != nullptr);
  std::string dir = dir_template;

  std::vector<std::shared_ptr<Ring>> to_worker_tx, to_worker_rx, from_worker_tx, from_worker_rx;
  for (int i = 0; i < kWorkers; i++) {
    std::string in = dir + "/in." + std::to_string(i), outp = dir + "/out." + std::to_string(i);
    to_worker_tx.push_back(std::make_shared<Ring>(in, kRingBytes, true));
    to_worker_rx.push_back(std::make_shared<Ring>(in, 0, false));
    from_worker_tx.push_back(std::make_shared<Ring>(outp, kRingBytes, true));
    from_worker_rx.push_back(std::make_shared<Ring>(outp, 0, false));
  }

  std::atomic<bool> stop{false};
  std::atomic<int> answered{0};

  // ---- worker thread: consumes to_worker_rx, produces from_worker_tx ----
  std::thread worker([&] {
    RingHub hub(dir + "/worker.bell", 20);
    for (int i = 0; i < kWorkers; i++) hub.add_ring(i, to_worker_rx[i]);
    auto sched_bell = std::make_shared<BellFile>(dir + "/sched.bell", true);
    for (int i = 0; i < kWorkers; i++) from_worker_tx[i]->set_shared_bell(sched_bell);
    std::vector<int> last_seq(kWorkers, -1);
    std::vector<std::pair<int, std::string>> replies;
    while (!stop.load()) {
      wait_fd(hub.fd(), 50);
      replies.clear();
      hub.drain([&](int slot, const uint8_t* ptr, size_t len) {
        std::string body(reinterpret_cast<const char*>(ptr), len);
        int seq = std::atoi(body.c_str());
        CHECK(body == make_frame(seq));        // intact
        CHECK(seq > last_seq[slot]);           // submit order per worker
        last_seq[slot] = seq;
        replies.emplace_back(slot, encode_done("g:" + std::to_string(seq), kCount,
                                               std::string((size_t)(seq % 700), 'd')));
      });
      for (auto& reply : replies) {
        const auto* ptr = reinterpret_cast<const uint8_t*>(reply.second.data());
        while (!from_worker_tx[reply.first]->push(ptr, reply.second.size())) std::this_thread::yield();
        answered.fetch_add(1);
      }
    }
  });

  // ---- scheduler thread (this one): lane + hub over from_worker_rx ------
  {
    // the bell file may not exist yet when the hub creates it: both sides
    // open it with create=true, the mapping is the same file
    RingHub hub(dir + "/sched.bell", 20);
    ChunkLane lane;
    for (int i = 0; i < kWorkers; i++) {
      hub.add_ring(i, from_worker_rx[i]);
      auto bell = std::make_shared<BellFile>(dir + "/worker.bell", true);
      to_worker_tx[i]->set_shared_bell(bell);
      lane.add_worker(i, to_worker_tx[i]);
      lane.set_eligible(0, i, true);
    }
    lane.set_cap(0, kCapItems, kMinChunks);

    std::map<std::string, int> where;  // token -> worker, while in flight
    std::vector<uint64_t> held(kWorkers, 0);
    int completed = 0, submitted = 0, next_assigned = 0;
    auto assigned = [&](const std::string& token, int slot) {
      CHECK(std::atoi(token.c_str() + 2) == next_assigned);  // FIFO
      next_assigned++;
      CHECK(where.emplace(token, slot).second);
      held[slot] += kCount;
      CHECK(held[slot] <= kCapItems);  // credit never exceeded
    };
    std::vector<Assignment> assignments;
    while (completed < kChunks) {
      // keep a backlog of up to 8 queued frames ahead of the workers
      while (submitted < kChunks && lane.queued(0) < 8) {
        std::string frame = make_frame(submitted);
        std::string token = "g:" + std::to_string(submitted);
        int slot = lane.submit(0, token, kCount,
                               reinterpret_cast<const uint8_t*>(frame.data()), frame.size(), false);
        submitted++;
        if (slot >= 0) assigned(token, slot);
      }
      wait_fd(hub.fd(), 50);
      assignments.clear();
      // completions are applied before the refills they made room for
      std::vector<std::pair<int, std::string>> done_now;
      lane.drain(
          hub,
          [&](int slot, const ChunkDone& done) {
            CHECK(done.count == (int64_t)kCount && done.cis_nil);
            CHECK(done.data.size() == (size_t)(std::atoi(done.token.data() + 2) % 700));
            done_now.emplace_back(slot, std::string(done.token));
          },
          [&](int, const uint8_t*, size_t) { CHECK(false && "no raw frames expected"); },
          &assignments);
      for (auto& d : done_now) {
        auto it = where.find(d.second);
        CHECK(it != where.end() && it->second == d.first);  // exactly once, right worker
        where.erase(it);
        held[d.first] -= kCount;
        completed++;
      }
      for (auto& a : assignments) assigned(a.token, a.worker_slot);
    }
    CHECK(where.empty() && lane.queued(0) == 0);
    CHECK(lane.pushed() == (uint64_t)kChunks);
    std::printf("lane_stress ok: %d chunks, hub notifies=%llu waits=%llu producer_wakes=%llu\n",
                completed, (unsigned long long)hub.notifies(), (unsigned long long)hub.waits(),
                (unsigned long long)hub.producer_wakes());
    stop.store(true);
    worker.join();
  }
  CHECK(answered.load() == kChunks);
  std::string cmd = "rm -rf " + dir;
  return std::system(cmd.c_str()) == 0 ? 0 : 1;
}

// Chunk lane — native dispatch of map chunks (no Python types in here).
//
// In steady state the lane owns the per-chunk work of Function.map: picking
// a worker for a ready chunk, carrying its `inputs_chunk` frame to the
// worker's ring, receiving `chunk_done`, returning the credit and pushing
// the next queued chunk — all inside one drain() call on the loop thread.
// Python stays the authority for everything exceptional; it tells the lane
// which workers are eligible for which function and applies the
// assignments the lane reports to its own bookkeeping.

#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "ring.h"

namespace modal_amd {

// ---------------------------------------------------------------------------
// msgpack reader: just enough to recognise a chunk_done frame.

struct MsgReader {
  const uint8_t* p;
  const uint8_t* end;

  bool need(size_t n) const { return (size_t)(end - p) >= n; }

  bool be(size_t n, uint64_t* out) {
    if (!need(n)) return false;
    uint64_t v = 0;
    for (size_t i = 0; i < n; i++) v = (v << 8) | p[i];
    p += n;
    *out = v;
    return true;
  }

  bool read_str(std::string_view* out) {
    if (!need(1)) return false;
    uint8_t tag = *p++;
    uint64_t n;
    if ((tag & 0xe0) == 0xa0) n = tag & 0x1f;
    else if (tag == 0xd9) { if (!be(1, &n)) return false; }
    else if (tag == 0xda) { if (!be(2, &n)) return false; }
    else if (tag == 0xdb) { if (!be(4, &n)) return false; }
    else return false;
    if (!need(n)) return false;
    *out = std::string_view(reinterpret_cast<const char*>(p), (size_t)n);
    p += n;
    return true;
  }

  bool read_bin(std::string_view* out) {
    if (!need(1)) return false;
    uint8_t tag = *p++;
    uint64_t n;
    if (tag == 0xc4) { if (!be(1, &n)) return false; }
    else if (tag == 0xc5) { if (!be(2, &n)) return false; }
    else if (tag == 0xc6) { if (!be(4, &n)) return false; }
    else return false;
    if (!need(n)) return false;
    *out = std::string_view(reinterpret_cast<const char*>(p), (size_t)n);
    p += n;
    return true;
  }

  // any integer that fits int64
  bool read_int(int64_t* out) {
    if (!need(1)) return false;
    uint8_t tag = *p++;
    uint64_t v;
    if (tag <= 0x7f) { *out = tag; return true; }
    if (tag >= 0xe0) { *out = (int8_t)tag; return true; }
    switch (tag) {
      case 0xcc: if (!be(1, &v)) return false; *out = (int64_t)v; return true;
      case 0xcd: if (!be(2, &v)) return false; *out = (int64_t)v; return true;
      case 0xce: if (!be(4, &v)) return false; *out = (int64_t)v; return true;
      case 0xcf:
        if (!be(8, &v) || v > (uint64_t)INT64_MAX) return false;
        *out = (int64_t)v;
        return true;
      case 0xd0: if (!be(1, &v)) return false; *out = (int8_t)v; return true;
      case 0xd1: if (!be(2, &v)) return false; *out = (int16_t)v; return true;
      case 0xd2: if (!be(4, &v)) return false; *out = (int32_t)v; return true;
      case 0xd3: if (!be(8, &v)) return false; *out = (int64_t)v; return true;
      default: return false;
    }
  }

  bool read_map_header(uint64_t* n) {
    if (!need(1)) return false;
    uint8_t tag = *p++;
    if ((tag & 0xf0) == 0x80) { *n = tag & 0x0f; return true; }
    if (tag == 0xde) return be(2, n);
    if (tag == 0xdf) return be(4, n);
    return false;
  }

  bool read_array_header(uint64_t* n) {
    if (!need(1)) return false;
    uint8_t tag = *p++;
    if ((tag & 0xf0) == 0x90) { *n = tag & 0x0f; return true; }
    if (tag == 0xdc) return be(2, n);
    if (tag == 0xdd) return be(4, n);
    return false;
  }

  // step over one value of any type
  bool skip(int depth = 0) {
    if (depth > 32 || !need(1)) return false;
    uint8_t tag = *p++;
    uint64_t n;
    if (tag <= 0x7f || tag >= 0xe0) return true;
    if ((tag & 0xe0) == 0xa0) return adv(tag & 0x1f);
    if ((tag & 0xf0) == 0x90) return skip_n(tag & 0x0f, depth);
    if ((tag & 0xf0) == 0x80) return skip_n(2 * (uint64_t)(tag & 0x0f), depth);
    switch (tag) {
      case 0xc0: case 0xc2: case 0xc3: return true;
      case 0xc4: case 0xd9: return be(1, &n) && adv(n);
      case 0xc5: case 0xda: return be(2, &n) && adv(n);
      case 0xc6: case 0xdb: return be(4, &n) && adv(n);
      case 0xc7: return be(1, &n) && adv(n + 1);
      case 0xc8: return be(2, &n) && adv(n + 1);
      case 0xc9: return be(4, &n) && adv(n + 1);
      case 0xca: return adv(4);
      case 0xcb: return adv(8);
      case 0xcc: case 0xd0: return adv(1);
      case 0xcd: case 0xd1: return adv(2);
      case 0xce: case 0xd2: return adv(4);
      case 0xcf: case 0xd3: return adv(8);
      case 0xd4: return adv(2);
      case 0xd5: return adv(3);
      case 0xd6: return adv(5);
      case 0xd7: return adv(9);
      case 0xd8: return adv(17);
      case 0xdc: return be(2, &n) && skip_n(n, depth);
      case 0xdd: return be(4, &n) && skip_n(n, depth);
      case 0xde: return be(2, &n) && skip_n(2 * n, depth);
      case 0xdf: return be(4, &n) && skip_n(2 * n, depth);
      default: return false;  // 0xc1: never used
    }
  }

 private:
  bool adv(uint64_t n) {
    if (!need(n)) return false;
    p += n;
    return true;
  }
  bool skip_n(uint64_t n, int depth) {
    for (uint64_t i = 0; i < n; i++)
      if (!skip(depth + 1)) return false;
    return true;
  }
};

struct ChunkDone {
  std::string_view token, call_id, chunk_id, function_id, data;
  int64_t count = 0;
  bool cis_nil = true;
  std::vector<int64_t> cis;
};

enum class FrameKind {
  kOther,      // not a chunk_done, or not parseable: raw bytes for Python
  kDoneOther,  // a chunk_done that is not clean: credit returns, raw for Python
  kDoneClean,  // every field of `out` is set
};

inline bool ascii_only(std::string_view s) {
  for (unsigned char c : s)
    if (c >= 0x80) return false;
  return true;
}

// A chunk_done is clean when it has exactly the keys t, token, call_id,
// chunk_id, function_id, count, data, cis, each once, with data a bin and
// cis nil or an array of ints, and nothing follows the map. Strings must be
// ASCII, so the tuple equals what a UTF-8 decoding reader would produce.
// Never reads at or past buf + len. For kDoneOther only out->token is set.
inline FrameKind parse_chunk_done(const uint8_t* buf, size_t len, ChunkDone* out) {
  MsgReader r{buf, buf + len};
  uint64_t n_keys;
  if (!r.read_map_header(&n_keys)) return FrameKind::kOther;
  enum { T = 1, TOKEN = 2, CALL = 4, CHUNK = 8, FN = 16, COUNT = 32, DATA = 64, CIS = 128 };
  unsigned seen = 0;
  bool clean = n_keys == 8;
  bool is_done = false, has_token = false;
  std::string_view token;
  for (uint64_t i = 0; i < n_keys; i++) {
    std::string_view key;
    const uint8_t* key_at = r.p;
    if (!r.read_str(&key)) {
      // a non-string key: step over key and value
      r.p = key_at;
      if (!r.skip() || !r.skip()) return FrameKind::kOther;
      clean = false;
      continue;
    }
    unsigned bit = 0;
    if (key == "t") bit = T;
    else if (key == "token") bit = TOKEN;
    else if (key == "call_id") bit = CALL;
    else if (key == "chunk_id") bit = CHUNK;
    else if (key == "function_id") bit = FN;
    else if (key == "count") bit = COUNT;
    else if (key == "data") bit = DATA;
    else if (key == "cis") bit = CIS;
    if (bit == 0 || (seen & bit)) {
      // unknown or repeated key; a later "t"/"token" would win in a dict,
      // so a repeat makes the frame one Python has to read itself
      if (bit & (T | TOKEN)) return FrameKind::kOther;
      if (!r.skip()) return FrameKind::kOther;
      clean = false;
      continue;
    }
    seen |= bit;
    const uint8_t* value_at = r.p;
    bool ok = true;
    std::string_view sv;
    switch (bit) {
      case T:
        ok = r.read_str(&sv);
        if (ok) is_done = sv == "chunk_done";
        break;
      case TOKEN:
        ok = r.read_str(&sv) && ascii_only(sv);
        if (ok) { token = sv; has_token = true; }
        break;
      case CALL: ok = r.read_str(&out->call_id) && ascii_only(out->call_id); break;
      case CHUNK: ok = r.read_str(&out->chunk_id) && ascii_only(out->chunk_id); break;
      case FN: ok = r.read_str(&out->function_id) && ascii_only(out->function_id); break;
      case COUNT: ok = r.read_int(&out->count) && out->count >= 0; break;
      case DATA: ok = r.read_bin(&out->data); break;
      case CIS: {
        if (r.need(1) && *r.p == 0xc0) {
          r.p++;
          out->cis_nil = true;
          break;
        }
        uint64_t n;
        ok = r.read_array_header(&n) && n <= (uint64_t)(r.end - r.p);
        out->cis_nil = false;
        out->cis.clear();
        for (uint64_t k = 0; ok && k < n; k++) {
          int64_t v;
          ok = r.read_int(&v);
          if (ok) out->cis.push_back(v);
        }
        break;
      }
    }
    if (!ok) {
      // not the type a clean frame has there: step over it generically
      r.p = value_at;
      if (!r.skip()) return FrameKind::kOther;
      clean = false;
      if (bit == T) return FrameKind::kOther;
      if (bit == TOKEN) has_token = false;
    }
  }
  if (r.p != r.end) return FrameKind::kOther;  // trailing bytes
  if (!is_done || !has_token) return FrameKind::kOther;
  out->token = token;
  if (clean && seen == 255) return FrameKind::kDoneClean;
  return FrameKind::kDoneOther;
}

// ---------------------------------------------------------------------------

struct Assignment {
  std::string token;
  int worker_slot;
};

class ChunkLane {
 public:
  void add_worker(int slot, std::shared_ptr<Ring> ring) {
    Worker& w = workers_[slot];
    w.ring = std::move(ring);
  }

  // tokens in flight on that worker; the worker is gone from every function
  std::vector<std::string> remove_worker(int slot) {
    std::vector<std::string> tokens;
    auto it = workers_.find(slot);
    if (it == workers_.end()) return tokens;
    for (auto& entry : it->second.inflight) tokens.push_back(entry.first);
    workers_.erase(it);
    for (auto& fn : fns_) fn.second.eligible.erase(slot);
    return tokens;
  }

  void set_eligible(int fn_slot, int worker_slot, bool on) {
    Fn& fn = fns_[fn_slot];
    if (on && workers_.count(worker_slot)) fn.eligible.insert(worker_slot);
    else fn.eligible.erase(worker_slot);
  }

  void set_cap(int fn_slot, uint64_t items, uint32_t min_chunks) {
    Fn& fn = fns_[fn_slot];
    fn.cap_items = items;
    fn.min_chunks = min_chunks;
  }

  // Push the frame to the eligible worker with the least outstanding items
  // that still has credit and return its slot; otherwise queue it (FIFO per
  // function, `front` for requeues) and return -1.
  int submit(int fn_slot, const std::string& token, uint64_t count, const uint8_t* frame,
             size_t len, bool front) {
    Fn& fn = fns_[fn_slot];
    if (fn.queue.empty() || front) {
      int slot = place(fn_slot, fn, token, count, frame, len, fn.queue.size());
      if (slot >= 0) return slot;
    }
    Queued q{token, count, std::string(reinterpret_cast<const char*>(frame), len)};
    if (front) fn.queue.push_front(std::move(q));
    else fn.queue.push_back(std::move(q));
    return -1;
  }

  // dispatch whatever the function's queue and the workers' credit allow
  void kick(int fn_slot, std::vector<Assignment>* out) {
    auto it = fns_.find(fn_slot);
    if (it == fns_.end()) return;
    Fn& fn = it->second;
    while (!fn.queue.empty()) {
      Queued& q = fn.queue.front();
      int slot = place(fn_slot, fn, q.token, q.count,
                       reinterpret_cast<const uint8_t*>(q.frame.data()), q.frame.size(),
                       fn.queue.size());
      if (slot < 0) break;
      out->push_back(Assignment{std::move(q.token), slot});
      fn.queue.pop_front();
    }
  }

  // a chunk_done for `token` arrived from `worker_slot`: return the credit
  // and refill that function's queue. False when the token is not ours.
  bool complete(int worker_slot, std::string_view token, std::vector<Assignment>* out) {
    auto wit = workers_.find(worker_slot);
    if (wit == workers_.end()) return false;
    Worker& w = wit->second;
    auto it = w.inflight.find(std::string(token));
    if (it == w.inflight.end()) return false;
    int fn_slot = it->second.fn_slot;
    Load& load = w.load[fn_slot];
    load.items -= std::min(load.items, it->second.count);
    if (load.chunks) load.chunks--;
    w.inflight.erase(it);
    kick(fn_slot, out);
    return true;
  }

  // drop queued entries; returns the tokens that were dropped (chunks in
  // flight are not touched: their chunk_done still arrives)
  std::vector<std::string> cancel(const std::vector<std::string>& tokens) {
    std::unordered_set<std::string_view> drop(tokens.begin(), tokens.end());
    std::vector<std::string> dropped;
    for (auto& entry : fns_) {
      auto& q = entry.second.queue;
      auto keep = q.begin();
      for (auto it = q.begin(); it != q.end(); ++it) {
        if (drop.count(it->token)) {
          dropped.push_back(std::move(it->token));
        } else {
          if (keep != it) *keep = std::move(*it);
          ++keep;
        }
      }
      q.erase(keep, q.end());
    }
    return dropped;
  }

  // forget a function's queue (the function was deleted); returns its tokens
  std::vector<std::string> drop_queue(int fn_slot) {
    std::vector<std::string> tokens;
    auto it = fns_.find(fn_slot);
    if (it == fns_.end()) return tokens;
    for (auto& q : it->second.queue) tokens.push_back(std::move(q.token));
    it->second.queue.clear();
    return tokens;
  }

  // One call on the loop thread: pop every frame of every ring of the hub,
  // return credit for each chunk_done and refill before returning.
  //   on_clean(slot, const ChunkDone&)   a clean chunk_done
  //   on_raw(slot, ptr, len)             anything else, unparsed
  template <typename OnClean, typename OnRaw>
  void drain(RingHub& hub, OnClean&& on_clean, OnRaw&& on_raw, std::vector<Assignment>* out) {
    ChunkDone done;
    hub.drain([&](int slot, const uint8_t* ptr, size_t len) {
      FrameKind kind = parse_chunk_done(ptr, len, &done);
      if (kind != FrameKind::kOther) complete(slot, done.token, out);
      if (kind == FrameKind::kDoneClean) on_clean(slot, done);
      else on_raw(slot, ptr, len);
    });
  }

  size_t queued(int fn_slot) const {
    auto it = fns_.find(fn_slot);
    return it == fns_.end() ? 0 : it->second.queue.size();
  }

  size_t inflight(int worker_slot) const {
    auto it = workers_.find(worker_slot);
    return it == workers_.end() ? 0 : it->second.inflight.size();
  }

  uint64_t outstanding_items(int fn_slot, int worker_slot) const {
    auto it = workers_.find(worker_slot);
    if (it == workers_.end()) return 0;
    auto lit = it->second.load.find(fn_slot);
    return lit == it->second.load.end() ? 0 : lit->second.items;
  }

  uint64_t pushed() const { return pushed_; }

 private:
  struct Queued {
    std::string token;
    uint64_t count;
    std::string frame;
  };
  struct Load {
    uint64_t items = 0;
    uint32_t chunks = 0;
  };
  struct Inflight {
    int fn_slot;
    uint64_t count;
  };
  struct Worker {
    std::shared_ptr<Ring> ring;
    std::unordered_map<int, Load> load;
    std::unordered_map<std::string, Inflight> inflight;
  };
  struct Fn {
    uint64_t cap_items = 256;
    uint32_t min_chunks = 1;
    std::deque<Queued> queue;
    std::unordered_set<int> eligible;
  };

  // A worker may hold max(item cap, min_chunks chunks): it has credit while
  // it is under the item cap, or under min_chunks chunks. Chunks beyond the
  // item cap are prefetch, there to hide the completion round trip; they
  // are granted only while the backlog is deeper than the number of
  // eligible workers, so the last chunks of a map go to whichever worker
  // falls idle first instead of waiting behind a busy one.
  static bool has_credit(const Fn& fn, const Load& load, size_t backlog) {
    if (load.items < fn.cap_items) return true;
    return load.chunks < fn.min_chunks && backlog > fn.eligible.size();
  }

  int place(int fn_slot, Fn& fn, const std::string& token, uint64_t count,
            const uint8_t* frame, size_t len, size_t backlog) {
    // least outstanding items first, lowest slot on ties; a worker whose
    // ring is full right now is passed over
    std::vector<std::pair<uint64_t, int>> order;
    for (int slot : fn.eligible) {
      auto it = workers_.find(slot);
      if (it == workers_.end()) continue;
      const Load& load = it->second.load[fn_slot];
      if (has_credit(fn, load, backlog)) order.emplace_back(load.items, slot);
    }
    std::sort(order.begin(), order.end());
    for (auto& cand : order) {
      Worker& w = workers_[cand.second];
      if (w.ring->too_large(len) || !w.ring->push(frame, len)) continue;
      Load& load = w.load[fn_slot];
      load.items += count;
      load.chunks++;
      w.inflight[token] = Inflight{fn_slot, count};
      pushed_++;
      return cand.second;
    }
    return -1;
  }

  std::unordered_map<int, Worker> workers_;
  std::unordered_map<int, Fn> fns_;
  uint64_t pushed_ = 0;
};

}  // namespace modal_amd

// Stand-alone timing of the LZ4 pass of one 64 MiB window: the per-span
// entries (ma_lz4_compress, ma_lz4_compress_wave: one launch per span, back
// to back on one stream) against ma_lz4_compress_spans (csrc/lz4s.hip: one
// launch), as 8 spans of 8 MiB and as 2048 spans of 32 KiB, on three kinds of
// data made here from a seed: "distinct" (a different random 1 KiB unit tiled
// over every 8 MiB), zeros and random bytes. The lane parser is also timed
// with 64 and 16 parsing lanes per wavefront in place of the entry's 32. hipEvent times around each
// pass, the passes alternating, median (min - max) of 10 after 2 warm-ups;
// then every slot and comp_len of the new entry is compared with the per-span
// ones. The figures of profiles/README.md, "Span-table LZ4 encoder", come
// from it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature \
//       -Xclang -packed-fp32-ops scripts/lz4_spans_bench.hip -o lz4_spans_bench
//   lz4_spans_bench

#include "../modal_amd/ops/csrc/lz4.hip"
#include "../modal_amd/ops/csrc/lz4w.hip"
#include "../modal_amd/ops/csrc/lz4s.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (hipError_t)(x);                                            \
    if (e_ != hipSuccess) {                                                     \
      printf("%s at line %d\n", hipGetErrorString(e_), __LINE__);               \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

static const size_t TOTAL = 64u << 20;
static const long SEGS = TOTAL / SEG_SIZE;
static const int STRIDE = SEG_SIZE + 256;
static hipEvent_t e0, e1;

struct Times {
  std::vector<float> ms;
  void print(const char* name) {
    std::sort(ms.begin(), ms.end());
    const size_t h = ms.size() / 2;
    printf("    %-34s median %8.1f us (%8.1f - %8.1f)\n", name, 500 * (ms[h - 1] + ms[h]),
           1000 * ms.front(), 1000 * ms.back());
  }
};

template <typename Launch>
static void timed(Times& t, bool keep, Launch launch) {
  float ms;
  CK(hipEventRecord(e0, 0));
  launch();
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  CK(hipEventElapsedTime(&ms, e0, e1));
  if (keep) t.ms.push_back(ms);
}

template <typename T>
static T* dev_alloc(size_t n, const T* from = nullptr) {
  T* p;
  CK(hipMalloc(&p, n * sizeof(T)));
  if (from) CK(hipMemcpy(p, from, n * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint8_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint8_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 56);
}

int main() {
  std::vector<uint8_t> host(TOTAL);
  uint8_t* src = dev_alloc<uint8_t>(TOTAL);
  uint8_t* slots[2] = {dev_alloc<uint8_t>(SEGS * STRIDE), dev_alloc<uint8_t>(SEGS * STRIDE)};
  int32_t* lens[2] = {dev_alloc<int32_t>(SEGS), dev_alloc<int32_t>(SEGS)};
  std::vector<uint8_t> h_slots[2];
  std::vector<int32_t> h_lens[2];
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (const char* kind : {"distinct", "zeros", "random"}) {
    for (size_t i = 0; i < TOTAL; ++i) {
      if (kind[0] == 'z') host[i] = 0;
      else if (kind[0] == 'r' || i % (8u << 20) < 1024) host[i] = rnd();
      else host[i] = host[i - 1024];
    }
    CK(hipMemcpy(src, host.data(), TOTAL, hipMemcpyHostToDevice));
    for (int n : {8, 2048}) {
      const int64_t len = TOTAL / n;
      const int per = (int)(len / SEG_SIZE);
      std::vector<int64_t> offs(n), raw(n, len);
      std::vector<int32_t> first(n);
      for (int k = 0; k < n; ++k) offs[k] = k * len, first[k] = k * per;
      int64_t* d_off = dev_alloc(n, offs.data());
      int64_t* d_raw = dev_alloc(n, raw.data());
      int32_t* d_first = dev_alloc(n, first.data());
      printf("  %s, %d spans of %lld KiB\n", kind, n, (long long)(len >> 10));
      for (int parser = 0; parser < 2; ++parser) {
        for (int b = 0; b < 2; ++b) {
          CK(hipMemset(slots[b], 0, SEGS * STRIDE));
          CK(hipMemset(lens[b], 0xFF, SEGS * 4));
        }
        auto per_span = [&] {
          for (int k = 0; k < n; ++k)
            CK((parser ? ma_lz4_compress_wave : ma_lz4_compress)(
                src + offs[k], len, slots[0] + (size_t)first[k] * STRIDE, lens[0] + first[k],
                STRIDE, per, 0));
        };
        auto table = [&] {
          CK(ma_lz4_compress_spans(src, d_off, d_raw, d_first, n, SEGS, slots[1], STRIDE, lens[1],
                                   parser, 0));
        };
        Times t[4];
        for (int it = 0; it < 12; ++it) {
          timed(t[0], it >= 2, per_span);
          timed(t[1], it >= 2, table);
          if (parser) continue;
          timed(t[2], it >= 2, [&] {
            CK(lzs_launch_lane<64>(src, d_off, d_raw, d_first, n, SEGS, slots[1], STRIDE, lens[1], 0));
          });
          timed(t[3], it >= 2, [&] {
            CK(lzs_launch_lane<16>(src, d_off, d_raw, d_first, n, SEGS, slots[1], STRIDE, lens[1], 0));
          });
        }
        for (int b = 0; b < 2; ++b) {
          h_slots[b].resize(SEGS * STRIDE);
          h_lens[b].resize(SEGS);
          CK(hipMemcpy(h_slots[b].data(), slots[b], SEGS * STRIDE, hipMemcpyDeviceToHost));
          CK(hipMemcpy(h_lens[b].data(), lens[b], SEGS * 4, hipMemcpyDeviceToHost));
        }
        const bool same = h_slots[0] == h_slots[1] && h_lens[0] == h_lens[1];
        printf("   %s parser: slots and comp_lens %s\n", parser ? "wave" : "lane",
               same ? "equal" : "DIFFER");
        t[0].print("per-span launches");
        t[1].print("ma_lz4_compress_spans");
        if (!parser) t[2].print("  64 lanes a wavefront");
        if (!parser) t[3].print("  16 lanes a wavefront");
        if (!same) return 4;
      }
      for (void* p : {(void*)d_off, (void*)d_raw, (void*)d_first}) CK(hipFree(p));
    }
  }
  return 0;
}

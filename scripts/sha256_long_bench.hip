// Stand-alone timing of the wavefront SHA-256 (csrc/sha256w.hip) beside the
// lane kernel it relieves (sha256_many_kernel, csrc/sha256.hip) on the same
// bytes: one message of 4 KiB, 64 KiB, 1 MiB and 8 MiB - 1, then 256 messages
// of 4 MiB in one launch. hipEvent times around each launch, the kernels
// alternating, 10 launches each after a warm-up round, median (min..max), and
// every digest of the three kernels compared. The wavefront kernel is timed
// with its rounds on two lanes and on one. The figures of profiles/README.md,
// "Wavefront tail hash", come from it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature \
//       -Xclang -packed-fp32-ops scripts/sha256_long_bench.hip -o sha256_long_bench
//   sha256_long_bench

#include "../modal_amd/ops/csrc/sha256.hip"
#include "../modal_amd/ops/csrc/sha256w.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      printf("%s at line %d\n", hipGetErrorString(e_), __LINE__);               \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

// the round phase the library was not built with
extern "C" __global__ __launch_bounds__(SW_BATCH_BLOCKS) void sha256_long_other_kernel(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ lengths, uint8_t* __restrict__ out) {
  __shared__ uint32_t raw_lds[SW_RAW_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t wk_lds[SW_BATCH_BLOCKS * SW_WK_STRIDE];
  sw_message<3 - SHA256W_ROUND_LANES>(buf, offsets, lengths, out, raw_lds, wk_lds);
}

static hipEvent_t e0, e1;

struct Times {
  std::vector<float> ms;
  void print(const char* name) {
    std::sort(ms.begin(), ms.end());
    const size_t h = ms.size() / 2;
    printf("    %-34s median %10.1f us (%10.1f .. %10.1f)\n", name, 500 * (ms[h - 1] + ms[h]),
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

int main() {
  const int64_t MiB = 1 << 20;
  const size_t total = 1024 * MiB;
  std::vector<uint8_t> host(64 * MiB);
  uint32_t x = 1234;
  for (auto& b : host) b = static_cast<uint8_t>((x = x * 1664525u + 1013904223u) >> 24);
  uint8_t* src;
  CK(hipMalloc(&src, total));
  for (size_t at = 0; at < total; at += host.size()) {
    host[0] = static_cast<uint8_t>(at >> 26);  // no two 4 MiB messages equal
    host[4 * MiB] = static_cast<uint8_t>(at >> 26);
    CK(hipMemcpy(src + at, host.data(), host.size(), hipMemcpyHostToDevice));
  }
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("library rounds on %d lane(s)\n", SHA256W_ROUND_LANES);

  struct Case { int n; int64_t len; };
  const Case cases[] = {{1, 4096}, {1, 64 * 1024}, {1, MiB}, {1, 8 * MiB - 1}, {256, 4 * MiB}};
  for (const Case& c : cases) {
    std::vector<int64_t> offs(c.n), lens(c.n, c.len);
    for (int k = 0; k < c.n; ++k) offs[k] = k * c.len;
    int64_t *d_off, *d_len;
    uint8_t* d_out[3];
    CK(hipMalloc(&d_off, c.n * 8));
    CK(hipMalloc(&d_len, c.n * 8));
    CK(hipMemcpy(d_off, offs.data(), c.n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_len, lens.data(), c.n * 8, hipMemcpyHostToDevice));
    for (auto& o : d_out) CK(hipMalloc(&o, c.n * 32));
    Times t[3];
    for (int it = 0; it < 11; ++it) {
      timed(t[0], it >= 1, [&] { ma_sha256_many(src, d_off, d_len, d_out[0], c.n, 0); });
      timed(t[1], it >= 1, [&] { ma_sha256_long(src, d_off, d_len, d_out[1], c.n, 0); });
      timed(t[2], it >= 1, [&] {
        hipLaunchKernelGGL(sha256_long_other_kernel, dim3(c.n), dim3(SW_BATCH_BLOCKS), 0, 0,
                           (const uint8_t*)src, (const int64_t*)d_off, (const int64_t*)d_len, d_out[2]);
      });
    }
    std::vector<uint8_t> h[3];
    for (int k = 0; k < 3; ++k) {
      h[k].resize(c.n * 32);
      CK(hipMemcpy(h[k].data(), d_out[k], c.n * 32, hipMemcpyDeviceToHost));
      CK(hipFree(d_out[k]));
    }
    const bool same = h[0] == h[1] && h[0] == h[2];
    printf("  %d x %lld B: digests %s\n", c.n, (long long)c.len, same ? "equal" : "DIFFER");
    t[0].print("sha256_many_kernel (lane)");
    t[1].print(SHA256W_ROUND_LANES == 2 ? "sha256_long_kernel, 2 round lanes" : "sha256_long_kernel, 1 round lane");
    t[2].print(SHA256W_ROUND_LANES == 2 ? "sha256_long_kernel, 1 round lane" : "sha256_long_kernel, 2 round lanes");
    fflush(stdout);
    CK(hipFree(d_off));
    CK(hipFree(d_len));
    if (!same) return 4;
  }
  return 0;
}

// Stand-alone timing of the five instances of the histogram kernel
// (csrc/rankhist.hip) through their entries, on the same 64 MiB: ma_rank_hist
// at element size 1, 2 and 4 (the histogram and the rank pass behind it),
// ma_fpz_probe and ma_rank_probe. hipEvent times around each call, the
// entries alternating, median of 10 after 2 warm-ups, in 8 x 8 MiB and
// 64 x 1 MiB spans, then every table of the five compared with the three-way
// probe's. The figures of profiles/README.md, "One histogram kernel", come
// from it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature \
//       -Xclang -packed-fp32-ops scripts/probe_bench.hip -o probe_bench
//   probe_bench bf16.bin e4m3.bin
//
// Each input is 64 MiB of raw bytes, e.g. from torch:
//   x = torch.randn(64 << 20, generator=torch.Generator().manual_seed(1234))
//   x[: 32 << 20].to(torch.bfloat16).view(torch.uint8).numpy().tofile("bf16.bin")
//   x.to(torch.float8_e4m3fn).view(torch.uint8).numpy().tofile("e4m3.bin")

#include "../modal_amd/ops/csrc/rankhist.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      printf("%s at line %d\n", hipGetErrorString(e_), __LINE__);               \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

static const size_t TOTAL = 64u << 20;
static hipEvent_t e0, e1;

struct Times {
  std::vector<float> ms;
  void print(const char* name) {
    std::sort(ms.begin(), ms.end());
    const size_t h = ms.size() / 2;
    printf("    %-26s median %6.2f us (%6.2f - %6.2f)\n", name, 500 * (ms[h - 1] + ms[h]),
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

int main(int argc, char** argv) {
  std::vector<uint8_t> host(TOTAL);
  uint8_t* src = dev_alloc<uint8_t>(TOTAL);
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int f = 1; f < argc; ++f) {
    FILE* fp = fopen(argv[f], "rb");
    if (!fp || fread(host.data(), 1, TOTAL, fp) != TOTAL) return printf("cannot read %s\n", argv[f]), 1;
    fclose(fp);
    CK(hipMemcpy(src, host.data(), TOTAL, hipMemcpyHostToDevice));
    for (int n : {8, 64}) {
      const int64_t len = TOTAL / n;
      std::vector<int64_t> offs(n), lens(n, len);
      for (int k = 0; k < n; ++k) offs[k] = k * len;
      int64_t* d_off = dev_alloc(n, offs.data());
      int64_t* d_len = dev_alloc(n, lens.data());
      uint8_t* order = dev_alloc<uint8_t>(n * 256);
      uint8_t* rank_of = dev_alloc<uint8_t>(n * 256);
      // ma_rank_hist at es 1, 2 and 4, the two-way probe, the three-way probe
      const int es[3] = {1, 2, 4};
      const size_t rows[5] = {256, 256, 256, 512, 768};
      uint32_t* c[5];
      std::vector<uint32_t> h[5];
      for (int k = 0; k < 5; ++k) c[k] = dev_alloc<uint32_t>(n * rows[k]);
      Times t[5];
      for (int it = 0; it < 12; ++it) {
        for (int k = 0; k < 5; ++k) CK(hipMemset(c[k], 0, n * rows[k] * 4));
        CK(hipDeviceSynchronize());
        for (int k = 0; k < 3; ++k)
          timed(t[k], it >= 2, [&] {
            ma_rank_hist(src, d_off, d_len, es[k], c[k], order, rank_of, n, 0);
          });
        timed(t[3], it >= 2, [&] { ma_fpz_probe(src, d_off, d_len, c[3], n, 0); });
        timed(t[4], it >= 2, [&] { ma_rank_probe(src, d_off, d_len, c[4], n, 0); });
      }
      for (int k = 0; k < 5; ++k) {
        h[k].resize(n * rows[k]);
        CK(hipMemcpy(h[k].data(), c[k], n * rows[k] * 4, hipMemcpyDeviceToHost));
        CK(hipFree(c[k]));
      }
      bool same = true;
      for (int k = 0; k < n; ++k)
        for (int b = 0; b < 256; ++b) {
          const uint32_t* three = &h[4][k * 768 + b];
          same = same && h[0][k * 256 + b] == three[0] && h[1][k * 256 + b] == three[256] &&
                 h[2][k * 256 + b] == three[512] && h[3][k * 512 + b] == three[256] &&
                 h[3][k * 512 + 256 + b] == three[512];
        }
      printf("  %s, %d x %lld MiB: tables %s\n", argv[f], n, (long long)(len >> 20),
             same ? "equal" : "DIFFER");
      t[0].print("ma_rank_hist, es 1");
      t[1].print("ma_rank_hist, es 2");
      t[2].print("ma_rank_hist, es 4");
      t[3].print("ma_fpz_probe");
      t[4].print("ma_rank_probe");
      for (void* p : {(void*)d_off, (void*)d_len, (void*)order, (void*)rank_of}) CK(hipFree(p));
      if (!same) return 4;
    }
  }
  return 0;
}

// Stand-alone timing of the three-way probe (csrc/rankprobe.hip) beside the two
// kernels it stands for, fpz_probe_kernel and bytez_hist_kernel, on the same
// 64 MiB: hipEvent times around each launch, the kernels alternating, median
// of 10 after 2 warm-ups, in 8 x 8 MiB and 64 x 1 MiB spans, then every table
// of the probe compared with the other two kernels'. The figures of
// profiles/README.md, "Three-way probe", come from it.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature \
//       -Xclang -packed-fp32-ops [-DRP_COPIES=8] scripts/probe_bench.hip -o probe_bench
//   probe_bench bf16.bin e4m3.bin
//
// Each input is 64 MiB of raw bytes, e.g. from torch:
//   x = torch.randn(64 << 20, generator=torch.Generator().manual_seed(1234))
//   x[: 32 << 20].to(torch.bfloat16).view(torch.uint8).numpy().tofile("bf16.bin")
//   x.to(torch.float8_e4m3fn).view(torch.uint8).numpy().tofile("e4m3.bin")

#include "../modal_amd/ops/csrc/fpz.hip"
#include "../modal_amd/ops/csrc/bytez.hip"
#include "../modal_amd/ops/csrc/rankprobe.hip"

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
  printf("RP_COPIES %d\n", RP_COPIES);
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
      // the probe's tables on its own grid rule and on 64 groups, the two-way
      // probe's, the byte histogram's
      const size_t rows[4] = {768, 768, 512, 256};
      uint32_t* c[4];
      std::vector<uint32_t> h[4];
      for (int k = 0; k < 4; ++k) c[k] = dev_alloc<uint32_t>(n * rows[k]);
      Times t[4];
      for (int it = 0; it < 12; ++it) {
        for (int k = 0; k < 4; ++k) CK(hipMemset(c[k], 0, n * rows[k] * 4));
        CK(hipDeviceSynchronize());
        timed(t[0], it >= 2, [&] { ma_rank_probe(src, d_off, d_len, c[0], n, 0); });
        timed(t[2], it >= 2, [&] { ma_fpz_probe(src, d_off, d_len, c[2], n, 0); });
        timed(t[3], it >= 2, [&] {
          hipLaunchKernelGGL(bytez_hist_kernel, dim3(BZ_HIST_GROUPS, n), dim3(BZ_HIST_BLOCK), 0, 0,
                             (const uint8_t*)src, (const int64_t*)d_off, (const int64_t*)d_len, c[3], 0);
        });
        timed(t[1], it >= 2, [&] {
          hipLaunchKernelGGL(rank_probe_kernel, dim3(RP_MAX_GROUPS, n), dim3(RP_BLOCK), 0, 0,
                             (const uint8_t*)src, (const int64_t*)d_off, (const int64_t*)d_len, c[1], 0);
        });
      }
      for (int k = 0; k < 4; ++k) {
        h[k].resize(n * rows[k]);
        CK(hipMemcpy(h[k].data(), c[k], n * rows[k] * 4, hipMemcpyDeviceToHost));
        CK(hipFree(c[k]));
      }
      bool same = h[0] == h[1];
      for (int k = 0; k < n; ++k)
        for (int b = 0; b < 256; ++b)
          same = same && h[0][k * 768 + b] == h[3][k * 256 + b] &&
                 h[0][k * 768 + 256 + b] == h[2][k * 512 + b] &&
                 h[0][k * 768 + 512 + b] == h[2][k * 512 + 256 + b];
      printf("  %s, %d x %lld MiB: tables %s\n", argv[f], n, (long long)(len >> 20),
             same ? "equal" : "DIFFER");
      t[0].print("rank_probe_kernel");
      t[1].print("rank_probe_kernel, 64 groups");
      t[2].print("fpz_probe_kernel");
      t[3].print("bytez_hist_kernel");
      CK(hipFree(d_off));
      CK(hipFree(d_len));
      if (!same) return 4;
    }
  }
  return 0;
}

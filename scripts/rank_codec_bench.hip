// Stand-alone timing of the six segment entries of the rank codecs
// (csrc/fpz.hip, bytez.hip, ricez.hip) of the tree it is built in: encode and
// decode of MAFP10 and MARC10 on 64 MiB of bf16 (element size 2), of MAFB10
// and MARC10 on 64 MiB of float8_e4m3fn (element size 1), in 8 x 8 MiB spans.
// hipEvent times around each call, the two codecs of an input alternating,
// median (min - max) of 10 after 2 warm-ups. The decoders read the segments
// where the encoders put them, in the stride buffer, a declined segment
// copied raw into its slot; their output is compared with the source. The
// figures of profiles/README.md, "One segment frame", come from it, built
// once in this tree and once beside the csrc/ of the commit before.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xclang -target-feature \
//       -Xclang -packed-fp32-ops scripts/rank_codec_bench.hip -o rank_codec_bench
//   rank_codec_bench bf16.bin e4m3.bin
//
// Each input is 64 MiB of raw bytes, e.g. from torch:
//   x = torch.randn(64 << 20, generator=torch.Generator().manual_seed(1234))
//   x[: 32 << 20].to(torch.bfloat16).view(torch.uint8).numpy().tofile("bf16.bin")
//   x.to(torch.float8_e4m3fn).view(torch.uint8).numpy().tofile("e4m3.bin")

#include "../modal_amd/ops/csrc/rankhist.hip"
#include "../modal_amd/ops/csrc/fpz.hip"
#include "../modal_amd/ops/csrc/bytez.hip"
#include "../modal_amd/ops/csrc/ricez.hip"

#include <algorithm>
#include <climits>
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
static const int N_SPANS = 8, N_SEG = TOTAL / SEG_SIZE, STRIDE = SEG_SIZE + 256;
static hipEvent_t e0, e1;

struct Times {
  std::vector<float> ms;
  void print(const char* what, const char* codec) {
    std::sort(ms.begin(), ms.end());
    const size_t h = ms.size() / 2;
    printf("    %-7s %-6s median %7.2f us (%7.2f - %7.2f)\n", what, codec,
           500 * (ms[h - 1] + ms[h]), 1000 * ms.front(), 1000 * ms.back());
  }
};

template <typename Launch>
static void timed(Times& t, bool keep, Launch launch) {
  float ms;
  CK(hipEventRecord(e0, 0));
  CK(launch());
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
  if (argc != 3) return printf("usage: rank_codec_bench bf16.bin e4m3.bin\n"), 1;
  std::vector<uint8_t> host(TOTAL), back(TOTAL);
  uint8_t* src = dev_alloc<uint8_t>(TOTAL);
  uint8_t* dst = dev_alloc<uint8_t>(TOTAL);
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  // the block tables of the encoders and the segment tables of the decoders
  const int64_t span = TOTAL / N_SPANS;
  std::vector<int64_t> offs(N_SPANS), lens(N_SPANS, span), comp_offs(N_SEG), dst_offs(N_SEG);
  std::vector<int32_t> first(N_SPANS), seg_raw(N_SEG, SEG_SIZE), seg_blk(N_SEG);
  for (int k = 0; k < N_SPANS; ++k) offs[k] = k * span, first[k] = k * (int)(span / SEG_SIZE);
  for (int s = 0; s < N_SEG; ++s) {
    comp_offs[s] = (int64_t)s * STRIDE;
    dst_offs[s] = (int64_t)s * SEG_SIZE;
    seg_blk[s] = s / (int)(span / SEG_SIZE);
  }
  int64_t* d_off = dev_alloc(N_SPANS, offs.data());
  int64_t* d_len = dev_alloc(N_SPANS, lens.data());
  int32_t* d_first = dev_alloc(N_SPANS, first.data());
  int64_t* d_comp_offs = dev_alloc(N_SEG, comp_offs.data());
  int64_t* d_dst_offs = dev_alloc(N_SEG, dst_offs.data());
  int32_t* d_seg_raw = dev_alloc(N_SEG, seg_raw.data());
  int32_t* d_seg_blk = dev_alloc(N_SEG, seg_blk.data());
  uint32_t* counts = dev_alloc<uint32_t>(N_SPANS * 256);
  uint8_t* order = dev_alloc<uint8_t>(N_SPANS * 256);
  uint8_t* rank_of = dev_alloc<uint8_t>(N_SPANS * 256);
  uint8_t* d_es = dev_alloc<uint8_t>(N_SPANS);
  int32_t* status = dev_alloc<int32_t>(1);
  uint8_t* slots[2];
  int32_t* clens[2];
  for (int c = 0; c < 2; ++c) {
    slots[c] = dev_alloc<uint8_t>((size_t)N_SEG * STRIDE);
    clens[c] = dev_alloc<int32_t>(N_SEG);
  }

  bool all_same = true;
  for (int f = 1; f < argc; ++f) {
    const int es = f == 1 ? 2 : 1;
    const char* names[2] = {es == 2 ? "fpz" : "bytez", "ricez"};
    FILE* fp = fopen(argv[f], "rb");
    if (!fp || fread(host.data(), 1, TOTAL, fp) != TOTAL) return printf("cannot read %s\n", argv[f]), 1;
    fclose(fp);
    CK(hipMemcpy(src, host.data(), TOTAL, hipMemcpyHostToDevice));
    CK(hipMemset(counts, 0, N_SPANS * 256 * 4));
    CK(hipMemset(d_es, es, N_SPANS));
    CK(ma_rank_hist(src, d_off, d_len, es, counts, order, rank_of, N_SPANS, 0));
    auto encode = [&](int c) {
      if (c == 1)
        return ma_ricez_encode(src, d_off, d_len, d_first, rank_of, es, slots[c], STRIDE, clens[c],
                               N_SPANS, span / SEG_SIZE, 0);
      if (es == 2)
        return ma_fpz_encode(src, d_off, d_len, d_first, rank_of, es, slots[c], STRIDE, clens[c],
                             N_SPANS, span / SEG_SIZE, 0);
      return ma_bytez_encode(src, d_off, d_len, d_first, rank_of, slots[c], STRIDE, clens[c],
                             N_SPANS, span / SEG_SIZE, 0);
    };
    auto decode = [&](int c) {
      if (c == 1)
        return ma_ricez_decode(slots[c], d_comp_offs, d_dst_offs, clens[c], d_seg_raw, d_seg_blk,
                               order, d_es, dst, status, N_SEG, 0);
      if (es == 2)
        return ma_fpz_decode(slots[c], d_comp_offs, d_dst_offs, clens[c], d_seg_raw, d_seg_blk,
                             order, d_es, dst, status, N_SEG, 0);
      return ma_bytez_decode(slots[c], d_comp_offs, d_dst_offs, clens[c], d_seg_raw, d_seg_blk,
                             order, dst, status, N_SEG, 0);
    };

    Times enc[2], dec[2];
    for (int it = 0; it < 12; ++it)
      for (int c = 0; c < 2; ++c) timed(enc[c], it >= 2, [&] { return encode(c); });
    double kept[2];
    for (int c = 0; c < 2; ++c) {  // a declined segment goes raw into its slot
      std::vector<int32_t> h(N_SEG);
      CK(hipMemcpy(h.data(), clens[c], N_SEG * 4, hipMemcpyDeviceToHost));
      int64_t bytes = 0;
      for (int s = 0; s < N_SEG; ++s) {
        bytes += h[s] ? h[s] : SEG_SIZE;
        if (!h[s])
          CK(hipMemcpy(slots[c] + (size_t)s * STRIDE, src + (size_t)s * SEG_SIZE, SEG_SIZE,
                       hipMemcpyDeviceToDevice));
      }
      kept[c] = (double)bytes / TOTAL;
    }
    const int32_t clean = INT32_MAX;
    CK(hipMemcpy(status, &clean, 4, hipMemcpyHostToDevice));
    bool same[2];
    for (int it = 0; it < 12; ++it)
      for (int c = 0; c < 2; ++c) {
        if (it == 11) CK(hipMemset(dst, 0, TOTAL));  // the last launch is the one compared
        timed(dec[c], it >= 2, [&] { return decode(c); });
        if (it == 11) {
          CK(hipMemcpy(back.data(), dst, TOTAL, hipMemcpyDeviceToHost));
          same[c] = memcmp(back.data(), host.data(), TOTAL) == 0;
        }
      }
    int32_t st;
    CK(hipMemcpy(&st, status, 4, hipMemcpyDeviceToHost));
    printf("  %s, es %d, %d x %lld MiB: status %s\n", argv[f], es, N_SPANS, (long long)(span >> 20),
           st == INT32_MAX ? "clean" : "CORRUPT");
    for (int c = 0; c < 2; ++c) {
      printf("   %s: segments %.4f of raw, decoded %s\n", names[c], kept[c],
             same[c] ? "equal" : "DIFFERS");
      enc[c].print("encode", names[c]);
      dec[c].print("decode", names[c]);
      all_same = all_same && same[c];
    }
    all_same = all_same && st == INT32_MAX;
  }
  return all_same ? 0 : 4;
}

// Span-table LZ4 encoder for gfx950 (MI355X, CDNA4): every 4 KiB segment of
// every span of a window in ONE launch, with either parser.
//
// lz4.hip and lz4w.hip take one span a launch, so a 64 MiB snapshot window of
// 8 MiB blocks is eight launches of 2048 segments back to back on one stream,
// and a put_many of small buffers one launch of a few wavefronts per buffer.
// Here the grid runs over the window's stride slots: slot g is segment
// g - span_first_seg[k] of the span k that holds it, reads
// base + span_src_off[k] + 4096 s and writes slot g of stride_buf and
// comp_lens, the bytes the per-span entries write there (the parsers are
// theirs: lz4_lane.h, lz4_wave.h). The tables are container.span_tables(),
// what the assemble kernel takes. A slot that no span holds is left alone.
//
// Finding the span. span_first_seg ascends, so a slot's span is the last k
// with span_first_seg[k] <= g: a binary search. Spans end anywhere, so a
// workgroup straddles them freely; nothing is padded.
//   lane  the workgroup searches once for its first slot (a uniform search,
//         scalar loads), copies the SEGS + 1 table entries from there into
//         LDS, and every lane searches that window: its span is among them
//         unless spans in between are empty, and then the lane searches the
//         table itself. 300 spans or 30000, the LDS is the same SEGS + 1 words.
//   wave  one search per wavefront, uniform, on scalar loads. A workgroup is
//         one segment, so there is nothing to cache.
//
// Work split of the lane parser. Its time is a chain of dependent byte loads
// per lane, so what counts is how many SIMDs have a chain to follow. The
// per-span kernel has 128 lanes and 32 KiB of LDS per workgroup: 16
// workgroups a block, two wavefronts on each of 16 compute units out of 256.
// Here a workgroup is one wavefront in which SEGS = 32 lanes parse, with 8 KiB
// of tables (the 256 B per lane that the parser needs), so the 16384 segments
// of a window are 512 workgroups, two for every compute unit, and nineteen fit
// a compute unit (160 KiB of LDS) when a call has more. Half a wavefront of
// chains diverges less and asks for fewer cache lines per load than a whole
// one: a window of tiled units or zeros took 596 us with 32 lanes, 677 us
// with 64 and 596 us with 16; random bytes 527, 515 and 521 us. The per-span
// launches took 5795 us. A segment alone takes about 510 us, so the window's
// time is now the time of its slowest chain: what is left to gain is in the
// latency of the parser's loads (not tried: staging a wavefront's segments
// in LDS), no longer in how the work is split.
//
// Resources (hipcc -O3, -Rpass-analysis=kernel-resource-usage):
//   lz4_spans_lane_kernel<32>  82 SGPRs, 42 VGPRs, 8324 B LDS, no scratch,
//                              occupancy 5 wavefronts per SIMD
//   lz4_spans_wave_kernel      90 SGPRs, 78 VGPRs, 37984 B LDS, no scratch,
//                              occupancy 1 (lz4_compress_wave_kernel: 77, 70,
//                              the same LDS)
// Measurements and the variants that were tried are in profiles/README.md,
// "Span-table LZ4 encoder".
//
// Bounds. Table reads are at k in [0, n_spans). A slot is encoded only if
// 0 <= 4096 s < span_raw_len[k], so every source byte read is inside its
// span (the wave parser's dword loads each hold one of them). Slots are
// g < total_segs, which the caller's buffers hold.

#include "lz4_lane.h"
#include "lz4_wave.h"

#include <limits.h>

#define LZS_SEGS 32             // segments, and parsing lanes, per lane-parser workgroup
#define LZS_MAX_GRID (1 << 20)  // workgroups a launch; the kernels stride beyond

// The last k in [lo, hi) with first[k] <= g, or lo when there is none.
__device__ __forceinline__ int lzs_span_of(const int32_t* first, int lo, int hi, int g) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// Slot g in span k, whose first slot is first_k: its source bytes and their
// number, 0 when the span does not reach the slot.
__device__ __forceinline__ int lzs_segment(
    const uint8_t* __restrict__ base, const int64_t* __restrict__ span_src_off,
    const int64_t* __restrict__ span_raw_len, int k, int first_k, int64_t g,
    const uint8_t** sp) {
  const int64_t start = (g - first_k) * SEG_SIZE;
  const int64_t left = span_raw_len[k] - start;
  if (start < 0 || left <= 0) return 0;
  *sp = base + span_src_off[k] + start;
  return (int)(left < SEG_SIZE ? left : SEG_SIZE);
}

// SEGS: the lanes of the wavefront that parse, one slot each.
template <int SEGS>
__global__ __launch_bounds__(WAVE) void lz4_spans_lane_kernel(
    const uint8_t* __restrict__ base, const int64_t* __restrict__ span_src_off,
    const int64_t* __restrict__ span_raw_len, const int32_t* __restrict__ span_first_seg,
    int n_spans, int64_t total_segs, uint8_t* __restrict__ stride_buf, int out_stride,
    int32_t* __restrict__ comp_lens) {
  __shared__ uint16_t tables[SEGS][HASH_SIZE];
  __shared__ int32_t win[SEGS + 1];  // span_first_seg from the workgroup's first span on
  const int lane = threadIdx.x;
  for (int64_t g0 = (int64_t)blockIdx.x * SEGS; g0 < total_segs;
       g0 += (int64_t)gridDim.x * SEGS) {
    __syncthreads();  // the last round's readers of win are done
    const int k0 = lzs_span_of(span_first_seg, 0, n_spans, (int)g0);
    for (int i = lane; i <= SEGS; i += WAVE)
      win[i] = k0 + i < n_spans ? span_first_seg[k0 + i] : INT_MAX;
    __syncthreads();
    const int64_t g = g0 + lane;
    if (lane >= SEGS || g >= total_segs) continue;
    int k, first_k;
    if (win[SEGS] <= g) {  // more than SEGS spans begin in [g0, g]: some are empty
      k = lzs_span_of(span_first_seg, k0 + SEGS, n_spans, (int)g);
      first_k = span_first_seg[k];
    } else {
      const int i = lzs_span_of(win, 0, SEGS + 1, (int)g);
      k = k0 + i;
      first_k = win[i];
    }
    const uint8_t* sp;
    const int n = lzs_segment(base, span_src_off, span_raw_len, k, first_k, g, &sp);
    if (n == 0) continue;
    const int out = lz4_compress_segment(sp, n, stride_buf + g * out_stride, out_stride,
                                         tables[lane]);
    // only worth keeping if it actually shrank
    comp_lens[g] = (out > 0 && out < n) ? out : 0;
  }
}

extern "C" __global__ __launch_bounds__(WAVE) void lz4_spans_wave_kernel(
    const uint8_t* __restrict__ base, const int64_t* __restrict__ span_src_off,
    const int64_t* __restrict__ span_raw_len, const int32_t* __restrict__ span_first_seg,
    int n_spans, int64_t total_segs, uint8_t* __restrict__ stride_buf, int out_stride,
    int32_t* __restrict__ comp_lens) {
  const int lane = threadIdx.x;
  for (int64_t g = blockIdx.x; g < total_segs; g += gridDim.x) {
    const int k = lzs_span_of(span_first_seg, 0, n_spans, (int)g);  // uniform
    const uint8_t* sp;
    const int n = lzs_segment(base, span_src_off, span_raw_len, k, span_first_seg[k], g, &sp);
    if (n == 0) continue;  // uniform: every lane of the wavefront leaves
    lz4_wave_segment(sp, n, stride_buf + g * out_stride, comp_lens + g, out_stride, lane);
  }
}

template <int SEGS>
static inline int lzs_launch_lane(const void* base, const void* span_src_off,
                                  const void* span_raw_len, const void* span_first_seg,
                                  int n_spans, long total_segs, void* stride_buf, int out_stride,
                                  void* comp_lens, void* stream) {
  const long groups = (total_segs + SEGS - 1) / SEGS;
  hipLaunchKernelGGL(lz4_spans_lane_kernel<SEGS>,
                     dim3((unsigned)(groups < LZS_MAX_GRID ? groups : LZS_MAX_GRID)), dim3(WAVE),
                     0, (hipStream_t)stream, (const uint8_t*)base, (const int64_t*)span_src_off,
                     (const int64_t*)span_raw_len, (const int32_t*)span_first_seg, n_spans,
                     (int64_t)total_segs, (uint8_t*)stride_buf, out_stride, (int32_t*)comp_lens);
  return (int)hipGetLastError();
}

// parser: 0 lane, 1 wave. Slots are int32 in span_first_seg, so total_segs is.
extern "C" int ma_lz4_compress_spans(const void* base, const void* span_src_off,
                                     const void* span_raw_len, const void* span_first_seg,
                                     int n_spans, long total_segs, void* stride_buf,
                                     int out_stride, void* comp_lens, int parser, void* stream) {
  if ((parser != 0 && parser != 1) || total_segs > INT_MAX) return (int)hipErrorInvalidValue;
  if (n_spans <= 0 || total_segs <= 0) return 0;
  if (parser == 0)
    return lzs_launch_lane<LZS_SEGS>(base, span_src_off, span_raw_len, span_first_seg, n_spans,
                                     total_segs, stride_buf, out_stride, comp_lens, stream);
  hipLaunchKernelGGL(lz4_spans_wave_kernel,
                     dim3((unsigned)(total_segs < LZS_MAX_GRID ? total_segs : LZS_MAX_GRID)),
                     dim3(WAVE), 0, (hipStream_t)stream, (const uint8_t*)base,
                     (const int64_t*)span_src_off, (const int64_t*)span_raw_len,
                     (const int32_t*)span_first_seg, n_spans, (int64_t)total_segs,
                     (uint8_t*)stride_buf, out_stride, (int32_t*)comp_lens);
  return (int)hipGetLastError();
}

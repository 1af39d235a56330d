// Three-way element-size probe for the rank-plane codecs on gfx950 (MI355X,
// CDNA4): the histograms MAFB10 (es 1) and MAFP10 (es 2 and 4) rank by, of
// every span, in one pass over its bytes. ops/probe.py holds the numpy twin
// and the rule that picks the element size from the three tables.
//
// counts[b][0] is what bytez_hist_kernel gives for span b (every byte),
// counts[b][1] what fpz_hist_kernel gives at es = 2 (the byte at 2k+1 of every
// whole 2-byte element), counts[b][2] what it gives at es = 4 (the byte at
// 4k+3). A byte at span offset i is a top byte at es 2 when i is odd and at
// es 4 when i % 4 == 3, and "i < raw_len" is then the same as "the element is
// whole", so no table needs more than the span's own bounds.
//
// Tables. Every byte is counted once, into one of THREE LDS histograms by its
// offset: i even, i % 4 == 1, i % 4 == 3. The merge forms the outputs as
// sums: es 4 = the third, es 2 = second + third, es 1 = all three. A fourth
// table (i % 4 == 0 and 2 apart) would buy nothing the rule reads. That is 16
// LDS atomics per 16-byte chunk, what bytez_hist_kernel issues for its one
// table and twice fpz_probe_kernel's 8.
//
// Loads. As in fpz_probe_kernel: a lane reads aligned 16-byte chunks, from
// the chunk the span's first byte lives in, RP_UNROLL of them in flight, so
// every chunk loaded holds a byte of the span and every source byte is read
// once at any source alignment. Byte k of an aligned dword is at span offset
// i with i % 4 == (k - mis16) % 4, mis16 the span's misalignment, the same for
// the whole span: the four table pointers of a lane, one per byte of a dword,
// are worked out once and the full-chunk path is 16 extractions and 16
// atomics with no branch. Only the first and the last chunk of a span can
// hold bytes outside it; those two check 0 <= i < raw_len per byte.
//
// LDS layout. bins[table][bin][copy], copy = lane % RP_COPIES the minor index,
// so the bank is set by the lane and hardly by the data (bank = (bin % 2) * 16
// + lane % 16 at 16 copies: lanes l and l + 16 of an LDS lane group share a
// bank only when their bins have the same parity). That is what holds up under
// hot bins: fp8 Gaussians put a fifth of the bytes on four bins and e8m0
// scales nearly all of them on a handful, and with the bin as the minor index
// every copy of a hot bin would sit on one bank. What no layout removes is
// lanes with the same copy AND the same bin: at 16 copies four lanes of a
// wavefront share a copy, and on a one-valued span their atomics serialise
// four deep. Three tables of 16 copies are 48 KiB a workgroup, three
// workgroups a CU (160 KiB of LDS) against the five of fpz_probe_kernel's
// 32 KiB; 8 copies (24 KiB, six a CU) halve the zeroing and the merge but put
// eight lanes on a copy and four on a bank. Both were built and timed (below):
// 8 copies are slower wherever the counting sets the time, so 16 it is.
//
// Grid. Zeroing and merging 48 KiB is a fixed cost that a workgroup spreads
// over its source, and at 16 KiB of source it shows (28 us against 21 us,
// below), so a workgroup should have several times that. The grid is
// groups x spans with groups = RP_TARGET_WGS / spans, between RP_MIN_GROUPS
// and RP_MAX_GROUPS: the 8 x 8 MiB blocks of a snapshot window get 64 groups
// of 128 KiB each, 64 spans of 1 MiB get 16 groups of 64 KiB each (at 64
// groups they would have 16 KiB each and pay the tables four times as often).
// A workgroup that has no chunk returns before it zeroes anything.
//
// Merge. Thread t sums bin t's copies of the three tables, rotated by t to
// stay off one bank, and adds the three sums to the global tables, skipping a
// sum that is zero: an e8m0 span touches a handful of the 768 rows.
//
// Compiler (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; the same
// with packed fp32 off, as ops/build.py builds it, and on): 44 SGPRs,
// 40 VGPRs, scratch 0, LDS 49152 bytes, occupancy 3 waves a SIMD (the LDS
// sets it). At 8 copies: the same registers, LDS 24576, occupancy 6.
//
// Measured on an MI355X (hipEvent times, median of 10 launches after 2
// warm-ups, the kernels alternating on the same 64 MiB, spans at 0 mod 16;
// every table of the probe equal to the other two kernels'), N(0,1) as
// float8_e4m3fn / as bf16:
//                              8 x 8 MiB spans    64 x 1 MiB spans
//   fpz_probe_kernel           17.6 / 18.0 us     20.2 / 20.7 us
//   bytez_hist_kernel          18.6 / 19.3 us     18.9 / 20.1 us
//   this kernel                19.5 / 20.2 us     21.3 / 21.6 us
//   this kernel, 64 groups     19.4 / 20.2 us     28.1 / 29.2 us
//   8 copies                   22.2 / 25.3 us     21.4 / 25.1 us
//   8 copies, 64 groups        21.9 / 25.3 us     25.6 / 29.7 us
// One launch costs 0.54 of the two it stands for on e4m3 bytes (1.11 of
// fpz_probe_kernel alone, for twice the bytes counted). More in
// profiles/README.md, "Three-way probe".

#include "malz_common.h"

#ifndef RP_COPIES
#define RP_COPIES 16
#endif
#define RP_BLOCK 256
#define RP_UNROLL 4  // 16-byte loads a lane has in flight
#define RP_TABLE (256 * RP_COPIES)
#define RP_MIN_GROUPS 8
#define RP_MAX_GROUPS 64
#define RP_TARGET_WGS 1024

// at[k]: the lane's copy of bin 0 in the table that byte k of an aligned dword
// counts into.
struct RpTables {
  uint32_t* at[4];
};

// Every byte of chunk q of a span of n bytes.
__device__ __forceinline__ void rp_count(const uint4 v, int64_t q, int mis16, int64_t n,
                                         const RpTables t) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const int64_t i0 = 16 * q - mis16;  // span offset of the chunk's first byte
  if (i0 >= 0 && i0 + 16 <= n) {
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        atomicAdd(t.at[k] + ((w[d] >> (8 * k)) & 255u) * RP_COPIES, 1u);
  } else {  // the span's first or last chunk: count only its own bytes
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + 4 * d + k;
        if (i >= 0 && i < n) atomicAdd(t.at[k] + ((w[d] >> (8 * k)) & 255u) * RP_COPIES, 1u);
      }
  }
}

extern "C" __global__ __launch_bounds__(RP_BLOCK) void rank_probe_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, uint32_t* __restrict__ counts, int blk_base) {
  // [0]: bytes at even span offsets, [1]: at i % 4 == 1, [2]: at i % 4 == 3
  __shared__ __attribute__((aligned(16))) uint32_t bins[3 * RP_TABLE];
  const int b = blk_base + blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t n = blk_raw_len[b];
  if (n <= 0) return;
  const uint8_t* first = src + blk_src_off[b];
  const int mis16 = (int)(reinterpret_cast<uintptr_t>(first) & 15);
  const int64_t n_chunks = (mis16 + n + 15) >> 4;  // the last one holds byte n - 1
  if ((int64_t)blockIdx.x * RP_BLOCK >= n_chunks) return;  // nothing here: no merge either

  uint4* z = reinterpret_cast<uint4*>(bins);
  for (int k = tid; k < 3 * RP_TABLE / 4; k += RP_BLOCK) z[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  RpTables t;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = (k - mis16) & 3;  // the span offset of byte k, mod 4
    t.at[k] = bins + ((c & 1) ? (c + 1) >> 1 : 0) * RP_TABLE + (tid & (RP_COPIES - 1));
  }
  const uint4* chunks = reinterpret_cast<const uint4*>(first - mis16);
  const int64_t step = (int64_t)gridDim.x * RP_BLOCK;
  int64_t q = (int64_t)blockIdx.x * RP_BLOCK + tid;
  for (; q + (RP_UNROLL - 1) * step < n_chunks; q += RP_UNROLL * step) {
    uint4 v[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) v[u] = chunks[q + u * step];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) rp_count(v[u], q + u * step, mis16, n, t);
  }
  for (; q < n_chunks; q += step) rp_count(chunks[q], q, mis16, n, t);
  __syncthreads();

  uint32_t even = 0, at1 = 0, at3 = 0;
  for (int k = 0; k < RP_COPIES; ++k) {
    const int c = tid * RP_COPIES + ((k + tid) & (RP_COPIES - 1));
    even += bins[c];
    at1 += bins[RP_TABLE + c];
    at3 += bins[2 * RP_TABLE + c];
  }
  uint32_t* out = counts + (int64_t)b * 768;
  const uint32_t odd = at1 + at3;
  if (even + odd) atomicAdd(&out[tid], even + odd);
  if (odd) atomicAdd(&out[256 + tid], odd);
  if (at3) atomicAdd(&out[512 + tid], at3);
}

// counts (n_blocks x 3 x 256 u32) must come in zeroed: [b][0] the histogram of
// every byte of block b (es 1), [b][1] the es = 2 one, [b][2] the es = 4 one.
extern "C" int ma_rank_probe(const void* src, const void* blk_src_off, const void* blk_raw_len,
                             void* counts, int n_blocks, void* stream) {
  return launch_chunked(n_blocks, [&](int base, int ny) {
    int groups = RP_TARGET_WGS / ny;
    groups = groups < RP_MIN_GROUPS ? RP_MIN_GROUPS : groups > RP_MAX_GROUPS ? RP_MAX_GROUPS : groups;
    hipLaunchKernelGGL(rank_probe_kernel, dim3(groups, ny), dim3(RP_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const int64_t*)blk_raw_len,
                       (uint32_t*)counts, base);
  });
}

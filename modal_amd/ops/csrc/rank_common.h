// Shared by the rank codecs (fpz.hip, bytez.hip, ricez.hip) for gfx950: the
// frame around a segment's code. Their containers' header size, staging and
// the split of a segment among the lanes of its wavefront, wavefront sums and
// scans, an encoder's view of its block, the low-byte plane, a decoder's view
// of its segment and its copy from LDS to any destination, the host's grids.
//
// Encode and decode run one wavefront per workgroup, so __syncthreads() is a
// wave-level LDS fence and every branch around it is wave-uniform.

#pragma once

#include "malz_common.h"

#define RANK_HEADER_FIXED 276  // magic 6, raw_len 8, es 1, reserved 1, n_seg 4, order 256

// Staging of fpz.hip and ricez.hip (the comment at the top of fpz.hip; bytez.hip
// has no stride to read and stages at offset 0 with its own stage_at_zero):
// mis (<= 3) + 4096 bytes, rounded up to dwords, plus a pad dword per 16
#define IN_DWORDS (((SEG_SIZE + 3 + 3) / 4) * 17 / 16 + 2)

__device__ __forceinline__ int pad(int x) { return x + ((x >> 6) << 2); }

// len bytes at src -> LDS, padded; byte i of the segment is in[pad(mis + i)].
// Every dword loaded holds at least one of the segment's own bytes.
__device__ __forceinline__ int stage_in(const uint8_t* __restrict__ src, int len,
                                        uint32_t* in32, int lane) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src - mis);
  const int n_dw = (mis + len + 3) >> 2;
  for (int k = lane; k < n_dw; k += WAVE) in32[k + (k >> 4)] = s1[k];
  return mis;
}

// Row `row` of 256-byte tables (an encoder's rank_of, a decoder's order) -> LDS.
__device__ __forceinline__ void table_in(const uint8_t* __restrict__ tabs, int64_t row,
                                         uint32_t* tab32, int lane) {
  tab32[lane] = reinterpret_cast<const uint32_t*>(tabs + row * 256)[lane];
}

// Elements per lane: ceil(m/64) rounded up to a multiple of 8, so a lane's
// codes are whole bytes at every width. 32 for m = 2048, 16 for m = 1024.
__device__ __forceinline__ int lane_run(int m) { return (((m + 63) >> 6) + 7) & ~7; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

__device__ __forceinline__ int wave_excl_scan(int v, int lane) {
  int incl = v;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    int up = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += up;
  }
  return incl - v;
}

// len bytes of LDS -> dst at any alignment: byte lanes up to dst's 16-byte
// boundary, dwordx4 stores on the body, byte lanes on the tail.
__device__ __forceinline__ void lds_to_global(const uint8_t* from, uint8_t* __restrict__ dst, int len,
                              int lane) {
  int head = (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
  if (head > len) head = len;
  if (lane < head) dst[lane] = from[lane];
  from += head; dst += head; len -= head;
  const int n_vec = len >> 4;
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int k = lane; k < n_vec; k += WAVE) {
    uint4 v;
    __builtin_memcpy(&v, from + 16 * k, 16);
    d4[k] = v;
  }
  const int tail_start = n_vec << 4;
  if (lane < len - tail_start) dst[tail_start + lane] = from[tail_start + lane];
}

// --- encoder side: a grid of (segments, blocks) ---

struct RankBlock {
  const uint8_t* src;             // the block's first byte
  int64_t raw_len, n_seg, first;  // first: its row 0 in comp_lens and the stride buffer
};

// The block of this workgroup's grid row, and its rank table into rank32 if
// the workgroup has a segment (blockIdx.x < n_seg; the others return).
__device__ __forceinline__ RankBlock rank_block(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, const int32_t* __restrict__ blk_first_seg,
    const uint8_t* __restrict__ rank_tab, int blk_base, uint32_t* rank32, int lane) {
  const int bk = blk_base + blockIdx.y;
  const int64_t raw_len = blk_raw_len[bk], n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  if ((int64_t)blockIdx.x < n_seg) table_in(rank_tab, bk, rank32, lane);
  return {src + blk_src_off[bk], raw_len, n_seg, blk_first_seg[bk]};
}

// The segment does not code: the assemble kernel will store it raw.
__device__ __forceinline__ void decline(int32_t* clen, int lane) {
  if (lane == 0) *clen = 0;
}

// --- the low-byte plane: the es - 1 low bytes of each of a segment's m
// elements, lo = m * (es - 1) bytes at the head of its slot (es 2 or 4) ---

// Byte o of the plane is byte o % (es - 1) of element o / (es - 1): where in the raw segment.
__device__ __forceinline__ int low_byte_at(int o, int es) {
  const int i = es == 2 ? o : o / 3;
  return i * es + (o - i * (es - 1));
}

// Raw segment staged by stage_in -> the plane at out: four bytes per store
// when out is 4-aligned (it is for a Workspace: aligned base, stride a
// multiple of 256), a byte per store otherwise and on the tail.
__device__ __forceinline__ void low_bytes_out(const uint8_t* in, int mis, int es, int lo,
                                              uint8_t* __restrict__ out, int lane) {
  const int lo_vec = (reinterpret_cast<uintptr_t>(out) & 3) == 0 ? lo >> 2 : 0;
  for (int q = lane; q < lo_vec; q += WAVE) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= (uint32_t)in[pad(mis + low_byte_at(4 * q + k, es))] << (8 * k);
    reinterpret_cast<uint32_t*>(out)[q] = v;
  }
  for (int o = 4 * lo_vec + lane; o < lo; o += WAVE) out[o] = in[pad(mis + low_byte_at(o, es))];
}

// Coded segment staged by stage_in, the plane first -> the raw image outb.
__device__ __forceinline__ void low_bytes_in(const uint8_t* in, int mis, int es, int lo,
                                             uint8_t* outb, int lane) {
  for (int o = lane; o < lo; o += WAVE) outb[low_byte_at(o, es)] = in[pad(mis + o)];
}

// --- decoder side: one wavefront per segment of a run of containers ---

// *status comes in as INT32_MAX and leaves as the min of seg + 1 over the
// segments that are malformed (untouched: none): the FIRST one, whatever the
// order the wavefronts run in. A malformed segment writes nothing; no segment
// reads outside its seg_len bytes (rounded out to aligned dwords) or writes
// outside its raw bytes.
__device__ __forceinline__ void malformed(int32_t* status, int seg, int lane) {
  if (lane == 0) atomicMin(status, seg + 1);
}

struct RankSeg {
  const uint8_t* sp;  // its bytes in the payloads
  uint8_t* d;         // its raw bytes
  int L, slen;        // raw length, seg_len
  int blk, es;        // its container in the run, that one's element size
  int m, lo;          // elements, bytes of the low plane
};

// Segment seg of a run, from the host's tables. Stored raw (seg_len 0): copied
// here, false. Malformed: *status takes it, false. Else true, with lengths a
// decoder may index with: 0 < L <= SEG_SIZE is m whole elements of an admitted
// size (bit es of ES_MASK; blk_es null means es = 1) and lo + MIN_HI <= slen < L,
// MIN_HI the least the codec's part after the plane can be. Wave-uniform.
template <int ES_MASK, int MIN_HI>
__device__ __forceinline__ bool rank_seg(
    RankSeg& g, int seg, const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_offs,
    const int64_t* __restrict__ dst_offs, const int32_t* __restrict__ seg_lens,
    const int32_t* __restrict__ seg_raw, const int32_t* __restrict__ seg_blk,
    const uint8_t* __restrict__ blk_es, uint8_t* __restrict__ dst,
    int32_t* __restrict__ status, int lane) {
  g.sp = comp + comp_offs[seg];
  g.d = dst + dst_offs[seg];
  g.L = seg_raw[seg];
  g.slen = seg_lens[seg];
  g.blk = seg_blk[seg];
  g.es = blk_es ? blk_es[g.blk] : 1;
  const bool sized = g.L > 0 && g.L <= SEG_SIZE;
  const bool typed = g.es <= 4 && ((ES_MASK >> g.es) & 1);
  g.m = typed ? g.L / g.es : 0;
  g.lo = g.m * (g.es - 1);
  const bool coded = sized && typed && g.L % g.es == 0 && g.slen >= g.lo + MIN_HI && g.slen < g.L;
  if (sized && g.slen == 0) wave_copy(g.sp, g.d, g.L, lane);
  else if (!coded) malformed(status, seg, lane);
  return coded;
}

// --- host side: the entries' untyped pointers become the kernel's parameter
// types, and the grids of the encode and decode entries ---
template <typename... P, typename... A>
static inline void launch_as(void (*kernel)(P...), dim3 grid, int block, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, static_cast<P>(args)...);
}

// kernel(args..., first block of the grid's rows) over n_blocks blocks of at
// most max_segs segments (which bounds the grid): a wavefront per segment up
// to 16384 per block, which stride over the rest.
template <typename Kernel, typename... A>
static inline int launch_rank_encode(Kernel kernel, bool es_ok, int n_blocks, long max_segs,
                                     void* stream, A... args) {
  if (n_blocks <= 0 || max_segs <= 0) return 0;
  if (!es_ok) return (int)hipErrorInvalidValue;
  const int gx = (int)(max_segs < 16384 ? max_segs : 16384);
  return launch_chunked(n_blocks, [&](int base, int ny) {
    launch_as(kernel, dim3(gx, ny), WAVE, stream, args..., base);
  });
}

// kernel(args..., n_segments): a wavefront per segment up to 1 << 20.
template <typename Kernel, typename... A>
static inline int launch_rank_decode(Kernel kernel, int n_segments, void* stream, A... args) {
  if (n_segments <= 0) return 0;
  const int gx = n_segments < (1 << 20) ? n_segments : (1 << 20);
  launch_as(kernel, dim3(gx), WAVE, stream, args..., n_segments);
  return (int)hipGetLastError();
}

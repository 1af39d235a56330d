// MAFP10 float-plane codec on the device for gfx950 (MI355X, CDNA4).
//
// The container (layout and rules in ops/fpcodec.py, whose numpy codec is the
// model these kernels match byte for byte) codes the top byte of every
// element as its rank in a per-block frequency order, at a bit width chosen
// per 4 KiB segment, and leaves the low bytes alone.
//
//   probe     per block: the histograms at es 2 AND 4 in one pass over the
//             bytes, for callers that have to find the element size
//   hist      per block: LDS histogram of the top bytes, one global merge
//   rank      per block: 256 threads each find their byte's rank by counting
//   encode    one wavefront per segment -> its stride slot + comp_lens, the
//             same tables the MALZ41 plan kernel (malz.hip) then scans
//   assemble  header + order + seg_len table + segments, like malz_assemble
//   decode    one wavefront per segment of a run of containers
//
// Encode and decode run one wavefront per workgroup, so __syncthreads() is a
// wave-level LDS fence and every branch around it is wave-uniform.
//
// Staging. A lane owns a RUN of consecutive elements (32 of a full bf16
// segment), so that its codes are whole bytes and its escapes are contiguous.
// Read straight from global memory that would be 64 lanes 64 bytes apart per
// load; instead the segment is staged into LDS with coalesced aligned dword
// loads (any source alignment: the first dword is the one the segment's
// first byte lives in) and the lanes read their runs from LDS. Runs 16 dwords
// apart would all fall on two banks, so one pad dword follows every 16.
// The decoder builds the raw segment in a second LDS buffer and copies it out
// with aligned 16-byte stores. Its per-lane top-byte writes there are 64 bytes
// apart and do conflict; at 4 KiB per wavefront that is far below the cost of
// the global traffic and is left alone.

#include "malz_common.h"

#define FPZ_HEADER_FIXED 276  // magic 6, raw_len 8, es 1, reserved 1, n_seg 4, order 256
#define HIST_BLOCK 256
#define HIST_GROUPS 64
#define HIST_COPIES 8
// mis (<= 3) + 4096 bytes, rounded up to dwords, plus a pad dword per 16
#define IN_DWORDS (((SEG_SIZE + 3 + 3) / 4) * 17 / 16 + 2)

__device__ __forceinline__ int pad(int x) { return x + ((x >> 6) << 2); }

// Elements per lane: ceil(m/64) rounded up to a multiple of 8, so a lane's
// codes are whole bytes at every width. 32 for m = 2048, 16 for m = 1024.
__device__ __forceinline__ int lane_run(int m) { return (((m + 63) >> 6) + 7) & ~7; }

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

// ---------------------------------------------------------------------------
// histogram and rank
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(HIST_BLOCK) void fpz_hist_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, int es, uint32_t* __restrict__ counts,
    int blk_base) {
  // Gaussian data puts most elements on a handful of bins: eight copies
  // spread the lanes of a wavefront that hit the same bin
  __shared__ uint32_t bins[HIST_COPIES][256];
  const int b = blk_base + blockIdx.y;
  const int tid = threadIdx.x;
  for (int c = 0; c < HIST_COPIES; ++c) bins[c][tid] = 0;
  __syncthreads();
  const int64_t n_elem = blk_raw_len[b] / es;
  const uint8_t* top = src + blk_src_off[b] + (es - 1);
  for (int64_t e = (int64_t)blockIdx.x * HIST_BLOCK + tid; e < n_elem;
       e += (int64_t)gridDim.x * HIST_BLOCK)
    atomicAdd(&bins[tid & (HIST_COPIES - 1)][top[e * es]], 1u);
  __syncthreads();
  uint32_t total = 0;
  for (int c = 0; c < HIST_COPIES; ++c) total += bins[c][tid];
  if (total) atomicAdd(&counts[(int64_t)b * 256 + tid], total);
}

// order[r] = the byte of rank r, rank_of[byte] = its rank: count descending,
// byte value ascending on ties.
extern "C" __global__ __launch_bounds__(256) void fpz_rank_kernel(
    const uint32_t* __restrict__ counts, uint8_t* __restrict__ order,
    uint8_t* __restrict__ rank_of) {
  __shared__ uint32_t c[256];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t mine = counts[b * 256 + tid];
  c[tid] = mine;
  __syncthreads();
  int r = 0;
  for (int u = 0; u < 256; ++u) {
    const uint32_t cu = c[u];
    r += (cu > mine) || (cu == mine && u < tid);
  }
  order[b * 256 + r] = (uint8_t)tid;
  rank_of[b * 256 + tid] = (uint8_t)r;
}

// ---------------------------------------------------------------------------
// probe: both histograms of a block in one pass
// ---------------------------------------------------------------------------
//
// counts[b][0] is what fpz_hist_kernel gives at es = 2 (the byte at 2k+1 of
// every whole 2-byte element), counts[b][1] what it gives at es = 4 (the byte
// at 4k+3). A byte at span offset i is a top byte at es = 2 when i is odd and
// at es = 4 when i % 4 == 3, and "i < raw_len" is then the same as "the
// element is whole". So the kernel keeps two LDS histograms, one of the
// bytes at i % 4 == 1 and one of the bytes at i % 4 == 3, and the merge adds
// the second into both tables.
//
// Loads. A lane reads aligned 16-byte chunks, starting at the chunk the
// span's first byte lives in, so every chunk loaded holds a byte of the span
// and every source byte is read once at any source alignment. Within an
// aligned dword the two bytes wanted sit at (1 + mis) % 4 and (3 + mis) % 4,
// mis the span's misalignment: two shifts that are the same for the whole
// block. Only the first and the last chunk of a span can hold bytes outside
// it; those two take the path that checks 0 <= i < raw_len per byte.
//
// LDS layout. Gaussian floats put most elements on a few bins (two bins hold
// 57 % of N(0,1) bf16). fpz_hist_kernel's bins[copy][256] puts every copy of
// a bin on one bank (bank = bin % 32), so lanes of one wavefront that meet on
// a popular bin serialise whether or not they use different copies. Here the
// copy is the minor index, bins[bin][copy] with copy = lane % PROBE_COPIES,
// so the bank depends on the lane and hardly on the data. At 32 copies the
// bank is lane % 32 and the 32 lanes of an LDS lane group never meet, for
// 2 x 256 x 32 x 4 B = 64 KiB (two workgroups per CU). At 16 copies (32 KiB)
// lanes l and l + 16 of a group share a bank when their bins have the same
// parity, a two-way conflict at worst. The merge reads a bin's copies rotated
// by the thread index to stay off one bank.
//
// Measured on an MI355X (hipEvent times, median of 10 interleaved launches,
// 64 MiB of N(0,1) bf16, spans at 0 or 2 mod 16), fpz_hist_kernel at es = 2
// on the same bytes beside it:
//                     8 x 8 MiB spans   64 x 1 MiB spans
//   hist (es = 2)     67.8 us           44.6 us
//   probe, 32 copies  18.0 us           32.2 us
//   probe, 16 copies  17.8 us           20.6 us
// With 8 MiB spans the two layouts tie: the loads, not the LDS, set the time.
// With 1 MiB spans a workgroup has 16 KiB of source, and zeroing and merging
// 64 KiB of bins shows. So 16 copies. More in profiles/README.md,
// "Element-size probe".

#ifndef PROBE_COPIES
#define PROBE_COPIES 16
#endif
#define PROBE_BLOCK 256
#define PROBE_GROUPS 64

#define PROBE_UNROLL 4  // 16-byte loads a lane has in flight

// The two top-byte candidates of each dword of chunk q of a span of n bytes.
__device__ __forceinline__ void probe_count(const uint4 v, int64_t q, int mis16, int64_t n,
                                            uint32_t* mine1, uint32_t* mine3) {
  const int j1 = (1 + mis16) & 3, j3 = (3 + mis16) & 3;  // byte of a dword at i % 4 == 1, 3
  const int sh1 = 8 * j1, sh3 = 8 * j3;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const int64_t i0 = 16 * q - mis16;  // span offset of the chunk's first byte
  if (i0 >= 0 && i0 + 16 <= n) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      atomicAdd(mine1 + ((w[d] >> sh1) & 255u) * PROBE_COPIES, 1u);
      atomicAdd(mine3 + ((w[d] >> sh3) & 255u) * PROBE_COPIES, 1u);
    }
  } else {  // the span's first or last chunk: count only its own bytes
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int64_t i1 = i0 + 4 * d + j1, i3 = i0 + 4 * d + j3;
      if (i1 >= 0 && i1 < n) atomicAdd(mine1 + ((w[d] >> sh1) & 255u) * PROBE_COPIES, 1u);
      if (i3 >= 0 && i3 < n) atomicAdd(mine3 + ((w[d] >> sh3) & 255u) * PROBE_COPIES, 1u);
    }
  }
}

extern "C" __global__ __launch_bounds__(PROBE_BLOCK) void fpz_probe_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, uint32_t* __restrict__ counts, int blk_base) {
  __shared__ uint32_t bins[2][256 * PROBE_COPIES];
  const int b = blk_base + blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t n = blk_raw_len[b];
  if (n <= 0) return;
  const uint8_t* first = src + blk_src_off[b];
  const int mis16 = (int)(reinterpret_cast<uintptr_t>(first) & 15);
  const int64_t n_chunks = (mis16 + n + 15) >> 4;  // the last one holds byte n - 1
  if ((int64_t)blockIdx.x * PROBE_BLOCK >= n_chunks) return;  // nothing here: no merge either

  uint4* z = reinterpret_cast<uint4*>(&bins[0][0]);
  for (int k = tid; k < 2 * 256 * PROBE_COPIES / 4; k += PROBE_BLOCK) z[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  const uint4* chunks = reinterpret_cast<const uint4*>(first - mis16);
  uint32_t* mine1 = &bins[0][tid & (PROBE_COPIES - 1)];
  uint32_t* mine3 = &bins[1][tid & (PROBE_COPIES - 1)];
  const int64_t step = (int64_t)gridDim.x * PROBE_BLOCK;
  int64_t q = (int64_t)blockIdx.x * PROBE_BLOCK + tid;
  for (; q + (PROBE_UNROLL - 1) * step < n_chunks; q += PROBE_UNROLL * step) {
    uint4 v[PROBE_UNROLL];
#pragma unroll
    for (int u = 0; u < PROBE_UNROLL; ++u) v[u] = chunks[q + u * step];
#pragma unroll
    for (int u = 0; u < PROBE_UNROLL; ++u) probe_count(v[u], q + u * step, mis16, n, mine1, mine3);
  }
  for (; q < n_chunks; q += step) probe_count(chunks[q], q, mis16, n, mine1, mine3);
  __syncthreads();
  uint32_t t1 = 0, t3 = 0;
  for (int k = 0; k < PROBE_COPIES; ++k) {
    const int c = (k + tid) & (PROBE_COPIES - 1);
    t1 += bins[0][tid * PROBE_COPIES + c];
    t3 += bins[1][tid * PROBE_COPIES + c];
  }
  uint32_t* out = counts + (int64_t)b * 512;
  if (t1 + t3) atomicAdd(&out[tid], t1 + t3);
  if (t3) atomicAdd(&out[256 + tid], t3);
}

// ---------------------------------------------------------------------------
// encode: one wavefront per segment
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(WAVE) void fpz_encode_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, const int32_t* __restrict__ blk_first_seg,
    const uint8_t* __restrict__ rank_tab, int es,
    uint8_t* __restrict__ stride_buf, int out_stride,
    int32_t* __restrict__ comp_lens, int blk_base) {
  __shared__ uint32_t in32[IN_DWORDS];
  __shared__ uint32_t rank32[256 / 4];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  const uint8_t* rank = reinterpret_cast<const uint8_t*>(rank32);
  const int lane = threadIdx.x;
  const int bk = blk_base + blockIdx.y;
  const int64_t raw_len = blk_raw_len[bk];
  const int64_t n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  const int64_t first = blk_first_seg[bk];
  const uint8_t* blk_src = src + blk_src_off[bk];
  if ((int64_t)blockIdx.x >= n_seg) return;
  rank32[lane] = reinterpret_cast<const uint32_t*>(rank_tab + (int64_t)bk * 256)[lane];

  for (int64_t s = blockIdx.x; s < n_seg; s += gridDim.x) {
    __syncthreads();  // the last segment's readers are done; rank is visible
    const int L = seg_eff(0, raw_len, s);
    const int m = L / es;
    int32_t* clen = comp_lens + first + s;
    if (L % es != 0 || m < 3) {  // hi >= 2, so fewer than 3 elements never code
      if (lane == 0) *clen = 0;
      continue;
    }
    const int mis = stage_in(blk_src + s * SEG_SIZE, L, in32, lane);
    __syncthreads();

    const int per = lane_run(m);
    const int i0 = lane * per;
    const int i1 = min(i0 + per, m);
    const int top0 = mis + es - 1;
    // mine[b-1]: this lane's elements that width b would escape
    int mine[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = i0; i < i1; ++i) {
      const int r = rank[in[pad(top0 + i * es)]];
#pragma unroll
      for (int b = 1; b <= 7; ++b) mine[b - 1] += r >= (1 << b) - 1;
    }
    int b = 0, hi = m, my_esc = 0;  // a width must beat hi = m to be kept
#pragma unroll
    for (int w = 1; w <= 7; ++w) {
      const int cost = 1 + ((m * w + 7) >> 3) + wave_sum(mine[w - 1]);
      if (cost < hi) { hi = cost; b = w; my_esc = mine[w - 1]; }
    }
    if (b == 0) {
      if (lane == 0) *clen = 0;
      continue;
    }

    const int E = (1 << b) - 1;
    const int lo = m * (es - 1);
    const int nbytes = (m * b + 7) >> 3;
    uint8_t* out = stride_buf + (first + s) * out_stride;
    // low bytes of every element, four output bytes per store when the slot
    // allows (it does for a Workspace: aligned base, stride a multiple of 256)
    const int lo_vec = (reinterpret_cast<uintptr_t>(out) & 3) == 0 ? lo >> 2 : 0;
    for (int q = lane; q < lo_vec; q += WAVE) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int o = 4 * q + k;
        const int i = es == 2 ? o : o / 3;
        v |= (uint32_t)in[pad(mis + i * es + (o - i * (es - 1)))] << (8 * k);
      }
      reinterpret_cast<uint32_t*>(out)[q] = v;
    }
    for (int o = 4 * lo_vec + lane; o < lo; o += WAVE) {
      const int i = es == 2 ? o : o / 3;
      out[o] = in[pad(mis + i * es + (o - i * (es - 1)))];
    }
    if (lane == 0) out[lo] = (uint8_t)b;

    uint8_t* codes = out + lo + 1;
    uint8_t* escs = codes + nbytes + wave_excl_scan(my_esc, lane);
    for (int g = 0; g * 8 < per; ++g) {
      uint64_t v = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + g * 8 + j;
        if (i < m) {
          const uint8_t t = in[pad(top0 + i * es)];
          int r = rank[t];
          if (r >= E) { *escs++ = t; r = E; }
          v |= (uint64_t)r << (j * b);
        }
      }
      const int cb = ((i0 >> 3) + g) * b;  // this group's first code byte
      for (int k = 0; k < b; ++k)
        if (cb + k < nbytes) codes[cb + k] = (uint8_t)(v >> (8 * k));
    }
    if (lane == 0) *clen = lo + hi;
  }
}

// ---------------------------------------------------------------------------
// assemble
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(ASM_BLOCK) void fpz_assemble_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const uint8_t* __restrict__ stride_buf, int out_stride,
    const int32_t* __restrict__ comp_lens, const int64_t* __restrict__ seg_off,
    const int32_t* __restrict__ blk_first_seg, const int64_t* __restrict__ blk_raw_len,
    const uint8_t* __restrict__ order, int es,
    uint8_t* __restrict__ out, const int64_t* __restrict__ blk_out_off, int blk_base) {
  const int b = blk_base + blockIdx.y;
  const int64_t out_off = blk_out_off[b];
  if (out_off < 0) return;  // container not kept: nothing to assemble
  const int64_t raw_len = blk_raw_len[b];
  const int64_t n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  uint8_t* blk_out = out + out_off;

  if (blockIdx.x == 0 && threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    const uint64_t magic = 0x30315046414DULL;  // "MAFP10", little-endian
    put_le(blk_out, magic, 6, lane);
    put_le(blk_out + 6, (uint64_t)raw_len, 8, lane);
    put_le(blk_out + 14, (uint64_t)es, 2, lane);  // es, then the reserved 0
    put_le(blk_out + 16, (uint64_t)n_seg, 4, lane);
    wave_copy(order + (int64_t)b * 256, blk_out + 20, 256, lane);
  }
  assemble_segments(blk_out + FPZ_HEADER_FIXED, src + blk_src_off[b], stride_buf, out_stride,
                    comp_lens, seg_off, blk_first_seg[b], raw_len, n_seg);
}

// ---------------------------------------------------------------------------
// decode: one wavefront per segment of a run of containers
// ---------------------------------------------------------------------------

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

// The code bytes [cb, cb + b) of a lane's group of 8 elements as one word;
// bytes at or past nbytes (the stream's end) read as zero.
__device__ __forceinline__ uint64_t load_codes(const uint8_t* in, int at, int cb, int b,
                                               int nbytes) {
  uint64_t v = 0;
  for (int k = 0; k < b; ++k)
    if (cb + k < nbytes) v |= (uint64_t)in[pad(at + cb + k)] << (8 * k);
  return v;
}

// *status comes in as INT32_MAX and leaves as the min of seg + 1 over the
// segments that are malformed (untouched: none). A malformed segment writes
// nothing; no segment reads outside its seg_len bytes (rounded out to aligned
// dwords) or writes outside its raw bytes.
extern "C" __global__ __launch_bounds__(WAVE) void fpz_decode_kernel(
    const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_offs,
    const int64_t* __restrict__ dst_offs, const int32_t* __restrict__ seg_lens,
    const int32_t* __restrict__ seg_raw, const int32_t* __restrict__ seg_blk,
    const uint8_t* __restrict__ orders, const uint8_t* __restrict__ blk_es,
    uint8_t* __restrict__ dst, int32_t* __restrict__ status, int n_segments) {
  __shared__ uint32_t in32[IN_DWORDS];
  __shared__ uint32_t out32[SEG_SIZE / 4];
  __shared__ uint32_t order32[256 / 4];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  uint8_t* outb = reinterpret_cast<uint8_t*>(out32);
  const uint8_t* order = reinterpret_cast<const uint8_t*>(order32);
  const int lane = threadIdx.x;

  for (int seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
    __syncthreads();  // the last segment's LDS readers are done
    const uint8_t* sp = comp + comp_offs[seg];
    uint8_t* d = dst + dst_offs[seg];
    const int L = seg_raw[seg];
    const int slen = seg_lens[seg];
    bool ok = L > 0 && L <= SEG_SIZE;
    if (ok && slen == 0) {  // stored raw
      wave_copy(sp, d, L, lane);
      continue;
    }
    const int blk = seg_blk[seg];
    const int es = blk_es[blk];
    ok = ok && (es == 2 || es == 4);
    const int m = ok ? L / es : 0;
    const int lo = m * (es - 1);
    ok = ok && L % es == 0 && slen >= lo + 2 && slen < L;
    int mis = 0, b = 0, nbytes = 0;
    if (ok) {
      order32[lane] = reinterpret_cast<const uint32_t*>(orders + (int64_t)blk * 256)[lane];
      mis = stage_in(sp, slen, in32, lane);
    }
    __syncthreads();
    if (ok) {
      b = in[pad(mis + lo)];
      nbytes = (m * b + 7) >> 3;
      ok = b >= 1 && b <= 7 && lo + 1 + nbytes <= slen;
    }
    if (!ok) b = 0;
    const int per = lane_run(m);
    const int i0 = lane * per;
    const int E = (1 << b) - 1;
    const int at = mis + lo + 1;  // the code stream
    int my_esc = 0;
    if (ok) {
      for (int g = 0; g * 8 < per; ++g) {
        const uint64_t v = load_codes(in, at, ((i0 >> 3) + g) * b, b, nbytes);
        for (int j = 0; j < 8; ++j)
          my_esc += (i0 + g * 8 + j < m) && (int)((v >> (j * b)) & E) == E;
      }
      // the escapes must be exactly what is left of seg_len
      ok = wave_sum(my_esc) == slen - lo - 1 - nbytes;
    }
    if (!ok) {
      if (lane == 0) atomicMin(status, seg + 1);  // the FIRST malformed one
      continue;
    }
    int esc_at = at + nbytes + wave_excl_scan(my_esc, lane);
    for (int g = 0; g * 8 < per; ++g) {
      const uint64_t v = load_codes(in, at, ((i0 >> 3) + g) * b, b, nbytes);
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + g * 8 + j;
        if (i < m) {
          const int code = (int)((v >> (j * b)) & E);
          outb[i * es + es - 1] = code == E ? in[pad(esc_at++)] : order[code];
        }
      }
    }
    for (int o = lane; o < lo; o += WAVE) {
      const int i = es == 2 ? o : o / 3;
      outb[i * es + (o - i * (es - 1))] = in[pad(mis + o)];
    }
    __syncthreads();
    lds_to_global(outb, d, L, lane);
  }
}

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------

// The rank tables of histograms the caller already has (n_blocks x 256 u32,
// a probe's for instance): ma_fpz_rank without its histogram pass.
extern "C" int ma_fpz_rank_counts(const void* counts, void* order, void* rank_of, int n_blocks,
                                  void* stream) {
  if (n_blocks <= 0) return 0;
  hipLaunchKernelGGL(fpz_rank_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint32_t*)counts, (uint8_t*)order, (uint8_t*)rank_of);
  return (int)hipGetLastError();
}

// counts (n_blocks x 256 u32) must come in zeroed.
extern "C" int ma_fpz_rank(const void* src, const void* blk_src_off, const void* blk_raw_len,
                           int es, void* counts, void* order, void* rank_of, int n_blocks,
                           void* stream) {
  if (n_blocks <= 0) return 0;
  if (es != 2 && es != 4) return (int)hipErrorInvalidValue;
  const int rc = launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(fpz_hist_kernel, dim3(HIST_GROUPS, ny), dim3(HIST_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const int64_t*)blk_raw_len, es,
                       (uint32_t*)counts, base);
  });
  return rc ? rc : ma_fpz_rank_counts(counts, order, rank_of, n_blocks, stream);
}

// counts (n_blocks x 2 x 256 u32) must come in zeroed: [b][0] the es = 2
// histogram of block b, [b][1] the es = 4 one.
extern "C" int ma_fpz_probe(const void* src, const void* blk_src_off, const void* blk_raw_len,
                            void* counts, int n_blocks, void* stream) {
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(fpz_probe_kernel, dim3(PROBE_GROUPS, ny), dim3(PROBE_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const int64_t*)blk_raw_len,
                       (uint32_t*)counts, base);
  });
}

// max_segs: the largest segment count of any block (bounds the grid).
extern "C" int ma_fpz_encode(const void* src, const void* blk_src_off,
                             const void* blk_raw_len, const void* blk_first_seg,
                             const void* rank_of, int es, void* stride_buf, int out_stride,
                             void* comp_lens, int n_blocks, long max_segs, void* stream) {
  if (n_blocks <= 0 || max_segs <= 0) return 0;
  if (es != 2 && es != 4) return (int)hipErrorInvalidValue;
  const int gx = (int)(max_segs < 16384 ? max_segs : 16384);
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(fpz_encode_kernel, dim3(gx, ny), dim3(WAVE), 0, (hipStream_t)stream,
                       (const uint8_t*)src, (const int64_t*)blk_src_off,
                       (const int64_t*)blk_raw_len, (const int32_t*)blk_first_seg,
                       (const uint8_t*)rank_of, es, (uint8_t*)stride_buf, out_stride,
                       (int32_t*)comp_lens, base);
  });
}

extern "C" int ma_fpz_assemble(const void* src, const void* blk_src_off,
                               const void* stride_buf, int out_stride,
                               const void* comp_lens, const void* seg_off,
                               const void* blk_first_seg, const void* blk_raw_len,
                               const void* order, int es, void* out,
                               const void* blk_out_off, int n_blocks, void* stream) {
  if (es != 2 && es != 4) return (int)hipErrorInvalidValue;
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(fpz_assemble_kernel, dim3(ASM_GROUPS, ny), dim3(ASM_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const uint8_t*)stride_buf, out_stride,
                       (const int32_t*)comp_lens, (const int64_t*)seg_off,
                       (const int32_t*)blk_first_seg, (const int64_t*)blk_raw_len,
                       (const uint8_t*)order, es, (uint8_t*)out,
                       (const int64_t*)blk_out_off, base);
  });
}

extern "C" int ma_fpz_decode(const void* comp, const void* comp_offs, const void* dst_offs,
                             const void* seg_lens, const void* seg_raw, const void* seg_blk,
                             const void* orders, const void* blk_es, void* dst, void* status,
                             int n_segments, void* stream) {
  if (n_segments <= 0) return 0;
  const int gx = n_segments < (1 << 20) ? n_segments : (1 << 20);
  hipLaunchKernelGGL(fpz_decode_kernel, dim3(gx), dim3(WAVE), 0, (hipStream_t)stream,
                     (const uint8_t*)comp, (const int64_t*)comp_offs,
                     (const int64_t*)dst_offs, (const int32_t*)seg_lens,
                     (const int32_t*)seg_raw, (const int32_t*)seg_blk,
                     (const uint8_t*)orders, (const uint8_t*)blk_es, (uint8_t*)dst,
                     (int32_t*)status, n_segments);
  return (int)hipGetLastError();
}

// MAFP10 float-plane codec on the device for gfx950 (MI355X, CDNA4).
//
// The container (layout and rules in ops/fpcodec.py, whose numpy codec is the
// model these kernels match byte for byte) codes the top byte of every
// element as its rank in a per-block frequency order, at a bit width chosen
// per 4 KiB segment, and leaves the low bytes alone.
//
//   hist,     rankhist.hip (ma_rank_hist): the top bytes' histogram and rank
//   rank      tables of a block, for every rank-plane codec
//   encode   one wavefront per segment -> its stride slot + comp_lens, the
//             same tables the MALZ41 plan kernel (malz.hip) then scans
//   assemble  rank_assemble_kernel: header + order + seg_len table +
//             segments, like malz_assemble; the one assemble kernel of MAFP10
//             and MAFB10, which gives it its magic and es = 1
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
#include "rank_common.h"

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
// assemble: MAFP10 and MAFB10 containers (bytez.hip encodes the segments of
// the latter), which differ in the magic and in the value of es
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(ASM_BLOCK) void rank_assemble_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const uint8_t* __restrict__ stride_buf, int out_stride,
    const int32_t* __restrict__ comp_lens, const int64_t* __restrict__ seg_off,
    const int32_t* __restrict__ blk_first_seg, const int64_t* __restrict__ blk_raw_len,
    const uint8_t* __restrict__ order, uint64_t magic, int es,
    uint8_t* __restrict__ out, const int64_t* __restrict__ blk_out_off, int blk_base) {
  const int b = blk_base + blockIdx.y;
  const int64_t out_off = blk_out_off[b];
  if (out_off < 0) return;  // container not kept: nothing to assemble
  const int64_t raw_len = blk_raw_len[b];
  const int64_t n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  uint8_t* blk_out = out + out_off;

  if (blockIdx.x == 0 && threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    put_le(blk_out, magic, 6, lane);  // the six magic bytes, little-endian
    put_le(blk_out + 6, (uint64_t)raw_len, 8, lane);
    put_le(blk_out + 14, (uint64_t)es, 2, lane);  // es, then the reserved 0
    put_le(blk_out + 16, (uint64_t)n_seg, 4, lane);
    wave_copy(order + (int64_t)b * 256, blk_out + 20, 256, lane);
  }
  assemble_segments(blk_out + RANK_HEADER_FIXED, src + blk_src_off[b], stride_buf, out_stride,
                    comp_lens, seg_off, blk_first_seg[b], raw_len, n_seg);
}

// ---------------------------------------------------------------------------
// decode: one wavefront per segment of a run of containers
// ---------------------------------------------------------------------------

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

// magic: the container's six magic bytes as a little-endian integer.
extern "C" int ma_rank_assemble(const void* src, const void* blk_src_off,
                                const void* stride_buf, int out_stride,
                                const void* comp_lens, const void* seg_off,
                                const void* blk_first_seg, const void* blk_raw_len,
                                const void* order, unsigned long long magic, int es, void* out,
                                const void* blk_out_off, int n_blocks, void* stream) {
  if (es != 1 && es != 2 && es != 4) return (int)hipErrorInvalidValue;
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(rank_assemble_kernel, dim3(ASM_GROUPS, ny), dim3(ASM_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const uint8_t*)stride_buf, out_stride,
                       (const int32_t*)comp_lens, (const int64_t*)seg_off,
                       (const int32_t*)blk_first_seg, (const int64_t*)blk_raw_len,
                       (const uint8_t*)order, (uint64_t)magic, es, (uint8_t*)out,
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

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

#include "rank_common.h"

#define FPZ_ES_MASK (1 << 2 | 1 << 4)  // element sizes 2 and 4

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
  const RankBlock blk = rank_block(src, blk_src_off, blk_raw_len, blk_first_seg, rank_tab,
                                   blk_base, rank32, lane);
  if ((int64_t)blockIdx.x >= blk.n_seg) return;

  for (int64_t s = blockIdx.x; s < blk.n_seg; s += gridDim.x) {
    __syncthreads();  // the last segment's readers are done; rank is visible
    const int L = seg_eff(0, blk.raw_len, s);
    const int m = L / es;
    int32_t* clen = comp_lens + blk.first + s;
    // hi >= 2, so fewer than 3 elements never code
    if (L % es != 0 || m < 3) { decline(clen, lane); continue; }
    const int mis = stage_in(blk.src + s * SEG_SIZE, L, in32, lane);
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
    if (b == 0) { decline(clen, lane); continue; }

    const int E = (1 << b) - 1;
    const int lo = m * (es - 1);
    const int nbytes = (m * b + 7) >> 3;
    uint8_t* out = stride_buf + (blk.first + s) * out_stride;
    low_bytes_out(in, mis, es, lo, out, lane);
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
    RankSeg sg;
    if (!rank_seg<FPZ_ES_MASK, 2>(sg, seg, comp, comp_offs, dst_offs, seg_lens, seg_raw, seg_blk,
                                  blk_es, dst, status, lane))
      continue;
    const int es = sg.es, m = sg.m, lo = sg.lo, slen = sg.slen;
    table_in(orders, sg.blk, order32, lane);
    const int mis = stage_in(sg.sp, slen, in32, lane);
    __syncthreads();
    const int b = in[pad(mis + lo)];
    const int nbytes = (m * b + 7) >> 3;
    if (b < 1 || b > 7 || lo + 1 + nbytes > slen) { malformed(status, seg, lane); continue; }
    const int per = lane_run(m);
    const int i0 = lane * per;
    const int E = (1 << b) - 1;
    const int at = mis + lo + 1;  // the code stream
    int my_esc = 0;
    for (int g = 0; g * 8 < per; ++g) {
      const uint64_t v = load_codes(in, at, ((i0 >> 3) + g) * b, b, nbytes);
      for (int j = 0; j < 8; ++j)
        my_esc += (i0 + g * 8 + j < m) && (int)((v >> (j * b)) & E) == E;
    }
    // the escapes must be exactly what is left of seg_len
    if (wave_sum(my_esc) != slen - lo - 1 - nbytes) { malformed(status, seg, lane); continue; }
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
    low_bytes_in(in, mis, es, lo, outb, lane);
    __syncthreads();
    lds_to_global(outb, sg.d, sg.L, lane);
  }
}

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------

extern "C" int ma_fpz_encode(const void* src, const void* blk_src_off,
                             const void* blk_raw_len, const void* blk_first_seg,
                             const void* rank_of, int es, void* stride_buf, int out_stride,
                             void* comp_lens, int n_blocks, long max_segs, void* stream) {
  return launch_rank_encode(fpz_encode_kernel, es == 2 || es == 4, n_blocks, max_segs, stream,
                            src, blk_src_off, blk_raw_len, blk_first_seg, rank_of, es,
                            stride_buf, out_stride, comp_lens);
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
    launch_as(rank_assemble_kernel, dim3(ASM_GROUPS, ny), ASM_BLOCK, stream, src, blk_src_off,
              stride_buf, out_stride, comp_lens, seg_off, blk_first_seg, blk_raw_len, order,
              magic, es, out, blk_out_off, base);
  });
}

extern "C" int ma_fpz_decode(const void* comp, const void* comp_offs, const void* dst_offs,
                             const void* seg_lens, const void* seg_raw, const void* seg_blk,
                             const void* orders, const void* blk_es, void* dst, void* status,
                             int n_segments, void* stream) {
  return launch_rank_decode(fpz_decode_kernel, n_segments, stream, comp, comp_offs, dst_offs,
                            seg_lens, seg_raw, seg_blk, orders, blk_es, dst, status);
}

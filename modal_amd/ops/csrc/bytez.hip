// MAFB10 byte-plane codec on the device for gfx950 (MI355X, CDNA4).
//
// The container (layout and rules in ops/bytecodec.py, whose numpy codec is
// the model these kernels match byte for byte) is MAFP10's with 1-byte
// elements: EVERY byte of a block is coded as its rank in the block's
// frequency order, at a bit width chosen per 4 KiB segment, the rare ranks
// escaped. It is for fp8 tensors, fp8 KV caches and e8m0 scale tensors.
//
//   hist,     rankhist.hip (ma_rank_hist at es = 1): the histogram of all a
//   rank      block's bytes and its rank tables
//   encode   one wavefront per segment -> its stride slot + comp_lens
//   assemble  rank_assemble_kernel (fpz.hip), given this magic and es = 1
//   decode    one wavefront per segment of a run of containers
//
// Data path. fpz.hip reads strided top bytes out of a staged segment; here
// there is no stride, so a segment is staged into LDS AT OFFSET 0 (aligned
// dword loads, funnel-shifted by the source misalignment on the way in) and
// a lane's run of lane_run(m) consecutive bytes, 64 of a full segment, is
// whole dwords. The lane reads them once into registers, looks every byte's
// rank up in the 256-byte LDS table and keeps raw bytes and ranks in
// registers for both passes. Runs 16 dwords apart would fall on two banks, so
// one pad dword follows every 16 (dword k of the segment is in32[k + k/16]).
//
// Escapes of all seven widths come from one value per element: rank r escapes
// at width b exactly when floor(log2(r + 1)) >= b, so a lane counts
// 31 - clz(r + 1) into nine 7-bit bins of one 64-bit register and the suffix
// sums of the bins are its escapes at b = 7 .. 1.
//
// The code stream begins one byte into the segment (after the width byte),
// so a lane's codes, whole bytes at a dword-multiple offset, sit one byte off
// the slot's dwords. A lane therefore takes the last code byte of the lane
// before it (lane 0: the width byte) in front of its own and stores aligned
// dwords; the one byte left at the end is stored alone. Where the dword
// stores do not apply (a partial last run, an unaligned slot) the code groups
// pass through the staging buffer and go out a byte per lane.
//
// The decoder rebuilds a lane's 64 output bytes in registers and stores them
// straight to global memory with 16-byte stores when the destination allows,
// else through a linear LDS buffer and lds_to_global: dword writes, no
// strided LDS byte writes.
//
// Measured on an MI355X (hipEvent times, median of 10 interleaved launches,
// 64 MiB in 8 x 8 MiB spans: N(0,1) as float8_e4m3fn here, as bf16 for the
// MAFP10 kernels of fpz.hip at es = 2 beside it; containers 0.8855 and 0.7127
// of raw):
//                  bytez (64 Mi elements)   fpz es 2 (32 Mi elements)
//   hist + rank    29.5 us                  78.5 us
//   encode         101.0 us                 67.2 us
//   decode         87.8 us                  76.7 us
// Encoder and decoder are slower per source byte than MAFP10's (1.50x, 1.15x)
// and faster per element. LDS counters say it is not the LDS: fewer LDS
// instructions than the fpz kernels, a tenth of the decoder's bank conflicts,
// LDS busy under 2 % of the wave cycles; the per-element code extraction and
// the stores are what is left. More in profiles/README.md, "Byte-plane codec".

#include "rank_common.h"

#define BZ_RUN_DWORDS 16  // a lane's run is at most 64 bytes
// 4096 bytes, a pad dword per 16, and the two dwords an unaligned 8-byte read
// of the last code bytes may touch behind them
#define BZ_IN_DWORDS (SEG_SIZE / 4 + SEG_SIZE / 64 + 4)

__device__ __forceinline__ int padw(int k) { return k + (k >> 4); }  // dword k; byte i: pad(i)

// len bytes at src -> LDS so that byte i of the segment is byte pad(i):
// aligned dword loads, each lane's dword completed with the next lane's.
// Every dword loaded holds at least one of the segment's own bytes.
__device__ __forceinline__ void stage_at_zero(const uint8_t* __restrict__ src, int len,
                                              uint32_t* in32, int lane) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src - mis);
  const int n_src = (mis + len + 3) >> 2;
  const int n_out = (len + 3) >> 2;
  const int sh = 8 * mis;
  for (int base = 0; base < n_out; base += WAVE) {  // wave-uniform: the shuffle needs all lanes
    const int k = base + lane;
    const uint32_t w0 = k < n_src ? s1[k] : 0u;
    uint32_t w1 = __shfl_down(w0, 1, WAVE);
    if (lane == WAVE - 1) w1 = (mis && k + 1 < n_src) ? s1[k + 1] : 0u;
    if (k < n_out) in32[padw(k)] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
  }
}

// ---------------------------------------------------------------------------
// encode: one wavefront per segment
// ---------------------------------------------------------------------------

// Append nb (<= 4) bytes to a lane's pending output (acc holds nacc <= 3
// bytes) and store the dword that completes.
__device__ __forceinline__ void push_bytes(uint32_t x, int nb, uint64_t& acc, int& nacc,
                                           uint32_t*& o32) {
  acc |= (uint64_t)x << (8 * nacc);
  nacc += nb;
  if (nacc >= 4) {
    *o32++ = (uint32_t)acc;
    acc >>= 32;
    nacc -= 4;
  }
}

extern "C" __global__ __launch_bounds__(WAVE) void bytez_encode_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, const int32_t* __restrict__ blk_first_seg,
    const uint8_t* __restrict__ rank_tab, uint8_t* __restrict__ stride_buf, int out_stride,
    int32_t* __restrict__ comp_lens, int blk_base) {
  __shared__ __attribute__((aligned(16))) uint32_t in32[BZ_IN_DWORDS];
  __shared__ uint32_t rank32[256 / 4];
  const uint8_t* rank = reinterpret_cast<const uint8_t*>(rank32);
  const int lane = threadIdx.x;
  const RankBlock blk = rank_block(src, blk_src_off, blk_raw_len, blk_first_seg, rank_tab,
                                   blk_base, rank32, lane);
  if ((int64_t)blockIdx.x >= blk.n_seg) return;

  for (int64_t s = blockIdx.x; s < blk.n_seg; s += gridDim.x) {
    __syncthreads();  // the last segment's readers are done; rank is visible
    const int m = seg_eff(0, blk.raw_len, s);
    int32_t* clen = comp_lens + blk.first + s;
    // hi >= 2, so fewer than 3 elements never code
    if (m < 3) { decline(clen, lane); continue; }
    stage_at_zero(blk.src + s * SEG_SIZE, m, in32, lane);
    __syncthreads();

    const int per = lane_run(m);
    const int ndw = per >> 2, ngrp = per >> 3;
    const int i0 = lane * per;
    // The lane's bytes and their ranks, four to a register. No branch per
    // element: a run is read whole (the staging buffer covers 64 whole runs,
    // what lies past m is stale), every byte is looked up, and the ranks past
    // m are masked to 0. Rank 0 never escapes, codes as zero bits and counts
    // into bin 0, which no width reads.
    const int mine_n = min(max(m - i0, 0), per);  // the lane's elements
    uint32_t raw[BZ_RUN_DWORDS], rk[BZ_RUN_DWORDS];
    uint64_t bins = 0;  // nine 7-bit counts of floor(log2(rank + 1))
#pragma unroll
    for (int d = 0; d < BZ_RUN_DWORDS; ++d) {
      raw[d] = 0;
      rk[d] = 0;
      if (d < ndw) {  // wave-uniform
        const uint32_t w = in32[padw((i0 >> 2) + d)];
        const int inside = min(max(mine_n - 4 * d, 0), 4);
        uint32_t r4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) r4 |= (uint32_t)rank[(w >> (8 * k)) & 255u] << (8 * k);
        r4 &= (uint32_t)((1ull << (8 * inside)) - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          bins += 1ull << (7 * (31 - __clz((int)(((r4 >> (8 * k)) & 255u) + 1))));
        raw[d] = w;
        rk[d] = r4;
      }
    }
    // mine[b-1]: this lane's elements that width b would escape
    int mine[7];
    int suffix = (int)(bins >> 56) & 127;
#pragma unroll
    for (int w = 7; w >= 1; --w) {
      suffix += (int)(bins >> (7 * w)) & 127;
      mine[w - 1] = suffix;
    }
    // a segment has at most 4096 escapes: two widths share one wave_sum
    int total[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int both = wave_sum(mine[2 * p] | (p < 3 ? mine[2 * p + 1] << 16 : 0));
      total[2 * p] = both & 0xFFFF;
      total[2 * p + 1] = both >> 16;
    }
    int b = 0, hi = m, my_esc = 0;  // a width must beat hi = m to be kept
#pragma unroll
    for (int w = 1; w <= 7; ++w) {
      const int cost = 1 + ((m * w + 7) >> 3) + total[w - 1];
      if (cost < hi) { hi = cost; b = w; my_esc = mine[w - 1]; }
    }
    if (b == 0) { decline(clen, lane); continue; }

    const uint32_t E = (1u << b) - 1;
    const int nbytes = (m * b + 7) >> 3;
    uint8_t* out = stride_buf + (blk.first + s) * out_stride;
    uint8_t* escs = out + 1 + nbytes + wave_excl_scan(my_esc, lane);
    // v[g]: the b code bytes of the lane's g-th group of 8 elements
    uint64_t v[BZ_RUN_DWORDS / 2];
    uint32_t last = 0;  // the last code byte of the lane's run
#pragma unroll
    for (int g = 0; g < BZ_RUN_DWORDS / 2; ++g) {
      v[g] = 0;
      if (g < ngrp) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d = 2 * g + (j >> 2), sh = 8 * (j & 3);
          uint32_t r = (rk[d] >> sh) & 255u;
          if (r >= E) { *escs++ = (uint8_t)(raw[d] >> sh); r = E; }
          v[g] |= (uint64_t)r << (j * b);
        }
        if (g == ngrp - 1) last = (uint32_t)(v[g] >> (8 * (b - 1))) & 255u;
      }
    }
    // Lanes whose whole run is inside the segment store dwords: the slot's
    // dword at the lane's offset begins with the byte before its codes.
    const int lb = ngrp * b;  // code bytes per lane
    const int nfull = m / per;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 3) == 0 && (lb & 3) == 0;
    const uint32_t before = __shfl_up(last, 1, WAVE);
    if (vec && lane < nfull) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(out + lane * lb);
      uint64_t acc = lane == 0 ? (uint32_t)b : before;
      int nacc = 1;
#pragma unroll
      for (int g = 0; g < BZ_RUN_DWORDS / 2; ++g)
        if (g < ngrp) {
          push_bytes((uint32_t)v[g], b < 4 ? b : 4, acc, nacc, o32);
          if (b > 4) push_bytes((uint32_t)(v[g] >> 32), b - 4, acc, nacc, o32);
        }
      if (lane == nfull - 1) out[nfull * lb] = (uint8_t)last;
    }
    // What the dword stores leave (all of the stream without them, a partial
    // last run with them) goes out as bytes, a lane per byte: the groups pass
    // through the staging buffer, which every lane has read by now.
    if (!vec || m % per) {  // wave-uniform
      __syncthreads();
      uint64_t* groups = reinterpret_cast<uint64_t*>(in32);
#pragma unroll
      for (int g = 0; g < BZ_RUN_DWORDS / 2; ++g)
        if (g < ngrp) groups[lane * ngrp + g] = v[g];
      __syncthreads();
      for (int t = (vec ? nfull * lb : 0) + lane; t < nbytes; t += WAVE) {
        const int g = t / b;
        out[1 + t] = (uint8_t)(groups[g] >> (8 * (t - g * b)));
      }
      if (lane == 0 && (!vec || nfull == 0)) out[0] = (uint8_t)b;
    }
    if (lane == 0) *clen = hi;
  }
}

// ---------------------------------------------------------------------------
// decode: one wavefront per segment of a run of containers
// ---------------------------------------------------------------------------

// The 8 staged bytes from byte `at` on, as one word.
__device__ __forceinline__ uint64_t lds_bytes8(const uint32_t* in32, int at) {
  const int k = at >> 2, sh = 8 * (at & 3);
  const uint32_t d0 = in32[padw(k)], d1 = in32[padw(k + 1)], d2 = in32[padw(k + 2)];
  const uint32_t lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
  const uint32_t hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
  return ((uint64_t)hi << 32) | lo;
}

extern "C" __global__ __launch_bounds__(WAVE) void bytez_decode_kernel(
    const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_offs,
    const int64_t* __restrict__ dst_offs, const int32_t* __restrict__ seg_lens,
    const int32_t* __restrict__ seg_raw, const int32_t* __restrict__ seg_blk,
    const uint8_t* __restrict__ orders, uint8_t* __restrict__ dst,
    int32_t* __restrict__ status, int n_segments) {
  __shared__ uint32_t in32[BZ_IN_DWORDS];
  __shared__ uint32_t out32[SEG_SIZE / 4];
  __shared__ uint32_t order32[256 / 4];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  const uint8_t* order = reinterpret_cast<const uint8_t*>(order32);
  const int lane = threadIdx.x;

  for (int seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
    __syncthreads();  // the last segment's LDS readers are done
    RankSeg sg;  // es = 1: m = L, no low plane
    if (!rank_seg<1 << 1, 2>(sg, seg, comp, comp_offs, dst_offs, seg_lens, seg_raw, seg_blk,
                             nullptr, dst, status, lane))
      continue;
    const int m = sg.m, slen = sg.slen;
    table_in(orders, sg.blk, order32, lane);
    stage_at_zero(sg.sp, slen, in32, lane);
    __syncthreads();
    const int b = in[0];
    const int nbytes = (m * b + 7) >> 3;
    if (b < 1 || b > 7 || 1 + nbytes > slen) { malformed(status, seg, lane); continue; }
    const int per = lane_run(m);
    const int ndw = per >> 2, ngrp = per >> 3;
    const int i0 = lane * per;
    const uint32_t E = (1u << b) - 1;
    uint64_t v[BZ_RUN_DWORDS / 2];  // the lane's codes, 8 elements a word
    int my_esc = 0;
#pragma unroll
    for (int g = 0; g < BZ_RUN_DWORDS / 2; ++g) {
      v[g] = 0;
      if (g < ngrp && i0 + 8 * g < m) {
        v[g] = lds_bytes8(in32, 1 + ((i0 >> 3) + g) * b);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          my_esc += (i0 + 8 * g + j < m) && (uint32_t)((v[g] >> (j * b)) & E) == E;
      }
    }
    // the escapes must be exactly what is left of seg_len
    if (wave_sum(my_esc) != slen - 1 - nbytes) { malformed(status, seg, lane); continue; }
    int esc_at = 1 + nbytes + wave_excl_scan(my_esc, lane);
    uint32_t o[BZ_RUN_DWORDS];
#pragma unroll
    for (int q = 0; q < BZ_RUN_DWORDS; ++q) {
      o[q] = 0;
      if (q < ndw) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i0 + 4 * q + k < m) {
            const uint32_t code = (uint32_t)(v[q >> 1] >> ((4 * (q & 1) + k) * b)) & E;
            const uint32_t byte = code == E ? in[pad(esc_at++)] : order[code];
            o[q] |= byte << (8 * k);
          }
      }
    }
    // whole runs to a 16-byte aligned destination: straight from registers
    const bool direct = (reinterpret_cast<uintptr_t>(sg.d) & 15) == 0 && (per & 15) == 0 && m % per == 0;
    if (direct) {
      uint4* d4 = reinterpret_cast<uint4*>(sg.d + i0);
#pragma unroll
      for (int q = 0; q < BZ_RUN_DWORDS / 4; ++q)
        if (4 * q < ndw && i0 < m) d4[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < BZ_RUN_DWORDS; ++q)
        if (q < ndw && i0 + 4 * q < m) out32[(i0 >> 2) + q] = o[q];
      __syncthreads();
      lds_to_global(reinterpret_cast<const uint8_t*>(out32), sg.d, m, lane);
    }
  }
}

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------

extern "C" int ma_bytez_encode(const void* src, const void* blk_src_off,
                               const void* blk_raw_len, const void* blk_first_seg,
                               const void* rank_of, void* stride_buf, int out_stride,
                               void* comp_lens, int n_blocks, long max_segs, void* stream) {
  return launch_rank_encode(bytez_encode_kernel, true, n_blocks, max_segs, stream, src,
                            blk_src_off, blk_raw_len, blk_first_seg, rank_of, stride_buf,
                            out_stride, comp_lens);
}

extern "C" int ma_bytez_decode(const void* comp, const void* comp_offs, const void* dst_offs,
                               const void* seg_lens, const void* seg_raw, const void* seg_blk,
                               const void* orders, void* dst, void* status, int n_segments,
                               void* stream) {
  return launch_rank_decode(bytez_decode_kernel, n_segments, stream, comp, comp_offs, dst_offs,
                            seg_lens, seg_raw, seg_blk, orders, dst, status);
}

// MARC10 Rice-coded rank planes on the device for gfx950 (MI355X, CDNA4).
//
// The container (layout and rules in ops/ricecodec.py, whose numpy codec is
// the model these kernels match byte for byte) codes the top byte of every
// es-byte element, es 1, 2 or 4, as the Golomb-Rice code of its rank in the
// block's frequency order, with one parameter k per 4 KiB segment, and leaves
// the low bytes alone. Histogram, rank and assemble are MAFP10's and MAFB10's
// (fpz.hip, bytez.hip); this file has the two kernels a variable-length code
// needs of its own:
//
//   encode    one wavefront per segment -> its stride slot + comp_lens
//   decode    one wavefront per segment of a run of containers
//
// Both stage a segment as fpz.hip does (rank_common.h): a lane's run of a
// full segment is 64 bytes at every element size, which is what the pad dword
// per 16 is for.
//
// A variable-length code decodes serially, so a segment's m elements are cut
// into 16 sub-streams of per = ceil(m/16) elements, byte-aligned, with a
// table of their ends in front: 16 lanes can walk a segment at once.
//
// Encode. Four lanes share a sub-stream, each with a run of ceil(per/4)
// consecutive elements. Pass 1: a lane sums the code bits of its run at all
// eight k in registers; two shuffles give the bits of its sub-stream, which
// round up to bytes, and wave sums (two k to a register) give hi(k). Pass 2,
// at the k chosen: a scan over the four lanes gives a lane its bit offset in
// the sub-stream and a wave scan the sub-stream's first byte. The lane shifts
// its codes into a 64-bit accumulator and flushes whole dwords into a zeroed
// LDS image of the segment's hi part (k, the end table, the streams). The
// first dword it flushes and the partial one it ends with can hold bits of a
// neighbour, a lane of the same sub-stream or of the next, and go in with an
// LDS atomic OR; the dwords between are the lane's alone and are stored. The
// image is at most hi < m bytes, because a segment is only emitted then, and
// goes out with 16-byte stores.
//
// Decode. A lane walks one sub-stream through a 64-bit window that is
// refilled a dword at a time from the staged segment; the unary part of a
// code is a count of trailing ones of the window. Top bytes go into an LDS
// image of the raw segment, then all 64 lanes put the low bytes between them
// and copy the image out. That leaves 48 lanes idle in the walk; a variant
// that walked four segments per wavefront was measured, lost and removed
// (profiles/README.md, "Rice-coded rank planes").
//
// Measured on an MI355X (hipEvent times, median of 10 interleaved launches,
// 64 MiB of N(0,1) in 8 x 8 MiB spans, as bf16 beside fpz.hip and as
// float8_e4m3fn beside bytez.hip; containers 0.6781 and 0.8346 of raw for
// their 0.7127 and 0.8855):
//                       es 2: ricez    fpz       es 1: ricez    bytez
//   encode              95.2 us        65.2 us   144.6 us       99.2 us
//   decode              238.4 us       82.5 us   430.6 us       105.9 us
// The serial walk is the decoder's cost, 2.9x and 4.1x the fixed-width
// kernels. More in profiles/README.md, "Rice-coded rank planes".
//
// Bounds. Before any lane walks, the 16 lanes of a segment check k, that the
// end table does not decrease and that end[15] is exactly what seg_len
// leaves, so every sub-stream lies inside the staged bytes. A walk stops at
// the first code that ends past its sub-stream; a window refill therefore
// reads at most 8 bytes past it, and the dword index is clamped to the
// staging buffer besides. A rank is checked against 255 before it indexes
// the order table.

#include "rank_common.h"

#define RZ_SUBS 16
#define RZ_Q_ESC 12                    // a unary run this long announces a raw byte
#define RZ_HI_FIXED (1 + 2 * RZ_SUBS)  // k and the end table
#define RZ_HI_DWORDS (SEG_SIZE / 4 + 2)
#define RZ_ES_MASK (1 << 1 | 1 << 2 | 1 << 4)  // element sizes 1, 2 and 4
// the last dword a window refill may name, and a staging buffer that has it
#define RZ_MAX_DW ((SEG_SIZE + 3 + 3) / 4 + 8)
#define RZ_IN_DWORDS (IN_DWORDS + 16)

// ---------------------------------------------------------------------------
// encode: one wavefront per segment
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(WAVE) void ricez_encode_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, const int32_t* __restrict__ blk_first_seg,
    const uint8_t* __restrict__ rank_tab, int es,
    uint8_t* __restrict__ stride_buf, int out_stride,
    int32_t* __restrict__ comp_lens, int blk_base) {
  __shared__ uint32_t in32[IN_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t hi32[RZ_HI_DWORDS];
  __shared__ uint32_t rank32[256 / 4];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  uint8_t* hib = reinterpret_cast<uint8_t*>(hi32);
  const uint8_t* rank = reinterpret_cast<const uint8_t*>(rank32);
  const int lane = threadIdx.x;
  const int sub = lane >> 2, quarter = lane & 3;
  const RankBlock blk = rank_block(src, blk_src_off, blk_raw_len, blk_first_seg, rank_tab,
                                   blk_base, rank32, lane);
  if ((int64_t)blockIdx.x >= blk.n_seg) return;

  for (int64_t s = blockIdx.x; s < blk.n_seg; s += gridDim.x) {
    __syncthreads();  // the last segment's readers are done; rank is visible
    const int L = seg_eff(0, blk.raw_len, s);
    const int m = L / es;
    int32_t* clen = comp_lens + blk.first + s;
    // hi > 33, so no fewer elements ever code
    if (L % es != 0 || m <= RZ_HI_FIXED) { decline(clen, lane); continue; }
    const int mis = stage_in(blk.src + s * SEG_SIZE, L, in32, lane);
    __syncthreads();

    const int per = (m + RZ_SUBS - 1) / RZ_SUBS;
    const int run = (per + 3) >> 2;
    const int sub_end = min((sub + 1) * per, m);
    const int i0 = min(sub * per + quarter * run, sub_end);
    const int i1 = min(i0 + run, sub_end);
    const int top0 = mis + es - 1;

    // pass 1: bits[k] of the lane's run, then of its sub-stream, then hi(k)
    int bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = i0; i < i1; ++i) {
      const int r = rank[in[pad(top0 + i * es)]];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int q = r >> k;
        bits[k] += q < RZ_Q_ESC ? q + 1 + k : RZ_Q_ESC + 8;
      }
    }
    // a sub-stream has at most 256 * 20 bits and a segment 16 * 640 bytes:
    // two k share a register through the shuffles
    int sub_bytes[8], total[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      int v = bits[2 * p] | (bits[2 * p + 1] << 16);
      v += __shfl_xor(v, 1, WAVE);
      v += __shfl_xor(v, 2, WAVE);
      sub_bytes[2 * p] = ((v & 0xFFFF) + 7) >> 3;
      sub_bytes[2 * p + 1] = ((v >> 16) + 7) >> 3;
      const int both =
          wave_sum(quarter == 0 ? sub_bytes[2 * p] | (sub_bytes[2 * p + 1] << 16) : 0);
      total[2 * p] = both & 0xFFFF;
      total[2 * p + 1] = both >> 16;
    }
    int k = -1, hi = m, my_bits = 0, my_sub_bytes = 0;  // a k must beat hi = m to be kept
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int cost = RZ_HI_FIXED + total[w];
      if (cost < hi) { hi = cost; k = w; my_bits = bits[w]; my_sub_bytes = sub_bytes[w]; }
    }
    if (k < 0) { decline(clen, lane); continue; }

    // pass 2: where the lane's bits begin
    int off = 0;  // bits of the sub-stream's lanes before this one
    const int b1 = __shfl_up(my_bits, 1, WAVE), b2 = __shfl_up(my_bits, 2, WAVE);
    const int b3 = __shfl_up(my_bits, 3, WAVE);
    if (quarter >= 1) off += b1;
    if (quarter >= 2) off += b2;
    if (quarter >= 3) off += b3;
    const int before = wave_excl_scan(quarter == 0 ? my_sub_bytes : 0, lane);
    const int start = __shfl(before, lane & ~3, WAVE);  // the sub-stream's first byte

    const int n_hi_dw = (hi + 3) >> 2;  // hi < m <= 4096: inside hi32
    for (int q = lane; q < n_hi_dw; q += WAVE) hi32[q] = 0;
    __syncthreads();
    if (lane == 0) hib[0] = (uint8_t)k;
    if (quarter == 0) {
      const int e = start + my_sub_bytes;
      hib[1 + 2 * sub] = (uint8_t)e;
      hib[2 + 2 * sub] = (uint8_t)(e >> 8);
    }
    __syncthreads();

    if (i0 < i1) {
      const int P = 8 * (RZ_HI_FIXED + start) + off;  // the lane's first bit in the image
      uint32_t* at = hi32 + (P >> 5);
      uint64_t acc = 0;
      int nacc = P & 31;
      bool shared = true;  // the next dword flushed may hold a neighbour's bits
      const uint32_t low_mask = (1u << k) - 1;
      for (int i = i0; i < i1; ++i) {
        const uint32_t t = in[pad(top0 + i * es)];
        const uint32_t r = rank[t];
        const int q = (int)(r >> k);
        uint32_t code;
        int len;
        if (q < RZ_Q_ESC) {
          code = ((1u << q) - 1) | ((r & low_mask) << (q + 1));
          len = q + 1 + k;
        } else {
          code = ((1u << RZ_Q_ESC) - 1) | (t << RZ_Q_ESC);
          len = RZ_Q_ESC + 8;
        }
        acc |= (uint64_t)code << nacc;  // nacc < 32, len <= 20
        nacc += len;
        if (nacc >= 32) {
          if (shared) atomicOr(at, (uint32_t)acc); else *at = (uint32_t)acc;
          shared = false;
          ++at;
          acc >>= 32;
          nacc -= 32;
        }
      }
      if (nacc > 0) atomicOr(at, (uint32_t)acc);
    }
    __syncthreads();

    const int lo = m * (es - 1);
    uint8_t* out = stride_buf + (blk.first + s) * out_stride;
    low_bytes_out(in, mis, es, lo, out, lane);
    lds_to_global(hib, out + lo, hi, lane);
    if (lane == 0) *clen = lo + hi;
  }
}

// ---------------------------------------------------------------------------
// decode: one wavefront per segment of a run of containers
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(WAVE) void ricez_decode_kernel(
    const uint8_t* __restrict__ comp, const int64_t* __restrict__ comp_offs,
    const int64_t* __restrict__ dst_offs, const int32_t* __restrict__ seg_lens,
    const int32_t* __restrict__ seg_raw, const int32_t* __restrict__ seg_blk,
    const uint8_t* __restrict__ orders, const uint8_t* __restrict__ blk_es,
    uint8_t* __restrict__ dst, int32_t* __restrict__ status, int n_segments) {
  __shared__ uint32_t in32[RZ_IN_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t out32[SEG_SIZE / 4];
  __shared__ uint32_t order32[256 / 4];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  uint8_t* outb = reinterpret_cast<uint8_t*>(out32);
  const uint8_t* order = reinterpret_cast<const uint8_t*>(order32);
  const int lane = threadIdx.x;
  const int sub = lane;  // the sub-stream a lane walks, if it walks
  const bool walks = sub < RZ_SUBS;

  for (int64_t s = blockIdx.x; s < n_segments; s += gridDim.x) {
    __syncthreads();  // the last segment's LDS readers are done
    const int seg = (int)s;
    RankSeg g;
    if (!rank_seg<RZ_ES_MASK, RZ_HI_FIXED>(g, seg, comp, comp_offs, dst_offs, seg_lens, seg_raw,
                                           seg_blk, blk_es, dst, status, lane))
      continue;
    table_in(orders, g.blk, order32, lane);
    const int mis = stage_in(g.sp, g.slen, in32, lane);
    __syncthreads();

    // the 16 walking lanes check k and the end table together: only a sound
    // table keeps every sub-stream inside the staged bytes
    const int hi_at = mis + g.lo;
    bool bad = false;
    int k = 0, e0 = 0, e1 = 0;
    if (walks) {
      k = in[pad(hi_at)];
      e1 = in[pad(hi_at + 1 + 2 * sub)] | (in[pad(hi_at + 2 + 2 * sub)] << 8);
      if (sub) e0 = in[pad(hi_at - 1 + 2 * sub)] | (in[pad(hi_at + 2 * sub)] << 8);
      bad = k > 7 || e0 > e1 || (sub == RZ_SUBS - 1 && g.lo + RZ_HI_FIXED + e1 != g.slen);
    }
    const bool sound = __ballot(walks && bad) == 0;

    if (walks && sound) {
      const int per = (g.m + RZ_SUBS - 1) / RZ_SUBS;
      const int count = min(max(g.m - sub * per, 0), per);
      const int S = hi_at + RZ_HI_FIXED + e0;  // the sub-stream's first staged byte
      const int n_bits = 8 * (e1 - e0);
      const uint32_t low_mask = (1u << k) - 1;
      int dw = S >> 2;
      const int sh = 8 * (S & 3);
      uint64_t w = (uint64_t)in32[dw + (dw >> 4)] >> sh;  // `have` bits, zeros above them
      int have = 32 - sh, pos = 0;
      int o = sub * per * g.es + g.es - 1;
      for (int j = 0; j < count; ++j) {
        if (have < 32) {
          dw = min(dw + 1, RZ_MAX_DW);
          w |= (uint64_t)in32[dw + (dw >> 4)] << have;
          have += 32;
        }
        const int q = __builtin_ctzll(~w | (1ull << RZ_Q_ESC));
        uint32_t top;
        int len;
        if (q < RZ_Q_ESC) {
          const uint32_t r = ((uint32_t)q << k) | ((uint32_t)(w >> (q + 1)) & low_mask);
          len = q + 1 + k;
          if (r > 255u) { bad = true; break; }
          top = order[r];
        } else {
          top = (uint32_t)(w >> RZ_Q_ESC) & 255u;
          len = RZ_Q_ESC + 8;
        }
        pos += len;
        if (pos > n_bits) { bad = true; break; }  // the code ends past the sub-stream
        w >>= len;
        have -= len;
        outb[o] = (uint8_t)top;
        o += g.es;
      }
      // exactly ceil(pos/8) bytes, and the pad bits (have >= 12 here) zero
      bad = bad || ((pos + 7) >> 3) != e1 - e0 ||
            ((pos & 7) && ((uint32_t)w & ((1u << (8 - (pos & 7))) - 1)) != 0);
    }
    if (__ballot(walks && bad)) { malformed(status, seg, lane); continue; }

    // all 64 lanes: the low bytes between the top bytes, then the copy out
    low_bytes_in(in, mis, g.es, g.lo, outb, lane);
    __syncthreads();
    lds_to_global(outb, g.d, g.L, lane);
  }
}

// ---------------------------------------------------------------------------
// host entry points: the table ABI of ma_fpz_encode and ma_fpz_decode
// ---------------------------------------------------------------------------

extern "C" int ma_ricez_encode(const void* src, const void* blk_src_off,
                               const void* blk_raw_len, const void* blk_first_seg,
                               const void* rank_of, int es, void* stride_buf, int out_stride,
                               void* comp_lens, int n_blocks, long max_segs, void* stream) {
  return launch_rank_encode(ricez_encode_kernel, es == 1 || es == 2 || es == 4, n_blocks,
                            max_segs, stream, src, blk_src_off, blk_raw_len, blk_first_seg,
                            rank_of, es, stride_buf, out_stride, comp_lens);
}

extern "C" int ma_ricez_decode(const void* comp, const void* comp_offs, const void* dst_offs,
                               const void* seg_lens, const void* seg_raw, const void* seg_blk,
                               const void* orders, const void* blk_es, void* dst, void* status,
                               int n_segments, void* stream) {
  return launch_rank_decode(ricez_decode_kernel, n_segments, stream, comp, comp_offs, dst_offs,
                            seg_lens, seg_raw, seg_blk, orders, blk_es, dst, status);
}

// Wavefront LZ4 segment encoder for gfx950 (MI355X, CDNA4): the sibling of the
// lane encoder in lz4_lane.h, opt-in as lz_parser="wave" (ops/compress.py).
// lz4_wave_segment() is the encoder of one segment; lz4w.hip (one span a
// launch) and lz4s.hip (a table of spans a launch) are the kernels around it.
//
// Same MALZ41 stride slots and comp_lens as lz4_compress_kernel, same
// standard LZ4 block per 4 KiB segment, read by every decoder the project
// has. What differs is the parse and who does it: one wavefront per segment
// (one wavefront per workgroup, so __syncthreads() is a wave-level LDS fence
// and every branch around it is wave-uniform), a 12-bit hash, and EVERY
// position of the segment both looked up and inserted. The parse is pinned
// byte for byte by utils/lz4ref.compress_block_wave:
//
//   cand(p)  the largest q < p with hash(q) == hash(p), p in [0, n - 12)
//   match    cand(p) exists and its four bytes equal the four at p;
//            len(p) the common extension, capped at n - 5 - p
//   select   greedy from 0: at a match emit and jump len(p), else step 1
//
// Phases, all on the segment staged in LDS (each source byte is read from
// global memory once, by aligned dword loads at any source alignment):
//
//   1 candidates  64 positions a round. A lane reads the table slot of its
//                 hash, the latest position of EARLIER rounds, and then writes
//                 its own position there. Lanes of one round with one hash
//                 collide on the slot and one of them, any, wins; a lane that
//                 reads back another's position has lost, and only the hashes
//                 of losers are resolved, one ballot each: a lane's candidate
//                 is the nearest earlier lane of the ballot (later than
//                 anything the table had), and the ballot's last lane rewrites
//                 the slot, so it never goes stale. An atomicMax on the table
//                 alone would hand every lane the round's LATEST position,
//                 its own or a later one. Random bytes resolve about one hash
//                 in two rounds, an all-zero segment one per round.
//   2 lengths     rounds in descending order. Consecutive matches with the
//                 same offset end at the same byte (len(p) = len(p+1) + 1), so
//                 only the last position of such a run compares bytes, a dword
//                 at a time; the others take the run's end from a ballot and a
//                 shuffle, or from the round above through LDS. A head whose
//                 comparison walks onto a match of a later round with its own
//                 offset stops there and takes that end: runs that a hash
//                 collision cut apart (a tiled 1 KiB unit: one position in
//                 five) cost a round's length each, not the segment's. An
//                 all-zero segment compares 8 bytes, not 8 M.
//   3 selection   pointer jumping over next(p) = end of the match at p, or
//                 p + 1: the positions at chain distance < 2^k from 0 are
//                 marked after k doubling rounds, at most ceil(log2 4096) = 12,
//                 fewer when the chain is short (next^(2^k)(0) is the end).
//                 The jump table is double-buffered: an in-place round would
//                 compose jumps of different powers. A lane takes 8 positions
//                 at a time, so that their dependent LDS reads overlap.
//   4 emit        marked matches are the sequences. Popcounts and a wave scan
//                 list them in order, a second scan over their encoded sizes
//                 gives every sequence its place, a lane writes its sequence's
//                 token, lengths and offset into an LDS image of the block and
//                 short literal runs too; long runs are copied by the whole
//                 wavefront. The image leaves with 16-byte stores
//                 (rank_common.h: lds_to_global), exactly comp_len bytes of it.
//
// A block that is not shorter than its segment, or longer than out_stride, is
// never built: comp_len 0 and nothing written, the lane kernel's rule.
//
// LDS per wavefront: the staged segment 4.0 KiB, buf_a (hash table, then jump
// table, then the sequence lists) 8.0 KiB, buf_b (jump table, then the block
// image) 8.0 KiB, offsets 8.0 KiB, match ends 8.0 KiB, mark and match bits
// 1.1 KiB: 37.3 KiB, four wavefronts per CU out of 160 KiB, one per SIMD.
//
// Measured on an MI355X (hipEvent times, median of 12 interleaved launches,
// one 64 MiB window, lane encoder first): text 3474 us and 3276 us with 12 %
// fewer stored bytes; zeros 719 us and 922 us; random bytes 589 us and
// 2186 us; a tiled 1 KiB unit 735 us and 4201 us. One wavefront per SIMD hides
// no LDS latency, and the lane encoder skips through what does not match.
// More in profiles/README.md, "Wavefront LZ4 encoder".
//
// Bounds. Every LDS index is a position < 4096 or the end node 4096; the
// arrays have 8 spare entries. A dword read for position p touches the dword
// after the one p is in, which the staging buffer has. The image is written
// only once its size is known to be < n <= 4096.

#pragma once

#include "malz_common.h"
#include "rank_common.h"

#define LZW_HASH_BITS 12
#define LZW_HASH_SIZE (1 << LZW_HASH_BITS)
#define LZW_MIN_MATCH 4
#define LZW_MFLIMIT 12
#define LZW_LASTLITERALS 5
#define LZW_NONE 0xFFFFu
#define LZW_END SEG_SIZE  // the node every chain of the selection ends in
#define LZW_IN_DWORDS ((SEG_SIZE + 3 + 3) / 4 + 2)
#define LZW_SLOTS (SEG_SIZE + 8)
#define LZW_MAX_SEQ (SEG_SIZE / LZW_MIN_MATCH)
#define LZW_BATCH 8         // positions a lane jumps side by side
#define LZW_JUMP_ROUNDS 12  // 2^12 = SEG_SIZE: no chain is longer
#define LZW_LANE_LITERALS 16  // literal runs up to this long are copied by their lane

// the four bytes at byte address a of the staged segment
__device__ __forceinline__ uint32_t lzw_load32(const uint32_t* in32, int a) {
  const uint32_t lo = in32[a >> 2], hi = in32[(a >> 2) + 1];
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (a & 3)));
}

__device__ __forceinline__ int lzw_ext_bytes(int v) { return v >= 15 ? 1 + (v - 15) / 255 : 0; }

__device__ __forceinline__ uint8_t* lzw_put_ext(uint8_t* o, int v) {
  if (v >= 15) {
    int rest = v - 15;
    while (rest >= 255) { *o++ = 255; rest -= 255; }
    *o++ = (uint8_t)rest;
  }
  return o;
}

// The n <= SEG_SIZE bytes at sp -> an LZ4 block at slot and its length in
// *comp_len (0 => incompressible, store raw: nothing written to slot). Called
// by every lane of a workgroup that is ONE wavefront, for a segment all of
// them share; the LDS below is the workgroup's, reused segment after segment.
__device__ __forceinline__ void lz4_wave_segment(
    const uint8_t* __restrict__ sp, const int n, uint8_t* __restrict__ slot,
    int32_t* __restrict__ comp_len, const int out_stride, const int lane) {
  __shared__ uint32_t in32[LZW_IN_DWORDS];
  __shared__ __attribute__((aligned(16))) uint16_t buf_a[LZW_SLOTS];
  __shared__ __attribute__((aligned(16))) uint16_t buf_b[LZW_SLOTS];
  __shared__ uint16_t off16[LZW_SLOTS];  // match offset of a position, 0: no match
  __shared__ uint16_t end16[LZW_SLOTS];  // where its match ends, or position + 1
  __shared__ uint64_t match64[WAVE];     // bit l of word r: position 64 r + l has a match
  __shared__ uint32_t reach32[2 * WAVE + 2];  // bit p: the greedy walk visits p
  const uint8_t* in = reinterpret_cast<const uint8_t*>(in32);
  {
    __syncthreads();  // the last segment's LDS readers are done
    const int mfl = n - LZW_MFLIMIT;  // positions [0, mfl) are looked up and inserted
    if (mfl <= 0) {                   // no position may match: literals only, longer than n
      if (lane == 0) *comp_len = 0;
      return;
    }
    const int rounds = (mfl + WAVE - 1) / WAVE;

    // stage: byte i of the segment is in[mis + i]
    const int mis = (int)(reinterpret_cast<uintptr_t>(sp) & 3);
    {
      const uint32_t* s1 = reinterpret_cast<const uint32_t*>(sp - mis);
      const int n_dw = (mis + n + 3) >> 2;  // each holds at least one byte of the segment
      for (int k = lane; k < n_dw; k += WAVE) in32[k] = s1[k];
      uint32_t* table32 = reinterpret_cast<uint32_t*>(buf_a);
      for (int k = lane; k < LZW_HASH_SIZE / 2; k += WAVE) table32[k] = 0xFFFFFFFFu;
    }
    __syncthreads();

    // 1: candidates, off16
    uint16_t* table = buf_a;
    for (int r = 0; r < rounds; ++r) {
      const int base = r * WAVE;
      const int p = base + lane;
      const bool valid = p < mfl;
      const uint32_t v = valid ? lzw_load32(in32, mis + p) : 0;
      const uint32_t h = (v * 2654435761u) >> (32 - LZW_HASH_BITS);
      uint32_t cand = valid ? table[h] : LZW_NONE;  // the latest of the rounds before
      __syncthreads();  // every slot is read before any is written
      if (valid) table[h] = (uint16_t)p;  // lanes with one hash: any one of them wins
      __syncthreads();
      // a lane that lost its slot shares its hash with others of the round
      uint64_t losers = __ballot(valid && table[h] != p);
      while (losers) {
        const uint32_t hh = __builtin_amdgcn_readlane(h, __builtin_ctzll(losers));
        const bool same = valid && h == hh;
        const uint64_t group = __ballot(same);  // every lane of the round with this hash
        if (same) {
          const uint64_t below = group & ((1ull << lane) - 1);
          // an earlier lane of this round is later than anything the table had
          if (below) cand = base + 63 - __builtin_clzll(below);
          if ((group >> lane) == 1) table[hh] = (uint16_t)p;  // the slot keeps the latest
        }
        losers &= ~group;
      }
      const bool m = valid && cand != LZW_NONE && lzw_load32(in32, mis + (int)cand) == v;
      off16[p] = m ? (uint16_t)(p - cand) : 0;  // p <= 64 * rounds - 1 <= 4095
      __syncthreads();
    }

    // 2: match ends, end16 and match64
    for (int r = rounds - 1; r >= 0; --r) {
      const int p = r * WAVE + lane;
      const int o = p < mfl ? off16[p] : 0;
      const int o1 = p + 1 < mfl ? off16[p + 1] : 0;
      const bool m = o != 0;
      // a run: consecutive matches with one offset; its last position is the head
      const bool head = m && o1 != o;
      int e = p + 1;
      if (head) {
        const int cap = n - LZW_LASTLITERALS - p;  // >= 8
        int i = LZW_MIN_MATCH, known = 0;
        while (i < cap) {  // reads end before byte p + cap + 3 < n
          // bytes [p, x) match at offset o: a match at x with the same offset,
          // in a round already done, ends where this one does
          const int x = p + i;
          if (x >= (r + 1) * WAVE && x < mfl && off16[x] == o) {
            known = end16[x];
            break;
          }
          const uint32_t d = lzw_load32(in32, mis + x) ^ lzw_load32(in32, mis + x - o);
          if (d) {
            i += __builtin_ctz(d) >> 3;
            break;
          }
          i += 4;
        }
        e = known ? known : p + min(i, cap);
      }
      const uint64_t heads = __ballot(head) >> lane;  // bit 0: this lane
      const uint64_t matches = __ballot(m);
      const int head_lane = heads ? lane + __builtin_ctzll(heads) : lane;
      const int e_head = __shfl(e, head_lane, WAVE);
      // no head above in this round: the run goes on into the round above,
      // whose lane 0 is in it and already has the end
      if (m) e = heads ? e_head : end16[(r + 1) * WAVE];
      end16[p] = (uint16_t)e;
      if (lane == 0) match64[r] = matches;
      __syncthreads();
    }

    // 3: selection by pointer jumping
    uint16_t* cur = buf_a;
    uint16_t* nxt = buf_b;
    for (int p = lane; p < mfl; p += WAVE) {
      const int e = end16[p];
      cur[p] = (uint16_t)(e >= mfl ? LZW_END : e);
    }
    if (lane == 0) cur[LZW_END] = nxt[LZW_END] = LZW_END;
    for (int k = lane; k < 2 * WAVE + 2; k += WAVE) reach32[k] = k == 0 ? 1u : 0u;
    __syncthreads();
    // before round k: cur = next^(2^k), marked = chain distance < 2^k from 0.
    // A mark set and read within one round only marks a visited position early.
    for (int k = 0; k < LZW_JUMP_ROUNDS && cur[0] != LZW_END; ++k) {
      // LZW_BATCH positions a lane at a time, their dependent reads side by side
      for (int i0 = 0; i0 < rounds; i0 += LZW_BATCH) {
        int j[LZW_BATCH], jj[LZW_BATCH];
        uint32_t marks[LZW_BATCH];
#pragma unroll
        for (int u = 0; u < LZW_BATCH; ++u) {
          const int p = (i0 + u) * WAVE + lane;
          j[u] = p < mfl ? cur[p] : LZW_END;
          marks[u] = p < mfl ? reach32[p >> 5] : 0;
        }
#pragma unroll
        for (int u = 0; u < LZW_BATCH; ++u) jj[u] = cur[j[u]];
#pragma unroll
        for (int u = 0; u < LZW_BATCH; ++u) {
          const int p = (i0 + u) * WAVE + lane;
          if (p < mfl) {
            if (((marks[u] >> (p & 31)) & 1u) && j[u] != LZW_END)
              atomicOr(&reach32[j[u] >> 5], 1u << (j[u] & 31));
            nxt[p] = (uint16_t)jj[u];
          }
        }
      }
      __syncthreads();
      uint16_t* t = cur; cur = nxt; nxt = t;
    }
    __syncthreads();

    // 4: the sequences in order, their places, the block
    uint16_t* seq_pos = buf_a;                // the match position of sequence i
    uint16_t* seq_at = buf_a + LZW_MAX_SEQ;   // its first byte in the block
    uint8_t* image = reinterpret_cast<uint8_t*>(buf_b);
    uint64_t mine = 0;
    if (lane < rounds)
      mine = ((uint64_t)reach32[2 * lane] | ((uint64_t)reach32[2 * lane + 1] << 32)) & match64[lane];
    const int count = __popcll(mine);
    int at_seq = wave_excl_scan(count, lane);
    const int n_seq = wave_sum(count);  // <= (n - 5) / 4 < LZW_MAX_SEQ
    if (n_seq == 0) {
      if (lane == 0) *comp_len = 0;
      return;
    }
    for (; mine; mine &= mine - 1) seq_pos[at_seq++] = (uint16_t)(lane * WAVE + __builtin_ctzll(mine));
    __syncthreads();

    int total = 0;
    for (int c = 0; c < n_seq; c += WAVE) {
      const int i = c + lane;
      int size = 0;
      if (i < n_seq) {
        const int p = seq_pos[i];
        const int anchor = i ? end16[seq_pos[i - 1]] : 0;
        const int lit = p - anchor, ml = end16[p] - p - LZW_MIN_MATCH;
        size = 1 + lzw_ext_bytes(lit) + lit + 2 + lzw_ext_bytes(ml);
      }
      const int before = wave_excl_scan(size, lane);
      if (i < n_seq) seq_at[i] = (uint16_t)(total + before);  // < 3 * 4096
      total += wave_sum(size);
    }
    const int last_anchor = end16[seq_pos[n_seq - 1]];
    const int last_lit = n - last_anchor;  // >= 5
    const int block_len = total + 1 + lzw_ext_bytes(last_lit) + last_lit;
    if (block_len >= n || block_len > out_stride) {
      if (lane == 0) *comp_len = 0;
      return;
    }
    __syncthreads();

    for (int c = 0; c < n_seq; c += WAVE) {
      const int i = c + lane;
      int anchor = 0, lit = 0, lit_at = 0;
      if (i < n_seq) {
        const int p = seq_pos[i];
        anchor = i ? end16[seq_pos[i - 1]] : 0;
        lit = p - anchor;
        const int ml = end16[p] - p - LZW_MIN_MATCH;
        const int o = off16[p];
        uint8_t* out = image + seq_at[i];
        *out++ = (uint8_t)(((lit < 15 ? lit : 15) << 4) | (ml < 15 ? ml : 15));
        out = lzw_put_ext(out, lit);
        lit_at = (int)(out - image);
        if (lit <= LZW_LANE_LITERALS)
          for (int k = 0; k < lit; ++k) out[k] = in[mis + anchor + k];
        out += lit;
        *out++ = (uint8_t)(o & 0xFF);
        *out++ = (uint8_t)(o >> 8);
        lzw_put_ext(out, ml);
      }
      // long literal runs: one at a time, by the whole wavefront
      for (uint64_t big = __ballot(lit > LZW_LANE_LITERALS); big; big &= big - 1) {
        const int from_lane = __builtin_ctzll(big);
        const int a = __shfl(anchor, from_lane, WAVE), len = __shfl(lit, from_lane, WAVE);
        const int to = __shfl(lit_at, from_lane, WAVE);
        for (int k = lane; k < len; k += WAVE) image[to + k] = in[mis + a + k];
      }
    }
    {
      uint8_t* out = image + total;
      if (lane == 0) {
        *out = (uint8_t)((last_lit < 15 ? last_lit : 15) << 4);
        lzw_put_ext(out + 1, last_lit);
      }
      out += 1 + lzw_ext_bytes(last_lit);
      for (int k = lane; k < last_lit; k += WAVE) out[k] = in[mis + last_anchor + k];
    }
    __syncthreads();
    lds_to_global(image, slot, block_len, lane);
    if (lane == 0) *comp_len = block_len;
  }
}

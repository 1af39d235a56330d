// The lane parser of the LZ4 segment encoders for gfx950: one lane compresses
// one 4 KiB segment into a standard LZ4 block (greedy, a 128-entry hash table
// in the lane's 256 B of LDS). Shared by lz4.hip (one span a launch) and
// lz4s.hip (a table of spans a launch), so that both write the same bytes.

#pragma once

#include "malz_common.h"

#define HASH_BITS 7
#define HASH_SIZE (1 << HASH_BITS)  // 128 u16 entries = 256 B LDS per lane
#define MIN_MATCH 4
// stop emitting matches near the end per the LZ4 spec (last 5 literals,
// no match within the last 12 bytes)
#define MFLIMIT 12
#define LASTLITERALS 5

__device__ __forceinline__ uint32_t load32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__device__ __forceinline__ uint32_t lz4_hash(uint32_t v) {
  return (v * 2654435761u) >> (32 - HASH_BITS);
}

// Compress one segment (<= SEG_SIZE bytes) into dst; returns compressed size,
// or 0 when the result would not fit in max_out (caller stores raw).
__device__ int lz4_compress_segment(const uint8_t* __restrict__ src, int src_len,
                                    uint8_t* __restrict__ dst, int max_out,
                                    uint16_t* __restrict__ table) {
#pragma unroll 8
  for (int i = 0; i < HASH_SIZE; ++i) table[i] = 0xFFFFu;

  int ip = 0;       // current position
  int anchor = 0;   // start of pending literals
  int op = 0;       // output position
  int misses = 0;   // LZ4-style skip acceleration through matchless regions
  const int mflimit = src_len - MFLIMIT;

  if (src_len >= MIN_MATCH + LASTLITERALS) {
    while (ip < mflimit) {
      uint32_t seq = load32(src + ip);
      uint32_t h = lz4_hash(seq);
      int cand = table[h];
      table[h] = (uint16_t)ip;
      if (cand != 0xFFFF && cand < ip && (ip - cand) <= 0xFFFF &&
          load32(src + cand) == seq) {
        misses = 0;
        // extend the match
        int mlen = MIN_MATCH;
        const int maxm = src_len - LASTLITERALS - ip;
        while (mlen < maxm && src[cand + mlen] == src[ip + mlen]) ++mlen;
        int lit = ip - anchor;
        // token + extended literal length + literals + offset + ext match len
        int need = 1 + (lit >= 15 ? 1 + lit / 255 : 0) + lit + 2 +
                   ((mlen - MIN_MATCH) >= 15 ? 1 + (mlen - MIN_MATCH) / 255 : 0);
        if (op + need + 8 > max_out) return 0;
        int ml = mlen - MIN_MATCH;
        uint8_t token = (uint8_t)((lit < 15 ? lit : 15) << 4) |
                        (uint8_t)(ml < 15 ? ml : 15);
        dst[op++] = token;
        if (lit >= 15) {
          int rest = lit - 15;
          while (rest >= 255) { dst[op++] = 255; rest -= 255; }
          dst[op++] = (uint8_t)rest;
        }
        {
          int i = 0;
          for (; i + 4 <= lit; i += 4) {  // word-wise literal copy
            uint32_t v;
            __builtin_memcpy(&v, src + anchor + i, 4);
            __builtin_memcpy(dst + op + i, &v, 4);
          }
          for (; i < lit; ++i) dst[op + i] = src[anchor + i];
          op += lit;
        }
        uint16_t off = (uint16_t)(ip - cand);
        dst[op++] = (uint8_t)(off & 0xFF);
        dst[op++] = (uint8_t)(off >> 8);
        if (ml >= 15) {
          int rest = ml - 15;
          while (rest >= 255) { dst[op++] = 255; rest -= 255; }
          dst[op++] = (uint8_t)rest;
        }
        ip += mlen;
        anchor = ip;
      } else {
        ip += 1 + (misses >> 6);  // accelerate through incompressible runs
        ++misses;
      }
    }
  }
  // trailing literals
  int lit = src_len - anchor;
  int need = 1 + (lit >= 15 ? 1 + lit / 255 : 0) + lit;
  if (op + need > max_out) return 0;
  dst[op++] = (uint8_t)((lit < 15 ? lit : 15) << 4);
  if (lit >= 15) {
    int rest = lit - 15;
    while (rest >= 255) { dst[op++] = 255; rest -= 255; }
    dst[op++] = (uint8_t)rest;
  }
  for (int i = 0; i < lit; ++i) dst[op++] = src[anchor + i];
  return op;
}

// Shared by the rank codecs (fpz.hip, bytez.hip, ricez.hip) for gfx950: the size of the
// header their containers have, how a
// segment's elements are split among the lanes of its wavefront, wavefront
// sums and scans, and the copy of a decoded segment from LDS to any
// destination.

#pragma once

#include "malz_common.h"

#define RANK_HEADER_FIXED 276  // magic 6, raw_len 8, es 1, reserved 1, n_seg 4, order 256

// Staging of fpz.hip and ricez.hip (the comment at the top of fpz.hip):
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

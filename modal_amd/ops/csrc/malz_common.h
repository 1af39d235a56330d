// Device helpers shared by the container kernels (malz.hip, fpz.hip) for
// gfx950: the raw length of a segment and byte-exact wavefront copies.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define SEG_SIZE 4096
#define WAVE 64
#define MAX_GRID_Y 65535

__device__ __forceinline__ int seg_eff(int clen, int64_t raw_len, int64_t s) {
  if (clen) return clen;
  int64_t left = raw_len - s * SEG_SIZE;
  return (int)(left < SEG_SIZE ? left : SEG_SIZE);
}

// Copy len bytes with one wavefront, byte-exact for any src/dst alignment:
// byte lanes up to dst's 16-byte boundary, dwordx4 stores on the body fed by
// aligned loads (dwordx4 when src is co-aligned, else five dwords funnelled
// to the byte shift), byte lanes on the tail.
__device__ void wave_copy(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                          int len, int lane) {
  int head = (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
  if (head > len) head = len;
  if (lane < head) dst[lane] = src[lane];
  src += head; dst += head; len -= head;

  const int n_vec = len >> 4;
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    for (int k = lane; k < n_vec; k += WAVE) d4[k] = s4[k];
  } else if (mis == 0) {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src);
    for (int k = lane; k < n_vec; k += WAVE) {
      uint4 v;
      v.x = s1[4 * k + 0]; v.y = s1[4 * k + 1];
      v.z = s1[4 * k + 2]; v.w = s1[4 * k + 3];
      d4[k] = v;
    }
  } else {
    // the five aligned dwords that cover src[16k .. 16k+15]; the first and
    // the last each hold at least one of those bytes, so no load leaves the
    // dwords the copy's own source bytes live in
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(src - mis);
    const int sh = mis * 8;
    for (int k = lane; k < n_vec; k += WAVE) {
      uint32_t w0 = s1[4 * k + 0], w1 = s1[4 * k + 1], w2 = s1[4 * k + 2];
      uint32_t w3 = s1[4 * k + 3], w4 = s1[4 * k + 4];
      uint4 v;
      v.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
      v.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
      v.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
      v.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
      d4[k] = v;
    }
  }
  const int tail_start = n_vec << 4;
  if (lane < len - tail_start) dst[tail_start + lane] = src[tail_start + lane];
}

__device__ __forceinline__ void put_le(uint8_t* dst, uint64_t v, int nbytes, int lane) {
  if (lane < nbytes) dst[lane] = (uint8_t)(v >> (8 * lane));
}

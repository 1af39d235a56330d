// Shared by the container kernels (malz.hip, fpz.hip) for gfx950: the raw
// length of a segment, byte-exact wavefront copies, the segment table and
// payload of a container, the launch loop for grids past MAX_GRID_Y rows.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define SEG_SIZE 4096
#define WAVE 64
#define MAX_GRID_Y 65535
#define ASM_BLOCK 256
#define ASM_WAVES (ASM_BLOCK / WAVE)  // one wavefront per segment
#define ASM_GROUPS 512                // x 4 waves = the 2048 segments of 8 MiB

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

// What follows a container's fixed header, for one block of an assemble grid
// (ASM_GROUPS x blocks, ASM_BLOCK threads): the comp_len table at `table` and
// behind it every segment's bytes at its seg_off, compressed segments from
// their stride slot (indexed, like comp_lens and seg_off, from `first`), raw
// ones from the source.
__device__ __forceinline__ void assemble_segments(
    uint8_t* table, const uint8_t* __restrict__ blk_src, const uint8_t* __restrict__ stride_buf,
    int out_stride, const int32_t* __restrict__ comp_lens, const int64_t* __restrict__ seg_off,
    int64_t first, int64_t raw_len, int64_t n_seg) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  uint8_t* payload = table + 4 * n_seg;
  for (int64_t s = (int64_t)blockIdx.x * ASM_WAVES + wave; s < n_seg;
       s += (int64_t)gridDim.x * ASM_WAVES) {
    const int clen = comp_lens[first + s];
    put_le(table + 4 * s, (uint32_t)clen, 4, lane);
    const uint8_t* from = clen ? stride_buf + (first + s) * out_stride
                               : blk_src + s * SEG_SIZE;
    wave_copy(from, payload + seg_off[first + s], seg_eff(clen, raw_len, s), lane);
  }
}

// A grid of n_blocks rows in chunks of at most MAX_GRID_Y: launch(base, ny)
// starts the kernel for rows [base, base + ny). Returns the first HIP error.
template <typename Launch>
static inline int launch_chunked(int n_blocks, Launch launch) {
  for (int base = 0; base < n_blocks; base += MAX_GRID_Y) {
    launch(base, n_blocks - base < MAX_GRID_Y ? n_blocks - base : MAX_GRID_Y);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
  }
  return 0;
}

// Wavefront LZ4 encoder for gfx950 (MI355X, CDNA4), one span a launch: the
// sibling of lz4_compress_kernel (lz4.hip), opt-in as lz_parser="wave"
// (ops/compress.py). One wavefront per segment, one wavefront per workgroup;
// the segment encoder, its phases, its LDS and its measurements are in
// lz4_wave.h, which lz4s.hip runs over a table of spans.

#include "lz4_wave.h"

extern "C" __global__ __launch_bounds__(WAVE) void lz4_compress_wave_kernel(
    const uint8_t* __restrict__ src, int64_t src_len,
    uint8_t* __restrict__ dst,        // n_segments * out_stride
    int32_t* __restrict__ comp_lens,  // 0 => incompressible, store raw
    int out_stride, int n_segments) {
  const int lane = threadIdx.x;
  for (int seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
    const int64_t start = (int64_t)seg * SEG_SIZE;
    const int n = (int)min((int64_t)SEG_SIZE, src_len - start);
    lz4_wave_segment(src + start, n, dst + (int64_t)seg * out_stride, comp_lens + seg,
                     out_stride, lane);
  }
}

// The argument list of ma_lz4_compress (lz4.hip).
extern "C" int ma_lz4_compress_wave(const void* src, long src_len, void* dst,
                                    void* comp_lens, int out_stride, int n_segments,
                                    void* stream) {
  if (n_segments <= 0) return 0;
  const int gx = n_segments < (1 << 20) ? n_segments : (1 << 20);
  hipLaunchKernelGGL(lz4_compress_wave_kernel, dim3(gx), dim3(WAVE), 0, (hipStream_t)stream,
                     (const uint8_t*)src, (int64_t)src_len, (uint8_t*)dst,
                     (int32_t*)comp_lens, out_stride, n_segments);
  return (int)hipGetLastError();
}

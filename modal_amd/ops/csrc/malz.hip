// MALZ41 container assembly on the device for gfx950 (MI355X, CDNA4).
//
// The LZ4 kernel (lz4.hip) leaves every 4 KiB segment's block in a fixed-
// stride slot plus a comp_len per segment. These two kernels finish the
// container (layout in ops/compress.py) where the data lives, for a batch of
// blocks at once, so the only large D2H is the dense container. They are the
// one device encoder, compress.compress_spans_gpu, behind blobs and snapshots
// alike; only the streamed upload pipeline (ops/pipeline.py) still reads the
// whole strided buffer back and compacts on the host.
//
//   plan      per block: eff[i] = comp_len ? comp_len : raw segment length,
//             exclusive scan -> seg_off, sum -> blk_payload (the host's
//             keep/raw decision needs only that one int64 per block)
//   assemble  per kept block: header, then comp_len table + every segment's
//             bytes at 18 + 4*n_seg + seg_off[s] (assemble_segments in
//             malz_common.h, which fpz.hip's assemble kernel shares)
//
// Segment arrays (comp_lens, seg_off, stride slots) are indexed by
// blk_first_seg[b] + s; a block's segment count is ceil(blk_raw_len[b]/4096).
// seg_off is int64: a block is a whole blob on the BlobStore.put path, with
// no bound on its size.

#include "malz_common.h"

#define PLAN_BLOCK 256
#define HEADER_FIXED 18               // magic(6) + u64 raw_len + u32 n_seg

extern "C" __global__ __launch_bounds__(PLAN_BLOCK) void malz_plan_kernel(
    const int32_t* __restrict__ comp_lens,
    const int32_t* __restrict__ blk_first_seg,
    const int64_t* __restrict__ blk_raw_len,
    int64_t* __restrict__ seg_off,
    int64_t* __restrict__ blk_payload) {
  __shared__ int64_t wave_sum[PLAN_BLOCK / WAVE];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const int64_t raw_len = blk_raw_len[b];
  const int64_t n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  const int32_t* cl = comp_lens + blk_first_seg[b];
  int64_t* so = seg_off + blk_first_seg[b];

  // each thread owns a run of consecutive segments (8 for an 8 MiB block)
  const int64_t per = (n_seg + PLAN_BLOCK - 1) / PLAN_BLOCK;
  const int64_t lo = min((int64_t)tid * per, n_seg);
  const int64_t hi = min(lo + per, n_seg);
  int64_t mine = 0;
  for (int64_t s = lo; s < hi; ++s) mine += seg_eff(cl[s], raw_len, s);

  // inclusive scan inside the wave, then across the 4 waves through LDS
  int64_t incl = mine;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    int64_t up = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += up;
  }
  if (lane == WAVE - 1) wave_sum[wave] = incl;
  __syncthreads();
  int64_t base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < PLAN_BLOCK / WAVE; ++w) {
    if (w < wave) base += wave_sum[w];
    total += wave_sum[w];
  }
  int64_t run = base + incl - mine;
  for (int64_t s = lo; s < hi; ++s) {
    so[s] = run;
    run += seg_eff(cl[s], raw_len, s);
  }
  if (tid == 0) blk_payload[b] = total;
}

extern "C" __global__ __launch_bounds__(ASM_BLOCK) void malz_assemble_kernel(
    const uint8_t* __restrict__ src,
    const int64_t* __restrict__ blk_src_off,
    const uint8_t* __restrict__ stride_buf, int out_stride,
    const int32_t* __restrict__ comp_lens,
    const int64_t* __restrict__ seg_off,
    const int32_t* __restrict__ blk_first_seg,
    const int64_t* __restrict__ blk_raw_len,
    uint8_t* __restrict__ out,
    const int64_t* __restrict__ blk_out_off,
    int blk_base) {
  const int b = blk_base + blockIdx.y;
  const int64_t out_off = blk_out_off[b];
  if (out_off < 0) return;  // block stored raw: nothing to assemble
  const int64_t raw_len = blk_raw_len[b];
  const int64_t n_seg = (raw_len + SEG_SIZE - 1) / SEG_SIZE;
  uint8_t* blk_out = out + out_off;

  if (blockIdx.x == 0 && threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    const uint64_t magic = 0x31345A4C414DULL;  // "MALZ41", little-endian
    put_le(blk_out, magic, 6, lane);
    put_le(blk_out + 6, (uint64_t)raw_len, 8, lane);
    put_le(blk_out + 14, (uint64_t)n_seg, 4, lane);
  }
  assemble_segments(blk_out + HEADER_FIXED, src + blk_src_off[b], stride_buf, out_stride,
                    comp_lens, seg_off, blk_first_seg[b], raw_len, n_seg);
}

extern "C" int ma_malz_plan(const void* comp_lens, const void* blk_first_seg,
                            const void* blk_raw_len, void* seg_off, void* blk_payload,
                            int n_blocks, void* stream) {
  if (n_blocks <= 0) return 0;
  hipLaunchKernelGGL(malz_plan_kernel, dim3(n_blocks), dim3(PLAN_BLOCK), 0,
                     (hipStream_t)stream, (const int32_t*)comp_lens,
                     (const int32_t*)blk_first_seg, (const int64_t*)blk_raw_len,
                     (int64_t*)seg_off, (int64_t*)blk_payload);
  return (int)hipGetLastError();
}

extern "C" int ma_malz_assemble(const void* src, const void* blk_src_off,
                                const void* stride_buf, int out_stride,
                                const void* comp_lens, const void* seg_off,
                                const void* blk_first_seg, const void* blk_raw_len,
                                void* out, const void* blk_out_off, int n_blocks,
                                void* stream) {
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(malz_assemble_kernel, dim3(ASM_GROUPS, ny), dim3(ASM_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src,
                       (const int64_t*)blk_src_off, (const uint8_t*)stride_buf, out_stride,
                       (const int32_t*)comp_lens, (const int64_t*)seg_off,
                       (const int32_t*)blk_first_seg, (const int64_t*)blk_raw_len,
                       (uint8_t*)out, (const int64_t*)blk_out_off, base);
  });
}

// Async copy on the caller's stream for the raw-pointer codec (ops/devcodec.py):
// kind 1 = host->device, 2 = device->host.
extern "C" int ma_malz_copy(void* dst, const void* src, unsigned long long nbytes,
                            int kind, void* stream) {
  if (nbytes == 0) return 0;
  return (int)hipMemcpyAsync(dst, src, nbytes,
                             kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
                             (hipStream_t)stream);
}

// Wavefront SHA-256 of long single messages for gfx950 (MI355X, CDNA4).
//
// A payload under 8 MiB has plain SHA-256 as its content digest, so a
// snapshot's tail blocks are single serial messages of up to 8 MiB - 1 B.
// sha256_many_kernel (sha256.hip) gives such a message one lane, which then
// does its own loads, byte swaps and message schedule between the rounds. Here
// a message gets one wavefront, and only the 64 rounds stay on the serial
// chain:
//
//   fill    the message is taken in batches of 64 blocks (4096 B). The
//           wavefront loads a batch as aligned dwords, 64 consecutive dwords
//           per load, and transposes it through LDS so that lane i holds block
//           i (17 dwords at a stride of 17, conflict-free). A source that is
//           not dword aligned is shifted into place with v_alignbyte. Lane i
//           writes the padding its block has (0x80, zeros, the bit count),
//           swaps to big-endian, expands W[16..63], adds the round constants
//           and stores the 64 W+K words of its block to LDS, as b128 at a
//           stride of 68 dwords: 16 lanes x 4 dwords cover the 64 banks once.
//   fetch   the next batch's raw dwords are loaded into 17 registers before
//           the rounds start, so global latency hides behind them.
//   rounds  the chain reads W+K back as b128 and runs on SHA256W_ROUND_LANES
//           lanes. With 2, lane 0 carries e,f,g,h and computes Sigma1 and Ch,
//           lane 1 carries a,b,c,d and computes Sigma0 and Maj, in one
//           instruction stream: the rotate amounts sit in a register and
//           differ per lane, Ch and Maj are one v_bitop3 of lane-specific
//           operands (they differ in a term that does not wait for the
//           chain), and the partial sums t1 and t2 (and d) cross lanes on
//           the final add (DPP quad_perm). With 1, lane 0 does a plain round.
//           12.1 VALU instructions a round against 14.1.
//
// One workgroup of one wavefront per message; LDS 21.8 KiB.

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef SHA256W_ROUND_LANES
#define SHA256W_ROUND_LANES 2  // profiles/README.md, "Wavefront tail hash"
#endif

#define SW_BATCH_BLOCKS 64     // blocks of 64 B per batch, one per lane
#define SW_RAW_STRIDE 17       // a block's 16 raw dwords and one of padding, in LDS
#define SW_RAW_WORDS (SW_BATCH_BLOCKS * SW_RAW_STRIDE + 1)
#define SW_WK_STRIDE 68        // dwords between two blocks' W+K in LDS

static __constant__ uint32_t SW_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u,
    0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u,
    0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
    0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au,
    0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

__device__ __forceinline__ uint32_t sw_rotr(uint32_t x, uint32_t n) {
  return __builtin_amdgcn_alignbit(x, x, n);  // n may differ per lane
}

// v_bitop3_b32: any function of three words, its truth table in the last
// argument (the function applied to 0xF0, 0xCC, 0xAA).
#define SW_XOR3(a, b, c) __builtin_amdgcn_bitop3_b32(a, b, c, 0x96)
#define SW_CH(e, f, g) __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA)   // (e & f) | (~e & g)
#define SW_MAJ(a, b, c) __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8)

// Raw dwords of batch `batch` for this lane: dword j*64 + lane of the batch
// for j < 16, and on lane 0 the dword after the batch, which an unaligned
// source's last block borrows from. A dword is read only if it holds a byte of
// the message, so nothing past the message's last dword is touched.
__device__ __forceinline__ void sw_fetch(uint32_t raw[17], const uint32_t* __restrict__ src,
                                         int64_t end, int64_t batch, int lane) {
  const int64_t r0 = batch * (SW_BATCH_BLOCKS * 16);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int64_t r = r0 + j * 64 + lane;
    raw[j] = (r << 2) < end ? src[r] : 0u;
  }
  const int64_t r = r0 + SW_BATCH_BLOCKS * 16;
  raw[16] = (lane == 0 && (r << 2) < end) ? src[r] : 0u;
}

// Lane's block of the batch, from its raw dwords in LDS to its 64 W+K
// words in LDS. `left` is the number of message bytes from the block's first
// byte on (at most 64 counts; negative in a block of padding only).
__device__ __forceinline__ void sw_fill(const uint32_t* __restrict__ raw_slot, uint32_t mis, int left,
                                        bool last, uint64_t bitlen, uint32_t* __restrict__ wk_slot) {
  uint32_t s[17], w[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = raw_slot[k];
  s[16] = raw_slot[SW_RAW_STRIDE];  // the next block's first dword, for the shift
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    uint32_t v = __builtin_amdgcn_alignbyte(s[k + 1], s[k], mis);
    const int nv = left - 4 * k;  // message bytes in this word
    if (nv < 4) {
      const uint32_t sh = static_cast<uint32_t>(nv & 3) * 8;
      v = nv < 0 ? 0u : ((v & ((1u << sh) - 1u)) | (0x80u << sh));
    }
    w[k] = __builtin_bswap32(v);
  }
  if (last) {
    w[14] = static_cast<uint32_t>(bitlen >> 32);
    w[15] = static_cast<uint32_t>(bitlen);
  }
#pragma unroll
  for (int t = 0; t < 64; t += 4) {
    uint32_t o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int tt = t + u;
      if (tt >= 16) {
        const uint32_t w15 = w[(tt - 15) & 15], w2 = w[(tt - 2) & 15];
        const uint32_t s0 = SW_XOR3(sw_rotr(w15, 7), sw_rotr(w15, 18), w15 >> 3);
        const uint32_t s1 = SW_XOR3(sw_rotr(w2, 17), sw_rotr(w2, 19), w2 >> 10);
        w[tt & 15] = w[tt & 15] + s0 + w[(tt - 7) & 15] + s1;
      }
      o[u] = w[tt & 15] + SW_K[tt];
    }
    *reinterpret_cast<uint4*>(wk_slot + t) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// The rounds of `cnt` blocks on one lane: st[0..7] is a..h.
__device__ __forceinline__ void sw_rounds1(uint32_t st[8], const uint32_t* __restrict__ wk, int cnt) {
  for (int blk = 0; blk < cnt; ++blk) {
    const uint4* p = reinterpret_cast<const uint4*>(wk + blk * SW_WK_STRIDE);
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    uint32_t e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint4 v = p[q];
      const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t t1 = (h + x[u]) + SW_XOR3(sw_rotr(e, 6), sw_rotr(e, 11), sw_rotr(e, 25)) + SW_CH(e, f, g);
        const uint32_t t2 = SW_XOR3(sw_rotr(a, 2), sw_rotr(a, 13), sw_rotr(a, 22)) + SW_MAJ(a, b, c);
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
      }
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
  }
}

// The rounds of `cnt` blocks on a pair of lanes. The even lane (E) holds
// e,f,g,h in st[0..3], the odd lane (A) holds a,b,c,d. With x the newest word
// of the lane's chain (e or a), y and z the two before it and w the oldest:
//   E: p = h + wk + Sigma1(e) + Ch(e, f, g)           = t1
//   A: p = 0      + Sigma0(a) + Maj(a, b, c)          = t2
//   E: x' = p + d   (d is A's w)     A: x' = p + t1   (t1 is E's p)
__device__ __forceinline__ void sw_rounds2(uint32_t st[4], const uint32_t* __restrict__ wk, int cnt,
                                           bool lane_a) {
  const uint32_t only_a = lane_a ? ~0u : 0u, only_e = ~only_a;
  const uint32_t r1 = lane_a ? 2 : 6, r2 = lane_a ? 13 : 11, r3 = lane_a ? 22 : 25;
  for (int blk = 0; blk < cnt; ++blk) {
    const uint4* ptr = reinterpret_cast<const uint4*>(wk + blk * SW_WK_STRIDE);
    uint32_t x = st[0], y = st[1], z = st[2], w = st[3];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint4 v = ptr[q];
      const uint32_t k[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t sig = SW_XOR3(sw_rotr(x, r1), sw_rotr(x, r2), sw_rotr(x, r3));
        // Ch = z ^ (x & (y ^ z)) and Maj = Ch ^ (z & (y ^ z)): the lanes differ
        // in a term that does not wait for x
        const uint32_t yz = y ^ z;
        const uint32_t zt = __builtin_amdgcn_bitop3_b32(z, yz, only_a, 0x70);  // z ^ (z & yz & only_a)
        const uint32_t fn = __builtin_amdgcn_bitop3_b32(x, yz, zt, 0x6A);      // (x & yz) ^ zt
        const uint32_t p = sig + fn + ((w + k[u]) & only_e);
        const uint32_t give = lane_a ? w : p;
        // quad_perm [1,0,3,2]: the other lane of the pair
        const uint32_t xn = p + __builtin_amdgcn_update_dpp(0u, give, 0xB1, 0xF, 0xF, true);
        w = z; z = y; y = x; x = xn;
      }
    }
    st[0] += x; st[1] += y; st[2] += z; st[3] += w;
  }
}

template <int ROUND_LANES>
__device__ __forceinline__ void sw_message(const uint8_t* __restrict__ buf,
                                           const int64_t* __restrict__ offsets,
                                           const int64_t* __restrict__ lengths,
                                           uint8_t* __restrict__ out, uint32_t* raw_lds,
                                           uint32_t* wk_lds) {
  static_assert(ROUND_LANES == 1 || ROUND_LANES == 2, "the chain runs on one lane or two");
  const int msg = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t len = lengths[msg];
  const uintptr_t addr = reinterpret_cast<uintptr_t>(buf + offsets[msg]);
  const uint32_t mis = static_cast<uint32_t>(addr & 3);
  const uint32_t* src = reinterpret_cast<const uint32_t*>(addr - mis);
  const int64_t end = len > 0 ? len + mis : 0;  // bytes from src on that hold the message
  const int64_t total = (len + 9 + 63) >> 6;    // blocks, padding included
  const int64_t batches = (total + SW_BATCH_BLOCKS - 1) / SW_BATCH_BLOCKS;
  const uint64_t bitlen = static_cast<uint64_t>(len) << 3;

  const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                          0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  const bool lane_a = lane & 1;
  uint32_t st[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) st[k] = iv[k];
  if (ROUND_LANES == 2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = lane_a ? iv[k] : iv[4 + k];
  }

  uint32_t raw[17];
  sw_fetch(raw, src, end, 0, lane);
  for (int64_t b = 0; b < batches; ++b) {
#pragma unroll
    for (int j = 0; j < 16; ++j) raw_lds[j * 68 + lane + (lane >> 4)] = raw[j];  // dword r at r + r/16
    if (lane == 0) raw_lds[SW_RAW_WORDS - 1] = raw[16];
    __syncthreads();
    const int64_t g = b * SW_BATCH_BLOCKS + lane;
    if (g < total) {
      const int64_t left = len - (g << 6);
      sw_fill(raw_lds + lane * SW_RAW_STRIDE, mis,
              left > 64 ? 64 : (left < -1 ? -1 : static_cast<int>(left)), g == total - 1, bitlen,
              wk_lds + lane * SW_WK_STRIDE);
    }
    if (b + 1 < batches) sw_fetch(raw, src, end, b + 1, lane);
    __syncthreads();
    const int64_t rest = total - b * SW_BATCH_BLOCKS;
    const int cnt = rest < SW_BATCH_BLOCKS ? static_cast<int>(rest) : SW_BATCH_BLOCKS;
    if (lane < ROUND_LANES) {
      if (ROUND_LANES == 2) {
        sw_rounds2(st, wk_lds, cnt, lane_a);
      } else {
        sw_rounds1(st, wk_lds, cnt);
      }
    }
  }

  uint32_t* dig = reinterpret_cast<uint32_t*>(out + static_cast<int64_t>(msg) * 32);
  if (ROUND_LANES == 2) {
    if (lane < 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) dig[(lane_a ? 0 : 4) + k] = __builtin_bswap32(st[k]);
    }
  } else if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dig[k] = __builtin_bswap32(st[k]);
  }
}

extern "C" __global__ __launch_bounds__(SW_BATCH_BLOCKS) void sha256_long_kernel(
    const uint8_t* __restrict__ buf,
    const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ lengths,
    uint8_t* __restrict__ out) {  // 32 bytes per message
  __shared__ uint32_t raw_lds[SW_RAW_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t wk_lds[SW_BATCH_BLOCKS * SW_WK_STRIDE];
  sw_message<SHA256W_ROUND_LANES>(buf, offsets, lengths, out, raw_lds, wk_lds);
}

// Same arguments as ma_sha256_many: message i is lengths[i] bytes at
// buf + offsets[i], its digest goes to out + 32 * i.
extern "C" int ma_sha256_long(const void* buf, const void* offsets, const void* lengths,
                              void* out, int n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(sha256_long_kernel, dim3(n), dim3(SW_BATCH_BLOCKS), 0, (hipStream_t)stream,
                     (const uint8_t*)buf, (const int64_t*)offsets, (const int64_t*)lengths,
                     (uint8_t*)out);
  return (int)hipGetLastError();
}

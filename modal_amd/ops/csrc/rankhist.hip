// The histograms the rank-plane codecs rank by, for gfx950 (MI355X, CDNA4): one
// kernel template under MAFP10, MAFB10 and MARC10 (ops/rankcodec.py,
// ops/ricecodec.py) and under both element-size probes (ops/fpcodec.py,
// ops/probe.py, which hold the numpy twins), and the rank pass behind it.
//
// What is counted. At element size es a codec ranks the top byte of every
// whole element of a span: every byte at es 1, the byte at 2k+1 at es 2, the
// byte at 4k+3 at es 4. A byte at span offset i is a top byte at es 2 when i
// is odd and at es 4 when i % 4 == 3, and "i < raw_len" is then the same as
// "the element is whole", so no table needs more than the span's own bounds.
// The kernel therefore sorts bytes by their CLASS i % 4 into 256-bin LDS
// tables and forms its output rows as sums of tables. A plan (RhPlan) says at
// compile time how many tables there are, which table, or none, each class
// counts into, and which tables add up to each output row. The three-way
// probe counts i even, i % 4 == 1 and i % 4 == 3 apart (a fourth table, 0 and
// 2 apart, would buy nothing any rule reads) and puts out es 1 = all three,
// es 2 = second + third, es 4 = the third.
//
// Loads. A lane reads aligned 16-byte chunks, starting at the chunk the span's
// first byte lives in, RH_UNROLL of them in flight, so every chunk loaded
// holds a byte of the span and every source byte is read once at any source
// alignment. Byte k of an aligned dword is at a span offset of class
// (k - mis16) % 4, mis16 the span's misalignment, the same for the whole span.
// A plan that counts every class walks the four bytes of a dword at constant
// shifts and finds each one's table from its class; one that leaves classes
// out walks the classes it counts, each at the one shift its byte has, and
// never touches the rest. Either way the full-chunk path has no branch. Only
// the first and the last chunk of a span can hold bytes outside it; those two
// check 0 <= i < raw_len per byte.
//
// LDS layout. bins[table][bin][copy], copy = lane % RH_COPIES the minor index,
// so the bank is set by the lane and hardly by the data (bank = (bin % 2) * 16
// + lane % 16 at 16 copies: lanes l and l + 16 of an LDS lane group share a
// bank only when their bins have the same parity, a two-way conflict at
// worst). That is what holds up under hot bins: two bins hold 57 % of N(0,1)
// bf16 top bytes, fp8 Gaussians put a fifth of the bytes on four bins and e8m0
// scales nearly all of them on a handful, and with the bin as the minor index
// every copy of a hot bin sits on one bank (bank = bin % 32), so lanes that
// meet on it serialise whether or not they use different copies. What no
// layout removes is lanes with the same copy AND the same bin: at 16 copies
// four lanes of a wavefront share a copy, and on a one-valued span their
// atomics serialise four deep.
//
// Copies. 16 a table: 16 KiB, so 8, 5 and 3 workgroups a CU (160 KiB of LDS)
// at one, two and three tables. 32 copies take every lane of an LDS lane group
// off every other's bank, but zeroing and merging twice the LDS shows as soon
// as a workgroup has little source; 8 copies halve that cost but put eight
// lanes on a copy and four on a bank, and are slower wherever the counting
// sets the time. Both were built and timed: profiles/README.md, "Element-size
// probe" and "Three-way probe".
//
// Grid. groups x spans. Zeroing and merging the tables is a fixed cost that a
// workgroup spreads over its source. One and two tables run RH_GROUPS groups a
// span. At three tables (48 KiB) the cost shows at 16 KiB of source a
// workgroup, so there groups = RP_TARGET_WGS / spans, between RP_MIN_GROUPS
// and RH_GROUPS: the 8 x 8 MiB blocks of a snapshot window get 64 groups of
// 128 KiB each, 64 spans of 1 MiB get 16 groups of 64 KiB each. A workgroup
// that has no chunk returns before it zeroes anything.
//
// Merge. Thread t sums bin t's copies of every table, rotated by t to stay off
// one bank, and adds each row's sum to the global table, skipping a sum that
// is zero: an e8m0 span touches a handful of the rows.
//
// Registers, LDS, occupancy and times of the five instances:
// profiles/README.md, "One histogram kernel".

#include "malz_common.h"

#define RH_BLOCK 256
#define RH_COPIES 16
#define RH_TABLE (256 * RH_COPIES)
#define RH_UNROLL 4  // 16-byte loads a lane has in flight
#define RH_GROUPS 64
#define RP_MIN_GROUPS 8
#define RP_TARGET_WGS 1024
#define RH_NONE 15u

// CLASSES: nibble c is the table that bytes at span offsets i % 4 == c count
// into, RH_NONE for none. SUMS: nibble r is the set of tables (bit t: table t)
// whose sum is output row r; counts has ROWS x 256 u32 per span.
template <int TABLES_, uint32_t CLASSES_, int ROWS_, uint32_t SUMS_>
struct RhPlan {
  static constexpr int TABLES = TABLES_, ROWS = ROWS_;
  static constexpr uint32_t CLASSES = CLASSES_, SUMS = SUMS_;
};
//                       class: 3210          row: 210
using RhEs1 = RhPlan<1, 0x0000u, 1, 0x1u>;    // every byte
using RhEs2 = RhPlan<1, 0x0F0Fu, 1, 0x1u>;    // the odd bytes
using RhEs4 = RhPlan<1, 0x0FFFu, 1, 0x1u>;    // the bytes at 3 mod 4
using RhEs24 = RhPlan<2, 0x1F0Fu, 2, 0x23u>;  // es 2 = both tables, es 4 = the second
using RhEs124 = RhPlan<3, 0x2010u, 3, 0x467u>;

__host__ __device__ constexpr uint32_t rh_table(uint32_t classes, int c) {
  return (classes >> (4 * c)) & 15u;
}

// The bytes of chunk q of a span of n bytes that the plan counts. mine: the
// lane's copy of bin 0 of table 0.
template <uint32_t CLASSES>
__device__ __forceinline__ void rh_count(const uint4 v, int64_t q, int mis16, int64_t n,
                                         uint32_t* mine) {
  constexpr bool every_class = rh_table(CLASSES, 0) != RH_NONE && rh_table(CLASSES, 1) != RH_NONE &&
                               rh_table(CLASSES, 2) != RH_NONE && rh_table(CLASSES, 3) != RH_NONE;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const int64_t i0 = 16 * q - mis16;  // span offset of the chunk's first byte
  auto count = [&](auto own) {        // own(i): span offset i is the span's
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (every_class) {  // byte k of the dword, whatever its class
          uint32_t* at = mine + rh_table(CLASSES, (k - mis16) & 3) * RH_TABLE;
          if (own(i0 + 4 * d + k)) atomicAdd(at + ((w[d] >> (8 * k)) & 255u) * RH_COPIES, 1u);
        } else if (rh_table(CLASSES, k) != RH_NONE) {  // class k, whichever byte it is
          const int j = (k + mis16) & 3;
          uint32_t* at = mine + rh_table(CLASSES, k) * RH_TABLE;
          if (own(i0 + 4 * d + j)) atomicAdd(at + ((w[d] >> (8 * j)) & 255u) * RH_COPIES, 1u);
        }
      }
  };
  if (i0 >= 0 && i0 + 16 <= n)
    count([](int64_t) { return true; });
  else  // the span's first or last chunk: count only its own bytes
    count([n](int64_t i) { return i >= 0 && i < n; });
}

// counts += the plan's rows for spans [blk_base, blk_base + gridDim.y).
template <typename Plan>
__global__ __launch_bounds__(RH_BLOCK) void rank_hist_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ blk_src_off,
    const int64_t* __restrict__ blk_raw_len, uint32_t* __restrict__ counts, int blk_base) {
  __shared__ __attribute__((aligned(16))) uint32_t bins[Plan::TABLES * RH_TABLE];
  const int b = blk_base + blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t n = blk_raw_len[b];
  if (n <= 0) return;
  const uint8_t* first = src + blk_src_off[b];
  const int mis16 = (int)(reinterpret_cast<uintptr_t>(first) & 15);
  const int64_t n_chunks = (mis16 + n + 15) >> 4;  // the last one holds byte n - 1
  if ((int64_t)blockIdx.x * RH_BLOCK >= n_chunks) return;  // nothing here: no merge either

  uint4* z = reinterpret_cast<uint4*>(bins);
  for (int k = tid; k < Plan::TABLES * RH_TABLE / 4; k += RH_BLOCK) z[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  const uint4* chunks = reinterpret_cast<const uint4*>(first - mis16);
  uint32_t* mine = bins + (tid & (RH_COPIES - 1));
  const int64_t step = (int64_t)gridDim.x * RH_BLOCK;
  int64_t q = (int64_t)blockIdx.x * RH_BLOCK + tid;
  for (; q + (RH_UNROLL - 1) * step < n_chunks; q += RH_UNROLL * step) {
    uint4 v[RH_UNROLL];
#pragma unroll
    for (int u = 0; u < RH_UNROLL; ++u) v[u] = chunks[q + u * step];
#pragma unroll
    for (int u = 0; u < RH_UNROLL; ++u) rh_count<Plan::CLASSES>(v[u], q + u * step, mis16, n, mine);
  }
  for (; q < n_chunks; q += step) rh_count<Plan::CLASSES>(chunks[q], q, mis16, n, mine);
  __syncthreads();

  uint32_t sum[Plan::TABLES] = {};
  for (int k = 0; k < RH_COPIES; ++k) {
    const int c = tid * RH_COPIES + ((k + tid) & (RH_COPIES - 1));
#pragma unroll
    for (int t = 0; t < Plan::TABLES; ++t) sum[t] += bins[t * RH_TABLE + c];
  }
  uint32_t* out = counts + (int64_t)b * (Plan::ROWS * 256);
#pragma unroll
  for (int r = 0; r < Plan::ROWS; ++r) {
    uint32_t total = 0;
#pragma unroll
    for (int t = 0; t < Plan::TABLES; ++t)
      if ((Plan::SUMS >> (4 * r + t)) & 1u) total += sum[t];
    if (total) atomicAdd(&out[256 * r + tid], total);
  }
}

// order[r] = the byte of rank r, rank_of[byte] = its rank: count descending,
// byte value ascending on ties.
extern "C" __global__ __launch_bounds__(256) void fpz_rank_kernel(
    const uint32_t* __restrict__ counts, uint8_t* __restrict__ order,
    uint8_t* __restrict__ rank_of) {
  __shared__ uint32_t c[256];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t mine = counts[b * 256 + tid];
  c[tid] = mine;
  __syncthreads();
  int r = 0;
  for (int u = 0; u < 256; ++u) {
    const uint32_t cu = c[u];
    r += (cu > mine) || (cu == mine && u < tid);
  }
  order[b * 256 + r] = (uint8_t)tid;
  rank_of[b * 256 + tid] = (uint8_t)r;
}

// ---------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------

static int rh_fixed_groups(int) { return RH_GROUPS; }

static int rh_spread_groups(int spans) {
  const int groups = RP_TARGET_WGS / spans;
  return groups < RP_MIN_GROUPS ? RP_MIN_GROUPS : groups > RH_GROUPS ? RH_GROUPS : groups;
}

// groups(ny): the workgroups a span gets in a launch of ny spans.
template <typename Plan>
static int rh_launch(const void* src, const void* blk_src_off, const void* blk_raw_len,
                     void* counts, int n_blocks, int (*groups)(int), void* stream) {
  return launch_chunked(n_blocks, [&](int base, int ny) {
    hipLaunchKernelGGL(rank_hist_kernel<Plan>, dim3(groups(ny), ny), dim3(RH_BLOCK), 0,
                       (hipStream_t)stream, (const uint8_t*)src, (const int64_t*)blk_src_off,
                       (const int64_t*)blk_raw_len, (uint32_t*)counts, base);
  });
}

// The rank tables of histograms the caller already has (n_blocks x 256 u32,
// a probe's for instance): ma_rank_hist without its histogram pass.
extern "C" int ma_fpz_rank_counts(const void* counts, void* order, void* rank_of, int n_blocks,
                                  void* stream) {
  if (n_blocks <= 0) return 0;
  hipLaunchKernelGGL(fpz_rank_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint32_t*)counts, (uint8_t*)order, (uint8_t*)rank_of);
  return (int)hipGetLastError();
}

// The histogram at element size es (1, 2 or 4) and its rank tables. counts
// (n_blocks x 256 u32) must come in zeroed.
extern "C" int ma_rank_hist(const void* src, const void* blk_src_off, const void* blk_raw_len,
                            int es, void* counts, void* order, void* rank_of, int n_blocks,
                            void* stream) {
  if (n_blocks <= 0) return 0;
  if (es != 1 && es != 2 && es != 4) return (int)hipErrorInvalidValue;
  const auto launch = es == 1 ? rh_launch<RhEs1> : es == 2 ? rh_launch<RhEs2> : rh_launch<RhEs4>;
  const int rc = launch(src, blk_src_off, blk_raw_len, counts, n_blocks, rh_fixed_groups, stream);
  return rc ? rc : ma_fpz_rank_counts(counts, order, rank_of, n_blocks, stream);
}

// counts (n_blocks x 2 x 256 u32) must come in zeroed: [b][0] the es = 2
// histogram of block b, [b][1] the es = 4 one.
extern "C" int ma_fpz_probe(const void* src, const void* blk_src_off, const void* blk_raw_len,
                            void* counts, int n_blocks, void* stream) {
  return rh_launch<RhEs24>(src, blk_src_off, blk_raw_len, counts, n_blocks, rh_fixed_groups,
                           stream);
}

// counts (n_blocks x 3 x 256 u32) must come in zeroed: [b][0] the histogram of
// every byte of block b (es 1), [b][1] the es = 2 one, [b][2] the es = 4 one.
extern "C" int ma_rank_probe(const void* src, const void* blk_src_off, const void* blk_raw_len,
                             void* counts, int n_blocks, void* stream) {
  return rh_launch<RhEs124>(src, blk_src_off, blk_raw_len, counts, n_blocks, rh_spread_groups,
                            stream);
}

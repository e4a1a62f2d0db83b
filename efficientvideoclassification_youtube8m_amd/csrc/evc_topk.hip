// Per-row top-k of an f32 matrix (evc_topk_rows): the selection behind the inference binary's prediction file
// (cs/inference_ensemble.py:63-74 format_lines: argpartition + sort of the top_k scores of each video), on the device,
// so that only [rows, k] values and indices leave it.
//
// One 256-thread workgroup per row:
//   1. the row is read once from HBM (16-byte loads when the row is 16-byte aligned) into LDS as raw bits; the digit
//      histogram of the first radix pass is built from the loaded registers;
//   2. radix select on order-preserving uint32 keys, up to 4 passes of 8 bits from the top (integer LDS histogram, suffix
//      scan over the 256 digits): the threshold key prefix and the number of ties at it that are admitted.  The walk
//      stops early when the selected digit's bucket is admitted whole;
//   3. compaction in column order: per 64-column group the counts of (key > threshold) and (key == threshold) from
//      ballots, one exclusive scan over the groups, then each survivor's slot = group base + mbcnt - ties are admitted
//      lowest columns first;
//   4. bitonic sort of the <= 256 survivors in LDS on (key << 32 | ~column), descending;
//   5. coalesced stores of the values (the input's own bits) and the column indices.
// No float atomics and no order-dependent placement: every launch gives the same bits.
#include "evc_common.h"

#include <mutex>

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_MAX_K = 256;
constexpr int TK_MAX_COLS = 32768;
constexpr int TK_GROUPS = TK_MAX_COLS / 64;
// dynamic LDS carve (every offset a multiple of 16): survivors | histogram | group counts | scan words | row
constexpr int TK_OFF_HIST = TK_MAX_K * 8;
constexpr int TK_OFF_GRP = TK_OFF_HIST + 256 * 4;
constexpr int TK_OFF_MISC = TK_OFF_GRP + TK_GROUPS * 4;
constexpr int TK_OFF_ROW = TK_OFF_MISC + 64;
constexpr int TK_MAX_LDS = TK_OFF_ROW + TK_MAX_COLS * 4;

// Total order of the selection as an unsigned key, larger = ranks first: -0 ties with +0; every NaN maps to the largest
// key (above +inf, all NaNs tied: numpy's sort order); otherwise the usual sign-flip map of the IEEE bits.
__device__ __forceinline__ uint32_t topk_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Inclusive scan of one value per thread over the 256-thread block (4 waves); ws: 4 words of LDS.  Whole block calls it.
__device__ __forceinline__ uint32_t block_incl_scan(uint32_t v, uint32_t* ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += ws[w];
  return v;
}

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const float* __restrict__ x, long ld, int cols, int k, int sort_n,
                                                               float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  unsigned long long* sv = (unsigned long long*)tk_lds;              // [sort_n] survivors: key << 32 | ~column
  uint32_t* hist = (uint32_t*)(tk_lds + TK_OFF_HIST);                // [256]
  uint32_t* grp = (uint32_t*)(tk_lds + TK_OFF_GRP);                  // [cols / 64]: gt | eq << 16, then its exclusive prefix
  uint32_t* scan_ws = (uint32_t*)(tk_lds + TK_OFF_MISC);             // [4]
  uint32_t* sel = scan_ws + 4;                                       // prefix, ties to admit, walk done
  uint32_t* row = (uint32_t*)(tk_lds + TK_OFF_ROW);                  // [cols] raw bits of the row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* xr = (const uint32_t*)(x + (long)blockIdx.x * ld);

  hist[tid] = 0;
  __syncthreads();
  // ---- 1. row -> LDS, digit histogram of pass 0 on the way ----
  if ((((uintptr_t)xr) & 15) == 0) {
    const int n4 = cols >> 2;
#pragma unroll 4
    for (int i = tid; i < n4; i += TK_THREADS) {
      const u32x4_t v = *(const u32x4_t*)(xr + 4 * i);
      *(u32x4_t*)(row + 4 * i) = v;
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&hist[topk_key(v[j]) >> 24], 1u);
    }
    for (int i = 4 * n4 + tid; i < cols; i += TK_THREADS) {
      const uint32_t u = xr[i];
      row[i] = u;
      atomicAdd(&hist[topk_key(u) >> 24], 1u);
    }
  } else {                                                           // odd ld: rows that are not 16-byte aligned
    for (int i = tid; i < cols; i += TK_THREADS) {
      const uint32_t u = xr[i];
      row[i] = u;
      atomicAdd(&hist[topk_key(u) >> 24], 1u);
    }
  }
  __syncthreads();

  // ---- 2. radix select: the k-th key's prefix and the ties admitted at it ----
  uint32_t prefix = 0, mask = 0;
  uint32_t krem = (uint32_t)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (pass > 0) {
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < cols; i += TK_THREADS) {
        const uint32_t key = topk_key(row[i]);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
    }
    const uint32_t h = hist[255 - tid];                              // thread t: digit 255 - t
    const uint32_t incl = block_incl_scan(h, scan_ws);               // candidates with digit >= 255 - t
    const uint32_t excl = incl - h;                                  // ... with digit > 255 - t
    if (excl < krem && incl >= krem) {                               // exactly one thread
      sel[0] = prefix | ((uint32_t)(255 - tid) << shift);
      sel[1] = krem - excl;
      sel[2] = (h == krem - excl) ? 1u : 0u;                         // the whole bucket is admitted: the walk ends here
    }
    __syncthreads();
    prefix = sel[0];
    krem = sel[1];
    mask |= 255u << shift;
    const bool done = sel[2] != 0;
    __syncthreads();                                                 // sel and scan_ws are rewritten by the next pass
    if (done) break;
  }
  const uint32_t n_gt = (uint32_t)k - krem;                          // (key & mask) > prefix: all admitted; == prefix: krem of them

  // ---- 3. compaction in column order ----
  const int ngroups = (cols + 63) >> 6;
  for (int c = 0; c * TK_THREADS < cols; ++c) {
    const int i = c * TK_THREADS + tid;
    const uint32_t mk = i < cols ? (topk_key(row[i]) & mask) : 0u;
    const unsigned long long bgt = __ballot(i < cols && mk > prefix);
    const unsigned long long beq = __ballot(i < cols && mk == prefix);
    const int g = 4 * c + wave;
    if (lane == 0 && g < ngroups) grp[g] = (uint32_t)__popcll(bgt) | ((uint32_t)__popcll(beq) << 16);
  }
  __syncthreads();
  {
    const int g0 = 2 * tid;
    const uint32_t a = g0 < ngroups ? grp[g0] : 0u;
    const uint32_t b = g0 + 1 < ngroups ? grp[g0 + 1] : 0u;
    const uint32_t incl = block_incl_scan(a + b, scan_ws);           // gt sums < 256, eq sums <= 32768: the halves never carry
    if (g0 < ngroups) grp[g0] = incl - a - b;
    if (g0 + 1 < ngroups) grp[g0 + 1] = incl - b;
  }
  for (int j = k + tid; j < sort_n; j += TK_THREADS) sv[j] = 0ull;   // padding: below every real entry
  __syncthreads();
  for (int c = 0; c * TK_THREADS < cols; ++c) {
    const int i = c * TK_THREADS + tid;
    const uint32_t key = i < cols ? topk_key(row[i]) : 0u;
    const uint32_t mk = key & mask;
    const bool gt = i < cols && mk > prefix, eq = i < cols && mk == prefix;
    const unsigned long long bgt = __ballot(gt);
    const unsigned long long beq = __ballot(eq);
    if (gt || eq) {
      const uint32_t base = grp[4 * c + wave];
      const uint32_t slot = gt ? (base & 0xffffu) + lanes_below(bgt) : n_gt + (base >> 16) + lanes_below(beq);
      if (slot < (uint32_t)k) sv[slot] = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)i;
    }
  }

  // ---- 4. bitonic sort, descending ----
  for (int size = 2; size <= sort_n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      if (tid < (sort_n >> 1)) {
        const int lo = 2 * tid - (tid & (stride - 1));
        const int hi = lo + stride;
        const unsigned long long a = sv[lo], b = sv[hi];
        if ((a < b) == ((lo & size) == 0)) {
          sv[lo] = b;
          sv[hi] = a;
        }
      }
    }
  }
  __syncthreads();

  // ---- 5. stores ----
  const long o = (long)blockIdx.x * k;
  for (int j = tid; j < k; j += TK_THREADS) {
    const uint32_t col = ~(uint32_t)sv[j];
    out_idx[o + j] = (int32_t)col;
    out_val[o + j] = __uint_as_float(row[col]);
  }
}

}  // namespace

extern "C" int evc_topk_rows(const float* x, int ld, int rows, int cols, int k, float* out_val, int32_t* out_idx, void* stream) {
  EVC_REQUIRE(cols >= 1 && cols <= TK_MAX_COLS, EVC_ERR_BAD_ARG, "evc_topk_rows: cols=%d (1 .. %d)", cols, TK_MAX_COLS);
  EVC_REQUIRE(k >= 1 && k <= cols && k <= TK_MAX_K, EVC_ERR_BAD_ARG, "evc_topk_rows: k=%d (1 .. min(cols=%d, %d))", k, cols, TK_MAX_K);
  EVC_REQUIRE(ld >= cols, EVC_ERR_BAD_ARG, "evc_topk_rows: ld=%d < cols=%d", ld, cols);
  EVC_REQUIRE(rows >= 0, EVC_ERR_BAD_ARG, "evc_topk_rows: rows=%d", rows);
  if (rows == 0) return EVC_OK;
  EVC_REQUIRE(x != nullptr && out_val != nullptr && out_idx != nullptr, EVC_ERR_BAD_ARG, "evc_topk_rows: NULL argument");
  int sort_n = 1;
  while (sort_n < k) sort_n <<= 1;
  const size_t lds = (size_t)TK_OFF_ROW + (size_t)((cols + 3) & ~3) * sizeof(uint32_t);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)topk_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TK_MAX_LDS);
  });
  hipLaunchKernelGGL(topk_rows_kernel, dim3(rows), dim3(TK_THREADS), lds, (hipStream_t)stream, x, (long)ld, cols, k, sort_n, out_val,
                     out_idx);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

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
//
// evc_eval_select_rows runs the same steps (shared __device__ helpers) for the evaluation binaries and adds what Hit@1 / PERR /
// mAP need from the label row - the labels of the selected columns, the row's positive count, the PERR numerator and the
// per-class positive counts - so that validate.py fetches [rows, k] + a few [rows] vectors instead of two [rows, cols] matrices.
//
// evc_ensemble_topk_rows puts a combination in front of the same steps: the rows of M member matrices are loaded by the thread that owns the
// column group, combined in registers (per-class maximum in the total order, or a weighted mean with one rounding per operation) and written
// to the LDS row once; the sparse lists of P earlier prediction files are then applied to that row, one file after another; the combined row
// is selected from and / or stored whole.
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
constexpr int EV_MAX_LDS = TK_MAX_LDS + TK_GROUPS * 8;              // eval_select_rows_kernel: + one label bit per column behind the row

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

// ---- the steps of the selection, shared by topk_rows_kernel and eval_select_rows_kernel (whole block calls each) ----

// 1. row -> LDS as raw bits, digit histogram of radix pass 0 on the way.  hist is zeroed and synchronised by the caller, which
// also synchronises afterwards.
__device__ __forceinline__ void tk_load_row(const uint32_t* __restrict__ xr, int cols, uint32_t* row, uint32_t* hist) {
  const int tid = threadIdx.x;
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
}

// 2. radix select of the k-th key (1 <= k <= cols, block-uniform) of the row in LDS: (key & mask) > prefix are admitted whole
// (k - krem of them), (key & mask) == prefix are the ties of which krem are admitted.  hist0_ready: hist already holds the digit
// histogram of pass 0 (tk_load_row).  Leaves hist, scan_ws and sel free again (a barrier ends it).
__device__ __forceinline__ void tk_radix_select(const uint32_t* row, int cols, uint32_t k, bool hist0_ready, uint32_t* hist,
                                                uint32_t* scan_ws, uint32_t* sel, uint32_t& prefix, uint32_t& mask, uint32_t& krem) {
  const int tid = threadIdx.x;
  prefix = 0;
  mask = 0;
  krem = k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (pass > 0 || !hist0_ready) {
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
}

// 3a. per 64-column group the counts of (key & mask) > prefix and == prefix from ballots, then their exclusive prefix over the
// groups in column order: grp[g] = gt | eq << 16 (gt sums < cols <= 32768, eq sums <= 32768: the halves never carry).  The caller
// synchronises before it reads grp.
__device__ __forceinline__ void tk_group_prefix(const uint32_t* row, int cols, uint32_t prefix, uint32_t mask, uint32_t* grp,
                                                uint32_t* scan_ws) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  const int g0 = 2 * tid;
  const uint32_t a = g0 < ngroups ? grp[g0] : 0u;
  const uint32_t b = g0 + 1 < ngroups ? grp[g0 + 1] : 0u;
  const uint32_t incl = block_incl_scan(a + b, scan_ws);
  if (g0 < ngroups) grp[g0] = incl - a - b;
  if (g0 + 1 < ngroups) grp[g0 + 1] = incl - b;
}

// 3b. compaction in column order into sv[0 .. k): slot = group base + mbcnt; ties are admitted lowest columns first.
__device__ __forceinline__ void tk_compact(const uint32_t* row, int cols, int k, uint32_t prefix, uint32_t mask, uint32_t n_gt,
                                           const uint32_t* grp, unsigned long long* sv) {
  const int tid = threadIdx.x, wave = tid >> 6;
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
}

// 4. bitonic sort of sv[0 .. sort_n), descending; a barrier ends it.
__device__ __forceinline__ void tk_sort_desc(unsigned long long* sv, int sort_n) {
  const int tid = threadIdx.x;
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
}

// Steps 2 - 4 for the row in LDS (hist0_ready: hist holds the pass-0 histogram): sv[0 .. k) = the k first elements in the total order,
// sorted.
__device__ __forceinline__ void tk_select_sorted(const uint32_t* row, int cols, int k, int sort_n, unsigned long long* sv, uint32_t* hist,
                                                 uint32_t* grp, uint32_t* scan_ws, uint32_t* sel, bool hist0_ready = true) {
  uint32_t prefix, mask, krem;
  tk_radix_select(row, cols, (uint32_t)k, hist0_ready, hist, scan_ws, sel, prefix, mask, krem);
  const uint32_t n_gt = (uint32_t)k - krem;                          // (key & mask) > prefix: all admitted; == prefix: krem of them
  tk_group_prefix(row, cols, prefix, mask, grp, scan_ws);
  for (int j = k + threadIdx.x; j < sort_n; j += TK_THREADS) sv[j] = 0ull;   // padding: below every real entry
  __syncthreads();
  tk_compact(row, cols, k, prefix, mask, n_gt, grp, sv);
  tk_sort_desc(sv, sort_n);
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
  const int tid = threadIdx.x;

  hist[tid] = 0;
  __syncthreads();
  tk_load_row((const uint32_t*)(x + (long)blockIdx.x * ld), cols, row, hist);
  __syncthreads();
  tk_select_sorted(row, cols, k, sort_n, sv, hist, grp, scan_ws, sel);

  // ---- 5. stores ----
  const long o = (long)blockIdx.x * k;
  for (int j = tid; j < k; j += TK_THREADS) {
    const uint32_t col = ~(uint32_t)sv[j];
    out_idx[o + j] = (int32_t)col;
    out_val[o + j] = __uint_as_float(row[col]);
  }
}

// evc_eval_select_rows: the selection above plus what Hit@1 / PERR / the per-class positive counts need from the label row.
// The label row is read once (one byte per thread, coalesced) into a bit per column in LDS behind the row; its population count
// n_pos is the k' of a second radix select over the same row in LDS, after which the PERR numerator is a ballot count:
// positives with a value > 0 above the threshold, plus those among the admitted ties (lowest columns first) - no sort.
__global__ __launch_bounds__(TK_THREADS) void eval_select_rows_kernel(const float* __restrict__ x, long ld, const uint8_t* __restrict__ labels,
                                                                      long ld_lab, int cols, int k, int sort_n, float* __restrict__ top_val,
                                                                      int32_t* __restrict__ top_idx, uint8_t* __restrict__ top_lab,
                                                                      int32_t* __restrict__ n_pos, int32_t* __restrict__ perr_hits,
                                                                      int32_t* __restrict__ class_pos) {
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  unsigned long long* sv = (unsigned long long*)tk_lds;
  uint32_t* hist = (uint32_t*)(tk_lds + TK_OFF_HIST);
  uint32_t* grp = (uint32_t*)(tk_lds + TK_OFF_GRP);
  uint32_t* scan_ws = (uint32_t*)(tk_lds + TK_OFF_MISC);
  uint32_t* sel = scan_ws + 4;
  uint32_t* wave_pos = scan_ws + 8;                                  // [4] positives seen by each wave
  uint32_t* wave_hits = scan_ws + 12;                                // [4] PERR hits seen by each wave
  uint32_t* row = (uint32_t*)(tk_lds + TK_OFF_ROW);
  uint32_t* lab = row + ((cols + 3) & ~3);                           // [2 * groups] label != 0, one bit per column
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ngroups = (cols + 63) >> 6;

  hist[tid] = 0;
  __syncthreads();
  tk_load_row((const uint32_t*)(x + (long)blockIdx.x * ld), cols, row, hist);
  {
    const uint8_t* lr = labels + (long)blockIdx.x * ld_lab;
    uint32_t seen = 0;                                               // wave-uniform
    for (int c = 0; c * TK_THREADS < cols; ++c) {
      const int i = c * TK_THREADS + tid;
      const bool on = i < cols && lr[i] != 0;
      const unsigned long long b = __ballot(on);
      seen += (uint32_t)__popcll(b);
      const int g = 4 * c + wave;
      if (lane == 0 && g < ngroups) {
        lab[2 * g] = (uint32_t)b;
        lab[2 * g + 1] = (uint32_t)(b >> 32);
      }
      if (on && class_pos != nullptr) atomicAdd(&class_pos[i], 1);   // integer: the sum does not depend on the order
    }
    if (lane == 0) wave_pos[wave] = seen;
  }
  __syncthreads();
  tk_select_sorted(row, cols, k, sort_n, sv, hist, grp, scan_ws, sel);

  const long o = (long)blockIdx.x * k;
  for (int j = tid; j < k; j += TK_THREADS) {
    const uint32_t col = ~(uint32_t)sv[j];
    top_idx[o + j] = (int32_t)col;
    top_val[o + j] = __uint_as_float(row[col]);
    top_lab[o + j] = (uint8_t)((lab[col >> 5] >> (col & 31)) & 1u);
  }

  // ---- PERR numerator: the first n_pos columns of the same total order ----
  const uint32_t npos = wave_pos[0] + wave_pos[1] + wave_pos[2] + wave_pos[3];   // block-uniform, <= cols
  uint32_t hits = 0;                                                 // wave-uniform
  if (npos > 0) {
    uint32_t prefix, mask, krem;
    tk_radix_select(row, cols, npos, false, hist, scan_ws, sel, prefix, mask, krem);
    tk_group_prefix(row, cols, prefix, mask, grp, scan_ws);
    __syncthreads();
    for (int c = 0; c * TK_THREADS < cols; ++c) {
      const int i = c * TK_THREADS + tid;
      const uint32_t u = i < cols ? row[i] : 0u;
      const uint32_t mk = topk_key(u) & mask;
      const bool gt = i < cols && mk > prefix, eq = i < cols && mk == prefix;
      const unsigned long long beq = __ballot(eq);
      const bool admitted = gt || (eq && (grp[4 * c + wave] >> 16) + lanes_below(beq) < krem);
      const uint32_t key = topk_key(u);
      const bool hit = admitted && ((lab[i >> 5] >> (i & 31)) & 1u) != 0 && key > 0x80000000u && key != 0xffffffffu;   // value > 0, not NaN
      hits += (uint32_t)__popcll(__ballot(hit));
    }
  }
  if (lane == 0) wave_hits[wave] = hits;
  __syncthreads();
  if (tid == 0) {
    n_pos[blockIdx.x] = (int32_t)npos;
    perr_hits[blockIdx.x] = (int32_t)(wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3]);
  }
}

// evc_ensemble_topk_rows: the combination of M member prediction matrices (and P sparse prior lists) in front of the selection above.
// The host arrays of the entry (member pointers, row strides, weights) travel by value in the kernel's argument block.
constexpr int ENS_MAX_M = 8;
constexpr int ENS_MAX_P = 8;
constexpr int ENS_MAX_KP = 256;
struct EnsArgs {
  const uint32_t* pred[ENS_MAX_M];
  long ld[ENS_MAX_M];
  float w[ENS_MAX_M + ENS_MAX_P];
};

// acc + w * x with the product and the sum each rounded to f32 (hipcc contracts a * b + c into one FMA by default, and its __fmul_rn /
// __fadd_rn are plain operators that contract as well: contraction is switched off for these two functions).
__device__ __forceinline__ float ens_mul(float w, float x) {
#pragma clang fp contract(off)
  return w * x;
}
__device__ __forceinline__ float ens_mul_add(float acc, float w, float x) {
#pragma clang fp contract(off)
  const float p = w * x;
  return acc + p;
}

// One element of the combined row from the M member values (static indices after unrolling: x stays in registers).
// mode 0: the value with the largest topk_key, the lowest member on equal keys; mode 1: w0 x0 + w1 x1 + ... left to right, every
// product and every sum rounded to f32 on its own (ens_mul / ens_mul_add).
__device__ __forceinline__ uint32_t ens_combine(const uint32_t (&x)[ENS_MAX_M], const EnsArgs& a, int M, int mode) {
  if (mode == 0) {
    uint32_t best = x[0], bk = topk_key(x[0]);
#pragma unroll
    for (int m = 1; m < ENS_MAX_M; ++m) {
      if (m < M) {
        const uint32_t km = topk_key(x[m]);
        if (km > bk) {
          best = x[m];
          bk = km;
        }
      }
    }
    return best;
  }
  float acc = ens_mul(a.w[0], __uint_as_float(x[0]));
#pragma unroll
  for (int m = 1; m < ENS_MAX_M; ++m)
    if (m < M) acc = ens_mul_add(acc, a.w[m], __uint_as_float(x[m]));
  return __float_as_uint(acc);
}

__global__ __launch_bounds__(TK_THREADS) void ensemble_topk_rows_kernel(const EnsArgs a, int M, const int32_t* __restrict__ prior_idx,
                                                                        const float* __restrict__ prior_val, int P, int kp, int rows, int cols,
                                                                        int mode, int k, int sort_n, float* __restrict__ out_val,
                                                                        int32_t* __restrict__ out_idx, float* __restrict__ out_dense,
                                                                        long ld_dense) {
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  unsigned long long* sv = (unsigned long long*)tk_lds;
  uint32_t* hist = (uint32_t*)(tk_lds + TK_OFF_HIST);
  uint32_t* grp = (uint32_t*)(tk_lds + TK_OFF_GRP);
  uint32_t* scan_ws = (uint32_t*)(tk_lds + TK_OFF_MISC);
  uint32_t* sel = scan_ws + 4;
  uint32_t* row = (uint32_t*)(tk_lds + TK_OFF_ROW);                  // [cols] raw bits of the combined row
  const int tid = threadIdx.x;
  const long r = blockIdx.x;
  const bool hist0 = P == 0 && k > 0;                                // the pass-0 histogram comes from the combined registers

  hist[tid] = 0;
  __syncthreads();

  // ---- 1. the M member rows -> one combined row in LDS; a thread owns the same columns in every member ----
  const uint32_t* xr[ENS_MAX_M];
  bool al[ENS_MAX_M];
#pragma unroll
  for (int m = 0; m < ENS_MAX_M; ++m) {
    xr[m] = m < M ? a.pred[m] + r * a.ld[m] : nullptr;
    al[m] = (((uintptr_t)xr[m]) & 15) == 0;
  }
  const int n4 = cols >> 2;
  for (int i = tid; i < n4; i += TK_THREADS) {
    u32x4_t v[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {                            // the M loads of the column group, back to back
      if (m < M) {
        if (al[m]) {
          v[m] = *(const u32x4_t*)(xr[m] + 4 * i);
        } else {                                                     // this member's rows are not 16-byte aligned
          const uint32_t* q = xr[m] + 4 * i;
          v[m] = u32x4_t{q[0], q[1], q[2], q[3]};
        }
      }
    }
    u32x4_t c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t x[ENS_MAX_M];
#pragma unroll
      for (int m = 0; m < ENS_MAX_M; ++m) x[m] = m < M ? v[m][j] : 0u;
      c[j] = ens_combine(x, a, M, mode);
    }
    *(u32x4_t*)(row + 4 * i) = c;
    if (hist0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&hist[topk_key(c[j]) >> 24], 1u);
    }
  }
  for (int i = 4 * n4 + tid; i < cols; i += TK_THREADS) {
    uint32_t x[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) x[m] = m < M ? xr[m][i] : 0u;
    const uint32_t c = ens_combine(x, a, M, mode);
    row[i] = c;
    if (hist0) atomicAdd(&hist[topk_key(c) >> 24], 1u);
  }
  __syncthreads();

  // ---- 1b. the sparse prior lists of this row, one file after another (indices within a list are distinct: no two threads of a
  // file meet in one column); an index outside [0, cols) is padding ----
  for (int p = 0; p < P; ++p) {
    const long o = ((long)p * rows + r) * kp;
    const float w = mode == 1 ? a.w[M + p] : 0.f;
    for (int e = tid; e < kp; e += TK_THREADS) {
      const int32_t c = prior_idx[o + e];
      if (c >= 0 && c < cols) {
        const float val = prior_val[o + e];
        if (mode == 0) {
          if (topk_key(__float_as_uint(val)) > topk_key(row[c])) row[c] = __float_as_uint(val);
        } else {
          row[c] = __float_as_uint(ens_mul_add(__uint_as_float(row[c]), w, val));
        }
      }
    }
    __syncthreads();
  }

  // ---- the dense exit: the combined row as it stands in LDS ----
  if (out_dense != nullptr) {
    uint32_t* d = (uint32_t*)out_dense + r * ld_dense;
    if ((((uintptr_t)d) & 15) == 0) {
      for (int i = tid; i < n4; i += TK_THREADS) *(u32x4_t*)(d + 4 * i) = *(const u32x4_t*)(row + 4 * i);
      for (int i = 4 * n4 + tid; i < cols; i += TK_THREADS) d[i] = row[i];
    } else {
      for (int i = tid; i < cols; i += TK_THREADS) d[i] = row[i];
    }
  }
  if (k == 0) return;                                                // block-uniform

  tk_select_sorted(row, cols, k, sort_n, sv, hist, grp, scan_ws, sel, hist0);
  const long o = r * k;
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

extern "C" int evc_eval_select_rows(const float* pred, int ld, const uint8_t* labels, int ld_lab, int rows, int cols, int k, float* top_val,
                                    int32_t* top_idx, uint8_t* top_lab, int32_t* n_pos, int32_t* perr_hits, int32_t* class_pos,
                                    void* stream) {
  EVC_REQUIRE(cols >= 1 && cols <= TK_MAX_COLS, EVC_ERR_BAD_ARG, "evc_eval_select_rows: cols=%d (1 .. %d)", cols, TK_MAX_COLS);
  EVC_REQUIRE(k >= 1 && k <= cols && k <= TK_MAX_K, EVC_ERR_BAD_ARG, "evc_eval_select_rows: k=%d (1 .. min(cols=%d, %d))", k, cols, TK_MAX_K);
  EVC_REQUIRE(ld >= cols, EVC_ERR_BAD_ARG, "evc_eval_select_rows: ld=%d < cols=%d", ld, cols);
  EVC_REQUIRE(ld_lab >= cols, EVC_ERR_BAD_ARG, "evc_eval_select_rows: ld_lab=%d < cols=%d", ld_lab, cols);
  EVC_REQUIRE(rows >= 0, EVC_ERR_BAD_ARG, "evc_eval_select_rows: rows=%d", rows);
  if (rows == 0) return EVC_OK;
  EVC_REQUIRE(pred != nullptr && labels != nullptr && top_val != nullptr && top_idx != nullptr && top_lab != nullptr && n_pos != nullptr &&
                  perr_hits != nullptr,
              EVC_ERR_BAD_ARG, "evc_eval_select_rows: NULL argument");
  int sort_n = 1;
  while (sort_n < k) sort_n <<= 1;
  const size_t lds = (size_t)TK_OFF_ROW + (size_t)((cols + 3) & ~3) * sizeof(uint32_t) + (size_t)((cols + 63) >> 6) * 8;
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)eval_select_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, EV_MAX_LDS);
  });
  hipLaunchKernelGGL(eval_select_rows_kernel, dim3(rows), dim3(TK_THREADS), lds, (hipStream_t)stream, pred, (long)ld, labels, (long)ld_lab,
                     cols, k, sort_n, top_val, top_idx, top_lab, n_pos, perr_hits, class_pos);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_ensemble_topk_rows(const float* const* preds, const int64_t* ld, const float* weights, int M, const int32_t* prior_idx,
                                      const float* prior_val, int P, int kp, int rows, int cols, int mode, int k, float* out_val,
                                      int32_t* out_idx, float* out_dense, int64_t ld_dense, void* stream) {
  EVC_REQUIRE(M >= 1 && M <= ENS_MAX_M, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: M=%d (1 .. %d)", M, ENS_MAX_M);
  EVC_REQUIRE(P >= 0 && P <= ENS_MAX_P, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: P=%d (0 .. %d)", P, ENS_MAX_P);
  EVC_REQUIRE(P == 0 || (kp >= 1 && kp <= ENS_MAX_KP), EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: kp=%d (1 .. %d)", kp, ENS_MAX_KP);
  EVC_REQUIRE(mode == 0 || mode == 1, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: mode=%d (0 = max, 1 = weighted mean)", mode);
  EVC_REQUIRE(cols >= 1 && cols <= TK_MAX_COLS, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: cols=%d (1 .. %d)", cols, TK_MAX_COLS);
  EVC_REQUIRE(k >= 0 && k <= cols && k <= TK_MAX_K, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: k=%d (0 .. min(cols=%d, %d))", k, cols, TK_MAX_K);
  EVC_REQUIRE(rows >= 0, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: rows=%d", rows);
  EVC_REQUIRE(preds != nullptr && ld != nullptr && (mode == 0 || weights != nullptr), EVC_ERR_BAD_ARG,
              "evc_ensemble_topk_rows: NULL host array");
  for (int m = 0; m < M; ++m)
    EVC_REQUIRE(ld[m] >= cols, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: ld[%d]=%lld < cols=%d", m, (long long)ld[m], cols);
  EVC_REQUIRE(out_dense == nullptr || ld_dense >= cols, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: ld_dense=%lld < cols=%d",
              (long long)ld_dense, cols);
  if (rows == 0) return EVC_OK;                                      // (an empty tensor's pointer may be NULL: the pointers are looked at below)
  if (k == 0)
    EVC_REQUIRE(out_val == nullptr && out_idx == nullptr && out_dense != nullptr, EVC_ERR_BAD_ARG,
                "evc_ensemble_topk_rows: k=0 takes out_val = out_idx = NULL and a dense output");
  else
    EVC_REQUIRE(out_val != nullptr && out_idx != nullptr, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: NULL argument");
  for (int m = 0; m < M; ++m) EVC_REQUIRE(preds[m] != nullptr, EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: NULL member %d", m);
  EVC_REQUIRE(P == 0 || (prior_idx != nullptr && prior_val != nullptr), EVC_ERR_BAD_ARG, "evc_ensemble_topk_rows: NULL prior lists");
  EnsArgs a;
  memset(&a, 0, sizeof(a));
  for (int m = 0; m < M; ++m) {
    a.pred[m] = (const uint32_t*)preds[m];
    a.ld[m] = (long)ld[m];
  }
  if (mode == 1)
    for (int j = 0; j < M + P; ++j) a.w[j] = weights[j];
  int sort_n = 1;
  while (sort_n < k) sort_n <<= 1;
  const size_t lds = (size_t)TK_OFF_ROW + (size_t)((cols + 3) & ~3) * sizeof(uint32_t);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)ensemble_topk_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TK_MAX_LDS);
  });
  hipLaunchKernelGGL(ensemble_topk_rows_kernel, dim3(rows), dim3(TK_THREADS), lds, (hipStream_t)stream, a, M, prior_idx, prior_val, P, kp,
                     rows, cols, mode, k, sort_n, out_val, out_idx, out_dense, (long)ld_dense);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

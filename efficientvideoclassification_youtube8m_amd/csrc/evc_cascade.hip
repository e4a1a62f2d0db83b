// Confidence cascade (evc_cascade_confidence_rows, evc_cascade_pick_rows): the gate between two stages of cascade.CascadeGraph.
// A cheap tower predicts the whole batch, the gate measures how sure each row is, and only the unsure rows go on to the next tower.
//
// evc_cascade_confidence_rows, one 256-thread workgroup per row (the grid strides over the rows), rows whose `active` byte is 0 skipped whole:
//   the row is read from HBM once (16 bytes per lane when the stage's row and the merged row both start on a 16-byte boundary, 4 bytes
//   otherwise - decided per row); every loaded register goes straight to the merged row and into the thread's two largest order-preserving
//   keys; wave64 shuffles join the lanes' pairs, four LDS words the waves'; thread 0 decodes the keys, subtracts once and stores conf / stage_of.
// evc_cascade_pick_rows, one workgroup: the candidates' keys (NaN lowest, -0 = +0, ascending) are staged in LDS; when a cap is given and
//   exceeded, a radix select (4 passes of 8 bits, integer LDS histogram) finds the key of the last admitted row and the number of rows with
//   exactly that key that are admitted, lowest rows first (ballot counts per 64 rows + one scan).  Integer arithmetic only: every launch gives
//   the same bits.
// No atomics on global memory, no float atomics, no scratch; every store is an ordinary vector store.
#include "evc_common.h"

#include <mutex>

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_MAX_COLS = 32768;
constexpr int CS_MAX_ROWS = 16384;                                   // evc_cascade_pick_rows: the keys of one batch in LDS
constexpr int CS_MAX_GRID = 4096;
constexpr uint32_t CS_NAN = 0x7fc00000u;
constexpr uint32_t CS_NOT_CANDIDATE = 0xffffffffu;                    // above the key of +inf (0xff800000): no row's key
// dynamic LDS carve of pick_rows_kernel (every offset a multiple of 16): histogram | group counts | scan words | keys
constexpr int CS_OFF_GRP = 256 * 4;
constexpr int CS_OFF_MISC = CS_OFF_GRP + 256 * 4;
constexpr int CS_OFF_KEYS = CS_OFF_MISC + 64;
constexpr int CS_MAX_LDS = CS_OFF_KEYS + CS_MAX_ROWS * 4;

// Order-preserving key of a non-NaN f32, larger value = larger key; +0 ranks above -0 (IEEE 754-2019 maximum).  Every real key is > 0:
// 0 stands for "no value yet".
__device__ __forceinline__ uint32_t conf_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t conf_unkey(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
__device__ __forceinline__ bool is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }

// the two largest keys, duplicates counted: (k1 >= k2)
__device__ __forceinline__ void top2_insert(uint32_t k, uint32_t& k1, uint32_t& k2) {
  const uint32_t lo = k < k1 ? k : k1;                               // (min / max, no branch: a branch on k1 / k2 sends the pair to scratch)
  k2 = k2 > lo ? k2 : lo;
  k1 = k1 > k ? k1 : k;
}
__device__ __forceinline__ void top2_merge(uint32_t b1, uint32_t b2, uint32_t& k1, uint32_t& k2) {
  const uint32_t lo = k1 < b1 ? k1 : b1, hi2 = k2 > b2 ? k2 : b2;
  k1 = k1 > b1 ? k1 : b1;
  k2 = lo > hi2 ? lo : hi2;
}

__global__ __launch_bounds__(CS_THREADS) void cascade_confidence_rows_kernel(const uint32_t* __restrict__ pred, long ld,
                                                                             const uint8_t* __restrict__ active, int rows, int cols, int kind,
                                                                             int stage, float* __restrict__ conf, uint32_t* __restrict__ merged,
                                                                             long ld_merged, uint8_t* __restrict__ stage_of) {
  __shared__ uint32_t w1[4], w2[4], wnan[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    if (active != nullptr && active[r] == 0) continue;                // block-uniform: nothing of this row is read or written
    const uint32_t* xr = pred + (long)r * ld;
    uint32_t* mr = merged + (long)r * ld_merged;
    uint32_t k1 = 0, k2 = 0;
    bool nan = false;
    if (((((uintptr_t)xr) | ((uintptr_t)mr)) & 15) == 0) {
      const int n4 = cols >> 2;
      for (int i = tid; i < n4; i += CS_THREADS) {
        const u32x4_t v = *(const u32x4_t*)(xr + 4 * i);
        *(u32x4_t*)(mr + 4 * i) = v;
        nan |= is_nan_bits(v.x) | is_nan_bits(v.y) | is_nan_bits(v.z) | is_nan_bits(v.w);
        top2_insert(conf_key(v.x), k1, k2);
        top2_insert(conf_key(v.y), k1, k2);
        top2_insert(conf_key(v.z), k1, k2);
        top2_insert(conf_key(v.w), k1, k2);
      }
      for (int i = 4 * n4 + tid; i < cols; i += CS_THREADS) {
        const uint32_t u = xr[i];
        mr[i] = u;
        nan |= is_nan_bits(u);
        top2_insert(conf_key(u), k1, k2);
      }
    } else {                                                         // a row that does not start on a 16-byte boundary
      for (int i = tid; i < cols; i += CS_THREADS) {
        const uint32_t u = xr[i];
        mr[i] = u;
        nan |= is_nan_bits(u);
        top2_insert(conf_key(u), k1, k2);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t b1 = (uint32_t)__shfl_xor((int)k1, o, 64), b2 = (uint32_t)__shfl_xor((int)k2, o, 64);
      top2_merge(b1, b2, k1, k2);
    }
    const bool wave_nan = __ballot(nan) != 0ull;
    if (lane == 0) {
      w1[wave] = k1;
      w2[wave] = k2;
      wnan[wave] = wave_nan ? 1u : 0u;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t a1 = w1[0], a2 = w2[0];
      for (int w = 1; w < 4; ++w) top2_merge(w1[w], w2[w], a1, a2);
      float out;
      if ((wnan[0] | wnan[1] | wnan[2] | wnan[3]) != 0u) {
        out = __uint_as_float(CS_NAN);
      } else if (kind == EVC_CONF_TOP1) {
        out = __uint_as_float(conf_unkey(a1));
      } else {
        const float m1 = __uint_as_float(conf_unkey(a1));
        const float m2 = cols == 1 ? 0.0f : __uint_as_float(conf_unkey(a2));
        out = m1 - m2;                                               // one f32 subtraction; inf - inf: NaN
        if (out != out) out = __uint_as_float(CS_NAN);
      }
      conf[r] = out;
      stage_of[r] = (uint8_t)stage;
    }
    __syncthreads();                                                 // the LDS words are rewritten by the block's next row
  }
}

// Ascending key of the pick: NaN = 0 (first), -0 = +0, then the value.  Real keys are <= 0xff800000.
__device__ __forceinline__ uint32_t pick_key(uint32_t u) {
  if (is_nan_bits(u)) return 0u;
  if (u == 0x80000000u) u = 0u;
  return conf_key(u);
}

// Inclusive scan of one value per thread over the 256-thread block; ws: 4 words of LDS.  Whole block calls it; the caller synchronises
// before ws is written again.
__device__ __forceinline__ uint32_t cs_block_incl_scan(uint32_t v, uint32_t* ws) {
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

__global__ __launch_bounds__(CS_THREADS) void cascade_pick_rows_kernel(const uint32_t* __restrict__ conf, const uint8_t* __restrict__ active,
                                                                       const int32_t* __restrict__ num_frames, int rows, float threshold,
                                                                       int max_rows, uint8_t* __restrict__ active_next,
                                                                       int32_t* __restrict__ num_frames_next, int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) char cs_lds[];
  uint32_t* hist = (uint32_t*)cs_lds;                                // [256]
  uint32_t* grp = (uint32_t*)(cs_lds + CS_OFF_GRP);                  // [rows / 64] ties per 64 rows, then their exclusive prefix
  uint32_t* scan_ws = (uint32_t*)(cs_lds + CS_OFF_MISC);             // [4]
  uint32_t* sel = scan_ws + 4;                                       // [2] prefix, rows still to admit
  uint32_t* wcnt = scan_ws + 8;                                      // [4] candidates seen by each wave
  uint32_t* keys = (uint32_t*)(cs_lds + CS_OFF_KEYS);                // [rows]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ngroups = (rows + 63) >> 6;                              // <= 256

  // ---- 1. the candidates: active rows for which conf >= threshold is false ----
  uint32_t seen = 0;                                                 // wave-uniform
  for (int c = 0; c * CS_THREADS < rows; ++c) {
    const int r = c * CS_THREADS + tid;
    bool cand = false;
    uint32_t u = 0;
    if (r < rows && (active == nullptr || active[r] != 0)) {
      u = conf[r];
      cand = !(__uint_as_float(u) >= threshold);
    }
    if (r < rows) keys[r] = cand ? pick_key(u) : CS_NOT_CANDIDATE;
    seen += (uint32_t)__popcll(__ballot(cand));
  }
  if (lane == 0) wcnt[wave] = seen;
  __syncthreads();
  const uint32_t n_cand = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];     // block-uniform
  const bool capped = max_rows >= 0 && n_cand > (uint32_t)max_rows;
  const uint32_t kept = capped ? (uint32_t)max_rows : n_cand;

  // ---- 2. capped: the key T of the last admitted row and the number of rows with key == T that are admitted ----
  uint32_t T = CS_NOT_CANDIDATE, need = 0;                           // not capped: every key below CS_NOT_CANDIDATE is admitted
  if (capped && kept > 0) {
    uint32_t prefix = 0, mask = 0, mrem = kept;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      for (int r = tid; r < rows; r += CS_THREADS) {
        const uint32_t key = keys[r];
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      const uint32_t h = hist[tid];                                  // thread t: digit t, ascending
      const uint32_t incl = cs_block_incl_scan(h, scan_ws);
      const uint32_t excl = incl - h;
      if (excl < mrem && incl >= mrem) {                             // exactly one thread (mrem <= the candidates under the prefix)
        sel[0] = prefix | ((uint32_t)tid << shift);
        sel[1] = mrem - excl;
      }
      __syncthreads();
      prefix = sel[0];
      mrem = sel[1];
      mask |= 255u << shift;
      __syncthreads();                                               // sel, scan_ws and hist are rewritten by the next pass
    }
    T = prefix;
    need = mrem;
  } else if (capped) {
    T = 0;                                                           // max_rows == 0: nothing is below key 0, and no tie is admitted
    need = 0;
  }

  // ---- 3. ties at T in row order: per 64 rows their count, one exclusive scan over the groups ----
  for (int c = 0; c * CS_THREADS < rows; ++c) {
    const int r = c * CS_THREADS + tid;
    const unsigned long long beq = __ballot(r < rows && keys[r] == T);
    const int g = 4 * c + wave;
    if (lane == 0 && g < ngroups) grp[g] = (uint32_t)__popcll(beq);
  }
  __syncthreads();
  {
    const uint32_t a = tid < ngroups ? grp[tid] : 0u;
    const uint32_t incl = cs_block_incl_scan(a, scan_ws);
    __syncthreads();
    if (tid < ngroups) grp[tid] = incl - a;
  }
  __syncthreads();

  // ---- 4. every row's outputs ----
  for (int c = 0; c * CS_THREADS < rows; ++c) {
    const int r = c * CS_THREADS + tid;
    const uint32_t key = r < rows ? keys[r] : CS_NOT_CANDIDATE;
    const bool eq = r < rows && key == T;
    const unsigned long long beq = __ballot(eq);
    if (r < rows) {
      bool keep;
      if (!capped) {
        keep = key != CS_NOT_CANDIDATE;
      } else {
        const uint32_t below = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(beq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)beq, 0u));
        keep = key < T || (eq && grp[4 * c + wave] + below < need);
      }
      active_next[r] = keep ? (uint8_t)1 : (uint8_t)0;
      num_frames_next[r] = keep ? num_frames[r] : 0;
    }
  }
  if (tid == 0) count[0] = (int32_t)kept;
}

}  // namespace

extern "C" int evc_cascade_confidence_rows(const float* pred, int64_t ld, const uint8_t* active, int rows, int cols, int kind, int stage,
                                           float* conf, float* merged, int64_t ld_merged, uint8_t* stage_of, void* stream) {
  EVC_REQUIRE(cols >= 1 && cols <= CS_MAX_COLS, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: cols=%d (1 .. %d)", cols, CS_MAX_COLS);
  EVC_REQUIRE(kind == EVC_CONF_TOP1 || kind == EVC_CONF_MARGIN, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: kind=%d (0 = top1, 1 = margin)", kind);
  EVC_REQUIRE(stage >= 0 && stage <= 255, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: stage=%d (0 .. 255)", stage);
  EVC_REQUIRE(ld >= cols, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: ld=%lld < cols=%d", (long long)ld, cols);
  EVC_REQUIRE(ld_merged >= cols, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: ld_merged=%lld < cols=%d", (long long)ld_merged, cols);
  EVC_REQUIRE(rows >= 0, EVC_ERR_BAD_ARG, "evc_cascade_confidence_rows: rows=%d", rows);
  if (rows == 0) return EVC_OK;
  EVC_REQUIRE(pred != nullptr && conf != nullptr && merged != nullptr && stage_of != nullptr, EVC_ERR_BAD_ARG,
              "evc_cascade_confidence_rows: NULL argument");
  const int grid = rows < CS_MAX_GRID ? rows : CS_MAX_GRID;
  hipLaunchKernelGGL(cascade_confidence_rows_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, (const uint32_t*)pred, (long)ld,
                     active, rows, cols, kind, stage, conf, (uint32_t*)merged, (long)ld_merged, stage_of);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_cascade_pick_rows(const float* conf, const uint8_t* active, const int32_t* num_frames, int rows, float threshold,
                                     int max_rows, uint8_t* active_next, int32_t* num_frames_next, int32_t* count, void* stream) {
  EVC_REQUIRE(rows >= 0, EVC_ERR_BAD_ARG, "evc_cascade_pick_rows: rows=%d", rows);
  EVC_REQUIRE(rows <= CS_MAX_ROWS, EVC_ERR_BAD_SHAPE, "evc_cascade_pick_rows: rows=%d (at most %d)", rows, CS_MAX_ROWS);
  EVC_REQUIRE(max_rows >= -1, EVC_ERR_BAD_ARG, "evc_cascade_pick_rows: max_rows=%d (-1 = no cap, or >= 0)", max_rows);
  if (rows == 0) return EVC_OK;
  EVC_REQUIRE(conf != nullptr && num_frames != nullptr && active_next != nullptr && num_frames_next != nullptr && count != nullptr,
              EVC_ERR_BAD_ARG, "evc_cascade_pick_rows: NULL argument");
  const size_t lds = (size_t)CS_OFF_KEYS + (size_t)((rows + 3) & ~3) * sizeof(uint32_t);
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)cascade_pick_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CS_MAX_LDS);
  });
  hipLaunchKernelGGL(cascade_pick_rows_kernel, dim3(1), dim3(CS_THREADS), lds, (hipStream_t)stream, (const uint32_t*)conf, active, num_frames,
                     rows, threshold, max_rows, active_next, num_frames_next, count);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

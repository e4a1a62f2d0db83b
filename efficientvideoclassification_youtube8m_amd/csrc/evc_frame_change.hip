// Content-aware student frames (--student_sampling change | segment_change): a score pass over the RAW frames that leaves one uint32 key
// per frame - the squared change from the frame before - and the selection that ranks by those keys.  Siblings of the kernels of
// evc_frame_select.hip, in a file of their own so that those keep their instructions.
#include "evc_common.h"

#define CHG_MAX_T 1024          // as evc_student_frame_select
#define CHG_RUN 8               // consecutive frames of one video per wave: the run's predecessor row is the only row read twice
#define CHG_MAX_F_U8 66051      // 66051 * 255^2 = 4294966275 <= 2^32 - 1 < 66052 * 255^2

typedef uint32_t chg_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
// sum over 4 bytes of a_i * b_i, added to c modulo 2^32 (v_dot4_u32_u8)
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
__device__ __forceinline__ uint32_t f32_key(float s) { return s != s ? 0xFFFFFFFFu : __float_as_uint(s); }

// Sum_f (q_t - q_p)^2 = Sum q_t^2 + Sum q_p^2 - 2 Sum q_t q_p: every term a dot-4, every sum modulo 2^32 - exact, because the result fits.
// The general forms: both rows from memory, by the widest access this row pair allows (wave-uniform choice).
__device__ __forceinline__ uint32_t change_u8_rows(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prv, int F, int lane) {
  uint32_t acc = 0;
  const uintptr_t al = (uintptr_t)cur | (uintptr_t)prv | (uintptr_t)(uint32_t)F;
  if ((al & 15) == 0) {
    const chg_u4 *c4 = (const chg_u4*)cur, *p4 = (const chg_u4*)prv;
    for (int j = lane; j < (F >> 4); j += 64) {
      const chg_u4 a = c4[j], b = p4[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = dot4(a[r], a[r], dot4(b[r], b[r], acc)) - 2u * dot4(a[r], b[r], 0u);
    }
  } else if ((al & 3) == 0) {
    const uint32_t *c1 = (const uint32_t*)cur, *p1 = (const uint32_t*)prv;
    for (int j = lane; j < (F >> 2); j += 64) {
      const uint32_t a = c1[j], b = p1[j];
      acc = dot4(a, a, dot4(b, b, acc)) - 2u * dot4(a, b, 0u);
    }
  } else {
    for (int j = lane; j < F; j += 64) {
      const int d = (int)cur[j] - (int)prv[j];
      acc += (uint32_t)(d * d);
    }
  }
  return wave_sum_u32(acc);
}
__device__ __forceinline__ float change_f32_rows(const float* __restrict__ cur, const float* __restrict__ prv, int F, int lane) {
  float acc = 0.f;
  const uintptr_t al = (uintptr_t)cur | (uintptr_t)prv;
  if ((al & 15) == 0 && (F & 3) == 0) {
    const float4 *c4 = (const float4*)cur, *p4 = (const float4*)prv;
    for (int j = lane; j < (F >> 2); j += 64) {
      const float4 a = c4[j], b = p4[j];
      const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
      acc += dx * dx; acc += dy * dy; acc += dz * dz; acc += dw * dw;
    }
  } else {
    for (int j = lane; j < F; j += 64) {
      const float d = cur[j] - prv[j];
      acc += d * d;
    }
  }
  return wave_sum(acc);
}

// One wave per run of CHG_RUN frames of one video.  NCH > 0: a row of at most NCH * 64 16-byte pieces that starts on a 16-byte boundary is
// kept in registers from one frame to the next (NCH pieces per lane), so each row comes from memory once per run; any other row pair
// takes the general form above.  One plain store per frame; no atomics, no scratch, no LDS.
template <bool U8, int NCH>
__global__ __launch_bounds__(256) void frame_change_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                           const int* __restrict__ nfr, int B, int T, int F, int runs,
                                                           uint32_t* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // b * runs + run
  if (w >= (long)B * runs) return;
  const int b = (int)(w / runs), t0 = (int)(w % runs) * CHG_RUN;
  int n = nfr[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  const int t1 = t0 + CHG_RUN < T ? t0 + CHG_RUN : T;            // this wave writes keys[b][t0 .. t1)
  const int tl = t1 < n ? t1 : n;                                // ... and reads the frames of [max(t0 - 1, 0), tl): all below n
  uint32_t* out = keys + (long)b * T;
  for (int t = (t0 > tl ? t0 : tl) + lane; t < t1; t += 64) out[t] = 0u;       // frames at or beyond n
  if (t0 >= tl) return;
  const size_t esz = U8 ? 1 : 4;
  const char* base = (U8 ? (const char*)xq : (const char*)x) + (size_t)b * T * F * esz;
  const size_t rowb = (size_t)F * esz;
  int t = t0;
  if (t == 0) {                                                  // the first frame opens the first shot
    if (lane == 0) out[0] = 0xFFFFFFFFu;
    t = 1;
  }
  const int nch = (int)(rowb >> 4);                              // 16-byte pieces of a row
  const bool regs = NCH > 0 && (rowb & 15) == 0 && (((uintptr_t)base) & 15) == 0 && nch <= NCH * 64;
  if (NCH > 0 && regs) {
    constexpr int N = NCH > 0 ? NCH : 1;
    chg_u4 prv[N], cur[N];
    uint32_t sq_prv = 0;                                         // this lane's share of Sum q_p^2 (uint8 only)
    if (t < tl) {
      const chg_u4* p = (const chg_u4*)(base + (size_t)(t - 1) * rowb);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int j = lane + i * 64;
        prv[i] = (chg_u4){0u, 0u, 0u, 0u};
        if (j < nch) prv[i] = p[j];
        if (U8) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sq_prv = dot4(prv[i][r], prv[i][r], sq_prv);
        }
      }
    }
    for (; t < tl; ++t) {
      const chg_u4* c = (const chg_u4*)(base + (size_t)t * rowb);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int j = lane + i * 64;
        cur[i] = (chg_u4){0u, 0u, 0u, 0u};
        if (j < nch) cur[i] = c[j];
      }
      uint32_t key;
      if (U8) {
        uint32_t sq = 0, cross = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            sq = dot4(cur[i][r], cur[i][r], sq);
            cross = dot4(cur[i][r], prv[i][r], cross);
          }
        }
        key = wave_sum_u32(sq + sq_prv - 2u * cross);
        sq_prv = sq;
      } else {
        float acc = 0.f;                                         // pieces in index order, x y z w inside a piece, then the wave's butterfly
#pragma unroll
        for (int i = 0; i < N; ++i) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d = __uint_as_float(cur[i][r]) - __uint_as_float(prv[i][r]);
            acc += d * d;
          }
        }
        key = f32_key(wave_sum(acc));
      }
      if (lane == 0) out[t] = key;
#pragma unroll
      for (int i = 0; i < N; ++i) prv[i] = cur[i];
    }
    return;
  }
  for (; t < tl; ++t) {
    const char *c = base + (size_t)t * rowb, *p = c - rowb;
    uint32_t key;
    if (U8) key = change_u8_rows((const uint8_t*)c, (const uint8_t*)p, F, lane);
    else key = f32_key(change_f32_rows((const float*)c, (const float*)p, F, lane));
    if (lane == 0) out[t] = key;
  }
}

extern "C" int evc_frame_change_keys(const float* x_f32, const uint8_t* x_u8, const int32_t* num_frames, int B, int T, int F,
                                     uint32_t* keys, void* stream) {
  EVC_REQUIRE(num_frames && keys, EVC_ERR_BAD_ARG, "evc_frame_change_keys: num_frames and keys are required");
  EVC_REQUIRE((x_f32 != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_frame_change_keys: exactly one of x_f32 / x_u8");
  EVC_REQUIRE(B > 0 && T > 0 && T <= CHG_MAX_T && F > 0, EVC_ERR_BAD_SHAPE, "evc_frame_change_keys: B=%d, T=%d (1 .. %d), F=%d", B, T, CHG_MAX_T, F);
  EVC_REQUIRE(!x_u8 || F <= CHG_MAX_F_U8, EVC_ERR_BAD_SHAPE,
              "evc_frame_change_keys: F=%d: the exact uint8 sum fits 32 bits up to F=%d only", F, CHG_MAX_F_U8);
  EVC_REQUIRE(!x_f32 || (((uintptr_t)x_f32) & 3) == 0, EVC_ERR_BAD_ARG, "evc_frame_change_keys: x_f32 is not aligned to 4 bytes");
  const int runs = ceil_div(T, CHG_RUN);
  const dim3 grid((unsigned)(((long)B * runs + 3) / 4)), block(256);
  const hipStream_t s = (hipStream_t)stream;
  const long rowb = (long)F * (x_u8 ? 1 : 4);
#define CHG_LAUNCH(U8, NCH) \
  hipLaunchKernelGGL((frame_change_kernel<U8, NCH>), grid, block, 0, s, x_f32, x_u8, num_frames, B, T, F, runs, keys)
  if (x_u8) {
    if (rowb <= 2 * 1024) CHG_LAUNCH(true, 2);
    else if (rowb <= 5 * 1024) CHG_LAUNCH(true, 5);
    else CHG_LAUNCH(true, 0);
  } else {
    if (rowb <= 2 * 1024) CHG_LAUNCH(false, 2);
    else if (rowb <= 5 * 1024) CHG_LAUNCH(false, 5);
    else CHG_LAUNCH(false, 0);
  }
#undef CHG_LAUNCH
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// scored selection: one workgroup per video, the keys staged in LDS; no atomics, no scratch
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void frame_select_scored_kernel(const int* __restrict__ nfr, const uint32_t* __restrict__ keys, int T,
                                                                  int every_n, int strategy, int* __restrict__ src) {
  __shared__ uint32_t key[CHG_MAX_T];
  __shared__ int wave_cnt[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = T / every_n;
  int* out = src + (long)b * S;
  int n = nfr[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  // the student's frame count, as frame_select_kernel: float64 true division, truncation (n - 1 at every_n = 1 for n = 55, 79, ...)
  const double q = (double)n / (double)T;
  const int k = (int)(long long)trunc(q * (double)S);         // k <= n because S <= T
  for (int t = tid; t < n; t += 256) key[t] = keys[(long)b * T + t];
  for (int j = k + tid; j < S; j += 256) out[j] = -1;
  __syncthreads();
  if (strategy == EVC_SELECT_SEGMENT_CHANGE) {
    // segment j = [j n / k, (j + 1) n / k): non-empty because k <= n; its frame of largest key, the smallest t on ties
    for (int j = tid; j < k; j += 256) {
      const int lo = (int)((long)j * n / k), hi = (int)((long)(j + 1) * n / k);
      int best = lo;
      uint32_t kb = key[lo];
      for (int t = lo + 1; t < hi; ++t) {
        const uint32_t kt = key[t];
        if (kt > kb) { kb = kt; best = t; }
      }
      out[j] = best;
    }
    return;
  }
  // change: the k frames of [0, n) with the largest (key, then smaller t), in ascending t.  Ranks by counting in LDS, compaction by ballots.
  int base = 0;                                                // selected frames below this pass's 256 (uniform over the workgroup)
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int t = t0 + tid;
    bool take = false;
    if (t < n) {
      const uint32_t kt = key[t];
      int rank = 0;
      for (int u = 0; u < n; ++u) {                            // every lane reads the same word: a broadcast
        const uint32_t ku = key[u];
        rank += (ku > kt || (ku == kt && u < t)) ? 1 : 0;
      }
      take = rank < k;
    }
    const unsigned long long m = __ballot(take);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = base, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (take) out[before + __popcll(m & ((1ull << lane) - 1ull))] = t;     // position < k: exactly k frames have rank < k
    base += total;
    __syncthreads();
  }
}

extern "C" int evc_student_frame_select_scored(const int32_t* num_frames, const uint32_t* keys, int B, int T, int every_n, int strategy,
                                               int32_t* src, void* stream) {
  EVC_REQUIRE(num_frames && keys && src, EVC_ERR_BAD_ARG, "evc_student_frame_select_scored: num_frames, keys and src are required");
  EVC_REQUIRE(B > 0 && T > 0 && T <= CHG_MAX_T && every_n > 0 && every_n <= T, EVC_ERR_BAD_SHAPE,
              "evc_student_frame_select_scored: B=%d, T=%d (1 .. %d), every_n=%d (1 .. T)", B, T, CHG_MAX_T, every_n);
  EVC_REQUIRE(strategy == EVC_SELECT_CHANGE || strategy == EVC_SELECT_SEGMENT_CHANGE, EVC_ERR_BAD_ARG,
              "evc_student_frame_select_scored: strategy=%d (6 change, 7 segment_change)", strategy);
  hipLaunchKernelGGL(frame_select_scored_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, num_frames, keys, T, every_n, strategy, src);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// Student frame selection (first / middle / last / first + middle + last / k random frames next to the uniform grid) and the input pass
// that gathers the selected frames: the student-only form of evc_l2norm_chunk_fwd / evc_l2norm_chunk_int with a source-frame table in
// place of the rule s2 * every_n.  The row code is restated here, so that the kernels of evc_elementwise.hip stay byte for byte what they were.
#include "evc_common.h"

// ---------------------------------------------------------------------------
// selection table: one workgroup per video, no atomics, no scratch
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// evc.h: the key of frame t of global video row `row` under (seed, draw); uint32 arithmetic throughout
__device__ __forceinline__ uint32_t frame_key(uint32_t seed, uint32_t draw, uint32_t row, uint32_t t) {
  uint32_t h = fmix32(seed * 0x9E3779B1u + draw);
  h = fmix32(h ^ (row * 0x85EBCA77u));
  return fmix32(h ^ (t * 0xC2B2AE3Du));
}

#define SEL_MAX_T 1024
__global__ __launch_bounds__(256) void frame_select_kernel(const int* __restrict__ nfr, int T, int every_n, int strategy, uint32_t seed,
                                                           uint32_t draw, int row0, int* __restrict__ src) {
  __shared__ uint32_t key[SEL_MAX_T];
  __shared__ int wave_cnt[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = T / every_n;
  int* out = src + (long)b * S;
  int n = nfr[b];
  n = n < 0 ? 0 : (n > T ? T : n);
  // the student's frame count, as frame_counts_kernel (subsampled): float64 true division, truncation (n - 1 at every_n = 1 for n = 55, 79, ...)
  const double q = (double)n / (double)T;
  const int k = (int)(long long)trunc(q * (double)S);         // k <= n because S <= T
  if (strategy != EVC_SELECT_RANDOM) {
    const int kf = (k + 2) / 3, km = (k + 1) / 3, kl = k / 3;
    int ms = (n - km) / 2;                                     // the middle run, kept clear of the first and the last one
    ms = ms < kf ? kf : ms;
    ms = ms > n - kl - km ? n - kl - km : ms;
    for (int j = tid; j < S; j += 256) {
      int f = -1;
      if (strategy == EVC_SELECT_UNIFORM) f = j * every_n;    // every slot: the table of the existing view
      else if (j < k) {
        if (strategy == EVC_SELECT_FIRST) f = j;
        else if (strategy == EVC_SELECT_LAST) f = n - k + j;
        else if (strategy == EVC_SELECT_MIDDLE) f = (n - k) / 2 + j;
        else f = j < kf ? j : (j < kf + km ? ms + (j - kf) : n - kl + (j - kf - km));
      }
      out[j] = f;
    }
    return;
  }
  // random: the k frames of [0, n) with the smallest (key, t), in ascending t.  Ranks by counting in LDS, compaction by ballots.
  for (int t = tid; t < n; t += 256) key[t] = frame_key(seed, draw, (uint32_t)(row0 + b), (uint32_t)t);
  for (int j = k + tid; j < S; j += 256) out[j] = -1;
  __syncthreads();
  int base = 0;                                                // selected frames below this pass's 256 (uniform over the workgroup)
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int t = t0 + tid;
    bool take = false;
    if (t < n) {
      const uint32_t kt = key[t];
      int rank = 0;
      for (int u = 0; u < n; ++u) {                            // every lane reads the same word: a broadcast
        const uint32_t ku = key[u];
        rank += (ku < kt || (ku == kt && u < t)) ? 1 : 0;
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

extern "C" int evc_student_frame_select(const int32_t* num_frames, int B, int T, int every_n, int strategy, uint32_t seed, uint32_t draw,
                                        int row0, int32_t* src, void* stream) {
  EVC_REQUIRE(num_frames && src, EVC_ERR_BAD_ARG, "evc_student_frame_select: num_frames and src are required");
  EVC_REQUIRE(B > 0 && T > 0 && T <= SEL_MAX_T && every_n > 0 && every_n <= T, EVC_ERR_BAD_SHAPE,
              "evc_student_frame_select: B=%d, T=%d (1 .. %d), every_n=%d (1 .. T)", B, T, SEL_MAX_T, every_n);
  EVC_REQUIRE(strategy >= EVC_SELECT_UNIFORM && strategy <= EVC_SELECT_RANDOM, EVC_ERR_BAD_ARG,
              "evc_student_frame_select: strategy=%d (0 uniform, 1 first, 2 middle, 3 last, 4 first_middle_last, 5 random)", strategy);
  EVC_REQUIRE(row0 >= 0, EVC_ERR_BAD_ARG, "evc_student_frame_select: row0=%d", row0);
  hipLaunchKernelGGL(frame_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, num_frames, T, every_n, strategy, seed, draw, row0, src);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// gathering input pass: one wave per student slot; slot j of video b reads frame src[b][j]
// ---------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(256) void l2norm_chunk_sel_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                               const int* __restrict__ nfr, const int* __restrict__ src, int B, int T, int F,
                                                               int S2, int C2, bf16_t* __restrict__ out2, int normalize,
                                                               bf16_t* __restrict__ out2_lo, int aux_mode,
                                                               const int* __restrict__ pos2, int P2, float* __restrict__ rs2) {
  const int lane = threadIdx.x & 63;
  const long slot = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // b*S2 + s2
  if (slot >= (long)B * S2) return;
  const int b = (int)(slot / S2), s2 = (int)(slot % S2);
  // Row plans (evc_sort_rows_by_len), as l2norm_chunk_kernel: slots >= P are rows of length 0 - neither loaded nor written.
  const int L2 = S2 / C2;
  const int t2 = s2 % L2;
  int slot2 = (s2 / L2) * B + b, rows2 = C2 * B;
  if (pos2) { slot2 = pos2[slot2]; rows2 = P2; }
  if (slot2 >= rows2) return;
  const int s = src[slot];                                      // source frame; -1 (or anything outside the tensor): a zero row
  const bool none = s < 0 || s >= T;
  const long row = (long)b * T + (none ? 0 : s);
  const int nv = F >> 2;
  float4 v[5];  // F <= 1280
  float ss = 0.f;
  const bool pad = none || (U8 && s >= nfr[b]);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + i * 64;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nv) {
      if (U8) {
        if (!pad) {
          const uchar4 q = ((const uchar4*)(xq + row * F))[j];
          const float sc = 4.0f / 255.0f, bs = 4.0f / 512.0f - 2.0f;   // cs/utils.py:22-25
          v[i] = make_float4(q.x * sc + bs, q.y * sc + bs, q.z * sc + bs, q.w * sc + bs);
        }
      } else {
        if (!pad) v[i] = ((const float4*)(x + row * F))[j];
      }
      ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
  }
  ss = wave_sum(ss);
  const float inv = normalize ? rsqrtf(fmaxf(ss, 1e-12f)) : 1.0f;   // tf.nn.l2_normalize epsilon
  const long off2 = ((long)t2 * rows2 + slot2) * F;
  bf16_t* o2 = out2 + off2;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + i * 64;
    if (j < nv) {
      ushort4 o;
      o.x = f32_to_bf16(v[i].x * inv); o.y = f32_to_bf16(v[i].y * inv);
      o.z = f32_to_bf16(v[i].z * inv); o.w = f32_to_bf16(v[i].w * inv);
      ((ushort4*)o2)[j] = o;
      if (out2_lo) {                // second image of the view (evc.h: aux_mode), the forms of l2norm_chunk_kernel
        ushort4 l;
        const float xv[4] = {v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv};
        if (aux_mode == 4) {          // wide split-bf16 image, rows of 2F: [lo | hi]
          l.x = f32_to_bf16(xv[0] - bf16_to_f32(o.x)); l.y = f32_to_bf16(xv[1] - bf16_to_f32(o.y));
          l.z = f32_to_bf16(xv[2] - bf16_to_f32(o.z)); l.w = f32_to_bf16(xv[3] - bf16_to_f32(o.w));
          ushort4* w = (ushort4*)(out2_lo + off2 * 2);
          w[j] = l; w[nv + j] = o;
          continue;
        }
        if (aux_mode == 6) {          // U8 only: rows of 3F bytes [f16(2q - 255) | e4m3(x 2^7)] and one f32 per frame, rs = (2/255) / |x_raw|
          ushort4 h16;
          float c8[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) c8[r] = fminf(fmaxf(xv[r] * 128.0f, -448.f), 448.f);
          if (U8 && !pad) {
            const uchar4 q = ((const uchar4*)(xq + row * F))[j];
            h16.x = f32_to_f16(2.0f * q.x - 255.0f); h16.y = f32_to_f16(2.0f * q.y - 255.0f);
            h16.z = f32_to_f16(2.0f * q.z - 255.0f); h16.w = f32_to_f16(2.0f * q.w - 255.0f);
          } else {
            h16 = make_ushort4(0, 0, 0, 0);
          }
          int w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[0], c8[1], 0, false);
          w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[2], c8[3], w8, true);
          const float rsv = pad ? 0.f : inv * (2.0f / 255.0f);
          bf16_t* rowp = out2_lo + (off2 / F) * (3L * F / 2);
          ((ushort4*)rowp)[j] = h16;
          ((int*)(rowp + F))[j] = w8;
          if (lane == 0 && i == 0) rs2[off2 / F] = rsv;
          continue;
        }
        if (aux_mode == 5) {          // rows of 4F bytes: [f16(x) | e4m3(x 2^7) | e4m3((x - f16(x)) 2^18)]
          ushort4 h16;
          h16.x = f32_to_f16(xv[0]); h16.y = f32_to_f16(xv[1]); h16.z = f32_to_f16(xv[2]); h16.w = f32_to_f16(xv[3]);
          const uint16_t hb[4] = {h16.x, h16.y, h16.z, h16.w};
          float c8[4], l8[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            c8[r] = fminf(fmaxf(xv[r] * 128.0f, -448.f), 448.f);
            l8[r] = fminf(fmaxf((xv[r] - f16_to_f32(hb[r])) * 262144.0f, -448.f), 448.f);
          }
          int w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[0], c8[1], 0, false);
          w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[2], c8[3], w8, true);
          int v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l8[0], l8[1], 0, false);
          v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l8[2], l8[3], v8, true);
          bf16_t* rowp = out2_lo + (off2 / F) * (2L * F);
          ((ushort4*)rowp)[j] = h16;
          ((int*)(rowp + F))[j] = w8;
          ((int*)(rowp + F))[nv + j] = v8;
          continue;
        }
        if (aux_mode >= 1) {          // IEEE f16 image, rows of nseg*F: [x | (x - f16(x))*64 | f16(x)/64]
          const int nseg = aux_mode;
          ushort4 h16, l16, s16;
          h16.x = f32_to_f16(xv[0]); h16.y = f32_to_f16(xv[1]); h16.z = f32_to_f16(xv[2]); h16.w = f32_to_f16(xv[3]);
          const uint16_t hb[4] = {h16.x, h16.y, h16.z, h16.w};
          uint16_t lb[4], sb[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float hf = f16_to_f32(hb[r]);
            lb[r] = f32_to_f16((xv[r] - hf) * 64.0f);
            sb[r] = f32_to_f16(hf * (1.0f / 64.0f));
          }
          l16 = make_ushort4(lb[0], lb[1], lb[2], lb[3]); s16 = make_ushort4(sb[0], sb[1], sb[2], sb[3]);
          ushort4* w = (ushort4*)(out2_lo + off2 * nseg);
          w[j] = h16;
          if (nseg >= 2) w[nv + j] = l16;
          if (nseg >= 3) w[2 * nv + j] = s16;
          continue;
        }
        l.x = f32_to_bf16(xv[0] - bf16_to_f32(o.x)); l.y = f32_to_bf16(xv[1] - bf16_to_f32(o.y));
        l.z = f32_to_bf16(xv[2] - bf16_to_f32(o.z)); l.w = f32_to_bf16(xv[3] - bf16_to_f32(o.w));
        ((ushort4*)(out2_lo + off2))[j] = l;
      }
    }
  }
}

static int l2norm_chunk_sel_impl(const char* who, const float* x_raw, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* src,
                                 int B, int T, int F, int every_n, int C2, evc_bf16* out2, int normalize, evc_bf16* out2_lo, int aux_mode,
                                 const int32_t* row_pos2, int rows2, float* rs2, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && F <= 1280, EVC_ERR_BAD_SHAPE, "%s: F=%d must be a multiple of 4 and <= 1280", who, F);
  EVC_REQUIRE(every_n > 0 && C2 > 0 && (T / every_n) % C2 == 0 && (T / every_n) > 0, EVC_ERR_BAD_SHAPE,
              "%s: student view T/every_n=%d not divisible by C2=%d", who, T / (every_n > 0 ? every_n : 1), C2);
  EVC_REQUIRE(src && out2, EVC_ERR_BAD_ARG, "%s: the table src and the view out2 are required", who);
  EVC_REQUIRE((x_raw != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "%s: exactly one of x_raw / x_u8", who);
  EVC_REQUIRE(!x_u8 || num_frames, EVC_ERR_BAD_ARG, "%s: uint8 input needs num_frames", who);
  EVC_REQUIRE(aux_mode >= 0 && aux_mode <= 6, EVC_ERR_BAD_ARG, "%s: aux_mode=%d (as evc_l2norm_chunk_fwd; 6: evc_l2norm_chunk_sel_int)", who, aux_mode);
  EVC_REQUIRE(aux_mode < 5 || F % 32 == 0, EVC_ERR_BAD_SHAPE, "%s: aux_mode 5 / 6 need F %% 32 == 0 (16-byte aligned row parts), F=%d", who, F);
  EVC_REQUIRE(aux_mode != 6 || (x_u8 && normalize && out2_lo && rs2), EVC_ERR_BAD_ARG,
              "%s: the integer image needs the uint8 input, the image and its row-scale array", who);
  EVC_REQUIRE(!row_pos2 || rows2 > 0, EVC_ERR_BAD_ARG, "%s: row plan with rows2=%d", who, rows2);
  const int S2 = T / every_n;
  const long rows = (long)B * S2;
  dim3 grid((unsigned)((rows + 3) / 4));
  if (x_u8)
    hipLaunchKernelGGL(l2norm_chunk_sel_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x_raw, x_u8, num_frames, src, B, T, F, S2, C2, out2,
                       normalize, out2_lo, aux_mode, row_pos2, rows2, rs2);
  else
    hipLaunchKernelGGL(l2norm_chunk_sel_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x_raw, x_u8, num_frames, src, B, T, F, S2, C2, out2,
                       normalize, out2_lo, aux_mode, row_pos2, rows2, rs2);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_l2norm_chunk_sel_fwd(const float* x_raw, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* src,
                                        int B, int T, int F, int every_n, int C2, evc_bf16* out2, int normalize,
                                        evc_bf16* out2_lo, int aux_mode, const int32_t* row_pos2, int rows2, void* stream) {
  EVC_REQUIRE(aux_mode != 6, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_sel_fwd: aux_mode 6 (integer frames) is evc_l2norm_chunk_sel_int");
  return l2norm_chunk_sel_impl("evc_l2norm_chunk_sel_fwd", x_raw, x_u8, num_frames, src, B, T, F, every_n, C2, out2, normalize, out2_lo, aux_mode,
                               row_pos2, rows2, nullptr, stream);
}

extern "C" int evc_l2norm_chunk_sel_int(const uint8_t* x_u8, const int32_t* num_frames, const int32_t* src, int B, int T, int F,
                                        int every_n, int C2, evc_bf16* out2, evc_f16* out2_int, float* rs2,
                                        const int32_t* row_pos2, int rows2, void* stream) {
  EVC_REQUIRE(x_u8 && num_frames, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_sel_int: uint8 frames and their counts are required");
  return l2norm_chunk_sel_impl("evc_l2norm_chunk_sel_int", nullptr, x_u8, num_frames, src, B, T, F, every_n, C2, out2, 1, (evc_bf16*)out2_int, 6,
                               row_pos2, rows2, rs2, stream);
}

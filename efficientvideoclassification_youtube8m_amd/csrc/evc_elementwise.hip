// HBM-bound kernels of the hot path: input preparation, layout changes, MoE
// tail, losses, regulariser + clip + Adam, pooling, batch-norm pieces.
// All are streaming kernels: 16-byte vector accesses where rows allow,
// grid-stride with >= 2048 workgroups on big tensors (256 CUs x 8).
#include <stdarg.h>
#include "evc_common.h"
#include <mutex>

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void evc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* evc_last_error(void) { return g_err; }
extern "C" int evc_version(void) { return EVC_VERSION; }
extern "C" int evc_check_device(int dev) {
  hipDeviceProp_t prop;
  EVC_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
  EVC_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, EVC_ERR_UNSUPPORTED_ARCH,
              "device %d is %s; libevc_hip is built for gfx950 only", dev, prop.gcnArchName);
  return EVC_OK;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}

// ---------------------------------------------------------------------------
// a1 + a2: l2-normalise, sub-sample, cast, re-layout.  One wave per frame.
// ---------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(256) void l2norm_chunk_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                           const int* __restrict__ nfr, int B, int T, int F, int C1,
                                                           bf16_t* __restrict__ out1, int every_n, int C2,
                                                           bf16_t* __restrict__ out2, int normalize,
                                                           bf16_t* __restrict__ out1_lo, bf16_t* __restrict__ out2_lo, int aux_mode,
                                                           const int* __restrict__ pos1, int P1,
                                                           const int* __restrict__ pos2, int P2,
                                                           float* __restrict__ rs1, float* __restrict__ rs2) {
  const int lane = threadIdx.x & 63;
  long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // b*T + s
  int b, s;
  if (!out1) {
    // Student-only graphs (out1 == NULL, round 6): the grid covers the SUB-SAMPLED frames only - frame s2 * every_n of video b - and nothing
    // else of the [B][T][F] tensor is read (cfg 5, every_n = 30: 47 MB instead of 1.4 GB in, no 0.7 GB teacher view out).
    const int S2 = T / every_n;
    if (row >= (long)B * S2) return;
    b = (int)(row / S2); s = (int)(row % S2) * every_n;
    row = (long)b * T + s;
  } else {
    if (row >= (long)B * T) return;
    b = (int)(row / T); s = (int)(row % T);
  }
  // Row plans (evc_sort_rows_by_len): chunk row (c, b) lives in slot pos[c*B + b] of a [steps][P] image; slots
  // >= P are rows of length 0, which no kernel reads - they are neither loaded nor written.
  const int L1 = T / C1;
  int slot1 = (s / L1) * B + b, rows1 = C1 * B;
  if (!out1) { slot1 = 0; rows1 = 0; }                // no teacher view: every frame is "dead" on that side
  else if (pos1) { slot1 = pos1[slot1]; rows1 = P1; }
  int slot2 = -1, rows2 = 0, t2 = 0;
  if (out2 && (s % every_n) == 0) {
    const int s2 = s / every_n, S2 = T / every_n;
    if (s2 < S2) {
      const int L2 = S2 / C2;
      t2 = s2 % L2;
      slot2 = (s2 / L2) * B + b; rows2 = C2 * B;
      if (pos2) { slot2 = pos2[slot2]; rows2 = P2; }
      if (slot2 >= rows2) slot2 = -1;
    }
  }
  if (slot1 >= rows1 && slot2 < 0) return;
  const int nv = F >> 2;
  float4 v[5];  // F <= 1280
  float ss = 0.f;
  const bool pad = U8 && s >= nfr[b];
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
        v[i] = ((const float4*)(x + row * F))[j];
      }
      ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
  }
  ss = wave_sum(ss);
  const float inv = normalize ? rsqrtf(fmaxf(ss, 1e-12f)) : 1.0f;   // tf.nn.l2_normalize epsilon
  const long off1 = ((long)(s % L1) * rows1 + slot1) * F;
  bf16_t* o1 = slot1 < rows1 ? out1 + off1 : nullptr;
  bf16_t* o2 = nullptr;
  long off2 = 0;
  if (slot2 >= 0) {
    off2 = ((long)t2 * rows2 + slot2) * F;
    o2 = out2 + off2;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + i * 64;
    if (j < nv) {
      ushort4 o;
      o.x = f32_to_bf16(v[i].x * inv); o.y = f32_to_bf16(v[i].y * inv);
      o.z = f32_to_bf16(v[i].z * inv); o.w = f32_to_bf16(v[i].w * inv);
      if (o1) ((ushort4*)o1)[j] = o;
      if (o2) ((ushort4*)o2)[j] = o;
      if (out1_lo || out2_lo) {     // "high" precision forward: second image of each view (evc.h: aux_mode)
        ushort4 l;
        const float xv[4] = {v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv};
        if (aux_mode == 4) {          // wide split-bf16 image, rows of 2F: [lo | hi] (the A operand of evc_gemm_nt_split / evc_lstm_layer_fwd_hp)
          l.x = f32_to_bf16(xv[0] - bf16_to_f32(o.x)); l.y = f32_to_bf16(xv[1] - bf16_to_f32(o.y));
          l.z = f32_to_bf16(xv[2] - bf16_to_f32(o.z)); l.w = f32_to_bf16(xv[3] - bf16_to_f32(o.w));
          if (o1) {
            ushort4* w = (ushort4*)(out1_lo + off1 * 2);
            w[j] = l; w[nv + j] = o;
          }
          if (o2 && out2_lo) {
            ushort4* w = (ushort4*)(out2_lo + off2 * 2);
            w[j] = l; w[nv + j] = o;
          }
          continue;
        }
        if (aux_mode == 6) {          // U8 only (round 6): rows of 3F bytes [f16(2q - 255) (F halfwords: odd integers, EXACT) | e4m3(x 2^7) (F bytes)] and one
                                      // f32 per frame, rs = (2/255) / |x_raw|: x = rs (c + 255/256), so layer 0 contracts the integers and applies rs to its
                                      // accumulators (evc_lstm_layer_fwd_f16_fp8lo x_int): no rounding of the input frames at all
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
          if (o1) {
            bf16_t* rowp = out1_lo + (off1 / F) * (3L * F / 2);
            ((ushort4*)rowp)[j] = h16;
            ((int*)(rowp + F))[j] = w8;
            if (lane == 0 && i == 0) rs1[off1 / F] = rsv;
          }
          if (o2 && out2_lo) {
            bf16_t* rowp = out2_lo + (off2 / F) * (3L * F / 2);
            ((ushort4*)rowp)[j] = h16;
            ((int*)(rowp + F))[j] = w8;
            if (lane == 0 && i == 0) rs2[off2 / F] = rsv;
          }
          continue;
        }
        if (aux_mode == 5) {          // rows of 4F bytes: [f16(x) (F halfwords) | e4m3(x 2^7) (F bytes) | e4m3((x - f16(x)) 2^18) (F bytes)] - the x rows of
                                      // evc_lstm_layer_fwd_f16_fp8lo (the low-order half of x: |.| <= 2^-12 |x|, against e4m3(Wx 2^6) - same 2^24 in all)
          ushort4 h16;
          h16.x = f32_to_f16(xv[0]); h16.y = f32_to_f16(xv[1]); h16.z = f32_to_f16(xv[2]); h16.w = f32_to_f16(xv[3]);
          const uint16_t hb[4] = {h16.x, h16.y, h16.z, h16.w};
          float c8[4], l8[4];           // (|x| <= 1 after l2norm; raw inputs are clamped: codes above 448 are NaN in OCP e4m3)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            c8[r] = fminf(fmaxf(xv[r] * 128.0f, -448.f), 448.f);
            l8[r] = fminf(fmaxf((xv[r] - f16_to_f32(hb[r])) * 262144.0f, -448.f), 448.f);
          }
          int w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[0], c8[1], 0, false);
          w8 = __builtin_amdgcn_cvt_pk_fp8_f32(c8[2], c8[3], w8, true);
          int v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l8[0], l8[1], 0, false);
          v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l8[2], l8[3], v8, true);
          if (o1) {
            bf16_t* row = out1_lo + (off1 / F) * (2L * F);      // (off1 = row * F)
            ((ushort4*)row)[j] = h16;
            ((int*)(row + F))[j] = w8;
            ((int*)(row + F))[nv + j] = v8;
          }
          if (o2 && out2_lo) {
            bf16_t* row = out2_lo + (off2 / F) * (2L * F);
            ((ushort4*)row)[j] = h16;
            ((int*)(row + F))[j] = w8;
            ((int*)(row + F))[nv + j] = v8;
          }
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
          if (o1) {
            ushort4* w = (ushort4*)(out1_lo + off1 * nseg);
            w[j] = h16;
            if (nseg >= 2) w[nv + j] = l16;
            if (nseg >= 3) w[2 * nv + j] = s16;
          }
          if (o2 && out2_lo) {
            ushort4* w = (ushort4*)(out2_lo + off2 * nseg);
            w[j] = h16;
            if (nseg >= 2) w[nv + j] = l16;
            if (nseg >= 3) w[2 * nv + j] = s16;
          }
          continue;
        }
        l.x = f32_to_bf16(xv[0] - bf16_to_f32(o.x)); l.y = f32_to_bf16(xv[1] - bf16_to_f32(o.y));
        l.z = f32_to_bf16(xv[2] - bf16_to_f32(o.z)); l.w = f32_to_bf16(xv[3] - bf16_to_f32(o.w));
        if (o1) ((ushort4*)(out1_lo + off1))[j] = l;
        if (o2 && out2_lo) ((ushort4*)(out2_lo + off2))[j] = l;
      }
    }
  }
}

static int l2norm_chunk_impl(const float* x_raw, const uint8_t* x_u8, const int32_t* num_frames,
                             int B, int T, int F, int C1, evc_bf16* out1,
                             int every_n, int C2, evc_bf16* out2, int normalize,
                             evc_bf16* out1_lo, evc_bf16* out2_lo, int aux_mode,
                             const int32_t* row_pos1, int rows1, const int32_t* row_pos2, int rows2, float* rs1, float* rs2, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && F <= 1280, EVC_ERR_BAD_SHAPE,
              "evc_l2norm_chunk_fwd: F=%d must be a multiple of 4 and <= 1280", F);
  EVC_REQUIRE(C1 > 0 && T % C1 == 0, EVC_ERR_BAD_SHAPE, "evc_l2norm_chunk_fwd: T=%d not divisible by C1=%d", T, C1);
  if (out2) {
    EVC_REQUIRE(every_n > 0 && C2 > 0 && (T / every_n) % C2 == 0 && (T / every_n) > 0, EVC_ERR_BAD_SHAPE,
                "evc_l2norm_chunk_fwd: student view T/every_n=%d not divisible by C2=%d", T / (every_n > 0 ? every_n : 1), C2);
  }
  EVC_REQUIRE(!x_u8 || num_frames, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_fwd: uint8 input needs num_frames");
  EVC_REQUIRE(aux_mode >= 0 && aux_mode <= 6, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_fwd: aux_mode=%d (0 bf16 low halves, 1..3 f16 segments, 4 wide bf16, 5 f16 + two e4m3 images, 6 integer frames + row scales)", aux_mode);
  EVC_REQUIRE(aux_mode < 5 || F % 32 == 0, EVC_ERR_BAD_SHAPE, "evc_l2norm_chunk_fwd: aux_mode 5 / 6 need F %% 32 == 0 (16-byte aligned row parts), F=%d", F);
  EVC_REQUIRE(aux_mode != 6 || (x_u8 && normalize && (!out1_lo || rs1) && (!out2_lo || rs2)), EVC_ERR_BAD_ARG,
              "evc_l2norm_chunk_int: the integer image needs the uint8 input, normalize = 1 and a row-scale array per second image");
  EVC_REQUIRE(out1 || out2, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_fwd: neither view requested");
  EVC_REQUIRE(out1 || !out1_lo, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_fwd: out1_lo without out1");
  const long rows = out1 ? (long)B * T : (long)B * (T / every_n);       // out1 == NULL: only the sub-sampled frames are touched
  dim3 grid((unsigned)((rows + 3) / 4));
  if (x_u8)
    hipLaunchKernelGGL(l2norm_chunk_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x_raw, x_u8, num_frames, B, T, F,
                       C1, out1, every_n > 0 ? every_n : 1, C2, out2, normalize, out1_lo, out2_lo, aux_mode, row_pos1, rows1, row_pos2, rows2, rs1, rs2);
  else
    hipLaunchKernelGGL(l2norm_chunk_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x_raw, x_u8, num_frames, B, T, F,
                       C1, out1, every_n > 0 ? every_n : 1, C2, out2, normalize, out1_lo, out2_lo, aux_mode, row_pos1, rows1, row_pos2, rows2, rs1, rs2);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_l2norm_chunk_fwd(const float* x_raw, const uint8_t* x_u8, const int32_t* num_frames,
                                    int B, int T, int F, int C1, evc_bf16* out1,
                                    int every_n, int C2, evc_bf16* out2, int normalize,
                                    evc_bf16* out1_lo, evc_bf16* out2_lo, int aux_mode,
                                    const int32_t* row_pos1, int rows1, const int32_t* row_pos2, int rows2, void* stream) {
  EVC_REQUIRE(aux_mode != 6, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_fwd: aux_mode 6 (integer frames) is evc_l2norm_chunk_int");
  return l2norm_chunk_impl(x_raw, x_u8, num_frames, B, T, F, C1, out1, every_n, C2, out2, normalize, out1_lo, out2_lo, aux_mode, row_pos1, rows1, row_pos2, rows2,
                           nullptr, nullptr, stream);
}
// The reader's uint8 frames as EXACT f16 integers (round 6, "high" precision on the input the pipeline actually delivers, cs/readers.py:146-174):
// Dequantize (cs/utils.py:22-25) is x = (2/255) (2q - 255) + 1/128, so the l2-normalised frame is rs (c + 255/256) with c = 2q - 255 an odd integer in
// [-255, 255] and rs = (2/255) / |x| one f32 per frame.  Second images: rows of 3F bytes [f16(c) | e4m3(x_hat 2^7)]; rs1 / rs2 [steps][rows] f32 in
// the images' row order (0 for padded frames, whose integers are 0 too).  Layer 0 contracts c against f16(Wx) - no rounding of the input at all -
// and applies rs to its accumulators before the recurrent part (evc_lstm_layer_fwd_f16_fp8lo with x_int).  The bf16 images are the usual ones.
extern "C" int evc_l2norm_chunk_int(const uint8_t* x_u8, const int32_t* num_frames, int B, int T, int F, int C1, evc_bf16* out1,
                                    int every_n, int C2, evc_bf16* out2, evc_f16* out1_int, evc_f16* out2_int, float* rs1, float* rs2,
                                    const int32_t* row_pos1, int rows1, const int32_t* row_pos2, int rows2, void* stream) {
  EVC_REQUIRE(x_u8 && num_frames, EVC_ERR_BAD_ARG, "evc_l2norm_chunk_int: uint8 frames and their counts are required");
  return l2norm_chunk_impl(nullptr, x_u8, num_frames, B, T, F, C1, out1, every_n, C2, out2, 1, (evc_bf16*)out1_int, (evc_bf16*)out2_int, 6,
                           row_pos1, rows1, row_pos2, rows2, rs1, rs2, stream);
}

// ---------------------------------------------------------------------------
// a2 integer part: frame counts (bit-exact vs the float64/float32 TF formulas)
// ---------------------------------------------------------------------------
__global__ void frame_counts_kernel(const int* __restrict__ nfr, int B, int every_n, int subsampled, int maxf, int C, int Lc,
                                    long long* __restrict__ n_out, int* __restrict__ len1, int* __restrict__ len2) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long long n = nfr[b];
  if (subsampled) {          // also at every_n = 1: float64 (n/300)*300 truncates to n-1 for n = 55, 79, 97, ... (kept)
    // tf.cast(tf.multiply(tf.divide(n, 300), S), tf.int64): float64 true division, truncation
    const int S = maxf / every_n;
    const double q = (double)nfr[b] / (double)maxf;
    n = (long long)trunc(q * (double)S);
  }
  if (n_out) n_out[b] = n;
  for (int i = 0; i < C; ++i) {
    long long v = n - (long long)Lc * i;
    v = v < 0 ? 0 : v;
    v = v > Lc ? Lc : v;
    len1[(long)i * B + b] = (int)v;
  }
  // tf.cast(tf.ceil(tf.cast(n, tf.float32) / Lc), tf.int32)
  len2[b] = (int)ceilf((float)n / (float)Lc);
}

extern "C" int evc_frame_counts(const int32_t* num_frames, int B, int every_n, int subsampled, int max_frames_before_sampling,
                                int num_chunks, int chunk_len, int64_t* n_out, int32_t* len_l1, int32_t* len_l2,
                                void* stream) {
  EVC_REQUIRE(B > 0 && every_n > 0 && num_chunks > 0 && chunk_len > 0, EVC_ERR_BAD_SHAPE, "evc_frame_counts: bad args");
  hipLaunchKernelGGL(frame_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, num_frames, B, every_n,
                     subsampled, max_frames_before_sampling, num_chunks, chunk_len, (long long*)n_out, len_l1, len_l2);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// Row plan: stable counting sort of the M rows of an LSTM stack by length, longest first.  With rows in that
// order the rows active at step t are the prefix [0, #{len > t}), so a step kernel is launched on that
// prefix only and the rows of length 0 (frames beyond num_frames: ~28% of the chunk rows of a YT8M batch)
// are never touched.  One workgroup; thread i owns rows [i*R, (i+1)*R).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sort_rows_kernel(const int* __restrict__ len, int M, int max_len,
                                                         int* __restrict__ pos, int* __restrict__ inv,
                                                         int* __restrict__ len_sorted) {
  extern __shared__ unsigned short cnt[];          // [max_len + 1][1024] -> exclusive start offsets
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = (M + 1023) / 1024;
  const int r0 = tid * R, r1 = min(M, r0 + R);
  const int NB = max_len + 1;
  for (int k = 0; k < NB; ++k) cnt[k * 1024 + tid] = 0;
  for (int r = r0; r < r1; ++r) {
    int l = len[r];
    l = l < 0 ? 0 : (l > max_len ? max_len : l);
    cnt[(max_len - l) * 1024 + tid] += 1;          // bucket 0 = longest rows
  }
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int k = 0; k < NB; ++k) {                   // block-wide exclusive scan of bucket k, carried base
    const int c = cnt[k * 1024 + tid];
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wave_tot[w];
    const int base = base_s;
    cnt[k * 1024 + tid] = (unsigned short)(base + wbase + incl - c);   // M <= 65535
    __syncthreads();
    if (tid == 1023) base_s = base + wbase + incl;
    __syncthreads();
  }
  for (int r = r0; r < r1; ++r) {
    int l = len[r];
    l = l < 0 ? 0 : (l > max_len ? max_len : l);
    const int k = max_len - l;
    const int p = cnt[k * 1024 + tid];
    cnt[k * 1024 + tid] = (unsigned short)(p + 1);
    pos[r] = p;
    inv[p] = r;
    len_sorted[p] = l;
  }
}

extern "C" int evc_sort_rows_by_len(const int32_t* len, int M, int max_len, int32_t* pos, int32_t* inv, int32_t* len_sorted,
                                    void* stream) {
  EVC_REQUIRE(M > 0 && M <= 65535 && max_len >= 0 && max_len <= 63, EVC_ERR_BAD_SHAPE,
              "evc_sort_rows_by_len: M=%d (<= 65535), max_len=%d (<= 63)", M, max_len);
  const size_t lds = (size_t)(max_len + 1) * 1024 * sizeof(unsigned short);
  static std::once_flag once;
  std::call_once(once, [&] { (void)hipFuncSetAttribute((const void*)sort_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024 * 2); });
  hipLaunchKernelGGL(sort_rows_kernel, dim3(1), dim3(1024), lds, (hipStream_t)stream, len, M, max_len, pos, inv, len_sorted);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// transpose (+cast) to bf16: out[c][r] = in[r][c]; columns [R,Rpad) zeroed
// ---------------------------------------------------------------------------
// 64x64 tile through LDS; every thread moves 4 elements per access on both sides (8-byte bf16 /
// 16-byte f32 loads along the input rows, 8-byte stores along the output rows), so each 16-lane
// group reads / writes one full 128-byte line.
template <bool F32>
__global__ __launch_bounds__(256) void transpose_kernel(const void* __restrict__ in, long ld_in, int R, int C,
                                                        bf16_t* __restrict__ out, long ld_out, int Rpad, int il_H) {
  __shared__ bf16_t tile[64][68];   // [input row][input col], 136-byte pitch
  const int q = threadIdx.x & 15, p = threadIdx.x >> 4;   // q: group of 4 elements, p: 0..15
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const bool vec_in = (ld_in % 4 == 0) && (((uintptr_t)in) % (F32 ? 16 : 8) == 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // il_H > 0: the tile's rows are 64 consecutive OUTPUT columns u*4 + g, i.e. input rows g*H + u (16 units x
    // 4 gate blocks) - so the stores below stay contiguous 8-byte vectors (scattered 2-byte stores ran at 0.8 TB/s)
    const int ro = r0 + p + 16 * i, c = c0 + q * 4;
    const int r = (il_H > 0 && ro < R) ? (ro & 3) * il_H + (ro >> 2) : ro;
    bf16_t v[4] = {0, 0, 0, 0};
    if (ro < R) {
      if (vec_in && c + 3 < C) {
        if (F32) {
          const float4 f = *(const float4*)((const float*)in + (long)r * ld_in + c);
          v[0] = f32_to_bf16(f.x); v[1] = f32_to_bf16(f.y); v[2] = f32_to_bf16(f.z); v[3] = f32_to_bf16(f.w);
        } else {
          const ushort4 u = *(const ushort4*)((const bf16_t*)in + (long)r * ld_in + c);
          v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < C) v[j] = F32 ? f32_to_bf16(((const float*)in)[(long)r * ld_in + c + j]) : ((const bf16_t*)in)[(long)r * ld_in + c + j];
      }
    }
    *(ushort4*)&tile[p + 16 * i][q * 4] = make_ushort4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  const bool vec_out = (ld_out % 4 == 0) && (((uintptr_t)out) % 8 == 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + p + 16 * i, r = r0 + q * 4;   // output row c (input column), 4 consecutive output columns r..r+3
    if (c >= C) continue;
    // il_H < 0: input COLUMN c = u*4 + g (gate-interleaved) lands in output row g*H + u (TF order), H = -il_H
    const int co = (il_H < 0) ? (c & 3) * (-il_H) + (c >> 2) : c;
    const int cl = p + 16 * i;
    if (vec_out && r + 3 < Rpad) {
      *(ushort4*)(out + (long)co * ld_out + r) = make_ushort4(tile[q * 4][cl], tile[q * 4 + 1][cl], tile[q * 4 + 2][cl], tile[q * 4 + 3][cl]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rr = r + j;
        if (rr < Rpad) out[(long)co * ld_out + rr] = tile[q * 4 + j][cl];
      }
    }
  }
}

extern "C" int evc_transpose_to_bf16(const void* in, int in_f32, int64_t ld_in, int R, int C,
                                     evc_bf16* out, int64_t ld_out, int Rpad, int interleave_H, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && Rpad >= R && ld_out >= Rpad, EVC_ERR_BAD_SHAPE, "evc_transpose_to_bf16: bad shape");
  EVC_REQUIRE(interleave_H <= 0 || R == 4 * interleave_H, EVC_ERR_BAD_SHAPE, "evc_transpose_to_bf16: interleave_H needs R == 4*H");
  EVC_REQUIRE(interleave_H >= 0 || C == -4 * interleave_H, EVC_ERR_BAD_SHAPE, "evc_transpose_to_bf16: interleave_H < 0 needs C == 4*H");
  dim3 grid((Rpad + 63) / 64, (C + 63) / 64);
  if (in_f32)
    hipLaunchKernelGGL(transpose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, out, ld_out, Rpad, interleave_H);
  else
    hipLaunchKernelGGL(transpose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, out, ld_out, Rpad, interleave_H);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ void cast_kernel(const float* __restrict__ in, long ld_in, int R, int C, bf16_t* __restrict__ out, long ld_out) {
  const long n = (long)R * C;
  const long stride = (long)gridDim.x * blockDim.x, tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ld_in == C && ld_out == C && (n & 3) == 0 && (((uintptr_t)in) & 15) == 0 && (((uintptr_t)out) & 7) == 0) {
    // dense: 16-byte loads, 8-byte stores, no index arithmetic
    for (long i = tid; i < (n >> 2); i += stride) {
      const float4 f = ((const float4*)in)[i];
      ((uint2*)out)[i] = make_uint2(pack_bf16x2_hw(f.x, f.y), pack_bf16x2_hw(f.z, f.w));
    }
    return;
  }
  for (long i = tid; i < n; i += stride) {
    const long r = i / C, c = i % C;
    out[r * ld_out + c] = f32_to_bf16(in[r * ld_in + c]);
  }
}
extern "C" int evc_cast_f32_to_bf16(const float* in, int64_t ld_in, int R, int C, evc_bf16* out, int64_t ld_out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_bf16: bad shape");
  const long n = (long)R * C;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, out, ld_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ void cast_f16_kernel(const float* __restrict__ in, long ld_in, int R, int C, f16_t* __restrict__ out, long ld_out) {
  const long n = (long)R * C;
  const long stride = (long)gridDim.x * blockDim.x, tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (ld_in == C && ld_out == C && (n & 3) == 0 && (((uintptr_t)in) & 15) == 0 && (((uintptr_t)out) & 7) == 0) {
    for (long i = tid; i < (n >> 2); i += stride) {
      const float4 f = ((const float4*)in)[i];
      ((uint2*)out)[i] = make_uint2(pack_f16x2_hw(f.x, f.y), pack_f16x2_hw(f.z, f.w));
    }
    return;
  }
  for (long i = tid; i < n; i += stride) {
    const long r = i / C, c = i % C;
    out[r * ld_out + c] = f32_to_f16(in[r * ld_in + c]);
  }
}
extern "C" int evc_cast_f32_to_f16(const float* in, int64_t ld_in, int R, int C, evc_f16* out, int64_t ld_out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_f16: bad shape");
  const long n = (long)R * C;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, out, ld_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// Time-dithered f16 images of a weight tensor (round 5; DESIGN.md 7 "dither"; oracle/lowprec.py::f16_dither_images is the bit-exact
// restatement): image t of element i is one of w's two f16 NEIGHBOURS dn <= w <= up - the upper one when the element's 32-bit phase at
// step t, fmix32(i ^ seed_mix) + t * 0x9E3779B9 (a golden-ratio rotation per step), lies below frac * 2^32, frac = (w - dn) / (up - dn).
// In any run of n consecutive images an element is rounded up n * frac times +- a few (2.03 measured over every run inside 20 steps): the rounding errors a recurrence integrates over its
// steps cancel instead of adding up.  4 elements per thread; every image row-major like the input, image t at out + t * img_stride.
__device__ __forceinline__ uint32_t fmix32_(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
__global__ __launch_bounds__(256) void cast_f16_dither_kernel(const float* __restrict__ in, long n4, int T, long img_stride, uint32_t seed_mix,
                                                              f16_t* __restrict__ out, long row_len, long col0) {
  for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (long)gridDim.x * blockDim.x) {
    const float4 f = ((const float4*)in)[i4];
    const float w[4] = {f.x, f.y, f.z, f.w};
    const bool plain = row_len > 0 && (i4 * 4) % row_len < col0;      // columns below col0: the round-to-nearest image in every step (row_len, col0 multiples of 4)
    uint32_t dn[4], up[4], thr[4], ph[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t hb = f32_to_f16(w[r]);
      const float hf = f16_to_f32((f16_t)hb);
      const bool zero = (hb & 0x7fffu) == 0, neg = (hb & 0x8000u) != 0;
      const uint32_t below = zero ? 0x8001u : (neg ? hb + 1u : hb - 1u);      // next f16 towards -inf
      const uint32_t above = zero ? 0x0001u : (neg ? hb - 1u : hb + 1u);      // next f16 towards +inf
      dn[r] = (hf > w[r] && !plain) ? below : hb;
      up[r] = (hf < w[r] && !plain) ? above : hb;
      const float dnf = f16_to_f32((f16_t)dn[r]), gap = f16_to_f32((f16_t)up[r]) - dnf;
      const float frac = gap > 0.f ? (w[r] - dnf) / gap : 0.f;                // exact: the numerator is exact, the gap a power of two (or inf: 0)
      thr[r] = (uint32_t)fminf(frac * 4294967296.0f, 4294967040.0f);
      ph[r] = fmix32_((uint32_t)(i4 * 4 + r) ^ seed_mix);
    }
    f16_t* o = out + i4 * 4;
    for (int t = 0; t < T; ++t) {
      const uint32_t rot = (uint32_t)t * 0x9E3779B9u;
      uint32_t b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = (ph[r] + rot) < thr[r] ? up[r] : dn[r];
      *(uint2*)(o + (long)t * img_stride) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
    }
  }
}
extern "C" int evc_cast_f32_to_f16_dither(const float* in, int64_t n, int T, int64_t img_stride, uint32_t seed, evc_f16* out, int64_t row_len, int64_t col0,
                                          void* stream) {
  EVC_REQUIRE(in && out && n > 0 && n % 4 == 0 && n < (1LL << 32) && T >= 1 && T <= 4096, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_f16_dither: n=%ld (%%4, < 2^32) T=%d", (long)n, T);
  EVC_REQUIRE(row_len >= 0 && col0 >= 0 && (row_len == 0 ? col0 == 0 : (row_len % 4 == 0 && col0 % 4 == 0 && col0 <= row_len && n % row_len == 0)), EVC_ERR_BAD_ARG,
              "evc_cast_f32_to_f16_dither: row_len=%ld col0=%ld (multiples of 4, col0 <= row_len, n a multiple of row_len; 0, 0: every element dithered)", (long)row_len, (long)col0);
  EVC_REQUIRE(img_stride >= n && img_stride % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 8) == 0, EVC_ERR_BAD_ALIGN,
              "evc_cast_f32_to_f16_dither: img_stride=%ld (>= n, %%4), in 16-byte, out 8-byte aligned", (long)img_stride);
  const long n4 = n / 4;
  const int grid = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(cast_f16_dither_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, n4, T, (long)img_stride, seed * 0x9E3779B9u, (f16_t*)out,
                     (long)row_len, (long)col0);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// IEEE f16 weight image of an LSTM kernel whose x-part is contracted as a K-extension (evc_lstm_layer_fwd_f16 on nseg x-segments):
// out row = [f16(Wx) | f16(Wx)/64 | (Wx - f16(Wx))*64 | f16(Wh)] (the first nseg of the three x blocks), in = [Wx(Kin) | Wh(H)] f32.
__global__ void cast_f16_wide_kernel(const float* __restrict__ in, long ld_in, int R, int Kin, int H, int nseg, int h_ext, f16_t* __restrict__ out) {
  const int C = Kin + H;
  const long n = (long)R * C, ldo = (long)nseg * Kin + (h_ext ? 2L : 1L) * H;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i % C);
    const float w = in[r * ld_in + c];
    const f16_t h = f32_to_f16(w);
    const float hf = f16_to_f32(h);
    f16_t* o = out + r * ldo;
    if (c >= Kin) {
      o[(long)nseg * Kin + (c - Kin)] = h;
      if (h_ext) o[(long)nseg * Kin + H + (c - Kin)] = f32_to_f16((w - hf) * 64.0f);
      continue;
    }
    o[c] = h;
    if (nseg >= 2) o[Kin + c] = f32_to_f16(hf * (1.0f / 64.0f));
    if (nseg >= 3) o[2L * Kin + c] = f32_to_f16((w - hf) * 64.0f);
  }
}
extern "C" int evc_cast_f32_to_f16_wide(const float* in, int64_t ld_in, int R, int Kin, int H, int nseg, int h_ext, evc_f16* out, void* stream) {
  EVC_REQUIRE(R > 0 && Kin > 0 && H >= 0 && nseg >= 1 && nseg <= 3 && (h_ext == 0 || h_ext == 1), EVC_ERR_BAD_SHAPE,
              "evc_cast_f32_to_f16_wide: bad shape / nseg=%d / h_ext=%d", nseg, h_ext);
  const long n = (long)R * (Kin + H);
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_f16_wide_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, Kin, H, nseg, h_ext, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// Activation rows for evc_gemm_nt_f16_fp8: out rows of 4C bytes = [f16(x) (C halfwords) | e4m3(x 2^hi_exp) (C bytes) | e4m3((x - f16(x)) 2^lo_exp) (C bytes)]
// (the layout evc_l2norm_chunk_fwd's aux_mode 5 writes for the input frames, for any other operand: the state in front of the MoE head).
__global__ void cast_f16_fp8x_kernel(const float* __restrict__ in, long ld_in, int R, int C, float hi_scale, float lo_scale, bf16_t* __restrict__ out,
                                     const float* __restrict__ amax_ws, int hi_exp) {
  if (amax_ws) {          // dynamic range: both e4m3 images shifted down by the bits the largest element needs (the reader applies the same shift)
    const float down = ldexpf(1.0f, -fp8_range_drop(amax_ws, hi_exp));
    hi_scale *= down; lo_scale *= down;
  }
  const int c4 = C >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * c4; i += (long)gridDim.x * blockDim.x) {
    const long r = i / c4;
    const int j = (int)(i - r * c4);
    const float4 v = *(const float4*)(in + r * ld_in + j * 4);
    const float x[4] = {v.x, v.y, v.z, v.w};
    const uint32_t h01 = pack_f16x2_hw(x[0], x[1]), h23 = pack_f16x2_hw(x[2], x[3]);
    const float hf[4] = {f16_to_f32((f16_t)(h01 & 0xffffu)), f16_to_f32((f16_t)(h01 >> 16)), f16_to_f32((f16_t)(h23 & 0xffffu)), f16_to_f32((f16_t)(h23 >> 16))};
    float a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = fminf(fmaxf(x[k] * hi_scale, -448.f), 448.f);
      b[k] = fminf(fmaxf((x[k] - hf[k]) * lo_scale, -448.f), 448.f);
    }
    int wa = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
    wa = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], wa, true);
    int wb = __builtin_amdgcn_cvt_pk_fp8_f32(b[0], b[1], 0, false);
    wb = __builtin_amdgcn_cvt_pk_fp8_f32(b[2], b[3], wb, true);
    bf16_t* row = out + r * 2L * C;
    ((uint2*)row)[j] = make_uint2(h01, h23);
    ((int*)(row + C))[j] = wa;
    ((int*)(row + C))[c4 + j] = wb;
  }
}

extern "C" int evc_cast_f32_to_f16_fp8x(const float* in, int64_t ld_in, int R, int C, int hi_exp, int lo_exp, evc_f16* out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 32 == 0 && ld_in % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, EVC_ERR_BAD_ALIGN,
              "evc_cast_f32_to_f16_fp8x: C=%d (%%32: 16-byte aligned row parts), ld_in=%ld (%%4), 16-byte aligned buffers", C, (long)ld_in);
  EVC_REQUIRE(hi_exp >= -30 && hi_exp <= 30 && lo_exp >= 0 && lo_exp <= 60, EVC_ERR_BAD_ARG, "evc_cast_f32_to_f16_fp8x: hi_exp=%d lo_exp=%d", hi_exp, lo_exp);
  const long n = (long)R * (C / 4);
  const int grid = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(cast_f16_fp8x_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, ldexpf(1.0f, hi_exp), ldexpf(1.0f, lo_exp),
                     (bf16_t*)out, (const float*)nullptr, 0);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- dynamic e4m3 range of an activation operand (round 6) ----------------------------------------------------------------------------------
// The state in front of the MoE head is [c | h] of both L2 layers: the cell-state half is unbounded (trained towers: |c| ~ 16 after 512 steps)
// and e4m3(x 2^6) saturates at |x| = 7 - the correction it carries is then partly lost, silently.  evc_absmax_partials leaves EVC_AMAX_SLOTS
// partial maxima of |x| (plain stores: no atomics, nothing to zero, the same bits on every run); the writer of the images
// (evc_cast_f32_to_f16_fp8x_dyn) and the product that reads them (evc_gemm_nt_f16_fp8_dyn) both derive d = fp8_range_drop() from those 64 floats.
__global__ __launch_bounds__(256) void absmax_partials_kernel(const float* __restrict__ in, long ld_in, int R, int C, float* __restrict__ ws) {
  __shared__ float sh[4];
  const int c4 = C >> 2;
  float m = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * c4; i += (long)gridDim.x * blockDim.x) {
    const long r = i / c4;
    const float4 v = *(const float4*)(in + r * ld_in + (i - r * c4) * 4);
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
extern "C" int evc_absmax_partials(const float* in, int64_t ld_in, int R, int C, float* ws, void* stream) {
  EVC_REQUIRE(in && ws && R > 0 && C > 0 && C % 4 == 0 && ld_in % 4 == 0 && ((uintptr_t)in % 16) == 0, EVC_ERR_BAD_ALIGN,
              "evc_absmax_partials: C=%d, ld_in=%ld must be multiples of 4, 16-byte aligned input", C, (long)ld_in);
  hipLaunchKernelGGL(absmax_partials_kernel, dim3(EVC_AMAX_SLOTS), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, ws);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_cast_f32_to_f16_fp8x_dyn(const float* in, int64_t ld_in, int R, int C, int hi_exp, int lo_exp, const float* amax_ws, evc_f16* out,
                                            void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 32 == 0 && ld_in % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, EVC_ERR_BAD_ALIGN,
              "evc_cast_f32_to_f16_fp8x_dyn: C=%d (%%32: 16-byte aligned row parts), ld_in=%ld (%%4), 16-byte aligned buffers", C, (long)ld_in);
  EVC_REQUIRE(hi_exp >= -30 && hi_exp <= 30 && lo_exp >= 0 && lo_exp <= 60 && amax_ws, EVC_ERR_BAD_ARG,
              "evc_cast_f32_to_f16_fp8x_dyn: hi_exp=%d lo_exp=%d amax_ws=%p", hi_exp, lo_exp, (const void*)amax_ws);
  const long n = (long)R * (C / 4);
  const int grid = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(cast_f16_fp8x_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, ldexpf(1.0f, hi_exp), ldexpf(1.0f, lo_exp),
                     (bf16_t*)out, amax_ws, hi_exp);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// Low-order halves of an f32 matrix next to its f16 image, as OCP e4m3: lo(w) = e4m3(clamp((w - f16(w)) * 2^lo_exp, +-448)) - the B8 operand
// of evc_lstm_layer_fwd_f16_fp8lo (|w - f16(w)| <= 2^-12 |w|: with lo_exp = 17 weights up to |w| < 4 stay below 448 and those above ~2^-13 keep
// 3-4 significant bits of their low-order half).  hi_cols > 0 (the layer that reads the input frames): behind the first hi_cols columns'
// low-order halves comes a full-value image of those columns, hi(w) = e4m3(clamp(w * 2^hi_exp)) - what the INPUT's low-order half
// e4m3((x - f16(x)) 2^18) is contracted against: out rows [lo(W[:, :hi_cols]) | hi(W[:, :hi_cols]) | lo(W[:, hi_cols:])].
// hi_tail (round 6): the columns behind the first hi_cols get their full-value image too - rows [lo(A) | hi(A) | lo(B) | hi(B)] with A = W[:, :hi_cols],
// B = the rest (2C bytes): what a step contracts [a8 | a_lo8 | b8 | b_lo8] activation rows against (both operands' roundings corrected).
__global__ void cast_fp8_lo_kernel(const float* __restrict__ in, long ld_in, int R, int C, float lo_scale, int hi_cols, float hi_scale,
                                   uint8_t* __restrict__ out, long ld_out, int hi_tail) {
  const int c4 = C >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)R * c4; i += (long)gridDim.x * blockDim.x) {
    const long r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const float4 v = *(const float4*)(in + r * ld_in + c);
    const float x[4] = {v.x, v.y, v.z, v.w};
    float d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = fminf(fmaxf((x[k] - f16_to_f32(f32_to_f16(x[k]))) * lo_scale, -448.f), 448.f);
    int w8 = __builtin_amdgcn_cvt_pk_fp8_f32(d[0], d[1], 0, false);
    w8 = __builtin_amdgcn_cvt_pk_fp8_f32(d[2], d[3], w8, true);
    *(int*)(out + r * ld_out + (c < hi_cols ? c : c + hi_cols)) = w8;
    if (c < hi_cols || hi_tail) {
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = fminf(fmaxf(x[k] * hi_scale, -448.f), 448.f);
      int h8 = __builtin_amdgcn_cvt_pk_fp8_f32(d[0], d[1], 0, false);
      h8 = __builtin_amdgcn_cvt_pk_fp8_f32(d[2], d[3], h8, true);
      *(int*)(out + r * ld_out + (c < hi_cols ? hi_cols + c : (long)C + c)) = h8;      // (B part: 2 hi_cols + (C - hi_cols) + (c - hi_cols))
    }
  }
}

static int cast_fp8_lo_impl(const float* in, int64_t ld_in, int R, int C, int lo_exp, int hi_cols, int hi_exp, int hi_tail, uint8_t* out, int64_t ld_out,
                            void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 4) == 0,
              EVC_ERR_BAD_ALIGN, "evc_cast_f32_to_fp8_lo: C=%d, ld_in=%ld, ld_out=%ld must be multiples of 4 (16-byte loads, 4-byte stores)", C, (long)ld_in, (long)ld_out);
  EVC_REQUIRE(lo_exp >= 0 && lo_exp <= 60 && hi_cols >= 0 && hi_cols <= C && hi_cols % 4 == 0 && hi_exp >= -30 && hi_exp <= 30 &&
              ld_out >= (hi_tail ? 2L * C : (long)C + hi_cols), EVC_ERR_BAD_ARG,
              "evc_cast_f32_to_fp8_lo: lo_exp=%d hi_cols=%d (%%4, <= C) hi_exp=%d ld_out=%ld (>= C + hi_cols; with hi_tail 2C)", lo_exp, hi_cols, hi_exp, (long)ld_out);
  const long n = (long)R * (C / 4);
  const int grid = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(cast_fp8_lo_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, ldexpf(1.0f, lo_exp), hi_cols,
                     ldexpf(1.0f, hi_exp), out, ld_out, hi_tail);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_cast_f32_to_fp8_lo(const float* in, int64_t ld_in, int R, int C, int lo_exp, int hi_cols, int hi_exp, uint8_t* out, int64_t ld_out,
                                      void* stream) {
  return cast_fp8_lo_impl(in, ld_in, R, C, lo_exp, hi_cols, hi_exp, 0, out, ld_out, stream);
}
// ... with the full-value image of EVERY column: out rows [lo(W[:, :hi_cols]) | hi(W[:, :hi_cols]) | lo(W[:, hi_cols:]) | hi(W[:, hi_cols:])] (2C bytes;
// hi_cols = 0: [lo(W) | hi(W)]) - the B8 rows of the h_lo = 1 forms of evc_lstm_layer_fwd_f16_fp8lo / evc_lstm_stack2_fwd_f16_fp8lo (round 6).
extern "C" int evc_cast_f32_to_fp8_lohi(const float* in, int64_t ld_in, int R, int C, int lo_exp, int hi_cols, int hi_exp, uint8_t* out, int64_t ld_out,
                                        void* stream) {
  return cast_fp8_lo_impl(in, ld_in, R, C, lo_exp, hi_cols, hi_exp, 1, out, ld_out, stream);
}

// K-extended f16 image of an ACTIVATION matrix [R][C] f32: out rows [f16(x) | (x - f16(x))*64 | f16(x)/64] (the first nseg segments) -
// what evc_l2norm_chunk_fwd's aux_mode writes for the input frames, for any other operand (the L2 level's input: the L1 states).
__global__ void cast_f16_segs_kernel(const float* __restrict__ in, long ld_in, int R, int C, int nseg, f16_t* __restrict__ out) {
  const long n = (long)R * C, ldo = (long)nseg * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i % C);
    const float x = in[r * ld_in + c];
    const f16_t h = f32_to_f16(x);
    const float hf = f16_to_f32(h);
    f16_t* o = out + r * ldo;
    o[c] = h;
    if (nseg >= 2) o[C + c] = f32_to_f16((x - hf) * 64.0f);
    if (nseg >= 3) o[2L * C + c] = f32_to_f16(hf * (1.0f / 64.0f));
  }
}
extern "C" int evc_cast_f32_to_f16_segs(const float* in, int64_t ld_in, int R, int C, int nseg, evc_f16* out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && nseg >= 1 && nseg <= 3, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_f16_segs: bad shape / nseg=%d", nseg);
  const long n = (long)R * C;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_f16_segs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, nseg, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// IEEE f16 image of an LSTM kernel with BOTH parts K-extended by the weights' low-order halves (evc_lstm_stack2_fwd_f16, upper layer):
// out row = [f16(Wx) | (Wx - f16(Wx))*64 | f16(Wh) | (Wh - f16(Wh))*64] (2Kin + 2H), in = [Wx(Kin) | Wh(H)] f32.
__global__ void cast_f16_wlo_kernel(const float* __restrict__ in, long ld_in, int R, int Kin, int H, f16_t* __restrict__ out) {
  const int C = Kin + H;
  const long n = (long)R * C, ldo = 2L * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C;
    const int c = (int)(i % C);
    const float w = in[r * ld_in + c];
    const f16_t h = f32_to_f16(w);
    const f16_t l = f32_to_f16((w - f16_to_f32(h)) * 64.0f);
    f16_t* o = out + r * ldo;
    if (c < Kin) { o[c] = h; o[Kin + c] = l; }
    else { o[2L * Kin + (c - Kin)] = h; o[2L * Kin + H + (c - Kin)] = l; }
  }
}
extern "C" int evc_cast_f32_to_f16_wlo(const float* in, int64_t ld_in, int R, int Kin, int H, evc_f16* out, void* stream) {
  EVC_REQUIRE(R > 0 && Kin > 0 && H > 0, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_f16_wlo: bad shape");
  const long n = (long)R * (Kin + H);
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_f16_wlo_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, Kin, H, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// wide split-bf16 image of a [R][C] f32 matrix: out row = [lo | hi] (lo_first, the A operand of evc_gemm_nt_split) or [hi | lo]
// (its B operand), hi = bf16(x), lo = bf16(x - hi); out rows have ld_out >= 2C elements.
__global__ void cast_split_wide_kernel(const float* __restrict__ in, long ld_in, int R, int C, bf16_t* __restrict__ out, long ld_out, int lo_first) {
  const long n4 = (long)R * (C >> 2);
  const int cv = C >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cv;
    const int c = (int)(i % cv) * 4;
    const float4 f = *(const float4*)(in + r * ld_in + c);
    const uint32_t h0 = pack_bf16x2_hw(f.x, f.y), h1 = pack_bf16x2_hw(f.z, f.w);
    const float l0 = f.x - __uint_as_float(h0 << 16), l1 = f.y - __uint_as_float(h0 & 0xffff0000u);
    const float l2 = f.z - __uint_as_float(h1 << 16), l3 = f.w - __uint_as_float(h1 & 0xffff0000u);
    bf16_t* o = out + r * ld_out + c;
    *(uint2*)(o + (lo_first ? C : 0)) = make_uint2(h0, h1);
    *(uint2*)(o + (lo_first ? 0 : C)) = make_uint2(pack_bf16x2_hw(l0, l1), pack_bf16x2_hw(l2, l3));
  }
}
extern "C" int evc_cast_f32_to_bf16_wide(const float* in, int64_t ld_in, int R, int C, evc_bf16* out, int64_t ld_out, int lo_first, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ld_out >= 2L * C && ((uintptr_t)in % 16) == 0 &&
              ((uintptr_t)out % 8) == 0, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_bf16_wide: C=%d, ld_in=%ld, ld_out=%ld must be multiples of 4, ld_out >= 2C, aligned",
              C, (long)ld_in, (long)ld_out);
  const long n = (long)R * (C / 4);
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_split_wide_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, out, ld_out, lo_first);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// split-bf16: hi = bf16(x), lo = bf16(x - hi): hi + lo carries ~16 mantissa bits of x
__global__ void cast_split_kernel(const float* __restrict__ in, long ld_in, int R, int C, bf16_t* __restrict__ hi,
                                  bf16_t* __restrict__ lo, long ld_out) {
  const long n = (long)R * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C, c = i % C;
    const float x = in[r * ld_in + c];
    const bf16_t h = f32_to_bf16(x);
    hi[r * ld_out + c] = h;
    lo[r * ld_out + c] = f32_to_bf16(x - bf16_to_f32(h));
  }
}
extern "C" int evc_cast_f32_to_bf16_split(const float* in, int64_t ld_in, int R, int C, evc_bf16* hi, evc_bf16* lo,
                                          int64_t ld_out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_cast_f32_to_bf16_split: bad shape");
  const long n = (long)R * C;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(cast_split_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, R, C, hi, lo, ld_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ __launch_bounds__(256) void rowsum_bf16_kernel(const bf16_t* __restrict__ in, long ld, int C, float* __restrict__ out) {
  __shared__ float sh[4];
  const bf16_t* row = in + (long)blockIdx.x * ld;
  float s = 0.f;
  const int nv = C >> 3;
  for (int j = threadIdx.x; j < nv; j += 256) {
    const uint4 q = ((const uint4*)row)[j];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) s += __uint_as_float(w[k] << 16) + __uint_as_float(w[k] & 0xffff0000u);
  }
  for (int j = (nv << 3) + threadIdx.x; j < C; j += 256) s += bf16_to_f32(row[j]);
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
extern "C" int evc_rowsum_bf16(const evc_bf16* in, int64_t ld_in, int R, int C, float* out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && ld_in % 8 == 0, EVC_ERR_BAD_SHAPE, "evc_rowsum_bf16: bad shape");
  hipLaunchKernelGGL(rowsum_bf16_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, in, ld_in, C, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// column sums of a bf16 [R][C] matrix (bias gradient straight from dz, no transposed copy):
// out[perm(c)] += sum_r in[r][c]; a wave reads 1 KiB contiguous per row (16 B per lane).
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ in, long ld, int R, int C, int il_H,
                                                          float* __restrict__ out) {
  const int c8 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c8 >= C) return;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const uint4 q = *(const uint4*)(in + (long)r * ld + c8);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { s[2 * k] += __uint_as_float(w[k] << 16); s[2 * k + 1] += __uint_as_float(w[k] & 0xffff0000u); }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c8 + k;
    const int co = il_H > 0 ? (c & 3) * il_H + (c >> 2) : c;     // gate-interleaved column u*4+g -> TF position g*H+u
    atomicAdd(&out[co], s[k]);
  }
}
// The same sums without atomics (EVC_DETERMINISTIC): row block y writes its partial column sums to ws[y][C] (plain stores), a second
// launch adds the gy partial rows in index order.
__global__ __launch_bounds__(256) void colsum_bf16_partial_kernel(const bf16_t* __restrict__ in, long ld, int R, int C, float* __restrict__ ws) {
  const int c8 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c8 >= C) return;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const uint4 q = *(const uint4*)(in + (long)r * ld + c8);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { s[2 * k] += __uint_as_float(w[k] << 16); s[2 * k + 1] += __uint_as_float(w[k] & 0xffff0000u); }
  }
  float* o = ws + (long)blockIdx.y * C + c8;
  *(float4*)o = make_float4(s[0], s[1], s[2], s[3]);
  *(float4*)(o + 4) = make_float4(s[4], s[5], s[6], s[7]);
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ ws, int gy, int C, int il_H, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int y = 0; y < gy; ++y) s += ws[(long)y * C + c];
  out[il_H > 0 ? (c & 3) * il_H + (c >> 2) : c] = s;
}
extern "C" int evc_colsum_bf16_det(const evc_bf16* in, int64_t ld_in, int R, int C, int deinterleave_H, float* out, float* ws, int ws_rows, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 8 == 0 && ld_in % 8 == 0 && ((uintptr_t)in % 16) == 0 && ws && ws_rows >= 1 && ((uintptr_t)ws % 16) == 0, EVC_ERR_BAD_SHAPE,
              "evc_colsum_bf16_det: bad shape / workspace");
  EVC_REQUIRE(deinterleave_H == 0 || C == 4 * deinterleave_H, EVC_ERR_BAD_SHAPE, "evc_colsum_bf16_det: deinterleave_H needs C == 4*H");
  hipStream_t st = (hipStream_t)stream;
  int gy = R / 64; gy = gy < 1 ? 1 : (gy > ws_rows ? ws_rows : gy);
  hipLaunchKernelGGL(colsum_bf16_partial_kernel, dim3(ceil_div(C / 8, 256), gy), dim3(256), 0, st, (const bf16_t*)in, (long)ld_in, R, C, ws);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, st, (const float*)ws, gy, C, deinterleave_H, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_colsum_bf16(const evc_bf16* in, int64_t ld_in, int R, int C, int deinterleave_H, float* out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && C % 8 == 0 && ld_in % 8 == 0 && ((uintptr_t)in % 16) == 0, EVC_ERR_BAD_SHAPE, "evc_colsum_bf16: bad shape");
  EVC_REQUIRE(deinterleave_H == 0 || C == 4 * deinterleave_H, EVC_ERR_BAD_SHAPE, "evc_colsum_bf16: deinterleave_H needs C == 4*H");
  hipStream_t st = (hipStream_t)stream;
  EVC_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float) * C, st));
  const int gx = ceil_div(C / 8, 256);
  int gy = R / 64; gy = gy < 1 ? 1 : (gy > 512 ? 512 : gy);
  if (evc_deterministic()) gy = 1;                  // one adder per column (large R: evc_colsum_bf16_det)
  hipLaunchKernelGGL(colsum_bf16_kernel, dim3(gx, gy), dim3(256), 0, st, in, ld_in, R, C, deinterleave_H, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// a5: MoE tail
// ---------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ float moe_elem(const float* ga, const float* ea, float* g, float* e) {
  float mx = ga[0];
#pragma unroll
  for (int m = 1; m <= M; ++m) mx = fmaxf(mx, ga[m]);
  float den = 0.f;
#pragma unroll
  for (int m = 0; m <= M; ++m) { g[m] = __expf(ga[m] - mx); den += g[m]; }
  const float inv = 1.f / den;
  float p = 0.f;
#pragma unroll
  for (int m = 0; m <= M; ++m) g[m] *= inv;
#pragma unroll
  for (int m = 0; m < M; ++m) { e[m] = sigmoidf_(ea[m]); p += g[m] * e[m]; }
  return p;
}

template <int M>
__global__ __launch_bounds__(256) void moe_tail_fwd_kernel(const float* __restrict__ gl, const float* __restrict__ el, int V,
                                                           float* __restrict__ pred, float* __restrict__ rowsum) {
  __shared__ float sh[4];
  const int b = blockIdx.x;
  const float* gr = gl + (long)b * V * (M + 1);
  const float* er = el + (long)b * V * M;
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) {
    float ga[M + 1], ea[M], g[M + 1], e[M];
#pragma unroll
    for (int m = 0; m <= M; ++m) ga[m] = gr[c * (M + 1) + m];
#pragma unroll
    for (int m = 0; m < M; ++m) ea[m] = er[c * M + m];
    const float p = moe_elem<M>(ga, ea, g, e);
    pred[(long)b * V + c] = p;
    s += p;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0 && rowsum) rowsum[b] = s;
}

template <int M>
__global__ __launch_bounds__(256) void moe_tail_bwd_kernel(const float* __restrict__ gl, const float* __restrict__ el,
                                                           const float* __restrict__ dpred, int V,
                                                           bf16_t* __restrict__ dg, long ld_dg, bf16_t* __restrict__ de, long ld_de) {
  const int b = blockIdx.x;
  const float* gr = gl + (long)b * V * (M + 1);
  const float* er = el + (long)b * V * M;
  for (int c = threadIdx.x; c < V; c += 256) {
    float ga[M + 1], ea[M], g[M + 1], e[M];
#pragma unroll
    for (int m = 0; m <= M; ++m) ga[m] = gr[c * (M + 1) + m];
#pragma unroll
    for (int m = 0; m < M; ++m) ea[m] = er[c * M + m];
    moe_elem<M>(ga, ea, g, e);
    const float dp = dpred[(long)b * V + c];
    float sdot = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) sdot += dp * e[m] * g[m];
#pragma unroll
    for (int m = 0; m <= M; ++m) {
      const float dgm = (m < M) ? dp * e[m < M ? m : 0] : 0.f;
      dg[(long)b * ld_dg + c * (M + 1) + m] = f32_to_bf16(g[m] * (dgm - sdot));
    }
#pragma unroll
    for (int m = 0; m < M; ++m) de[(long)b * ld_de + c * M + m] = f32_to_bf16(dp * g[m] * e[m] * (1.f - e[m]));
  }
}

#define MOE_DISPATCH(KERNEL, ...)                                                                              \
  switch (M) {                                                                                                 \
    case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(B), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;     \
    case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(B), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;     \
    case 3: hipLaunchKernelGGL(KERNEL<3>, dim3(B), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;     \
    case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(B), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); break;     \
    default: evc_set_error("moe: num_mixtures=%d unsupported (1..4)", M); return EVC_ERR_BAD_SHAPE;            \
  }

extern "C" int evc_moe_tail_fwd(const float* gate_logits, const float* expert_logits, int B, int V, int M,
                                float* pred, float* rowsum, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0, EVC_ERR_BAD_SHAPE, "evc_moe_tail_fwd: bad shape");
  MOE_DISPATCH(moe_tail_fwd_kernel, gate_logits, expert_logits, V, pred, rowsum);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_moe_tail_bwd(const float* gate_logits, const float* expert_logits, const float* dpred,
                                int B, int V, int M, evc_bf16* dgate, int64_t ld_dgate,
                                evc_bf16* dexpert, int64_t ld_dexpert, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0, EVC_ERR_BAD_SHAPE, "evc_moe_tail_bwd: bad shape");
  MOE_DISPATCH(moe_tail_bwd_kernel, gate_logits, expert_logits, dpred, V, dgate, (long)ld_dgate, dexpert, (long)ld_dexpert);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// a6 + a7: losses.  grid-stride, block partials, one atomic per block.
// ---------------------------------------------------------------------------
// part != NULL (EVC_DETERMINISTIC=1, round 5): every block leaves its partial sum in part[blockIdx.x] instead of an atomic on *loss, and
// loss_partials_finish_kernel adds them in block order - the full grid computes the gradient (round 4 ran ONE block over the 1.2 M elements so
// that the loss scalar had a fixed summation order: 2.5 ms per call on the critical path of the deterministic step).
__global__ __launch_bounds__(256) void loss_partials_finish_kernel(const float* __restrict__ part, int n, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += part[i];
    *loss += s;
  }
}

__global__ __launch_bounds__(256) void ce_loss_kernel(const float* __restrict__ p, const uint8_t* __restrict__ y, long n,
                                                      float inv_b, float gs, float* __restrict__ loss,
                                                      float* __restrict__ dp, int acc, float* __restrict__ part = nullptr) {
  __shared__ float sh[4];
  float s = 0.f;
  const float eps = 10e-6f;   // cs/losses.py:92
  // 4 elements per thread and trip (16-byte loads / stores) where the arrays allow it: 2.4 M elements on 256 workgroups were 37 dependent scalar trips
  const bool v4 = (n & 3) == 0 && ((uintptr_t)p & 15) == 0 && ((uintptr_t)y & 3) == 0 && (!dp || ((uintptr_t)dp & 15) == 0);
  if (v4) {
    for (long i4 = (long)blockIdx.x * 256 + threadIdx.x; i4 < (n >> 2); i4 += (long)gridDim.x * 256) {
      const float4 pq = ((const float4*)p)[i4];
      const uchar4 yq = ((const uchar4*)y)[i4];
      const float pv[4] = {pq.x, pq.y, pq.z, pq.w};
      const bool pos[4] = {yq.x != 0, yq.y != 0, yq.z != 0, yq.w != 0};
      float g[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = pv[r] + eps, bq = 1.f - pv[r] + eps;
        s -= pos[r] ? __logf(a) : __logf(bq);
        g[r] = (pos[r] ? -1.f / a : 1.f / bq) * gs;
      }
      if (dp) {
        float4 o = make_float4(g[0], g[1], g[2], g[3]);
        if (acc) { const float4 d = ((const float4*)dp)[i4]; o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w; }
        ((float4*)dp)[i4] = o;
      }
    }
  } else
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float pv = p[i];
    const bool pos = y[i] != 0;
    const float a = pv + eps, bq = 1.f - pv + eps;
    s -= pos ? __logf(a) : __logf(bq);
    if (dp) {
      const float g = (pos ? -1.f / a : 1.f / bq) * gs;
      dp[i] = acc ? dp[i] + g : g;
    }
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    if (part) part[blockIdx.x] = s * inv_b;
    else atomicAdd(loss, s * inv_b);
  }
}
static int ce_loss_impl(const float* pred, const uint8_t* labels, int B, int V, float grad_scale, float* loss, float* dpred, int accumulate_grad,
                        float* partials, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0, EVC_ERR_BAD_SHAPE, "evc_ce_loss: bad shape");
  const long n = (long)B * V;
  // every block ends in one atomic on the same address, and those serialise at ~12 ns each: 2048 blocks made this a
  // 30 us kernel for 1.2 M elements; 256 blocks (one per CU) keep the join at ~3 us
  int grid = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
  if (evc_deterministic() && !partials) grid = 1;               // no workspace: one block is the only fixed order available
  hipLaunchKernelGGL(ce_loss_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred, labels, n, 1.0f / B, grad_scale, loss,
                     dpred, accumulate_grad, partials);
  if (partials) hipLaunchKernelGGL(loss_partials_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)partials, grid, loss);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_ce_loss(const float* pred, const uint8_t* labels, int B, int V, float grad_scale,
                           float* loss, float* dpred, int accumulate_grad, void* stream) {
  return ce_loss_impl(pred, labels, B, V, grad_scale, loss, dpred, accumulate_grad, nullptr, stream);
}
extern "C" int evc_ce_loss_ordered(const float* pred, const uint8_t* labels, int B, int V, float grad_scale,
                                   float* loss, float* dpred, int accumulate_grad, float* partials, void* stream) {
  EVC_REQUIRE(partials, EVC_ERR_BAD_ARG, "evc_ce_loss_ordered: partials (256 floats of scratch) is required");
  return ce_loss_impl(pred, labels, B, V, grad_scale, loss, dpred, accumulate_grad, partials, stream);
}

__global__ __launch_bounds__(256) void kl_loss_kernel(const float* __restrict__ pt, const float* __restrict__ st,
                                                      const float* __restrict__ ps, const float* __restrict__ ss, int V,
                                                      float gs, float* __restrict__ loss, float* __restrict__ dps, int acc,
                                                      float* __restrict__ part = nullptr) {
  __shared__ float sh[4];
  const int b = blockIdx.x;
  // Degenerate rows (only reached once a tower has collapsed, e.g. on random labels after a few Adam steps, where
  // TF's log(0) / 0-division NaNs make slim's check_numerics abort the reference run): keep every value finite.
  //  * teacher row sum below the smallest normal float: the renormalised teacher distribution is 0/0 - the row
  //    contributes nothing (loss 0, gradient 0);
  //  * student probabilities / row sum are clamped at FLT_MIN inside log and 1/q.
  // Wherever the reference's result is finite these clamps are inactive.
  const float FMIN = 1.17549435e-38f;
  const bool t_ok = st[b] >= FMIN;
  const float it = t_ok ? 1.f / st[b] : 0.f, is = 1.f / fmaxf(ss[b], FMIN);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) {
    const long i = (long)b * V + c;
    const float P = pt[i] * it, q = fmaxf(ps[i], FMIN);
    // 0*log(0) := 0 (its limit).  TF evaluates 0*(-inf) = NaN here and slim's
    // check_numerics then aborts the reference run; see DESIGN.md "deviations".
    if (P >= FMIN) s += P * (__logf(P) - __logf(fmaxf(q * is, FMIN)));
    if (dps) {
      const float g = t_ok ? (-P / q + is) * gs : 0.f;
      dps[i] = acc ? dps[i] + g : g;
    }
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    if (part) part[b] = s;
    else atomicAdd(loss, s);
  }
}
static int kl_pred_loss_impl(const float* pred_t, const float* rowsum_t, const float* pred_s, const float* rowsum_s, int B, int V, float grad_scale,
                             float* loss, float* dpred_s, int accumulate_grad, float* partials, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0, EVC_ERR_BAD_SHAPE, "evc_kl_pred_loss: bad shape");
  hipLaunchKernelGGL(kl_loss_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pred_t, rowsum_t, pred_s, rowsum_s, V,
                     grad_scale, loss, dpred_s, accumulate_grad, partials);
  if (partials) hipLaunchKernelGGL(loss_partials_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)partials, B, loss);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_kl_pred_loss(const float* pred_t, const float* rowsum_t, const float* pred_s, const float* rowsum_s,
                                int B, int V, float grad_scale, float* loss, float* dpred_s, int accumulate_grad,
                                void* stream) {
  return kl_pred_loss_impl(pred_t, rowsum_t, pred_s, rowsum_s, B, V, grad_scale, loss, dpred_s, accumulate_grad, nullptr, stream);
}
// the row sums joined in row order instead of by float atomics (EVC_DETERMINISTIC=1 callers): partials = B floats of scratch
extern "C" int evc_kl_pred_loss_ordered(const float* pred_t, const float* rowsum_t, const float* pred_s, const float* rowsum_s,
                                        int B, int V, float grad_scale, float* loss, float* dpred_s, int accumulate_grad,
                                        float* partials, void* stream) {
  EVC_REQUIRE(partials, EVC_ERR_BAD_ARG, "evc_kl_pred_loss_ordered: partials (B floats of scratch) is required");
  return kl_pred_loss_impl(pred_t, rowsum_t, pred_s, rowsum_s, B, V, grad_scale, loss, dpred_s, accumulate_grad, partials, stream);
}

__global__ __launch_bounds__(256) void rep_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, long n,
                                                       float inv_b, float gs, float* __restrict__ loss,
                                                       float* __restrict__ db, int acc, float* __restrict__ part = nullptr) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = a[i] - b[i];
    s += d * d;
    if (db) {
      const float g = -2.f * d * inv_b * gs;
      db[i] = acc ? db[i] + g : g;
    }
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    if (part) part[blockIdx.x] = s * inv_b;
    else atomicAdd(loss, s * inv_b);
  }
}
static int rep_loss_impl(const float* state_t, const float* state_s, int B, int D, float grad_scale, float* loss, float* dstate_s,
                         int accumulate_grad, float* partials, void* stream) {
  EVC_REQUIRE(B > 0 && D > 0, EVC_ERR_BAD_SHAPE, "evc_rep_loss: bad shape");
  const long n = (long)B * D;
  int grid = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);     // one same-address atomic per block (see evc_ce_loss)
  if (evc_deterministic() && !partials) grid = 1;
  hipLaunchKernelGGL(rep_loss_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, state_t, state_s, n, 1.0f / B, grad_scale,
                     loss, dstate_s, accumulate_grad, partials);
  if (partials) hipLaunchKernelGGL(loss_partials_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)partials, grid, loss);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_rep_loss(const float* state_t, const float* state_s, int B, int D, float grad_scale,
                            float* loss, float* dstate_s, int accumulate_grad, void* stream) {
  return rep_loss_impl(state_t, state_s, B, D, grad_scale, loss, dstate_s, accumulate_grad, nullptr, stream);
}
extern "C" int evc_rep_loss_ordered(const float* state_t, const float* state_s, int B, int D, float grad_scale,
                                    float* loss, float* dstate_s, int accumulate_grad, float* partials, void* stream) {
  EVC_REQUIRE(partials, EVC_ERR_BAD_ARG, "evc_rep_loss_ordered: partials (256 floats of scratch) is required");
  return rep_loss_impl(state_t, state_s, B, D, grad_scale, loss, dstate_s, accumulate_grad, partials, stream);
}

// The loss section of the SERIAL distillation step (frozen teacher, DistillGraph(mode="serial")) as one launch: the teacher's CE (value
// only), L_REP, L_PRED and the student's CE with dpred_s = g_ce dCE_s + g_kl dKL written ONCE and dstate_s = g_rep dREP.  Workgroups
// [0, B): one prediction row each (pred_t, pred_s and the labels are read once); workgroups [B, B + NS): the [B, D] state part, grid-stride.
// The per-element arithmetic is that of ce_loss_kernel / kl_loss_kernel / rep_loss_kernel above (same eps, same degenerate-row rules).
// Every workgroup leaves its partial sums in the workspace - ws[0..B) teacher CE, [B..2B) L_PRED, [2B..3B) student CE, [3B..3B+NS) L_REP -
// and distill_losses_finish_kernel adds each list in block order: the same bits on every call, in every mode.  A scale of 0 switches its
// term off exactly (0, not 0 * inf).
struct DistillElem { float ce_t, kl, ce_s, g; };
__device__ __forceinline__ DistillElem distill_elem(float pt, float ps, bool pos, float it, float is, bool t_ok, float g_ce, float g_kl) {
  const float eps = 10e-6f;   // cs/losses.py:92
  const float FMIN = 1.17549435e-38f;
  DistillElem r;
  const float at = pt + eps, bt = 1.f - pt + eps;
  r.ce_t = -(pos ? __logf(at) : __logf(bt));
  const float a = ps + eps, bq = 1.f - ps + eps;
  r.ce_s = -(pos ? __logf(a) : __logf(bq));
  const float P = pt * it, q = fmaxf(ps, FMIN);
  r.kl = (P >= FMIN) ? P * (__logf(P) - __logf(fmaxf(q * is, FMIN))) : 0.f;
  const float gce = (g_ce != 0.f) ? (pos ? -1.f / a : 1.f / bq) * g_ce : 0.f;
  const float gkl = (t_ok && g_kl != 0.f) ? (-P / q + is) * g_kl : 0.f;
  r.g = gce + gkl;
  return r;
}

__global__ __launch_bounds__(256) void distill_losses_kernel(const float* __restrict__ pt, const float* __restrict__ st,
                                                             const float* __restrict__ ps, const float* __restrict__ ss,
                                                             const uint8_t* __restrict__ y, const float* __restrict__ a,
                                                             const float* __restrict__ b, int B, int V, long nd, int NS, float inv_b,
                                                             float g_ce, float g_kl, float g_rep, float* __restrict__ dps,
                                                             float* __restrict__ db, float* __restrict__ ws) {
  __shared__ float sh[4];
  if ((int)blockIdx.x < B) {
    const int row = blockIdx.x;
    const float FMIN = 1.17549435e-38f;
    const bool t_ok = st[row] >= FMIN;
    const float it = t_ok ? 1.f / st[row] : 0.f, is = 1.f / fmaxf(ss[row], FMIN);
    const long base = (long)row * V;
    float s_ct = 0.f, s_kl = 0.f, s_cs = 0.f;
    const bool v4 = (V & 3) == 0 && ((uintptr_t)pt & 15) == 0 && ((uintptr_t)ps & 15) == 0 && ((uintptr_t)y & 3) == 0 &&
                    (!dps || ((uintptr_t)dps & 15) == 0);
    if (v4) {
      const float4* pt4 = (const float4*)(pt + base);
      const float4* ps4 = (const float4*)(ps + base);
      const uchar4* y4 = (const uchar4*)(y + base);
      for (int c4 = threadIdx.x; c4 < (V >> 2); c4 += 256) {
        const float4 tq = pt4[c4], sq = ps4[c4];
        const uchar4 yq = y4[c4];
        const float tv[4] = {tq.x, tq.y, tq.z, tq.w}, sv[4] = {sq.x, sq.y, sq.z, sq.w};
        const bool pos[4] = {yq.x != 0, yq.y != 0, yq.z != 0, yq.w != 0};
        float g[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const DistillElem e = distill_elem(tv[r], sv[r], pos[r], it, is, t_ok, g_ce, g_kl);
          s_ct += e.ce_t; s_kl += e.kl; s_cs += e.ce_s; g[r] = e.g;
        }
        if (dps) ((float4*)(dps + base))[c4] = make_float4(g[0], g[1], g[2], g[3]);
      }
    } else {
      for (int c = threadIdx.x; c < V; c += 256) {
        const DistillElem e = distill_elem(pt[base + c], ps[base + c], y[base + c] != 0, it, is, t_ok, g_ce, g_kl);
        s_ct += e.ce_t; s_kl += e.kl; s_cs += e.ce_s;
        if (dps) dps[base + c] = e.g;
      }
    }
    s_ct = block_sum(s_ct, sh);
    s_kl = block_sum(s_kl, sh);
    s_cs = block_sum(s_cs, sh);
    if (threadIdx.x == 0) {
      ws[row] = s_ct * inv_b;
      ws[B + row] = s_kl;
      ws[2 * B + row] = s_cs * inv_b;
    }
    return;
  }
  const int blk = (int)blockIdx.x - B;
  float s = 0.f;
  const bool v4 = (nd & 3) == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && (!db || ((uintptr_t)db & 15) == 0);
  if (v4) {
    for (long i4 = (long)blk * 256 + threadIdx.x; i4 < (nd >> 2); i4 += (long)NS * 256) {
      const float4 aq = ((const float4*)a)[i4], bq = ((const float4*)b)[i4];
      const float d[4] = {aq.x - bq.x, aq.y - bq.y, aq.z - bq.z, aq.w - bq.w};
      float g[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s += d[r] * d[r];
        g[r] = (g_rep != 0.f) ? -2.f * d[r] * inv_b * g_rep : 0.f;
      }
      if (db) ((float4*)db)[i4] = make_float4(g[0], g[1], g[2], g[3]);
    }
  } else {
    for (long i = (long)blk * 256 + threadIdx.x; i < nd; i += (long)NS * 256) {
      const float d = a[i] - b[i];
      s += d * d;
      if (db) db[i] = (g_rep != 0.f) ? -2.f * d * inv_b * g_rep : 0.f;
    }
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) ws[3 * (long)B + blk] = s * inv_b;
}

// One workgroup, four waves: wave w owns loss slot w.  The partials pass through LDS in pieces of 1024 (loaded by all 256 threads), lane 0
// of each wave adds its piece in block order - the order loss_partials_finish_kernel adds in, without a chain of dependent global loads.
__global__ __launch_bounds__(256) void distill_losses_finish_kernel(const float* __restrict__ ws, int B, int NS, float* __restrict__ losses) {
  __shared__ float sh[4][1024];
  // loss slot (DistillGraph.LOSS_SLOTS) -> its list of partials: teacher CE, L_REP, L_PRED, student CE
  const long off[4] = {0, 3 * (long)B, (long)B, 2 * (long)B};
  const int cnt[4] = {B, NS, B, B};
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nmax = B > NS ? B : NS;
  float s = 0.f;
  for (int base = 0; base < nmax; base += 1024) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int i = threadIdx.x; i < 1024; i += 256)
        if (base + i < cnt[k]) sh[k][i] = ws[off[k] + base + i];
    __syncthreads();
    if (lane == 0) {
      const int n = cnt[w] - base < 1024 ? cnt[w] - base : 1024;
      for (int i = 0; i < n; ++i) s += sh[w][i];
    }
  }
  if (lane == 0) losses[w] += s;
}

extern "C" int evc_distill_losses(const float* pred_t, const float* rowsum_t, const float* pred_s, const float* rowsum_s,
                                  const uint8_t* labels, const float* state_t, const float* state_s, int B, int V, int D,
                                  float g_ce, float g_kl, float g_rep, float* losses, float* dpred_s, float* dstate_s,
                                  float* workspace, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0 && D > 0, EVC_ERR_BAD_SHAPE, "evc_distill_losses: bad shape");
  EVC_REQUIRE(pred_t && rowsum_t && pred_s && rowsum_s && labels && state_t && state_s && losses, EVC_ERR_BAD_ARG,
              "evc_distill_losses: a required pointer is NULL");
  EVC_REQUIRE(workspace, EVC_ERR_BAD_ARG, "evc_distill_losses: workspace (3 * B + 256 floats of scratch) is required");
  const long nd = (long)B * D;
  const long want = (nd + 1023) / 1024;                 // 4 elements per thread and trip
  const int NS = (int)(want < 1 ? 1 : (want < 256 ? want : 256));
  hipLaunchKernelGGL(distill_losses_kernel, dim3(B + NS), dim3(256), 0, (hipStream_t)stream, pred_t, rowsum_t, pred_s, rowsum_s, labels,
                     state_t, state_s, B, V, nd, NS, 1.0f / B, g_ce, g_kl, g_rep, dpred_s, dstate_s, workspace);
  hipLaunchKernelGGL(distill_losses_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, B, NS, losses);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// a8 + a9: regulariser, per-tensor clip, TF-Adam
// ---------------------------------------------------------------------------
template <bool WITH_P>
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, const float* __restrict__ p, float l2,
                                                          long n, float* __restrict__ sums) {
  __shared__ float sh[4];
  float sg = 0.f, sp = 0.f;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 gv = ((const float4*)g)[i];
    float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (WITH_P) pv = ((const float4*)p)[i];
    const float a = gv.x + l2 * pv.x, b = gv.y + l2 * pv.y, c = gv.z + l2 * pv.z, d = gv.w + l2 * pv.w;
    sg += a * a + b * b + c * c + d * d;
    sp += pv.x * pv.x + pv.y * pv.y + pv.z * pv.z + pv.w * pv.w;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float pi = WITH_P ? p[i] : 0.f;
    const float a = g[i] + l2 * pi;
    sg += a * a;
    sp += pi * pi;
  }
  sg = block_sum(sg, sh);
  if (WITH_P) sp = block_sum(sp, sh);
  if (threadIdx.x == 0) {
    atomicAdd(&sums[0], sg);
    if (WITH_P) atomicAdd(&sums[1], sp);
  }
}
extern "C" int evc_grad_sqnorm(const float* g, const float* p, float l2_coeff, int64_t n, float* sums, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_grad_sqnorm: n must be positive");
  EVC_REQUIRE(((uintptr_t)g % 16) == 0 && ((uintptr_t)p % 16) == 0, EVC_ERR_BAD_ALIGN, "evc_grad_sqnorm: 16-byte alignment");
  EVC_REQUIRE(p != nullptr || l2_coeff == 0.f, EVC_ERR_BAD_ARG, "evc_grad_sqnorm: p == NULL (gradient norm only) needs l2_coeff == 0");
  const long nb = (n / 4 + 255) / 256;
  int grid = (int)(nb < 1 ? 1 : (nb < 512 ? nb : 512));   // two blocks per CU; each ends in same-address atomics (~12 ns apiece)
  if (evc_deterministic()) grid = 1;                        // one adder: fixed order (the large tensors go through evc_sqnorm2_partials)
  if (p) hipLaunchKernelGGL(grad_sqnorm_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, p, l2_coeff, (long)n, sums);
  else hipLaunchKernelGGL(grad_sqnorm_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, p, 0.f, (long)n, sums);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

template <bool VEC>
__global__ __launch_bounds__(256) void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, float l2, const float* __restrict__ sums,
                                                        float clip, float lr_t, float b1, float b2, float eps,
                                                        bf16_t* __restrict__ pb) {
  float scale = 1.f;
  if (clip > 0.f) {
    const float nrm = sqrtf(sums[0]);
    scale = clip / fmaxf(nrm, clip);   // tf.clip_by_norm
  }
  const long n4 = VEC ? (n >> 2) : 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {   // 16-byte accesses
    const float4 pv = ((const float4*)p)[i], gv = ((const float4*)g)[i], mv = ((const float4*)m)[i], vv = ((const float4*)v)[i];
    const float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
    const float ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
    float pn[4], mn[4], vn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gc = (ga[r] + l2 * pa[r]) * scale;
      mn[r] = b1 * ma[r] + (1.f - b1) * gc;
      vn[r] = b2 * va[r] + (1.f - b2) * gc * gc;
      pn[r] = adam_step_(pa[r], mn[r], vn[r], lr_t, eps);
    }
    ((float4*)m)[i] = make_float4(mn[0], mn[1], mn[2], mn[3]);
    ((float4*)v)[i] = make_float4(vn[0], vn[1], vn[2], vn[3]);
    ((float4*)p)[i] = make_float4(pn[0], pn[1], pn[2], pn[3]);
    if (pb) ((uint2*)pb)[i] = make_uint2(pack_bf16x2_hw(pn[0], pn[1]), pack_bf16x2_hw(pn[2], pn[3]));
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float pv = p[i];
    const float gc = (g[i] + l2 * pv) * scale;
    const float mn = b1 * m[i] + (1.f - b1) * gc;
    const float vn = b2 * v[i] + (1.f - b2) * gc * gc;
    const float pn = adam_step_(pv, mn, vn, lr_t, eps);
    m[i] = mn; v[i] = vn; p[i] = pn;
    if (pb) pb[i] = f32_to_bf16(pn);
  }
}
extern "C" int evc_clip_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float l2_coeff,
                                  const float* sums, float clip_norm, float lr_t, float beta1, float beta2, float eps,
                                  evc_bf16* p_bf16, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_clip_adam_step: n must be positive");
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) == 0 && ((uintptr_t)p_bf16 % 8) == 0;
  const long nb = ((vec ? n / 4 : n) + 255) / 256;
  const int grid = (int)(nb < 1 ? 1 : (nb < 4096 ? nb : 4096));
  if (vec) hipLaunchKernelGGL(clip_adam_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, l2_coeff, sums,
                              clip_norm, lr_t, beta1, beta2, eps, p_bf16);
  else hipLaunchKernelGGL(clip_adam_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, l2_coeff, sums,
                          clip_norm, lr_t, beta1, beta2, eps, p_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// Many SMALL tensors (biases, batch-norm scales / offsets: <= 16 of them, a few thousand elements each) in ONE launch (round 5): workgroup i takes
// tensor i - its squared norm (block sum: a fixed order, no atomics), sums[i] = {|g|^2, 0} as evc_grad_sqnorm leaves it, then per-tensor clip + TF-Adam
// with clip_adam_kernel's arithmetic.  The DBoF step spent 14 launches (7 x grad_sqnorm + 7 x clip_adam, ~4.6 us each) on 12 k parameters.
struct SmallAdamTable {
  float* p[16]; const float* g[16]; float* m[16]; float* v[16]; float* sums[16]; int n[16];
};
__global__ __launch_bounds__(1024) void clip_adam_small_kernel(SmallAdamTable t, float clip, float lr_t, float b1, float b2, float eps) {
  // (1024 threads: one workgroup walks a whole tensor; with 256 an 8 k-element tensor was 2 x 32 dependent trips, 30 us for 12 k parameters)
  __shared__ float sh[16];
  __shared__ float total;
  const int i = blockIdx.x;
  float* __restrict__ p = t.p[i];
  const float* __restrict__ g = t.g[i];
  float* __restrict__ m = t.m[i];
  float* __restrict__ v = t.v[i];
  const int n = t.n[i];
  float s = 0.f;
  for (int k = threadIdx.x; k < n; k += 1024) s += g[k] * g[k];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) {
    total = s;
    t.sums[i][0] = s;
    t.sums[i][1] = 0.f;
  }
  __syncthreads();
  float scale = 1.f;
  if (clip > 0.f) scale = clip / fmaxf(sqrtf(total), clip);
  for (int k = threadIdx.x; k < n; k += 1024) {
    const float pv = p[k];
    const float gc = g[k] * scale;
    const float mn = b1 * m[k] + (1.f - b1) * gc;
    const float vn = b2 * v[k] + (1.f - b2) * gc * gc;
    m[k] = mn; v[k] = vn; p[k] = adam_step_(pv, mn, vn, lr_t, eps);
  }
}
extern "C" int evc_clip_adam_small(int count, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                                   float* const* sums, float clip_norm, float lr_t, float beta1, float beta2, float eps, void* stream) {
  EVC_REQUIRE(count >= 1 && count <= 16 && p && g && m && v && n && sums, EVC_ERR_BAD_ARG, "evc_clip_adam_small: 1..16 tensors (count=%d)", count);
  SmallAdamTable t;
  for (int i = 0; i < count; ++i) {
    EVC_REQUIRE(p[i] && g[i] && m[i] && v[i] && sums[i] && n[i] > 0 && n[i] <= (1 << 15), EVC_ERR_BAD_ARG,
                "evc_clip_adam_small: tensor %d: NULL pointer or size %ld outside 1..2^15 (one workgroup per tensor: larger ones take evc_grad_sqnorm + evc_clip_adam_step)", i, (long)n[i]);
    t.p[i] = p[i]; t.g[i] = g[i]; t.m[i] = m[i]; t.v[i] = v[i]; t.sums[i] = sums[i]; t.n[i] = (int)n[i];
  }
  hipLaunchKernelGGL(clip_adam_small_kernel, dim3(count), dim3(1024), 0, (hipStream_t)stream, t, clip_norm, lr_t, beta1, beta2, eps);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// a11: mean-pool over all padded frames / true n; sigmoid
// ---------------------------------------------------------------------------
// one wave per frame, TS frame-slices per video; per-lane register accumulators, LDS
// reduce across the 4 waves, one atomicAdd per (block, feature).
__global__ __launch_bounds__(256) void meanpool_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                       const int* __restrict__ nfr, int T, int F, int normalize,
                                                       float* __restrict__ avg) {
  __shared__ float red[4][1280];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y, nv = F >> 2;
  float4 acc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  // uint8 input (the reader's representation): frames >= num_frames are padding, i.e. zero after Dequantize
  // (cs/readers.py:170-173) - they add nothing to the sum and are not read
  const int t_end = xq ? min(T, nfr[b]) : T;
  for (int t = blockIdx.x * 4 + w; t < t_end; t += gridDim.x * 4) {
    float4 v[5];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int j = lane + i * 64;
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < nv) {
        if (xq) {                                      // Dequantize cs/utils.py:22-25
          const uchar4 q = ((const uchar4*)(xq + ((long)b * T + t) * F))[j];
          const float sc = 4.0f / 255.0f, bi = 4.0f / 512.0f - 2.0f;
          v[i] = make_float4(q.x * sc + bi, q.y * sc + bi, q.z * sc + bi, q.w * sc + bi);
        } else {
          v[i] = ((const float4*)(x + ((long)b * T + t) * F))[j];
        }
      }
      ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
    float inv = 1.f;
    if (normalize) inv = rsqrtf(fmaxf(wave_sum(ss), 1e-12f));
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      acc[i].x += v[i].x * inv; acc[i].y += v[i].y * inv; acc[i].z += v[i].z * inv; acc[i].w += v[i].w * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int j = lane + i * 64;
    if (j < nv) ((float4*)red[w])[j] = acc[i];
  }
  __syncthreads();
  const float invn = 1.f / (float)nfr[b];
  for (int f = threadIdx.x; f < F; f += 256)
    atomicAdd(&avg[(long)b * F + f], (red[0][f] + red[1][f] + red[2][f] + red[3][f]) * invn);
}
extern "C" int evc_meanpool_fwd(const float* x, const uint8_t* x_u8, const int32_t* num_frames, int B, int T, int F, int normalize,
                                float* avg_f32, evc_bf16* avg_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && F <= 1280 && avg_f32, EVC_ERR_BAD_SHAPE, "evc_meanpool_fwd: bad shape");
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_meanpool_fwd: exactly one of x / x_u8");
  hipStream_t st = (hipStream_t)stream;
  EVC_CHECK_HIP(hipMemsetAsync(avg_f32, 0, sizeof(float) * B * F, st));
  int ts = (T + 31) / 32;
  hipLaunchKernelGGL(meanpool_kernel, dim3(ts, B), dim3(256), 0, st, x, x_u8, num_frames, T, F, normalize, avg_f32);
  EVC_LAUNCH_CHECK();
  if (avg_bf16) return evc_cast_f32_to_bf16(avg_f32, F, B, F, avg_bf16, F, stream);
  return EVC_OK;
}

__global__ void sigmoid_fwd_kernel(float* z, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) z[i] = sigmoidf_(z[i]);
}
__global__ void sigmoid_bwd_kernel(const float* p, const float* dp, long n, bf16_t* dz) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dz[i] = f32_to_bf16(dp[i] * p[i] * (1.f - p[i]));
}
static inline int grid_for(long n) { long nb = (n + 255) / 256; return (int)(nb < 1 ? 1 : (nb < 4096 ? nb : 4096)); }
extern "C" int evc_sigmoid_fwd(float* z, int64_t n, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_sigmoid_fwd: n");
  hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, z, (long)n);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_sigmoid_bwd(const float* p, const float* dp, int64_t n, evc_bf16* dz, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_sigmoid_bwd: n");
  hipLaunchKernelGGL(sigmoid_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, dp, (long)n, dz);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// a10: DBoF pieces
// ---------------------------------------------------------------------------
template <bool SEQUENCE>
__global__ __launch_bounds__(256) void sample_gather_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                            const float* __restrict__ u, const int* __restrict__ nfr, int B, int T, int F,
                                                            int S, int normalize, float* __restrict__ out, int* __restrict__ idx_out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * S) return;
  const int b = (int)(row / S);
  const int n = nfr[b];
  int idx;
  if (SEQUENCE) {
    // SampleRandomSequence (cs/model_utils.py:22-36): start = int32(u[b] * float32(max(n - S, 0) + 1)); index = min(start + s, n - 1)
    const int mx = n - S > 0 ? n - S : 0;
    const int start = (int)(u[b] * (float)(mx + 1));
    const int s_ = (int)(row - (long)b * S);
    idx = start + s_ < n - 1 ? start + s_ : n - 1;
  } else {
    // tf.cast(tf.multiply(random_uniform, tf.cast(num_frames, tf.float32)), tf.int32)
    idx = (int)(u[row] * (float)n);
  }
  if (lane == 0 && idx_out) idx_out[row] = idx;
  idx = idx < 0 ? 0 : (idx >= T ? T - 1 : idx);
  const bool padded = xq && idx >= n;            // uint8 input: frames >= num_frames are padding (zero after Dequantize)
  float4* dst = (float4*)(out + row * F);
  const int F4 = F >> 2;
  auto load = [&](int j) {
    if (padded) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (xq) {                                    // Dequantize cs/utils.py:22-25
      const uchar4 q = ((const uchar4*)(xq + ((long)b * T + idx) * F))[j];
      const float sc = 4.0f / 255.0f, bi = 4.0f / 512.0f - 2.0f;
      return make_float4(q.x * sc + bi, q.y * sc + bi, q.z * sc + bi, q.w * sc + bi);
    }
    return ((const float4*)(x + ((long)b * T + idx) * F))[j];
  };
  float inv = 1.f;
  if (normalize) {   // tf.nn.l2_normalize of the gathered frame (cs/train.py:256 applied before create_model)
    float ss = 0.f;
    for (int j = lane; j < F4; j += 64) { const float4 v = load(j); ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
    inv = rsqrtf(fmaxf(wave_sum(ss), 1e-12f));
  }
  for (int j = lane; j < F4; j += 64) { float4 v = load(j); v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv; dst[j] = v; }
}
extern "C" int evc_sample_frames_gather(const float* x, const uint8_t* x_u8, const float* u, const int32_t* num_frames, int B, int T, int F,
                                        int S, int normalize, float* out, int32_t* idx_out, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && S > 0 && F % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_sample_frames_gather: bad shape");
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_sample_frames_gather: exactly one of x / x_u8");
  const long rows = (long)B * S;
  hipLaunchKernelGGL(sample_gather_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, u, num_frames,
                     B, T, F, S, normalize, out, idx_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// SampleRandomSequence (cs/model_utils.py:11-36, --sample_random_frames False): S consecutive frames from a random start; u [B] (one draw per video)
extern "C" int evc_sample_sequence_gather(const float* x, const uint8_t* x_u8, const float* u, const int32_t* num_frames, int B, int T, int F,
                                          int S, int normalize, float* out, int32_t* idx_out, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && S > 0 && F % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_sample_sequence_gather: bad shape");
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_sample_sequence_gather: exactly one of x / x_u8");
  const long rows = (long)B * S;
  hipLaunchKernelGGL(sample_gather_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, u, num_frames,
                     B, T, F, S, normalize, out, idx_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- a10, non-default branches (cs/frame_level_models.py:138-187 with --dbof_add_batch_norm False, cs/model_utils.py:75-76 'average'):
// plain relu6 forward / backward on a pre-activation that already carries its bias, and mean pooling over the S frames of a video
__global__ __launch_bounds__(256) void relu6_fwd_kernel(const float* __restrict__ x, long n, float* __restrict__ y, bf16_t* __restrict__ yb) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = fminf(fmaxf(x[i], 0.f), 6.f);
    if (y) y[i] = v;
    if (yb) yb[i] = f32_to_bf16(v);
  }
}
extern "C" int evc_relu6_fwd(const float* x, int64_t n, float* y_f32, evc_bf16* y_bf16, void* stream) {
  EVC_REQUIRE(x && n > 0 && (y_f32 || y_bf16), EVC_ERR_BAD_ARG, "evc_relu6_fwd: n=%ld", (long)n);
  const long nb = (n + 255) / 256;
  hipLaunchKernelGGL(relu6_fwd_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, x, (long)n, y_f32, (bf16_t*)y_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
__global__ __launch_bounds__(256) void relu6_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, long n, float* __restrict__ dx,
                                                        bf16_t* __restrict__ dxb) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float xv = x[i];
    const float v = (xv > 0.f && xv < 6.f) ? dy[i] : 0.f;          // tf.nn.relu6 gradient: 1 strictly inside (0, 6)
    if (dx) dx[i] = v;
    if (dxb) dxb[i] = f32_to_bf16(v);
  }
}
extern "C" int evc_relu6_bwd(const float* x, const float* dy, int64_t n, float* dx_f32, evc_bf16* dx_bf16, void* stream) {
  EVC_REQUIRE(x && dy && n > 0 && (dx_f32 || dx_bf16), EVC_ERR_BAD_ARG, "evc_relu6_bwd: n=%ld", (long)n);
  const long nb = (n + 255) / 256;
  hipLaunchKernelGGL(relu6_bwd_kernel, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, x, dy, (long)n, dx_f32, (bf16_t*)dx_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// pooled[b][c] = mean over the S frames of y[b][s][c] (FramePooling 'average': tf.reduce_mean(frames, 1)); dy[b][s][c] = dpooled[b][c] / S
__global__ __launch_bounds__(256) void framepool_mean_fwd_kernel(const float* __restrict__ y, int B, int S, int C, float* __restrict__ pooled,
                                                                 bf16_t* __restrict__ pooled_b) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * C) return;
  const int b = (int)(i / C), c = (int)(i % C);
  float s = 0.f;
  for (int f = 0; f < S; ++f) s += y[((long)b * S + f) * C + c];
  s = s / (float)S;
  if (pooled) pooled[i] = s;
  if (pooled_b) pooled_b[i] = f32_to_bf16(s);
}
extern "C" int evc_framepool_mean_fwd(const float* y, int B, int S, int C, float* pooled_f32, evc_bf16* pooled_bf16, void* stream) {
  EVC_REQUIRE(y && B > 0 && S > 0 && C > 0 && (pooled_f32 || pooled_bf16), EVC_ERR_BAD_ARG, "evc_framepool_mean_fwd: bad arguments");
  hipLaunchKernelGGL(framepool_mean_fwd_kernel, dim3((unsigned)(((long)B * C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, B, S, C, pooled_f32,
                     (bf16_t*)pooled_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
__global__ __launch_bounds__(256) void framepool_mean_bwd_kernel(const float* __restrict__ dpooled, int B, int S, int C, float* __restrict__ dy) {
  const long n = (long)B * S * C;
  const float inv = 1.0f / (float)S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long b = i / ((long)S * C);
    const int c = (int)(i % C);
    dy[i] = dpooled[b * C + c] * inv;
  }
}
extern "C" int evc_framepool_mean_bwd(const float* dpooled, int B, int S, int C, float* dy, void* stream) {
  EVC_REQUIRE(dpooled && dy && B > 0 && S > 0 && C > 0, EVC_ERR_BAD_ARG, "evc_framepool_mean_bwd: bad arguments");
  const long nb = ((long)B * S * C + 255) / 256;
  hipLaunchKernelGGL(framepool_mean_bwd_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, (hipStream_t)stream, dpooled, B, S, C, dy);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// column statistics: grid (C/64, RS); block 64 columns x 4 row phases; f64 partials via atomics into ws[2C]
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ x, int R, int C, double* __restrict__ ws) {
  __shared__ double sh[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double s = 0.0, q = 0.0;
  if (c < C)
    for (int r = blockIdx.y * 4 + ty; r < R; r += gridDim.y * 4) {
      const double v = x[(long)r * C + c];
      s += v; q += v * v;
    }
  sh[0][ty][tx] = s; sh[1][ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c < C) {
    s = sh[0][0][tx] + sh[0][1][tx] + sh[0][2][tx] + sh[0][3][tx];
    q = sh[1][0][tx] + sh[1][1][tx] + sh[1][2][tx] + sh[1][3][tx];
    atomicAdd(&ws[c], s);
    atomicAdd(&ws[C + c], q);
  }
}
__global__ void bn_stats_final_kernel(const double* __restrict__ ws, int R, int C, float* __restrict__ mean, float* __restrict__ var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mu = ws[c] / R;
  double vv = ws[C + c] / R - mu * mu;
  mean[c] = (float)mu;
  var[c] = (float)(vv > 0 ? vv : 0);
}
extern "C" int evc_bn_stats_partial(const float* x, int R, int C, double* ws, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && ws, EVC_ERR_BAD_SHAPE, "evc_bn_stats_partial: bad args");
  hipStream_t st = (hipStream_t)stream;
  EVC_CHECK_HIP(hipMemsetAsync(ws, 0, sizeof(double) * 2 * C, st));
  int rs = R / 256; rs = rs < 1 ? 1 : (rs > 64 ? 64 : rs);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((C + 63) / 64, rs), dim3(256), 0, st, x, R, C, ws);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_bn_stats_finalize(const double* ws, int R_total, int C, float* mean, float* var, void* stream) {
  EVC_REQUIRE(R_total > 0 && C > 0 && ws, EVC_ERR_BAD_SHAPE, "evc_bn_stats_finalize: bad args");
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, R_total, C, mean, var);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_bn_stats(const float* x, int R, int C, double* ws, float* mean, float* var, void* stream) {
  int rc = evc_bn_stats_partial(x, R, C, ws, stream);
  if (rc) return rc;
  return evc_bn_stats_finalize(ws, R, C, mean, var, stream);
}
__global__ void ema_kernel(float* __restrict__ moving, const float* __restrict__ batch, float decay, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) moving[i] -= (1.f - decay) * (moving[i] - batch[i]);   // slim.batch_norm UPDATE_OPS (assign_moving_average)
}
extern "C" int evc_ema_update(float* moving, const float* batch_value, float decay, int n, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_ema_update: n");
  hipLaunchKernelGGL(ema_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, moving, batch_value, decay, n);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ void bn_apply_kernel(const float* __restrict__ x, long n, int C, const float* __restrict__ mean,
                                const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
                                int relu6, float* __restrict__ yf, bf16_t* __restrict__ yb) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    float y = (x[i] - mean[c]) * rsqrtf(var[c] + 1e-3f) * gamma[c] + beta[c];
    if (relu6) y = fminf(fmaxf(y, 0.f), 6.f);
    if (yf) yf[i] = y;
    if (yb) yb[i] = f32_to_bf16(y);
  }
}
extern "C" int evc_bn_apply(const float* x, int R, int C, const float* mean, const float* var, const float* gamma,
                            const float* beta, int relu6, float* y_f32, evc_bf16* y_bf16, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_bn_apply: bad shape");
  const long n = (long)R * C;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, n, C, mean, var, gamma, beta,
                     relu6, y_f32, y_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// backward of y = relu6?(gamma*xh+beta): pass 1 column sums of dyh=dy*mask and dyh*xh; pass 2 dx
// dy of row r, column c: either dy[r][c], or (max-pool routing) dpooled[r/S][c] where argmax[r/S][c] == r%S.
__device__ __forceinline__ float routed_dy(const float* __restrict__ dy, const int* __restrict__ am, int S, long r, int c, int C) {
  if (!am) return dy[r * C + c];
  const long b = r / S;
  return (am[b * C + c] == (int)(r % S)) ? dy[b * C + c] : 0.f;
}
// ADD (evc_bn_bwd_partial_add / _finalize_add): the incoming gradient is dy[i] + dy2[i], one f32 add in front of the
// mask; the ADD = false instantiations are the code the plain entries always ran.
template <bool ADD>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ dy2, int R, int C,
                                                             const float* __restrict__ mean, const float* __restrict__ var,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             int relu6, const int* __restrict__ am, int S, double* __restrict__ ws) {
  __shared__ double sh[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double s = 0.0, q = 0.0;
  if (c < C) {
    const float mu = mean[c], inv = rsqrtf(var[c] + 1e-3f), ga = gamma[c], be = beta[c];
    for (int r = blockIdx.y * 4 + ty; r < R; r += gridDim.y * 4) {
      const long i = (long)r * C + c;
      const float xh = (x[i] - mu) * inv;
      float d = routed_dy(dy, am, S, r, c, C);
      if constexpr (ADD) d = d + dy2[i];
      if (relu6) { const float y = xh * ga + be; if (!(y > 0.f && y < 6.f)) d = 0.f; }
      s += d; q += (double)d * xh;
    }
  }
  sh[0][ty][tx] = s; sh[1][ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c < C) {
    atomicAdd(&ws[c], sh[0][0][tx] + sh[0][1][tx] + sh[0][2][tx] + sh[0][3][tx]);
    atomicAdd(&ws[C + c], sh[1][0][tx] + sh[1][1][tx] + sh[1][2][tx] + sh[1][3][tx]);
  }
}
template <bool ADD>
__global__ void bn_bwd_final_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ dy2, long n, int R, int C,
                                    const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, int relu6, const int* __restrict__ am, int S,
                                    const double* __restrict__ ws,
                                    float* __restrict__ dxf, bf16_t* __restrict__ dxb, float* __restrict__ dgamma,
                                    float* __restrict__ dbeta) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const float inv = rsqrtf(var[c] + 1e-3f), ga = gamma[c];
    const float xh = (x[i] - mean[c]) * inv;
    float d = routed_dy(dy, am, S, i / C, c, C);
    if constexpr (ADD) d = d + dy2[i];
    if (relu6) { const float y = xh * ga + beta[c]; if (!(y > 0.f && y < 6.f)) d = 0.f; }
    const float sd = (float)ws[c], sdx = (float)ws[C + c];
    // dx = gamma*inv/R * (R*d - sum(d) - xh*sum(d*xh))
    const float dx = ga * inv * (d - sd / R - xh * sdx / R);
    if (dxf) dxf[i] = dx;
    if (dxb) dxb[i] = f32_to_bf16(dx);
    if (i < C) { if (dgamma) dgamma[i] = (float)ws[C + i]; if (dbeta) dbeta[i] = (float)ws[i]; }
  }
}
static int bn_bwd_partial_launch(const char* who, const float* x, const float* dy, const float* dy2, int R, int C, const float* mean,
                                 const float* var, const float* gamma, const float* beta, int relu6, const int32_t* argmax, int S,
                                 double* ws, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && ws && (!argmax || (S > 0 && R % S == 0)), EVC_ERR_BAD_SHAPE, "%s: bad args", who);
  EVC_REQUIRE(!dy2 || !argmax, EVC_ERR_BAD_ARG, "%s: dy2 with argmax (max-pool routing: dy is [R/S][C], dy2 [R][C])", who);
  hipStream_t st = (hipStream_t)stream;
  EVC_CHECK_HIP(hipMemsetAsync(ws, 0, sizeof(double) * 2 * C, st));
  int rs = R / 256; rs = rs < 1 ? 1 : (rs > 64 ? 64 : rs);
  if (dy2)
    hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, dim3((C + 63) / 64, rs), dim3(256), 0, st, x, dy, dy2, R, C, mean, var, gamma, beta,
                       relu6, argmax, S, ws);
  else
    hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, dim3((C + 63) / 64, rs), dim3(256), 0, st, x, dy, dy2, R, C, mean, var, gamma, beta,
                       relu6, argmax, S, ws);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
static int bn_bwd_finalize_launch(const char* who, const float* x, const float* dy, const float* dy2, int R, int R_total, int C,
                                  const float* mean, const float* var, const float* gamma, const float* beta, int relu6,
                                  const int32_t* argmax, int S, const double* ws, float* dx_f32, evc_bf16* dx_bf16, float* dgamma,
                                  float* dbeta, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && ws && R_total >= R, EVC_ERR_BAD_SHAPE, "%s: bad args", who);
  EVC_REQUIRE(!dy2 || !argmax, EVC_ERR_BAD_ARG, "%s: dy2 with argmax (max-pool routing: dy is [R/S][C], dy2 [R][C])", who);
  const long n = (long)R * C;
  if (dy2)
    hipLaunchKernelGGL(bn_bwd_final_kernel<true>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dy2, n, R_total, C, mean,
                       var, gamma, beta, relu6, argmax, S, ws, dx_f32, dx_bf16, dgamma, dbeta);
  else
    hipLaunchKernelGGL(bn_bwd_final_kernel<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dy2, n, R_total, C, mean,
                       var, gamma, beta, relu6, argmax, S, ws, dx_f32, dx_bf16, dgamma, dbeta);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_bn_bwd_partial(const float* x, const float* dy, int R, int C, const float* mean, const float* var,
                                  const float* gamma, const float* beta, int relu6, const int32_t* argmax, int S,
                                  double* ws, void* stream) {
  return bn_bwd_partial_launch("evc_bn_bwd_partial", x, dy, nullptr, R, C, mean, var, gamma, beta, relu6, argmax, S, ws, stream);
}
extern "C" int evc_bn_bwd_finalize(const float* x, const float* dy, int R, int R_total, int C, const float* mean,
                                   const float* var, const float* gamma, const float* beta, int relu6,
                                   const int32_t* argmax, int S, const double* ws, float* dx_f32, evc_bf16* dx_bf16,
                                   float* dgamma, float* dbeta, void* stream) {
  return bn_bwd_finalize_launch("evc_bn_bwd_finalize", x, dy, nullptr, R, R_total, C, mean, var, gamma, beta, relu6, argmax, S, ws, dx_f32,
                                dx_bf16, dgamma, dbeta, stream);
}
extern "C" int evc_bn_bwd_partial_add(const float* x, const float* dy, const float* dy2, int R, int C, const float* mean, const float* var,
                                      const float* gamma, const float* beta, int relu6, const int32_t* argmax, int S, double* ws,
                                      void* stream) {
  return bn_bwd_partial_launch("evc_bn_bwd_partial_add", x, dy, dy2, R, C, mean, var, gamma, beta, relu6, argmax, S, ws, stream);
}
extern "C" int evc_bn_bwd_finalize_add(const float* x, const float* dy, const float* dy2, int R, int R_total, int C, const float* mean,
                                       const float* var, const float* gamma, const float* beta, int relu6, const int32_t* argmax, int S,
                                       const double* ws, float* dx_f32, evc_bf16* dx_bf16, float* dgamma, float* dbeta, void* stream) {
  return bn_bwd_finalize_launch("evc_bn_bwd_finalize_add", x, dy, dy2, R, R_total, C, mean, var, gamma, beta, relu6, argmax, S, ws, dx_f32,
                                dx_bf16, dgamma, dbeta, stream);
}
extern "C" int evc_bn_relu6_bwd(const float* x, const float* dy, int R, int C, const float* mean, const float* var,
                                const float* gamma, const float* beta, int relu6, const int32_t* argmax, int S, double* ws,
                                float* dx_f32, evc_bf16* dx_bf16, float* dgamma, float* dbeta, void* stream) {
  int rc = evc_bn_bwd_partial(x, dy, R, C, mean, var, gamma, beta, relu6, argmax, S, ws, stream);
  if (rc) return rc;
  return evc_bn_bwd_finalize(x, dy, R, R, C, mean, var, gamma, beta, relu6, argmax, S, ws, dx_f32, dx_bf16, dgamma, dbeta, stream);
}

// ---- context gate behind a batch norm (NetVLAD's gating_bn): out = h * sigmoid(bn(gl)).  The chain these entries replace is
// evc_bn_apply(gl -> gn), evc_nextvlad_gate_fwd(h, gn), evc_nextvlad_gate_bwd_add(h, gn, d, d2 -> dh, dgn), evc_bn_bwd_partial / _finalize(gl, dgn);
// they give its bits without gn, g or dgn in memory.  gn is bn_apply_kernel's expression, xh * ga + be with xh = (x - mu) * inv, which is also how
// bn_bwd_partial_kernel spells it.  dgn is an f32 the chain STORES before the batch norm's backward reads it, so it is formed with contraction
// switched off (gate_dy): left to the compiler, d - sd / R in the finalize pass would take the last product as an fma operand, unrounded.
__device__ __forceinline__ float gate_dy(float e, float h, float g) {
#pragma clang fp contract(off)
  return e * h * g * (1.0f - g);
}
__device__ __forceinline__ float bn_gate_out(float x, float h, float mu, float va, float ga, float be) {
  return h * sigmoidf_((x - mu) * rsqrtf(va + 1e-3f) * ga + be);
}
__global__ void bn_gate_fwd_kernel(const float* __restrict__ gl, const float* __restrict__ h, long n, int C, const float* __restrict__ mean,
                                   const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    out[i] = bn_gate_out(gl[i], h[i], mean[c], var[c], gamma[c], beta[c]);
  }
}
// C % 4 == 0 and every base 16-byte aligned: one quad per thread and iteration, the four per-column vectors as float4
__global__ void bn_gate_fwd_vec4_kernel(const float4* __restrict__ gl, const float4* __restrict__ h, long n4, int C4, const float4* __restrict__ mean,
                                        const float4* __restrict__ var, const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                        float4* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const float4 x = gl[i], hh = h[i], mu = mean[c], va = var[c], ga = gamma[c], be = beta[c];
    float4 o;
    o.x = bn_gate_out(x.x, hh.x, mu.x, va.x, ga.x, be.x);
    o.y = bn_gate_out(x.y, hh.y, mu.y, va.y, ga.y, be.y);
    o.z = bn_gate_out(x.z, hh.z, mu.z, va.z, ga.z, be.z);
    o.w = bn_gate_out(x.w, hh.w, mu.w, va.w, ga.w, be.w);
    out[i] = o;
  }
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
extern "C" int evc_bn_gate_fwd(const float* gl, const float* h, int R, int C, const float* mean, const float* var, const float* gamma,
                               const float* beta, float* out, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_bn_gate_fwd: bad shape (R=%d C=%d)", R, C);
  EVC_REQUIRE(gl && h && mean && var && gamma && beta && out, EVC_ERR_BAD_ARG, "evc_bn_gate_fwd: NULL operand");
  const long n = (long)R * C;
  if (C % 4 == 0 && aligned16(gl) && aligned16(h) && aligned16(mean) && aligned16(var) && aligned16(gamma) && aligned16(beta) && aligned16(out))
    hipLaunchKernelGGL(bn_gate_fwd_vec4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, (const float4*)gl, (const float4*)h, n / 4,
                       C / 4, (const float4*)mean, (const float4*)var, (const float4*)gamma, (const float4*)beta, (float4*)out);
  else
    hipLaunchKernelGGL(bn_gate_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, gl, h, n, C, mean, var, gamma, beta, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// bn_bwd_partial_kernel<false>'s grid, loop and summation order (relu6 = 0, no argmax) on dy = e * h * g * (1 - g), e = d (+ d2); stores dh = e * g
__global__ __launch_bounds__(256) void bn_gate_bwd_partial_kernel(const float* __restrict__ gl, const float* __restrict__ h, const float* __restrict__ d,
                                                                  const float* __restrict__ d2, int R, int C, const float* __restrict__ mean,
                                                                  const float* __restrict__ var, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, double* __restrict__ ws, float* __restrict__ dh) {
  __shared__ double sh[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double s = 0.0, q = 0.0;
  if (c < C) {
    const float mu = mean[c], inv = rsqrtf(var[c] + 1e-3f), ga = gamma[c], be = beta[c];
    for (int r = blockIdx.y * 4 + ty; r < R; r += gridDim.y * 4) {
      const long i = (long)r * C + c;
      const float xh = (gl[i] - mu) * inv;
      const float g = sigmoidf_(xh * ga + be);
      float e = d[i];
      if (d2) e = __fadd_rn(e, d2[i]);
      dh[i] = e * g;
      const float dy = gate_dy(e, h[i], g);
      s += dy; q += (double)dy * xh;
    }
  }
  sh[0][ty][tx] = s; sh[1][ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c < C) {
    atomicAdd(&ws[c], sh[0][0][tx] + sh[0][1][tx] + sh[0][2][tx] + sh[0][3][tx]);
    atomicAdd(&ws[C + c], sh[1][0][tx] + sh[1][1][tx] + sh[1][2][tx] + sh[1][3][tx]);
  }
}
__global__ void bn_gate_bwd_final_kernel(const float* __restrict__ gl, const float* __restrict__ h, const float* __restrict__ d,
                                         const float* __restrict__ d2, long n, int R, int C, const float* __restrict__ mean,
                                         const float* __restrict__ var, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const double* __restrict__ ws, float* __restrict__ dxf, bf16_t* __restrict__ dxb,
                                         float* __restrict__ dgamma, float* __restrict__ dbeta) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const float inv = rsqrtf(var[c] + 1e-3f), ga = gamma[c];
    const float xh = (gl[i] - mean[c]) * inv;
    const float g = sigmoidf_(xh * ga + beta[c]);
    float e = d[i];
    if (d2) e = __fadd_rn(e, d2[i]);
    const float dy = gate_dy(e, h[i], g);
    const float sd = (float)ws[c], sdx = (float)ws[C + c];
    const float dx = ga * inv * (dy - sd / R - xh * sdx / R);
    if (dxf) dxf[i] = dx;
    if (dxb) dxb[i] = f32_to_bf16(dx);
    if (i < C) { if (dgamma) dgamma[i] = (float)ws[C + i]; if (dbeta) dbeta[i] = (float)ws[i]; }
  }
}
extern "C" int evc_bn_gate_bwd_partial(const float* gl, const float* h, const float* d, const float* d2, int R, int C, const float* mean,
                                       const float* var, const float* gamma, const float* beta, double* ws, float* dh, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_bn_gate_bwd_partial: bad shape (R=%d C=%d)", R, C);
  EVC_REQUIRE(gl && h && d && mean && var && gamma && beta && ws && dh, EVC_ERR_BAD_ARG, "evc_bn_gate_bwd_partial: NULL operand (d2 may be NULL)");
  hipStream_t st = (hipStream_t)stream;
  EVC_CHECK_HIP(hipMemsetAsync(ws, 0, sizeof(double) * 2 * C, st));
  int rs = R / 256; rs = rs < 1 ? 1 : (rs > 64 ? 64 : rs);
  hipLaunchKernelGGL(bn_gate_bwd_partial_kernel, dim3((C + 63) / 64, rs), dim3(256), 0, st, gl, h, d, d2, R, C, mean, var, gamma, beta, ws, dh);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_bn_gate_bwd_finalize(const float* gl, const float* h, const float* d, const float* d2, int R, int R_total, int C,
                                        const float* mean, const float* var, const float* gamma, const float* beta, const double* ws,
                                        float* dgl_f32, evc_bf16* dgl_bf16, float* dgamma, float* dbeta, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && R_total >= R, EVC_ERR_BAD_SHAPE, "evc_bn_gate_bwd_finalize: bad shape (R=%d R_total=%d C=%d)", R, R_total, C);
  EVC_REQUIRE(gl && h && d && mean && var && gamma && beta && ws, EVC_ERR_BAD_ARG,
              "evc_bn_gate_bwd_finalize: NULL operand (d2 and each output may be NULL)");
  const long n = (long)R * C;
  hipLaunchKernelGGL(bn_gate_bwd_final_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, gl, h, d, d2, n, R_total, C, mean, var, gamma,
                     beta, ws, dgl_f32, (bf16_t*)dgl_bf16, dgamma, dbeta);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// fused cluster_bn + relu6 + FramePooling('max'): act [B][S][C] f32 -> pooled [B][C]
__global__ __launch_bounds__(256) void bn_relu6_pool_kernel(const float* __restrict__ act, int S, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ var,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ pf, bf16_t* __restrict__ pb, int* __restrict__ am) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float mu = mean[c], sc = rsqrtf(var[c] + 1e-3f) * gamma[c], be = beta[c];
  const float* ap = act + (long)b * S * C + c;
  float best = -1.f;
  int bi = 0;
  for (int s = 0; s < S; ++s) {
    const float y = fminf(fmaxf((ap[(long)s * C] - mu) * sc + be, 0.f), 6.f);
    if (y > best) { best = y; bi = s; }
  }
  const long o = (long)b * C + c;
  pf[o] = best;
  if (pb) pb[o] = f32_to_bf16(best);
  am[o] = bi;
}
extern "C" int evc_bn_relu6_framepool_fwd(const float* act, int B, int S, int C, const float* mean, const float* var,
                                          const float* gamma, const float* beta, float* pooled_f32, evc_bf16* pooled_bf16,
                                          int32_t* argmax, void* stream) {
  EVC_REQUIRE(B > 0 && S > 0 && C > 0 && pooled_f32 && argmax, EVC_ERR_BAD_SHAPE, "evc_bn_relu6_framepool_fwd: bad args");
  hipLaunchKernelGGL(bn_relu6_pool_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, act, S, C, mean, var, gamma,
                     beta, pooled_f32, pooled_bf16, argmax);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ __launch_bounds__(256) void framepool_max_fwd_kernel(const float* __restrict__ y, int S, int C, float* __restrict__ pf,
                                                                bf16_t* __restrict__ pb, int* __restrict__ am) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float* yp = y + (long)b * S * C + c;
  float best = yp[0];
  int bi = 0;
  for (int s = 1; s < S; ++s) {
    const float v = yp[(long)s * C];
    if (v > best) { best = v; bi = s; }   // first maximum wins (numpy argmax / TF max-grad tie -> see DESIGN.md)
  }
  const long o = (long)b * C + c;
  if (pf) pf[o] = best;
  if (pb) pb[o] = f32_to_bf16(best);
  if (am) am[o] = bi;
}
extern "C" int evc_framepool_max_fwd(const float* y, int B, int S, int C, float* pooled_f32, evc_bf16* pooled_bf16,
                                     int32_t* argmax, void* stream) {
  EVC_REQUIRE(B > 0 && S > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_framepool_max_fwd: bad shape");
  hipLaunchKernelGGL(framepool_max_fwd_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, y, S, C, pooled_f32,
                     pooled_bf16, argmax);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
__global__ void framepool_max_bwd_kernel(const float* __restrict__ dp, const int* __restrict__ am, int S, int C, long n,
                                         float* __restrict__ dy) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long bs = i / C;
    const int s = (int)(bs % S);
    const long b = bs / S;
    dy[i] = (am[b * C + c] == s) ? dp[b * C + c] : 0.f;
  }
}
extern "C" int evc_framepool_max_bwd(const float* dpooled, const int32_t* argmax, int B, int S, int C, float* dy, void* stream) {
  EVC_REQUIRE(B > 0 && S > 0 && C > 0, EVC_ERR_BAD_SHAPE, "evc_framepool_max_bwd: bad shape");
  const long n = (long)B * S * C;
  hipLaunchKernelGGL(framepool_max_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dpooled, argmax, S, C, n, dy);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

__global__ void fill_kernel(float* p, long n, float v) {
  const long stride = (long)gridDim.x * blockDim.x, tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if ((((uintptr_t)p) & 15) == 0) {      // 16-byte stores over the aligned body, scalar tail
    const long n4 = n >> 2;
    const float4 v4 = make_float4(v, v, v, v);
    for (long i = tid; i < n4; i += stride) ((float4*)p)[i] = v4;
    for (long i = (n4 << 2) + tid; i < n; i += stride) p[i] = v;
  } else {
    for (long i = tid; i < n; i += stride) p[i] = v;
  }
}
extern "C" int evc_fill_f32(float* p, int64_t n, float value, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_fill_f32: n");
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, (long)n, value);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// p[r*ld + c] = v for r < rows, c < cols: a column range of a row-major matrix (the columns of a weight gradient that a split-K launch joins
// with atomics, engine.LstmStack._wgrad_tn), 16-byte stores (cols4 = cols / 4)
__global__ void fill_cols_kernel(float* p, long ld, int rows, int cols4, float v) {
  const long n = (long)rows * cols4, stride = (long)gridDim.x * blockDim.x;
  const float4 v4 = make_float4(v, v, v, v);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long r = i / cols4, c = i - r * cols4;
    *(float4*)(p + r * ld + c * 4) = v4;
  }
}
extern "C" int evc_fill_f32_cols(float* p, int64_t ld, int rows, int cols, float value, void* stream) {
  EVC_REQUIRE(p && rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0 && ld >= cols && ((uintptr_t)p % 16) == 0, EVC_ERR_BAD_SHAPE,
              "evc_fill_f32_cols: rows=%d cols=%d (%%4) ld=%ld (%%4, >= cols), 16-byte aligned", rows, cols, (long)ld);
  hipLaunchKernelGGL(fill_cols_kernel, dim3(grid_for((long)rows * (cols / 4))), dim3(256), 0, (hipStream_t)stream, p, (long)ld, rows, cols / 4, value);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---------------------------------------------------------------------------
// Measurement aid (scripts/dp_occupancy_sim.sh): a stand-in for a collective's kernel on a one-GPU box.  `blocks`
// workgroups of `threads` threads, each holding `lds_bytes` of LDS, stay resident for `microseconds` (constant 100 MHz clock) and
// do nothing else - what an RCCL kernel with that many channels does to the compute streams while its bytes are on the wire: it
// holds CUs (a workgroup that owns LDS keeps the 160 KB ring tiles of the GEMM kernels off its CU), not HBM bandwidth.
// ---------------------------------------------------------------------------
__global__ void occupy_kernel(long long ticks) {
  extern __shared__ char occ_lds[];
  if (threadIdx.x == 0) occ_lds[0] = 0;
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
  if (occ_lds[0] == 1) occ_lds[1] = 2;     // (keeps the LDS allocation alive)
}
extern "C" int evc_debug_occupy(int blocks, int threads, int lds_bytes, double microseconds, void* stream) {
  EVC_REQUIRE(blocks > 0 && blocks <= 1024 && threads >= 64 && threads <= 1024 && lds_bytes >= 0 && lds_bytes <= 160 * 1024 && microseconds >= 0,
              EVC_ERR_BAD_ARG, "evc_debug_occupy: blocks=%d threads=%d lds=%d us=%g", blocks, threads, lds_bytes, microseconds);
  if (lds_bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)occupy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  hipLaunchKernelGGL(occupy_kernel, dim3(blocks), dim3(threads), lds_bytes, (hipStream_t)stream, (long long)(microseconds * 100.0));
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_stream_create_cu_mask(const unsigned* mask, int words, void** stream_out) {
  EVC_REQUIRE(mask != nullptr && stream_out != nullptr && words > 0 && words <= 32, EVC_ERR_BAD_ARG, "evc_stream_create_cu_mask: words=%d", words);
  hipStream_t s = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask);
  EVC_REQUIRE(e == hipSuccess, EVC_ERR_HIP, "hipExtStreamCreateWithCUMask: %s", hipGetErrorString(e));
  *stream_out = (void*)s;
  return EVC_OK;
}

extern "C" int evc_stream_destroy(void* stream) {
  EVC_REQUIRE(stream != nullptr, EVC_ERR_BAD_ARG, "evc_stream_destroy: null stream");
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  EVC_REQUIRE(e == hipSuccess, EVC_ERR_HIP, "hipStreamDestroy: %s", hipGetErrorString(e));
  return EVC_OK;
}

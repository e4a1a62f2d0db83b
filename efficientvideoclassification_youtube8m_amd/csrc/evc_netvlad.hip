// NetVLAD aggregation kernels (EXTENSION - SURVEY.md 8f row 4: the reference's NetVLADModel is an empty stub,
// cs/frame_level_models.py:341-347, so there is no reference math; the oracle is oracle/model_math.py::netvlad_fwd/bwd,
// checked against finite differences).  The GEMM-shaped parts of the tower (cluster assignment, hidden layer, their
// gradients) run on the library's NT / TN kernels; these are the f32 pieces in between:
//
//   evc_netvlad_softmax_fwd/bwd      a = softmax_k(cluster_bn(act)) per sampled frame, and its reverse mode
//   evc_netvlad_aggregate_fwd/bwd    V[b][k][:] = sum_s a[b,s,k] * (x_bn[b,s,:] - c2[k][:]); da, dx_bn from dV
//   evc_netvlad_aggregate_packed_fwd/bwd   the same over a ragged, packed list of frames per video, any number of them:
//                                    the forward on the f32 matrix cores, the backward as two tiled products; at the end of this file
//   evc_netvlad_dcenters             dc2[k][:] = - sum_b asum[b][k] * dV[b][k][:]
//   evc_netvlad_normalize_fwd/bwd    intra-normalisation per (video, cluster) then l2 over the whole descriptor
//
// Layouts: sampled frames row-major [B*S][..] (row b*S+s); V / dV / Y [B][K][F] (cluster-major: the hidden layer's
// weight rows are permuted accordingly, towers.NetVladTower converts to the TF order f*K+k in state_dict()).
#include "evc_common.h"

static inline int nv_grid(long n) { long nb = (n + 255) / 256; return (int)(nb < 1 ? 1 : (nb < 8192 ? nb : 8192)); }

// ---- softmax over the clusters of the batch-normalised assignment logits: one wave per sampled frame ----
__global__ __launch_bounds__(256) void netvlad_softmax_fwd_kernel(const float* __restrict__ act, int R, int K,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  float* __restrict__ a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  float y[16];                                   // K <= 1024
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    y[i] = -INFINITY;
    if (k < K) {
      y[i] = (act[(long)row * K + k] - mean[k]) * rsqrtf(var[k] + 1e-3f) * gamma[k] + beta[k];
      mx = fmaxf(mx, y[i]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    if (k < K) { y[i] = __expf(y[i] - mx); sum += y[i]; }
  }
  const float inv = 1.0f / wave_sum(sum);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    if (k < K) a[(long)row * K + k] = y[i] * inv;
  }
}
extern "C" int evc_netvlad_softmax_fwd(const float* act, int R, int K, const float* mean, const float* var, const float* gamma,
                                       const float* beta, float* a, void* stream) {
  EVC_REQUIRE(R > 0 && K > 0 && K <= 1024, EVC_ERR_BAD_SHAPE, "evc_netvlad_softmax_fwd: 1 <= clusters <= 1024 (K=%d)", K);
  hipLaunchKernelGGL(netvlad_softmax_fwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, act, R, K, mean, var, gamma, beta, a);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// dz = a * (da - sum_k a * da): gradient wrt the batch-normalised logits
__global__ __launch_bounds__(256) void netvlad_softmax_bwd_kernel(const float* __restrict__ a, const float* __restrict__ da, int R, int K,
                                                                  float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  float dot = 0.f;
  for (int k = lane; k < K; k += 64) dot += a[(long)row * K + k] * da[(long)row * K + k];
  dot = wave_sum(dot);
  for (int k = lane; k < K; k += 64) dz[(long)row * K + k] = a[(long)row * K + k] * (da[(long)row * K + k] - dot);
}
extern "C" int evc_netvlad_softmax_bwd(const float* a, const float* da, int R, int K, float* dz, void* stream) {
  EVC_REQUIRE(R > 0 && K > 0, EVC_ERR_BAD_SHAPE, "evc_netvlad_softmax_bwd: bad shape");
  hipLaunchKernelGGL(netvlad_softmax_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, da, R, K, dz);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- aggregation.  x_bn is recomputed from the sampled frames r and input_bn's statistics (no f32 copy of it is kept).
// grid (B, K / KT): a workgroup accumulates KT clusters of one video; thread t owns the float4 feature columns t, t+256, ...
static constexpr int NV_KT = 8;
__global__ __launch_bounds__(256) void netvlad_aggregate_fwd_kernel(const float* __restrict__ a, const float* __restrict__ r, int S, int K,
                                                                    int F, const float* __restrict__ mean, const float* __restrict__ var,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ c2, float* __restrict__ V,
                                                                    float* __restrict__ asum) {
  const int b = blockIdx.x, k0 = blockIdx.y * NV_KT;
  const int F4 = F >> 2;
  __shared__ float as[64][NV_KT];                // a[b, s, k0..k0+KT) for up to 64 frames
  for (int i = threadIdx.x; i < S * NV_KT; i += 256) {
    const int s = i / NV_KT, kk = i % NV_KT;
    as[s][kk] = (k0 + kk < K) ? a[((long)b * S + s) * K + k0 + kk] : 0.f;
  }
  __syncthreads();
  float sk[NV_KT];
#pragma unroll
  for (int kk = 0; kk < NV_KT; ++kk) {
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += as[s][kk];
    sk[kk] = t;
  }
  if (threadIdx.x < NV_KT && k0 + threadIdx.x < K) asum[(long)b * K + k0 + threadIdx.x] = sk[threadIdx.x];
  for (int f4 = threadIdx.x; f4 < F4; f4 += 256) {
    const float4 mu = ((const float4*)mean)[f4], va = ((const float4*)var)[f4], ga = ((const float4*)gamma)[f4], be = ((const float4*)beta)[f4];
    const float4 sc = make_float4(rsqrtf(va.x + 1e-3f) * ga.x, rsqrtf(va.y + 1e-3f) * ga.y, rsqrtf(va.z + 1e-3f) * ga.z, rsqrtf(va.w + 1e-3f) * ga.w);
    float4 acc[NV_KT];
#pragma unroll
    for (int kk = 0; kk < NV_KT; ++kk) acc[kk] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 x = ((const float4*)(r + ((long)b * S + s) * F))[f4];
      const float4 xb = make_float4((x.x - mu.x) * sc.x + be.x, (x.y - mu.y) * sc.y + be.y, (x.z - mu.z) * sc.z + be.z, (x.w - mu.w) * sc.w + be.w);
#pragma unroll
      for (int kk = 0; kk < NV_KT; ++kk) {
        const float w = as[s][kk];
        acc[kk].x += w * xb.x; acc[kk].y += w * xb.y; acc[kk].z += w * xb.z; acc[kk].w += w * xb.w;
      }
    }
#pragma unroll
    for (int kk = 0; kk < NV_KT; ++kk) {
      if (k0 + kk >= K) break;
      const float4 c = ((const float4*)(c2 + (long)(k0 + kk) * F))[f4];
      ((float4*)(V + ((long)b * K + k0 + kk) * F))[f4] =
          make_float4(acc[kk].x - sk[kk] * c.x, acc[kk].y - sk[kk] * c.y, acc[kk].z - sk[kk] * c.z, acc[kk].w - sk[kk] * c.w);
    }
  }
}
extern "C" int evc_netvlad_aggregate_fwd(const float* a, const float* r, int B, int S, int K, int F, const float* mean, const float* var,
                                         const float* gamma, const float* beta, const float* c2, float* V, float* asum, void* stream) {
  EVC_REQUIRE(B > 0 && S > 0 && S <= 64 && K > 0 && F > 0 && F % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_netvlad_aggregate_fwd: needs S <= 64, F %% 4 == 0");
  hipLaunchKernelGGL(netvlad_aggregate_fwd_kernel, dim3(B, (K + NV_KT - 1) / NV_KT), dim3(256), 0, (hipStream_t)stream, a, r, S, K, F, mean,
                     var, gamma, beta, c2, V, asum);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// backward of the aggregation, one workgroup per video:
//   dx_bn[b,s,:] = sum_k a[b,s,k] * dV[b,k,:]                      (thread per float4 feature column, all S frames in registers)
//   da[b,s,k]    = sum_f dV[b,k,f] * (x_bn[b,s,f] - c2[k][f])       (wave w takes clusters w, w+4, ...; wave-wide dot products)
__global__ __launch_bounds__(256) void netvlad_aggregate_bwd_kernel(const float* __restrict__ a, const float* __restrict__ r, int S, int K,
                                                                    int F, const float* __restrict__ mean, const float* __restrict__ var,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    const float* __restrict__ c2, const float* __restrict__ dV,
                                                                    float* __restrict__ da, float* __restrict__ dx) {
  const int b = blockIdx.x;
  const int F4 = F >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ---- dx_bn ----
  for (int f4 = threadIdx.x; f4 < F4; f4 += 256) {
    for (int s0 = 0; s0 < S; s0 += 16) {                       // 16 frames at a time (register budget)
      float4 acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < K; ++k) {
        const float4 d = ((const float4*)(dV + ((long)b * K + k) * F))[f4];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (s0 + i < S) {
            const float w = a[((long)b * S + s0 + i) * K + k];
            acc[i].x += w * d.x; acc[i].y += w * d.y; acc[i].z += w * d.z; acc[i].w += w * d.w;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (s0 + i < S) ((float4*)(dx + ((long)b * S + s0 + i) * F))[f4] = acc[i];
    }
  }
  // ---- da ----
  for (int k = wave; k < K; k += 4) {
    for (int s = 0; s < S; ++s) {
      float dot = 0.f;
      for (int f4 = lane; f4 < F4; f4 += 64) {
        const float4 d = ((const float4*)(dV + ((long)b * K + k) * F))[f4];
        const float4 x = ((const float4*)(r + ((long)b * S + s) * F))[f4];
        const float4 mu = ((const float4*)mean)[f4], va = ((const float4*)var)[f4], ga = ((const float4*)gamma)[f4], be = ((const float4*)beta)[f4];
        const float4 c = ((const float4*)(c2 + (long)k * F))[f4];
        dot += d.x * ((x.x - mu.x) * rsqrtf(va.x + 1e-3f) * ga.x + be.x - c.x) + d.y * ((x.y - mu.y) * rsqrtf(va.y + 1e-3f) * ga.y + be.y - c.y) +
               d.z * ((x.z - mu.z) * rsqrtf(va.z + 1e-3f) * ga.z + be.z - c.z) + d.w * ((x.w - mu.w) * rsqrtf(va.w + 1e-3f) * ga.w + be.w - c.w);
      }
      dot = wave_sum(dot);
      if (lane == 0) da[((long)b * S + s) * K + k] = dot;
    }
  }
}
extern "C" int evc_netvlad_aggregate_bwd(const float* a, const float* r, int B, int S, int K, int F, const float* mean, const float* var,
                                         const float* gamma, const float* beta, const float* c2, const float* dV, float* da, float* dx,
                                         void* stream) {
  EVC_REQUIRE(B > 0 && S > 0 && K > 0 && F > 0 && F % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_netvlad_aggregate_bwd: bad shape");
  hipLaunchKernelGGL(netvlad_aggregate_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, r, S, K, F, mean, var, gamma, beta, c2, dV, da, dx);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// dc2[k][f] = - sum_b asum[b][k] * dV[b][k][f]    (thread per (k, float4 column), b in order: run-to-run identical)
__global__ void netvlad_dcenters_kernel(const float* __restrict__ asum, const float* __restrict__ dV, int B, int K, int F,
                                        float* __restrict__ dc2) {
  const long n4 = (long)K * (F >> 2);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / (F >> 2));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < B; ++b) {
      const float w = asum[(long)b * K + k];
      const float4 d = ((const float4*)(dV + (long)b * K * F))[i];
      acc.x -= w * d.x; acc.y -= w * d.y; acc.z -= w * d.z; acc.w -= w * d.w;
    }
    ((float4*)dc2)[i] = acc;
  }
}
extern "C" int evc_netvlad_dcenters(const float* asum, const float* dV, int B, int K, int F, float* dc2, void* stream) {
  EVC_REQUIRE(B > 0 && K > 0 && F > 0 && F % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_netvlad_dcenters: bad shape");
  hipLaunchKernelGGL(netvlad_dcenters_kernel, dim3(nv_grid((long)K * (F >> 2))), dim3(256), 0, (hipStream_t)stream, asum, dV, B, K, F, dc2);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- normalisation: U_k = V_k / max(|V_k|, 1e-6) per cluster, Y = U / max(|U|, 1e-6) (tf.nn.l2_normalize's epsilon 1e-12 on the
// squared norms).  One workgroup per video; n1 [B][K], n2 [B] are kept for the backward pass.
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void netvlad_normalize_fwd_kernel(const float* __restrict__ V, int K, int F, float* __restrict__ n1,
                                                                    float* __restrict__ n2, float* __restrict__ Yf, bf16_t* __restrict__ Yb) {
  extern __shared__ float sn1[];                 // [K] cluster norms
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* Vb = V + (long)b * K * F;
  for (int k = wave; k < K; k += 4) {
    float s = 0.f;
    for (int f = lane; f < F; f += 64) { const float v = Vb[(long)k * F + f]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) sn1[k] = sqrtf(fmaxf(s, 1e-12f));
  }
  __syncthreads();
  float t = 0.f;                                 // |U|^2 = sum_k |V_k|^2 / n1_k^2
  for (long i = threadIdx.x; i < (long)K * F; i += 256) { const float u = Vb[i] / sn1[i / F]; t += u * u; }
  const float nn2 = sqrtf(fmaxf(block_sum_256(t, red), 1e-12f));
  if (threadIdx.x == 0) n2[b] = nn2;
  for (int k = threadIdx.x; k < K; k += 256) n1[(long)b * K + k] = sn1[k];
  for (long i = threadIdx.x; i < (long)K * F; i += 256) {
    const float y = Vb[i] / (sn1[i / F] * nn2);
    if (Yf) Yf[(long)b * K * F + i] = y;
    Yb[(long)b * K * F + i] = f32_to_bf16(y);
  }
}
extern "C" int evc_netvlad_normalize_fwd(const float* V, int B, int K, int F, float* n1, float* n2, float* Y_f32, evc_bf16* Y_bf16,
                                         void* stream) {
  EVC_REQUIRE(B > 0 && K > 0 && K <= 4096 && F > 0 && Y_bf16, EVC_ERR_BAD_SHAPE, "evc_netvlad_normalize_fwd: bad shape");
  hipLaunchKernelGGL(netvlad_normalize_fwd_kernel, dim3(B), dim3(256), K * sizeof(float), (hipStream_t)stream, V, K, F, n1, n2, Y_f32, Y_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// dU = (dY - Y (Y . dY)) / n2;  dV_k = (dU_k - U_k (U_k . dU_k)) / n1_k        (U, Y recomputed from V, n1, n2)
__global__ __launch_bounds__(256) void netvlad_normalize_bwd_kernel(const float* __restrict__ V, const float* __restrict__ n1,
                                                                    const float* __restrict__ n2, const float* __restrict__ dY, int K, int F,
                                                                    float* __restrict__ dV) {
  extern __shared__ float tk[];                  // [K] U_k . dU_k
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* Vb = V + (long)b * K * F;
  const float* dYb = dY + (long)b * K * F;
  const float* n1b = n1 + (long)b * K;
  const float nn2 = n2[b];
  float t = 0.f;
  for (long i = threadIdx.x; i < (long)K * F; i += 256) t += Vb[i] / (n1b[i / F] * nn2) * dYb[i];
  const float ydy = block_sum_256(t, red);
  for (int k = wave; k < K; k += 4) {
    float s = 0.f;
    const float in1 = 1.0f / n1b[k];
    for (int f = lane; f < F; f += 64) {
      const float u = Vb[(long)k * F + f] * in1;
      const float du = (dYb[(long)k * F + f] - (u / nn2) * ydy) / nn2;
      s += u * du;
    }
    s = wave_sum(s);
    if (lane == 0) tk[k] = s;
  }
  __syncthreads();
  for (long i = threadIdx.x; i < (long)K * F; i += 256) {
    const int k = (int)(i / F);
    const float in1 = 1.0f / n1b[k];
    const float u = Vb[i] * in1;
    const float du = (dYb[i] - (u / nn2) * ydy) / nn2;
    dV[(long)b * K * F + i] = (du - u * tk[k]) * in1;
  }
}
extern "C" int evc_netvlad_normalize_bwd(const float* V, const float* n1, const float* n2, const float* dY, int B, int K, int F, float* dV,
                                         void* stream) {
  EVC_REQUIRE(B > 0 && K > 0 && K <= 4096 && F > 0, EVC_ERR_BAD_SHAPE, "evc_netvlad_normalize_bwd: bad shape");
  hipLaunchKernelGGL(netvlad_normalize_bwd_kernel, dim3(B), dim3(256), K * sizeof(float), (hipStream_t)stream, V, n1, n2, dY, K, F, dV);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ==== ragged videos: video b owns the frame rows row_off[b] .. row_off[b+1] of a [R][K], r [R][F], da, dx, L_b of them
// in time order (L_b = 0: none; no limit on L_b other than T).  With xb = (r - mean) * (rsqrtf(var + 1e-3f) * gamma) + beta per column:
//   asum[b][k] = sum_l a[l][k];   V[b][k][f] = sum_l a[l][k] * xb[l][f] - asum[b][k] * c2[k][f]
//   dx[l][f] = sum_k a[l][k] * dV[b][k][f];   da[l][k] = sum_f dV[b][k][f] * xb[l][f] - q[b][k],  q[b][k] = sum_f dV[b][k][f] * c2[k][f]
// xb never exists in memory: it is formed in registers behind the load (forward) or while the operand is staged into LDS (da).
static inline bool nv_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
#define NV_PACKED_SHAPE_OK                                                                                                     \
  (B > 0 && B <= 65535 && T > 0 && K > 0 && K <= 1024 && F > 0 && F % 4 == 0 && max_k >= 0 && max_k <= T && R >= max_k && \
   (long)R <= (long)B * max_k)

// ---- forward on the f32 matrix cores, in the manner of nx_aggregate_mfma_kernel (csrc/evc_nextvlad.hip): V_b = A_b^T Xb_b
// - asum_b (x) c2 with v_mfma_f32_32x32x2_f32.  grid (n tiles * m tiles, B), 4 waves as 2 x 2: a workgroup owns 64 clusters x 192 columns,
// wave w the clusters m0 = 32 (w & 1) .. + 32 and the columns n0 = 96 (w >> 1) .. + 96 of it as three 32 x 32 accumulators - K = 64,
// F = 1152 is one cluster tile and six column tiles with every wave at work.  Both operands come from global memory in the layout the
// instruction wants - lane (i = lane & 31, kk = lane >> 5) holds a[l + kk][m0 + i] and r[l + kk][n0 + 32 c + i] - and xb is formed from r
// in registers with the lane's own three columns of the statistics; no LDS, no barrier.  Every element is ONE chain over l = 0 .. L_b - 1
// ascending from a zero accumulator: successive MFMAs take (l, l + 1) as k = 0, 1 on the same accumulator.  Cluster rows >= K, columns
// >= F and the slot l + kk >= L_b are zeros by predicate in the operand (never loaded; the slot's xb is zero too, not beta).  asum[k]:
// lanes 0 .. 31 add a[l][k], then a[l + 1][k] (from lane + 32): the sequential f32 sum; the epilogue is fmaf(-asum, c2, acc).
typedef float nv_f32x16 __attribute__((ext_vector_type(16)));
static constexpr int NVM_U = 4;                  // MFMA steps (pairs of l) per load batch
static constexpr int NVM_MT = 64, NVM_NT = 192;  // workgroup tile: clusters x columns
__global__ __launch_bounds__(256) void nv_aggregate_mfma_kernel(const float* __restrict__ a, const float* __restrict__ r,
                                                                const int* __restrict__ row_off, int K, int F, int ntiles,
                                                                const float* __restrict__ mean, const float* __restrict__ var,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ c2, float* __restrict__ V,
                                                                float* __restrict__ asum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int ntile = blockIdx.x % ntiles, mtile = blockIdx.x / ntiles;
  const int m0 = mtile * NVM_MT + (wave & 1) * 32;
  const int n0 = ntile * NVM_NT + (wave >> 1) * 96;
  if (m0 >= K || n0 >= F) return;                // (no barrier in this kernel)
  const int i = lane & 31, kk = lane >> 5;
  const int r0 = row_off[b];
  const int L = row_off[b + 1] - r0;
  const int ncb = min(3, (F - n0 + 31) / 32);    // column blocks of this wave that hold a column < F (>= 1)
  const bool mok = m0 + i < K;
  bool nok[3];
  float mu[3], sc[3], be[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int n = n0 + 32 * c + i;
    nok[c] = n < F;
    mu[c] = nok[c] ? mean[n] : 0.f;
    sc[c] = nok[c] ? rsqrtf(var[n] + 1e-3f) * gamma[n] : 0.f;
    be[c] = nok[c] ? beta[n] : 0.f;
  }
  const float* __restrict__ ap = a + ((long)r0 + kk) * K + m0 + i;
  const float* __restrict__ xp = r + ((long)r0 + kk) * F + n0 + i;
  nv_f32x16 acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[c][j] = 0.f;
  float s = 0.f;
  float ca[NVM_U], cx[NVM_U][3], na[NVM_U], nx[NVM_U][3];
  auto load = [&](int l0, float (&va)[NVM_U], float (&vx)[NVM_U][3]) {
#pragma unroll
    for (int u = 0; u < NVM_U; ++u) {
      const int l = l0 + 2 * u;
      const bool lok = l + kk < L;
      va[u] = (lok && mok) ? ap[(long)l * K] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) vx[u][c] = (lok && nok[c]) ? (xp[(long)l * F + 32 * c] - mu[c]) * sc[c] + be[c] : 0.f;
    }
  };
  load(0, ca, cx);
  for (int l0 = 0; l0 < L; l0 += 2 * NVM_U) {
    load(l0 + 2 * NVM_U, na, nx);                // (all zeros, nothing loaded, past the video's last row)
#pragma unroll
    for (int u = 0; u < NVM_U; ++u) {
      if (l0 + 2 * u < L) {                      // uniform over the wave
        const float other = __shfl_xor(ca[u], 32);
        s += ca[u];                              // lanes < 32: a[l][m0 + i], then a[l + 1][m0 + i] (0 when l + 1 = L)
        s += other;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (c < ncb) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[u], cx[u][c], acc[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < NVM_U; ++u) {
      ca[u] = na[u];
#pragma unroll
      for (int c = 0; c < 3; ++c) cx[u][c] = nx[u][c];
    }
  }
  if (ntile == 0 && (wave >> 1) == 0 && kk == 0 && mok) asum[(long)b * K + m0 + i] = s;
  // C/D map of the 32 x 32 shapes: register j of lane (i, kk) is row (j & 3) + 8 (j >> 2) + 4 kk, column i
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int row = (j & 3) + 8 * (j >> 2) + 4 * kk;
    const float sv = __shfl(s, row);             // asum of cluster m0 + row (lanes 0 .. 31 hold the sums)
    const int m = m0 + row;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int n = n0 + 32 * c + i;
      if (c < ncb && m < K && n < F) V[((long)b * K + m) * F + n] = fmaf(-sv, c2[(long)m * F + n], acc[c][j]);
    }
  }
}

extern "C" int evc_netvlad_aggregate_packed_fwd(const float* a, const float* r, const int32_t* row_off, int B, int T, int K, int F, int R,
                                                int max_k, const float* mean, const float* var, const float* gamma, const float* beta,
                                                const float* c2, float* V, float* asum, void* stream) {
  EVC_REQUIRE(NV_PACKED_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_netvlad_aggregate_packed_fwd: needs K <= 1024, F %% 4 == 0, B <= 65535, max_k <= T, max_k <= R <= B * max_k "
              "(B=%d T=%d K=%d F=%d R=%d max_k=%d)", B, T, K, F, R, max_k);
  EVC_REQUIRE(a && r && row_off && mean && var && gamma && beta && c2 && V && asum, EVC_ERR_BAD_ARG,
              "evc_netvlad_aggregate_packed_fwd: NULL operand");
  EVC_REQUIRE(nv_aligned16(a) && nv_aligned16(r) && nv_aligned16(c2) && nv_aligned16(V), EVC_ERR_BAD_ALIGN,
              "evc_netvlad_aggregate_packed_fwd: a, r, c2 and V must be 16-byte aligned (as for evc_netvlad_aggregate_packed_bwd)");
  const int ntiles = ceil_div(F, NVM_NT), mtiles = ceil_div(K, NVM_MT);
  hipLaunchKernelGGL(nv_aggregate_mfma_kernel, dim3(ntiles * mtiles, B), dim3(256), 0, (hipStream_t)stream, a, r, row_off, K, F, ntiles, mean,
                     var, gamma, beta, c2, V, asum);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- backward: two tiled f32 products over each video's rows, in the pattern of nx_product_kernel<1 / 2, PACKED> (csrc/evc_nextvlad.hip):
// C_b[m][n] = sum_l T_b[l][m] * Bm_b[l][n], m = the video's row, one sequential chain over l ascending per element.
//   MODE 1  dx   l = cluster, n = f:  T[l][m] = a[m][l] (transposed staging),                   Bm = dV_b [K][F]
//   MODE 2  da   l = f, n = cluster:  T[l][m] = xb[m][l], formed from r while it is staged,     Bm = dVt_b [F][Kp];  - q[b][n]
// written next to that template rather than through it: MODE 2 applies the batch-norm inside the staging loop and reads four more
// vectors, which the shared argument block and kernel would have to carry for the NeXtVLAD entries too.  grid (n tiles * m tiles, B)
// sized for the longest video; a workgroup whose row tile lies beyond L_b leaves before the first barrier (uniform over the
// workgroup).  Thread t holds rows mq*8 .. mq*8+8 (mq = t / DW) of float4 column t % DW; the [NV_LC][MT] slice of T is staged in LDS
// (row stride MT + 4), r and dV are read once per tile.  In MODE 2 thread t stages column l0 + t % 64 in every trip of the staging
// loop (256 % 64 == 0), so it loads that column's statistics once per pass.
static constexpr int NV_LC = 64;
struct NvArgs {
  const float* T; int t_ld;                      // a [R][K] (MODE 1) or r [R][F] (MODE 2): T[m*t_ld + l]
  const float* Bm; long b_batch; int b_ld;       // Bm[b*b_batch + l*b_ld + n]
  int L, M, N4;                                  // contraction length, rows of the longest video (sizes the grid), float4 columns
  int DW, MT, ntiles;
  float* C; int c_ld; int c_cols;                // C[m*c_ld + n], n < c_cols
  const float* q; int K;                         // MODE 2: q [B][K]
  const float *mean, *var, *gamma, *beta;        // MODE 2: input_bn over the columns of r
  const int* row_off;
};
template <int MODE>
__global__ __launch_bounds__(256) void nv_product_kernel(const NvArgs p) {
  extern __shared__ float tile[];                // [NV_LC][MT + 4]
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const int ntile = blockIdx.x % p.ntiles, mtile = blockIdx.x / p.ntiles;
  const int MT = p.MT, TS = p.MT + 4, DW = p.DW;
  const int m0 = mtile * MT;
  const int n4 = ntile * DW + t % DW, mq = t / DW;
  const bool active = n4 < p.N4;
  const int r0 = p.row_off[b];
  const int M = p.row_off[b + 1] - r0;
  if (m0 >= M) return;
  const int L = p.L;
  const float* __restrict__ Tb = p.T + (long)r0 * p.t_ld;
  const float* __restrict__ Bb = p.Bm + (long)b * p.b_batch + (long)n4 * 4;
  float4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int l0 = 0; l0 < L; l0 += NV_LC) {
    const int lend = min(NV_LC, L - l0);
    const int l = t % NV_LC;
    const bool lok = l < lend;
    float mu = 0.f, sc = 0.f, be = 0.f;
    if (MODE == 2 && lok) {
      const int f = l0 + l;
      mu = p.mean[f]; sc = rsqrtf(p.var[f] + 1e-3f) * p.gamma[f]; be = p.beta[f];
    }
    for (int i = t; i < NV_LC * MT; i += 256) {
      const int m = i / NV_LC;                   // (i % NV_LC == l)
      float v = 0.f;
      if (lok && m0 + m < M) {
        v = Tb[(long)(m0 + m) * p.t_ld + l0 + l];
        if (MODE == 2) v = (v - mu) * sc + be;
      }
      tile[l * TS + m] = v;
    }
    __syncthreads();
    if (active) {
      const float* tp = tile + mq * 8;
      const float* bp = Bb + (long)l0 * p.b_ld;
#pragma unroll 4
      for (int ll = 0; ll < lend; ++ll) {
        const float4 x = *(const float4*)(bp + (long)ll * p.b_ld);
        const float4 a0 = *(const float4*)(tp + ll * TS), a1 = *(const float4*)(tp + ll * TS + 4);
        const float w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc[j].x += w[j] * x.x; acc[j].y += w[j] * x.y; acc[j].z += w[j] * x.z; acc[j].w += w[j] * x.w;
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  float* __restrict__ Cb = p.C + (long)r0 * p.c_ld;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + mq * 8 + j;
    if (m >= M) break;
    const float4 v = acc[j];
    if (MODE == 1) {
      *(float4*)(Cb + (long)m * p.c_ld + n4 * 4) = v;
    } else {
      const float* __restrict__ q = p.q + (long)b * p.K;
      const int n = n4 * 4;
      if ((p.c_cols & 3) == 0) {                 // (n4 < N4 = c_cols / 4: the whole float4 is inside the row)
        const float4 qq = *(const float4*)(q + n);
        *(float4*)(Cb + (long)m * p.c_ld + n) = make_float4(v.x - qq.x, v.y - qq.y, v.z - qq.z, v.w - qq.w);
      } else {
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (n + c < p.c_cols) Cb[(long)m * p.c_ld + n + c] = vv[c] - q[n + c];
      }
    }
  }
}

// tile shape: the DW in {16, 32, 64} (MT = 128, 64, 32) that wastes the fewest lanes / rows, among those that fill the chip (nx_pick's rule)
template <int MODE>
static int nv_launch(NvArgs& p, int B, void* stream) {
  double best = -1.0;
  for (int dw = 16; dw <= 64; dw *= 2) {
    const int mt = 8 * (256 / dw);
    const int nt = ceil_div(p.N4, dw), mtl = ceil_div(p.M, mt);
    const double blocks = (double)B * nt * mtl;
    const double score = ((double)p.N4 / ((double)nt * dw)) * ((double)p.M / ((double)mtl * mt)) * (blocks < 512.0 ? blocks / 512.0 : 1.0);
    if (score > best) { best = score; p.DW = dw; p.MT = mt; p.ntiles = nt; }
  }
  const int mtl = ceil_div(p.M, p.MT);
  const size_t lds = (size_t)NV_LC * (p.MT + 4) * sizeof(float);       // <= 33792 bytes
  hipLaunchKernelGGL((nv_product_kernel<MODE>), dim3(p.ntiles * mtl, B), dim3(256), lds, (hipStream_t)stream, p);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// dVt[b][f][k] = dV[b][k][f] (k < K; zeros up to Kp = K rounded up to 4): the n-contiguous operand of the da product
__global__ __launch_bounds__(256) void netvlad_dvt_kernel(const float* __restrict__ dV, int K, int Kp, int F, float* __restrict__ dVt) {
  __shared__ float tl[32][33];
  const int b = blockIdx.z;
  const int f0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, f = f0 + tx;
    tl[i][tx] = (k < K && f < F) ? dV[((long)b * K + k) * F + f] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int f = f0 + i, k = k0 + tx;
    if (f < F && k < Kp) dVt[((long)b * F + f) * Kp + k] = tl[tx][i];
  }
}
// q[b][k] = sum_f dV[b][k][f] * c2[k][f]: one wave per (video, cluster)
__global__ __launch_bounds__(256) void netvlad_q_kernel(const float* __restrict__ dV, const float* __restrict__ c2, long BK, int K, int F,
                                                        float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const long bk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bk >= BK) return;
  const int k = (int)(bk % K);
  float s = 0.f;
  for (int f = lane; f < F; f += 64) s += dV[bk * F + f] * c2[(long)k * F + f];
  s = wave_sum(s);
  if (lane == 0) q[bk] = s;
}

// floats of scratch the packed backward entry needs (ops.netvlad_aggregate_packed_bwd_ws computes the same): dVt [B][F][Kp] and q [B][K]
static inline int64_t evc_netvlad_aggregate_packed_bwd_ws(int B, int K, int F) {
  return (int64_t)B * F * ((K + 3) / 4 * 4) + (int64_t)B * K;
}

extern "C" int evc_netvlad_aggregate_packed_bwd(const float* a, const float* r, const int32_t* row_off, int B, int T, int K, int F, int R,
                                                int max_k, const float* mean, const float* var, const float* gamma, const float* beta,
                                                const float* c2, const float* dV, float* da, float* dx, float* ws, int64_t ws_floats,
                                                void* stream) {
  EVC_REQUIRE(NV_PACKED_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_netvlad_aggregate_packed_bwd: needs K <= 1024, F %% 4 == 0, B <= 65535, max_k <= T, max_k <= R <= B * max_k "
              "(B=%d T=%d K=%d F=%d R=%d max_k=%d)", B, T, K, F, R, max_k);
  EVC_REQUIRE(a && r && row_off && mean && var && gamma && beta && c2 && dV && da && dx && ws, EVC_ERR_BAD_ARG,
              "evc_netvlad_aggregate_packed_bwd: NULL operand");
  EVC_REQUIRE(nv_aligned16(a) && nv_aligned16(r) && nv_aligned16(c2) && nv_aligned16(dV) && nv_aligned16(da) && nv_aligned16(dx), EVC_ERR_BAD_ALIGN,
              "evc_netvlad_aggregate_packed_bwd: a, r, c2, dV, da and dx must be 16-byte aligned (float4 access)");
  EVC_REQUIRE(ws_floats >= evc_netvlad_aggregate_packed_bwd_ws(B, K, F) && ((uintptr_t)ws % 16) == 0, EVC_ERR_BAD_ARG,
              "evc_netvlad_aggregate_packed_bwd: ws holds %ld floats, %ld needed (16-byte aligned)", (long)ws_floats,
              (long)evc_netvlad_aggregate_packed_bwd_ws(B, K, F));
  if (max_k == 0) return EVC_OK;                 // no video owns a row: nothing to write
  const int Kp = (K + 3) / 4 * 4;
  float* dVt = ws;
  float* q = ws + (long)B * F * Kp;              // (B * F * Kp is a multiple of 4: q stays 16-byte aligned)
  hipLaunchKernelGGL(netvlad_dvt_kernel, dim3(ceil_div(F, 32), ceil_div(Kp, 32), B), dim3(256), 0, (hipStream_t)stream, dV, K, Kp, F, dVt);
  EVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(netvlad_q_kernel, dim3((unsigned)(((long)B * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dV, c2, (long)B * K, K, F, q);
  EVC_LAUNCH_CHECK();
  {                                              // dx rows of video b: A_b dV_b   (written, not accumulated)
    NvArgs p{};
    p.T = a; p.t_ld = K;
    p.Bm = dV; p.b_batch = (long)K * F; p.b_ld = F;
    p.L = K; p.M = max_k; p.N4 = F / 4;          // (M sizes the grid; the kernel reads every video's own)
    p.C = dx; p.c_ld = F; p.c_cols = F;
    p.row_off = row_off;
    const int rc = nv_launch<1>(p, B, stream);
    if (rc) return rc;
  }
  {                                              // da rows of video b: Xb_b dV_b^T - q_b
    NvArgs p{};
    p.T = r; p.t_ld = F;
    p.Bm = dVt; p.b_batch = (long)F * Kp; p.b_ld = Kp;
    p.L = F; p.M = max_k; p.N4 = Kp / 4;
    p.C = da; p.c_ld = K; p.c_cols = K;
    p.q = q; p.K = K;
    p.mean = mean; p.var = var; p.gamma = gamma; p.beta = beta;
    p.row_off = row_off;
    return nv_launch<2>(p, B, stream);
  }
}

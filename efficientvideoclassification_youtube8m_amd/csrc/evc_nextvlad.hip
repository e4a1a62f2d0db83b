// NeXtVLAD aggregation kernels (EXTENSION - the reference's NeXtVLADModel is an empty stub, cs/frame_level_models.py:349-355, so
// there is no reference math; the binding definition is DESIGN.md 7.12, restated in float64 in tests/_nextvlad_ref.py and checked
// against finite differences).  The GEMM-shaped parts of the tower (expansion, cluster / attention logits, hidden layer, context
// gating, their gradients) run on the library's NT / TN kernels; these are the f32 pieces in between:
//
//   evc_nextvlad_assign_fwd/bwd      a[r,g,k] = softmax_k(cluster_bn(act)[r,g,:])[k] * sigmoid(att_logit[r,g]) and its reverse mode
//   evc_nextvlad_aggregate_fwd/bwd   V[b,k,:] = sum_{s,g} a[b,s,g,k] * xe[b,s,g*D:(g+1)*D] - asum[b,k] * c2[k,:]; da, dxe from dV
//   evc_nextvlad_aggregate_packed_fwd/bwd, evc_frames_gather_packed   the same over a ragged, packed list of frames per video (7.13)
//   evc_frames_gather_packed_sel, evc_scatter_rows   serving a subset of the batch's videos: packed rows of the selected videos, and their
//                                    result rows back to the batch's row numbers (7.15)
//   evc_frames_gather_packed_tab     the packed rows of the frames a source-frame table names (--student_sampling on grid towers, 7.20)
//   evc_nextvlad_aggregate_packed_fwd_mfma   the packed forward on the f32 matrix cores, for forward-only towers: the same bits (7.14)
//   evc_nextvlad_normalize_fwd/bwd   U[b,k,:] = V[b,k,:] / max(|V[b,k,:]|, 1e-12)
//   evc_nextvlad_gate_fwd/bwd        out = h * sigmoid(gl) (context gating); _bwd_add: with a second gradient on out (7.14)
//   evc_nextvlad_colsum              out[c] = sum_r x[r][c] in a fixed order (the two bias gradients)
//   evc_nextvlad_center_cast         bf16(xe - be): the centred operand of the cluster / attention products; with it
//   evc_nextvlad_bias_logits         be.W in f32 (the products' bias) and evc_nextvlad_wgrad_uncenter (the rank-one gradient term)
//   evc_nextvlad_dropout_fwd/bwd     dropout before the hidden layer: vlad_bn apply + stateless Philox mask + bf16 store; dY masked (7.17)
//
// Layouts: sampled frames row-major, row b*S+s; xe [R][E] with group g in columns g*D .. g*D+D, so that one video's xe is a
// contiguous [P][D] matrix X_b over the P = S*G (frame, group) pairs, and its assignment a [R][G][K] a contiguous [P][K] matrix
// A_b.  The aggregation is then V_b = A_b^T X_b, and its reverse mode dX_b = A_b dV_b, dA_b = X_b dV_b^T - q_b: three small f32
// products per video, all on nx_product_kernel below.  V / dV / U are [B][K][D] (cluster-major: towers.NeXtVladTower converts
// to the TF order d*K+k in state_dict()).  Every sum runs in a fixed order (no atomics): two runs give the same bits.
#include "evc_common.h"

static inline bool nx_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
static inline int nx_grid(long n) { long nb = (n + 255) / 256; return (int)(nb < 1 ? 1 : (nb < 8192 ? nb : 8192)); }

// ---- assignment: one wave per (sampled frame, group) ----
// y = cluster_bn(act)[row, g*K + k]; p = softmax_k(y) left in y[]; returns nothing, all lanes hold their y[i] for k = lane + 64 i
__device__ __forceinline__ void nx_group_softmax(const float* __restrict__ act, long base, int col0, int K, int lane,
                                                 const float* __restrict__ mean, const float* __restrict__ var,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float (&y)[16]) {
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    y[i] = -INFINITY;
    if (k < K) {
      const int c = col0 + k;
      y[i] = (act[base + k] - mean[c]) * rsqrtf(var[c] + 1e-3f) * gamma[c] + beta[c];
      mx = fmaxf(mx, y[i]);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    if (k < K) { y[i] = __expf(y[i] - mx); sum += y[i]; } else y[i] = 0.f;
  }
  const float inv = 1.0f / wave_sum(sum);
#pragma unroll
  for (int i = 0; i < 16; ++i) y[i] *= inv;
}

__global__ __launch_bounds__(256) void nextvlad_assign_fwd_kernel(const float* __restrict__ act, int R, int G, int K,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ attl, long ld_att,
                                                                  const float* __restrict__ att_bias, float* __restrict__ a) {
  const int lane = threadIdx.x & 63;
  const long rg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rg >= (long)R * G) return;
  const long row = rg / G;
  const int g = (int)(rg % G);
  float y[16];                                   // K <= 1024
  nx_group_softmax(act, rg * K, g * K, K, lane, mean, var, gamma, beta, y);
  const float att = sigmoidf_(attl[row * ld_att + g] + (att_bias ? att_bias[g] : 0.f));
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    if (k < K) a[rg * K + k] = y[i] * att;
  }
}
extern "C" int evc_nextvlad_assign_fwd(const float* act, int R, int G, int K, const float* mean, const float* var, const float* gamma,
                                       const float* beta, const float* att_logits, int64_t ld_att, const float* att_bias, float* a,
                                       void* stream) {
  EVC_REQUIRE(R > 0 && G > 0 && K > 0 && K <= 1024 && ld_att >= G && (long)R * G < (1L << 31), EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_assign_fwd: needs 1 <= clusters <= 1024, ld_att >= groups (R=%d G=%d K=%d ld_att=%ld)", R, G, K, (long)ld_att);
  EVC_REQUIRE(act && mean && var && gamma && beta && att_logits && a, EVC_ERR_BAD_ARG, "evc_nextvlad_assign_fwd: NULL operand");
  hipLaunchKernelGGL(nextvlad_assign_fwd_kernel, dim3((unsigned)(((long)R * G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, act, R, G, K,
                     mean, var, gamma, beta, att_logits, (long)ld_att, att_bias, a);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// dz = p * att * (da - sum_k p da), datt_logit = (sum_k p da) * att * (1 - att).  p is recomputed from act and the statistics
// (a / att would divide by a sigmoid that may have underflowed).
__global__ __launch_bounds__(256) void nextvlad_assign_bwd_kernel(const float* __restrict__ act, int R, int G, int K,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ attl, long ld_att,
                                                                  const float* __restrict__ att_bias, const float* __restrict__ da,
                                                                  float* __restrict__ dz, float* __restrict__ datt,
                                                                  bf16_t* __restrict__ datt_bf, long ld_bf) {
  const int lane = threadIdx.x & 63;
  const long rg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rg >= (long)R * G) return;
  const long row = rg / G;
  const int g = (int)(rg % G);
  float y[16];
  nx_group_softmax(act, rg * K, g * K, K, lane, mean, var, gamma, beta, y);
  float d[16];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    d[i] = (k < K) ? da[rg * K + k] : 0.f;
    dot += y[i] * d[i];
  }
  dot = wave_sum(dot);
  const float att = sigmoidf_(attl[row * ld_att + g] + (att_bias ? att_bias[g] : 0.f));
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = lane + 64 * i;
    if (k < K) dz[rg * K + k] = y[i] * att * (d[i] - dot);
  }
  if (lane == 0) {
    const float dl = dot * att * (1.0f - att);
    datt[rg] = dl;
    if (datt_bf) datt_bf[row * ld_bf + g] = f32_to_bf16(dl);
  }
}
extern "C" int evc_nextvlad_assign_bwd(const float* act, int R, int G, int K, const float* mean, const float* var, const float* gamma,
                                       const float* beta, const float* att_logits, int64_t ld_att, const float* att_bias, const float* da,
                                       float* dz, float* datt_logit, evc_bf16* datt_logit_bf16, int64_t ld_bf16, void* stream) {
  EVC_REQUIRE(R > 0 && G > 0 && K > 0 && K <= 1024 && ld_att >= G && (long)R * G < (1L << 31) && (!datt_logit_bf16 || ld_bf16 >= G),
              EVC_ERR_BAD_SHAPE, "evc_nextvlad_assign_bwd: needs 1 <= clusters <= 1024, ld_att / ld_bf16 >= groups (R=%d G=%d K=%d)", R, G, K);
  EVC_REQUIRE(act && mean && var && gamma && beta && att_logits && da && dz && datt_logit, EVC_ERR_BAD_ARG,
              "evc_nextvlad_assign_bwd: NULL operand");
  hipLaunchKernelGGL(nextvlad_assign_bwd_kernel, dim3((unsigned)(((long)R * G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, act, R, G, K,
                     mean, var, gamma, beta, att_logits, (long)ld_att, att_bias, da, dz, datt_logit, (bf16_t*)datt_logit_bf16, (long)ld_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- the per-video f32 product  C_b[m][n] = sum_l T_b[l][m] * Bm_b[l][n]  behind the aggregation and its reverse mode.
// grid (n tiles * m tiles, B).  A workgroup owns MT = 8 * (256 / DW) rows m and DW float4 columns n: thread t holds rows
// mq*8 .. mq*8+8 (mq = t / DW) of float4 column t % DW in registers.  The contraction runs in passes of NX_LC rows l: the
// [NX_LC][MT] slice of T is staged in LDS (row stride MT + 4 floats: 16-byte aligned rows; the transposed staging of MODE 1 / 2
// writes with stride MT + 4 between lanes, a 4-way bank conflict on 1/33 of the inner loop's LDS traffic), then every thread
// reads its 8 values of a row as two 16-byte LDS loads that are uniform over the DW lanes sharing mq (broadcast) and one
// float4 of Bm from global memory (consecutive lanes, consecutive 16 bytes): 32 FMAs per 3 loads.
//   MODE 0  aggregate forward  l = pair p, m = cluster, n = d:  T = A_b [P][K] (staged as is),       Bm = X_b [P][D]
//   MODE 1  dxe                l = cluster, m = pair,   n = d:  T[l][m] = A_b[m][l] (transposed),    Bm = dV_b [K][D]
//   MODE 2  da                 l = d,       m = pair,   n = k:  T[l][m] = X_b[m][l] (transposed),    Bm = dVt_b [D][Kp]
static constexpr int NX_LC = 64;
struct NxArgs {
  const float* T; long t_batch; int t_ld;        // source of T: MODE 0 T[l*t_ld + m], MODE 1 / 2 T[m*t_ld + l]
  const float* Bm; long b_batch; int b_ld;       // Bm[l*b_ld + n]
  int L, M, N4;                                  // contraction length, rows, float4 columns
  int DW, MT, ntiles;
  float* C; long c_batch; int c_ld; int c_cols;  // C[m*c_ld + n], n < c_cols
  const float* sub; long sub_batch;              // MODE 0: c2 [K][D] (sub_batch 0); MODE 2: q [B][K]
  float* asum;                                   // MODE 0: [B][K]
  const int* row_off; int G;                     // PACKED: first frame row of every video [B+1], groups (pairs per frame row)
};
// PACKED (ragged videos): video b owns the pairs row_off[b]*G .. row_off[b+1]*G of the pair-major operands (T in
// every mode, Bm in MODE 0, C in MODE 1 / 2) instead of a fixed batch stride, and its pair count P_b replaces L (MODE 0) or M
// (MODE 1 / 2); the grid is sized for the longest video and a workgroup whose row tile lies beyond P_b leaves before the first
// barrier (the condition is uniform over the workgroup).  Every element keeps the summation order of the fixed-length path.
template <int MODE, bool PACKED = false>
__global__ __launch_bounds__(256) void nx_product_kernel(const NxArgs p) {
  extern __shared__ float tile[];                // [NX_LC][MT + 4]
  __shared__ float sa[128];                      // MODE 0: column sums of T over all l (asum of this workgroup's clusters)
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const int ntile = blockIdx.x % p.ntiles, mtile = blockIdx.x / p.ntiles;
  const int MT = p.MT, TS = p.MT + 4, DW = p.DW;
  const int m0 = mtile * MT;
  const int n4 = ntile * DW + t % DW, mq = t / DW;
  const bool active = n4 < p.N4;
  int L = p.L, M = p.M;
  long t_base = (long)b * p.t_batch, b_base = (long)b * p.b_batch, c_base = (long)b * p.c_batch;
  if (PACKED) {
    const int r0 = p.row_off[b];
    const long pair0 = (long)r0 * p.G;
    const int Pb = (p.row_off[b + 1] - r0) * p.G;
    t_base = pair0 * p.t_ld;
    if (MODE == 0) { L = Pb; b_base = pair0 * p.b_ld; }
    else { M = Pb; c_base = pair0 * p.c_ld; if (m0 >= M) return; }
  }
  const float* __restrict__ Tb = p.T + t_base;
  const float* __restrict__ Bb = p.Bm + b_base + (long)n4 * 4;
  float4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  float colsum = 0.f;
  for (int l0 = 0; l0 < L; l0 += NX_LC) {
    const int lend = min(NX_LC, L - l0);
    if (MODE == 0) {
      for (int i = t; i < NX_LC * MT; i += 256) {
        const int l = i / MT, m = i % MT;
        tile[l * TS + m] = (l < lend && m0 + m < M) ? Tb[(long)(l0 + l) * p.t_ld + m0 + m] : 0.f;
      }
    } else {
      for (int i = t; i < NX_LC * MT; i += 256) {
        const int m = i / NX_LC, l = i % NX_LC;
        tile[l * TS + m] = (l < lend && m0 + m < M) ? Tb[(long)(m0 + m) * p.t_ld + l0 + l] : 0.f;
      }
    }
    __syncthreads();
    if (MODE == 0 && t < MT) {
      for (int l = 0; l < lend; ++l) colsum += tile[l * TS + t];
    }
    if (active) {
      const float* tp = tile + mq * 8;
      const float* bp = Bb + (long)l0 * p.b_ld;
#pragma unroll 4
      for (int l = 0; l < lend; ++l) {
        const float4 x = *(const float4*)(bp + (long)l * p.b_ld);
        const float4 a0 = *(const float4*)(tp + l * TS), a1 = *(const float4*)(tp + l * TS + 4);
        const float w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          acc[j].x += w[j] * x.x; acc[j].y += w[j] * x.y; acc[j].z += w[j] * x.z; acc[j].w += w[j] * x.w;
        }
      }
    }
    __syncthreads();
  }
  if (MODE == 0) {
    if (t < MT) {
      sa[t] = colsum;
      if (ntile == 0 && m0 + t < M) p.asum[(long)b * M + m0 + t] = colsum;
    }
    __syncthreads();
  }
  if (!active) return;
  float* __restrict__ Cb = p.C + c_base;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + mq * 8 + j;
    if (m >= M) break;
    float4 v = acc[j];
    if (MODE == 0) {
      const float s = sa[mq * 8 + j];
      const float4 c = *(const float4*)(p.sub + (long)m * p.c_ld + n4 * 4);
      v = make_float4(v.x - s * c.x, v.y - s * c.y, v.z - s * c.z, v.w - s * c.w);
      *(float4*)(Cb + (long)m * p.c_ld + n4 * 4) = v;
    } else if (MODE == 1) {
      *(float4*)(Cb + (long)m * p.c_ld + n4 * 4) = v;
    } else {
      const float* __restrict__ q = p.sub + (long)b * p.sub_batch;
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

// tile shape: the DW in {16, 32, 64} (MT = 128, 64, 32) that wastes the fewest lanes / rows, among those that give the chip
// two workgroups per CU where the shape allows it
static void nx_pick(NxArgs& p, int B) {
  double best = -1.0;
  for (int dw = 16; dw <= 64; dw *= 2) {
    const int mt = 8 * (256 / dw);
    const int nt = ceil_div(p.N4, dw), mtl = ceil_div(p.M, mt);
    const double blocks = (double)B * nt * mtl;
    const double score = ((double)p.N4 / ((double)nt * dw)) * ((double)p.M / ((double)mtl * mt)) * (blocks < 512.0 ? blocks / 512.0 : 1.0);
    if (score > best) { best = score; p.DW = dw; p.MT = mt; p.ntiles = nt; }
  }
}
template <int MODE, bool PACKED = false>
static int nx_launch(NxArgs& p, int B, void* stream) {
  nx_pick(p, B);
  const int mtl = ceil_div(p.M, p.MT);
  const size_t lds = (size_t)NX_LC * (p.MT + 4) * sizeof(float);       // <= 33792 bytes (+ 512 static)
  hipLaunchKernelGGL((nx_product_kernel<MODE, PACKED>), dim3(p.ntiles * mtl, B), dim3(256), lds, (hipStream_t)stream, p);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

#define NX_AGG_SHAPE_OK (B > 0 && B <= 65535 && S > 0 && S <= 64 && G > 0 && (long)S * G <= 1024 && K > 0 && K <= 1024 && D > 0 && D % 4 == 0)

extern "C" int evc_nextvlad_aggregate_fwd(const float* a, const float* xe, int B, int S, int G, int K, int D, const float* c2, float* V,
                                          float* asum, void* stream) {
  EVC_REQUIRE(NX_AGG_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_aggregate_fwd: needs S <= 64, S * G <= 1024, K <= 1024, D %% 4 == 0, B <= 65535 (B=%d S=%d G=%d K=%d D=%d)", B, S, G, K, D);
  EVC_REQUIRE(a && xe && c2 && V && asum, EVC_ERR_BAD_ARG, "evc_nextvlad_aggregate_fwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(a) && nx_aligned16(xe) && nx_aligned16(c2) && nx_aligned16(V), EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_aggregate_fwd: a, xe, c2 and V must be 16-byte aligned (float4 access)");
  const int P = S * G;
  NxArgs p{};
  p.T = a; p.t_batch = (long)P * K; p.t_ld = K;
  p.Bm = xe; p.b_batch = (long)P * D; p.b_ld = D;
  p.L = P; p.M = K; p.N4 = D / 4;
  p.C = V; p.c_batch = (long)K * D; p.c_ld = D; p.c_cols = D;
  p.sub = c2; p.sub_batch = 0; p.asum = asum;
  return nx_launch<0>(p, B, stream);
}

// dVt[b][d][k] = dV[b][k][d] (k < K; zeros up to Kp = K rounded up to 4): the n-contiguous operand of the da product
__global__ __launch_bounds__(256) void nextvlad_dvt_kernel(const float* __restrict__ dV, int K, int Kp, int D, float* __restrict__ dVt) {
  __shared__ float tl[32][33];
  const int b = blockIdx.z;
  const int d0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int k = k0 + i, d = d0 + tx;
    tl[i][tx] = (k < K && d < D) ? dV[((long)b * K + k) * D + d] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int d = d0 + i, k = k0 + tx;
    if (d < D && k < Kp) dVt[((long)b * D + d) * Kp + k] = tl[tx][i];
  }
}
// q[b][k] = sum_d dV[b][k][d] * c2[k][d]: one wave per (video, cluster)
__global__ __launch_bounds__(256) void nextvlad_q_kernel(const float* __restrict__ dV, const float* __restrict__ c2, long BK, int K, int D,
                                                         float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const long bk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bk >= BK) return;
  const int k = (int)(bk % K);
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += dV[bk * D + d] * c2[(long)k * D + d];
  s = wave_sum(s);
  if (lane == 0) q[bk] = s;
}

// floats of scratch the backward entry needs (ops.nextvlad_aggregate_bwd_ws computes the same): dVt [B][D][Kp] and q [B][K]
static inline int64_t evc_nextvlad_aggregate_bwd_ws(int B, int K, int D) {
  return (int64_t)B * D * ((K + 3) / 4 * 4) + (int64_t)B * K;
}

extern "C" int evc_nextvlad_aggregate_bwd(const float* a, const float* xe, int B, int S, int G, int K, int D, const float* c2,
                                          const float* dV, float* da, float* dxe, float* ws, int64_t ws_floats, void* stream) {
  EVC_REQUIRE(NX_AGG_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_aggregate_bwd: needs S <= 64, S * G <= 1024, K <= 1024, D %% 4 == 0, B <= 65535 (B=%d S=%d G=%d K=%d D=%d)", B, S, G, K, D);
  EVC_REQUIRE(a && xe && c2 && dV && da && dxe && ws, EVC_ERR_BAD_ARG, "evc_nextvlad_aggregate_bwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(a) && nx_aligned16(xe) && nx_aligned16(c2) && nx_aligned16(dV) && nx_aligned16(da) && nx_aligned16(dxe), EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_aggregate_bwd: a, xe, c2, dV, da and dxe must be 16-byte aligned (float4 access)");
  EVC_REQUIRE(ws_floats >= evc_nextvlad_aggregate_bwd_ws(B, K, D) && ((uintptr_t)ws % 16) == 0, EVC_ERR_BAD_ARG,
              "evc_nextvlad_aggregate_bwd: ws holds %ld floats, %ld needed (16-byte aligned)", (long)ws_floats,
              (long)evc_nextvlad_aggregate_bwd_ws(B, K, D));
  const int P = S * G, Kp = (K + 3) / 4 * 4;
  float* dVt = ws;
  float* q = ws + (long)B * D * Kp;              // (B * D * Kp is a multiple of 4: q stays 16-byte aligned)
  hipLaunchKernelGGL(nextvlad_dvt_kernel, dim3(ceil_div(D, 32), ceil_div(Kp, 32), B), dim3(256), 0, (hipStream_t)stream, dV, K, Kp, D, dVt);
  EVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(nextvlad_q_kernel, dim3((unsigned)(((long)B * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dV, c2, (long)B * K, K, D, q);
  EVC_LAUNCH_CHECK();
  {                                              // dxe[b][p][d] = sum_k a[b][p][k] dV[b][k][d]   (written, not accumulated)
    NxArgs p{};
    p.T = a; p.t_batch = (long)P * K; p.t_ld = K;
    p.Bm = dV; p.b_batch = (long)K * D; p.b_ld = D;
    p.L = K; p.M = P; p.N4 = D / 4;
    p.C = dxe; p.c_batch = (long)P * D; p.c_ld = D; p.c_cols = D;
    const int rc = nx_launch<1>(p, B, stream);
    if (rc) return rc;
  }
  {                                              // da[b][p][k] = sum_d xe[b][p][d] dV[b][k][d] - q[b][k]
    NxArgs p{};
    p.T = xe; p.t_batch = (long)P * D; p.t_ld = D;
    p.Bm = dVt; p.b_batch = (long)D * Kp; p.b_ld = Kp;
    p.L = D; p.M = P; p.N4 = Kp / 4;
    p.C = da; p.c_batch = (long)P * K; p.c_ld = K; p.c_cols = K;
    p.sub = q; p.sub_batch = K;
    return nx_launch<2>(p, B, stream);
  }
}

// ---- ragged videos: video b owns the frame rows row_off[b] .. row_off[b+1] of a, xe, da, dxe, k_b of them in
// time order (k_b = 0: none).  The same three products with a per-video length; B * K * D outputs and the scratch as above.
#define NX_PACKED_SHAPE_OK                                                                                                          \
  (B > 0 && B <= 65535 && T > 0 && G > 0 && (long)T * G < (1L << 31) && K > 0 && K <= 1024 && D > 0 && D % 4 == 0 && max_k >= 0 && \
   max_k <= T && R >= max_k && (long)R <= (long)B * max_k && (long)R * G < (1L << 31))

extern "C" int evc_nextvlad_aggregate_packed_fwd(const float* a, const float* xe, const int32_t* row_off, int B, int T, int G, int K, int D,
                                                 int R, int max_k, const float* c2, float* V, float* asum, void* stream) {
  EVC_REQUIRE(NX_PACKED_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_aggregate_packed_fwd: needs K <= 1024, D %% 4 == 0, B <= 65535, max_k <= T, max_k <= R <= B * max_k "
              "(B=%d T=%d G=%d K=%d D=%d R=%d max_k=%d)", B, T, G, K, D, R, max_k);
  EVC_REQUIRE(a && xe && row_off && c2 && V && asum, EVC_ERR_BAD_ARG, "evc_nextvlad_aggregate_packed_fwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(a) && nx_aligned16(xe) && nx_aligned16(c2) && nx_aligned16(V), EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_aggregate_packed_fwd: a, xe, c2 and V must be 16-byte aligned (float4 access)");
  NxArgs p{};
  p.T = a; p.t_ld = K;
  p.Bm = xe; p.b_ld = D;
  p.L = max_k * G; p.M = K; p.N4 = D / 4;        // (L is read per video in the kernel)
  p.C = V; p.c_batch = (long)K * D; p.c_ld = D; p.c_cols = D;
  p.sub = c2; p.sub_batch = 0; p.asum = asum;
  p.row_off = row_off; p.G = G;
  return nx_launch<0, true>(p, B, stream);
}

// ---- the packed forward aggregation on the f32 matrix cores: V_b = A_b^T X_b - asum_b (x) c2 with
// v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fmaf chain - the chain nx_product_kernel<0, true> computes with
// v_pk_fma_f32 - so this entry gives the bits of evc_nextvlad_aggregate_packed_fwd.  Forward only, mode 0 only (the frozen tower).
// grid (n tiles * m tiles, B), 4 waves: a workgroup owns 128 clusters x 96 columns, wave w the clusters m0 = 32 w .. 32 w + 32 of it
// and three 32 x 32 accumulators (the columns n0, n0 + 32, n0 + 64).  Both operands are read from global memory in the layout the
// instruction wants - lane (i = lane & 31, kk = lane >> 5) holds a[pair l + kk][m0 + i] and xe[pair l + kk][n0 + 32 c + i], 32
// consecutive floats per half-wave - so there is no LDS, no transpose and no barrier; the loads of the next NXM_U MFMA steps (2 NXM_U
// pairs) are issued before the MFMAs of the current ones.  Every element is ONE chain over l = 0 .. L_b - 1 ascending from a zero
// accumulator: successive MFMAs take (l, l + 1) as k = 0, 1 on the same accumulator, nothing is split over waves or workgroups.
// Cluster rows >= K, columns >= D and the slot l + kk >= L_b are zeros by predicate in the operand (never loaded: no address at or
// beyond the video's last pair is formed into a load, and 0 * NaN cannot enter).  asum[k]: lanes 0 .. 31 add a[l][k], then a[l+1][k]
// (fetched from lane + 32), the sequential sum of the existing entry; the epilogue is fmaf(-asum, c2, acc).
// gfx950: 66 VGPRs + 48 AGPRs (the three accumulators), 0 bytes of LDS, no scratch, no atomics (hipcc -O3).
typedef float nx_f32x16 __attribute__((ext_vector_type(16)));
static constexpr int NXM_U = 4;                  // MFMA steps (pairs of l) per load batch
static constexpr int NXM_MT = 128, NXM_NT = 96;  // workgroup tile: clusters x columns
__global__ __launch_bounds__(256) void nx_aggregate_mfma_kernel(const float* __restrict__ a, const float* __restrict__ xe,
                                                                const int* __restrict__ row_off, int G, int K, int D, int ntiles,
                                                                const float* __restrict__ c2, float* __restrict__ V,
                                                                float* __restrict__ asum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int ntile = blockIdx.x % ntiles, mtile = blockIdx.x / ntiles;
  const int m0 = mtile * NXM_MT + wave * 32;
  if (m0 >= K) return;                           // (no barrier in this kernel)
  const int n0 = ntile * NXM_NT;
  const int i = lane & 31, kk = lane >> 5;
  const int r0 = row_off[b];
  const long pair0 = (long)r0 * G;
  const int L = (row_off[b + 1] - r0) * G;
  const int ncb = min(3, (D - n0 + 31) / 32);    // column blocks of this workgroup that hold a column < D (>= 1)
  const bool mok = m0 + i < K;
  const bool nok[3] = {n0 + i < D, n0 + 32 + i < D, n0 + 64 + i < D};
  const float* __restrict__ ap = a + (pair0 + kk) * K + m0 + i;
  const float* __restrict__ xp = xe + (pair0 + kk) * D + n0 + i;
  nx_f32x16 acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  float s = 0.f;
  float ca[NXM_U], cx[NXM_U][3], na[NXM_U], nx[NXM_U][3];
  auto load = [&](int l0, float (&va)[NXM_U], float (&vx)[NXM_U][3]) {
#pragma unroll
    for (int u = 0; u < NXM_U; ++u) {
      const int l = l0 + 2 * u;
      const bool lok = l + kk < L;
      va[u] = (lok && mok) ? ap[(long)l * K] : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) vx[u][c] = (lok && nok[c]) ? xp[(long)l * D + 32 * c] : 0.f;
    }
  };
  load(0, ca, cx);
  for (int l0 = 0; l0 < L; l0 += 2 * NXM_U) {
    load(l0 + 2 * NXM_U, na, nx);                // (all zeros, nothing loaded, past the video's last pair)
#pragma unroll
    for (int u = 0; u < NXM_U; ++u) {
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
    for (int u = 0; u < NXM_U; ++u) {
      ca[u] = na[u];
#pragma unroll
      for (int c = 0; c < 3; ++c) cx[u][c] = nx[u][c];
    }
  }
  if (ntile == 0 && kk == 0 && mok) asum[(long)b * K + m0 + i] = s;
  // C/D map of the 32 x 32 shapes: register r of lane (i, kk) is row (r & 3) + 8 (r >> 2) + 4 kk, column i
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;
    const float sv = __shfl(s, row);             // asum of cluster m0 + row (lanes 0 .. 31 hold the sums)
    const int m = m0 + row;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int n = n0 + 32 * c + i;
      if (c < ncb && m < K && n < D) V[((long)b * K + m) * D + n] = fmaf(-sv, c2[(long)m * D + n], acc[c][r]);
    }
  }
}

extern "C" int evc_nextvlad_aggregate_packed_fwd_mfma(const float* a, const float* xe, const int32_t* row_off, int B, int T, int G, int K,
                                                      int D, int R, int max_k, const float* c2, float* V, float* asum, void* stream) {
  EVC_REQUIRE(NX_PACKED_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_aggregate_packed_fwd_mfma: needs K <= 1024, D %% 4 == 0, B <= 65535, max_k <= T, max_k <= R <= B * max_k "
              "(B=%d T=%d G=%d K=%d D=%d R=%d max_k=%d)", B, T, G, K, D, R, max_k);
  EVC_REQUIRE(a && xe && row_off && c2 && V && asum, EVC_ERR_BAD_ARG, "evc_nextvlad_aggregate_packed_fwd_mfma: NULL operand");
  EVC_REQUIRE(nx_aligned16(a) && nx_aligned16(xe) && nx_aligned16(c2) && nx_aligned16(V), EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_aggregate_packed_fwd_mfma: a, xe, c2 and V must be 16-byte aligned (as for evc_nextvlad_aggregate_packed_fwd)");
  const int ntiles = ceil_div(D, NXM_NT), mtiles = ceil_div(K, NXM_MT);
  hipLaunchKernelGGL(nx_aggregate_mfma_kernel, dim3(ntiles * mtiles, B), dim3(256), 0, (hipStream_t)stream, a, xe, row_off, G, K, D, ntiles, c2,
                     V, asum);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_nextvlad_aggregate_packed_bwd(const float* a, const float* xe, const int32_t* row_off, int B, int T, int G, int K, int D,
                                                 int R, int max_k, const float* c2, const float* dV, float* da, float* dxe, float* ws,
                                                 int64_t ws_floats, void* stream) {
  EVC_REQUIRE(NX_PACKED_SHAPE_OK, EVC_ERR_BAD_SHAPE,
              "evc_nextvlad_aggregate_packed_bwd: needs K <= 1024, D %% 4 == 0, B <= 65535, max_k <= T, max_k <= R <= B * max_k "
              "(B=%d T=%d G=%d K=%d D=%d R=%d max_k=%d)", B, T, G, K, D, R, max_k);
  EVC_REQUIRE(a && xe && row_off && c2 && dV && da && dxe && ws, EVC_ERR_BAD_ARG, "evc_nextvlad_aggregate_packed_bwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(a) && nx_aligned16(xe) && nx_aligned16(c2) && nx_aligned16(dV) && nx_aligned16(da) && nx_aligned16(dxe), EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_aggregate_packed_bwd: a, xe, c2, dV, da and dxe must be 16-byte aligned (float4 access)");
  EVC_REQUIRE(ws_floats >= evc_nextvlad_aggregate_bwd_ws(B, K, D) && ((uintptr_t)ws % 16) == 0, EVC_ERR_BAD_ARG,
              "evc_nextvlad_aggregate_packed_bwd: ws holds %ld floats, %ld needed (16-byte aligned)", (long)ws_floats,
              (long)evc_nextvlad_aggregate_bwd_ws(B, K, D));
  if (max_k == 0) return EVC_OK;                 // no video owns a row: nothing to write
  const int Pmax = max_k * G, Kp = (K + 3) / 4 * 4;
  float* dVt = ws;
  float* q = ws + (long)B * D * Kp;
  hipLaunchKernelGGL(nextvlad_dvt_kernel, dim3(ceil_div(D, 32), ceil_div(Kp, 32), B), dim3(256), 0, (hipStream_t)stream, dV, K, Kp, D, dVt);
  EVC_LAUNCH_CHECK();
  hipLaunchKernelGGL(nextvlad_q_kernel, dim3((unsigned)(((long)B * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dV, c2, (long)B * K, K, D, q);
  EVC_LAUNCH_CHECK();
  {                                              // dxe rows of video b: A_b dV_b   (written, not accumulated)
    NxArgs p{};
    p.T = a; p.t_ld = K;
    p.Bm = dV; p.b_batch = (long)K * D; p.b_ld = D;
    p.L = K; p.M = Pmax; p.N4 = D / 4;           // (M sizes the grid; the kernel reads every video's own)
    p.C = dxe; p.c_ld = D; p.c_cols = D;
    p.row_off = row_off; p.G = G;
    const int rc = nx_launch<1, true>(p, B, stream);
    if (rc) return rc;
  }
  {                                              // da rows of video b: X_b dV_b^T - q_b
    NxArgs p{};
    p.T = xe; p.t_ld = D;
    p.Bm = dVt; p.b_batch = (long)D * Kp; p.b_ld = Kp;
    p.L = D; p.M = Pmax; p.N4 = Kp / 4;
    p.C = da; p.c_ld = K; p.c_cols = K;
    p.sub = q; p.sub_batch = K;
    p.row_off = row_off; p.G = G;
    return nx_launch<2, true>(p, B, stream);
  }
}

// ---- the packed rows themselves: row row_off[b] + j is frame j * every_n of video b, dequantised / l2-normalised with the
// arithmetic of sample_gather_kernel (evc_elementwise.hip) in the same order, so that one source frame gives the same bits through
// either gather.  One wave per row; the row's video by a binary search of row_off (the last b with row_off[b] <= row: videos
// without a row are stepped over).  Rows R .. Rp are zeros (the padding of the TN products' contraction), also in the bf16 copy.
// SEL (evc_frames_gather_packed_sel, 7.15): packed video j is source video sel[j] of the unchanged batch - B counts the packed videos,
// nfr and x are indexed by the source video - and the f32 rows are optional (out NULL: the bf16 rows alone).
template <bool SEL>
__global__ __launch_bounds__(256) void frames_gather_packed_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                                   const int* __restrict__ nfr, const int* __restrict__ row_off,
                                                                   const int* __restrict__ sel, int B, int T, int F, int every_n, int R,
                                                                   int Rp, int normalize, float* __restrict__ out,
                                                                   uint2* __restrict__ out_bf) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Rp) return;
  const int F4 = F >> 2;
  float4* dst = (!SEL || out) ? (float4*)(out + row * F) : nullptr;
  uint2* dst_bf = out_bf ? out_bf + row * F4 : nullptr;
  if (row >= R) {
    for (int j = lane; j < F4; j += 64) {
      if (dst) dst[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dst_bf) dst_bf[j] = make_uint2(0u, 0u);
    }
    return;
  }
  int b = 0, hi = B;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (row_off[mid] <= (int)row) b = mid; else hi = mid;
  }
  long fr = (long)((int)row - row_off[b]) * every_n;
  if (SEL) b = sel[b];                           // from here on b is the source video
  const int n = nfr[b];
  const int idx = fr < 0 ? 0 : (fr >= T ? T - 1 : (int)fr);
  const bool padded = xq && idx >= n;            // uint8 input: frames >= num_frames are padding (zero after Dequantize)
  auto load = [&](int j) {
    if (padded) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (xq) {
      const uchar4 q = ((const uchar4*)(xq + ((long)b * T + idx) * F))[j];
      const float sc = 4.0f / 255.0f, bi = 4.0f / 512.0f - 2.0f;
      return make_float4(q.x * sc + bi, q.y * sc + bi, q.z * sc + bi, q.w * sc + bi);
    }
    return ((const float4*)(x + ((long)b * T + idx) * F))[j];
  };
  float inv = 1.f;
  if (normalize) {
    float ss = 0.f;
    for (int j = lane; j < F4; j += 64) { const float4 v = load(j); ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
    inv = rsqrtf(fmaxf(wave_sum(ss), 1e-12f));
  }
  for (int j = lane; j < F4; j += 64) {
    float4 v = load(j); v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    if (dst) dst[j] = v;
    if (dst_bf) dst_bf[j] = make_uint2(pack_bf16x2_hw(v.x, v.y), pack_bf16x2_hw(v.z, v.w));
  }
}
extern "C" int evc_frames_gather_packed(const float* x, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* row_off, int B, int T,
                                        int F, int every_n, int R, int Rp, int normalize, float* out, evc_bf16* out_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && every_n >= 1 && R >= 0 && Rp >= R && Rp - R < 32 &&
              (long)R <= (long)B * ((T + every_n - 1) / every_n), EVC_ERR_BAD_SHAPE,
              "evc_frames_gather_packed: needs F %% 4 == 0, every_n >= 1, R <= B * ceil(T / every_n), R <= Rp < R + 32 "
              "(B=%d T=%d F=%d every_n=%d R=%d Rp=%d)", B, T, F, every_n, R, Rp);
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_frames_gather_packed: exactly one of x / x_u8");
  EVC_REQUIRE(num_frames && row_off && out, EVC_ERR_BAD_ARG, "evc_frames_gather_packed: NULL operand");
  EVC_REQUIRE(nx_aligned16(x) && ((uintptr_t)x_u8 % 4) == 0 && nx_aligned16(out) && ((uintptr_t)out_bf16 % 8) == 0, EVC_ERR_BAD_ALIGN,
              "evc_frames_gather_packed: misaligned operand (float4 / uchar4 / 8-byte bf16 access)");
  if (Rp == 0) return EVC_OK;
  hipLaunchKernelGGL(frames_gather_packed_kernel<false>, dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, num_frames,
                     row_off, nullptr, B, T, F, every_n, R, Rp, normalize, out, (uint2*)out_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// ---- the input pass of a tower that knows its input batch-norm statistics before it sees the batch (a forward-only grid tower on its
// moving statistics): the packed rows as frames_gather_packed_kernel<false> makes them - the same loads, sums and
// products in the same order - and, from the registers that hold a row's quarter, its batch-normalised bf16 copy with
// bn_apply_kernel's expression (evc_elementwise.hip), so that neither output differs from the two launches in a bit.  The product
// v * inv is formed with contraction switched off (mul_rounded): the value that the batch norm reads is the f32 that is stored, never a
// fused v * inv - mean, whose missing rounding moves one bf16 in ~45 000 (an intrinsic such as __fmul_rn does not stop the fusion).
// One wave per row, 16-byte loads and stores (8 bytes for the bf16 quarter), the four per-column vectors as float4; no LDS, no atomics.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__global__ __launch_bounds__(256) void frames_gather_packed_bn_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                                      const int* __restrict__ nfr, const int* __restrict__ row_off, int B,
                                                                      int T, int F, int every_n, int R, int Rp, int normalize,
                                                                      const float4* __restrict__ mean, const float4* __restrict__ var,
                                                                      const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                                                      float* __restrict__ out, uint2* __restrict__ out_bn) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Rp) return;
  const int F4 = F >> 2;
  float4* dst = (float4*)(out + row * F);
  uint2* dst_bn = out_bn + row * F4;
  if (row >= R) {
    for (int j = lane; j < F4; j += 64) {
      dst[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      dst_bn[j] = make_uint2(0u, 0u);
    }
    return;
  }
  int b = 0, hi = B;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (row_off[mid] <= (int)row) b = mid; else hi = mid;
  }
  const long fr = (long)((int)row - row_off[b]) * every_n;
  const int n = nfr[b];
  const int idx = fr < 0 ? 0 : (fr >= T ? T - 1 : (int)fr);
  const bool padded = xq && idx >= n;            // uint8 input: frames >= num_frames are padding (zero after Dequantize)
  auto load = [&](int j) {
    if (padded) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (xq) {
      const uchar4 q = ((const uchar4*)(xq + ((long)b * T + idx) * F))[j];
      const float sc = 4.0f / 255.0f, bi = 4.0f / 512.0f - 2.0f;
      return make_float4(q.x * sc + bi, q.y * sc + bi, q.z * sc + bi, q.w * sc + bi);
    }
    return ((const float4*)(x + ((long)b * T + idx) * F))[j];
  };
  float inv = 1.f;
  if (normalize) {
    float ss = 0.f;
    for (int j = lane; j < F4; j += 64) { const float4 v = load(j); ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
    inv = rsqrtf(fmaxf(wave_sum(ss), 1e-12f));
  }
  auto bn = [](float r, float mu, float va, float ga, float be) { return (r - mu) * rsqrtf(va + 1e-3f) * ga + be; };
  for (int j = lane; j < F4; j += 64) {
    float4 v = load(j);
    v.x = mul_rounded(v.x, inv); v.y = mul_rounded(v.y, inv); v.z = mul_rounded(v.z, inv); v.w = mul_rounded(v.w, inv);
    dst[j] = v;
    const float4 mu = mean[j], va = var[j], ga = gamma[j], be = beta[j];
    dst_bn[j] = make_uint2(pack_bf16x2_hw(bn(v.x, mu.x, va.x, ga.x, be.x), bn(v.y, mu.y, va.y, ga.y, be.y)),
                           pack_bf16x2_hw(bn(v.z, mu.z, va.z, ga.z, be.z), bn(v.w, mu.w, va.w, ga.w, be.w)));
  }
}
extern "C" int evc_frames_gather_packed_bn(const float* x, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* row_off, int B,
                                           int T, int F, int every_n, int R, int Rp, int normalize, const float* mean, const float* var,
                                           const float* gamma, const float* beta, float* out, evc_bf16* out_bn_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && every_n >= 1 && R >= 0 && Rp >= R && Rp - R < 32 &&
              (long)R <= (long)B * ((T + every_n - 1) / every_n), EVC_ERR_BAD_SHAPE,
              "evc_frames_gather_packed_bn: needs F %% 4 == 0, every_n >= 1, R <= B * ceil(T / every_n), R <= Rp < R + 32 "
              "(B=%d T=%d F=%d every_n=%d R=%d Rp=%d)", B, T, F, every_n, R, Rp);
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_frames_gather_packed_bn: exactly one of x / x_u8");
  EVC_REQUIRE(num_frames && row_off && mean && var && gamma && beta && out && out_bn_bf16, EVC_ERR_BAD_ARG,
              "evc_frames_gather_packed_bn: NULL operand");
  EVC_REQUIRE(nx_aligned16(x) && ((uintptr_t)x_u8 % 4) == 0 && nx_aligned16(out) && ((uintptr_t)out_bn_bf16 % 8) == 0 && nx_aligned16(mean) &&
              nx_aligned16(var) && nx_aligned16(gamma) && nx_aligned16(beta), EVC_ERR_BAD_ALIGN,
              "evc_frames_gather_packed_bn: misaligned operand (float4 / uchar4 / 8-byte bf16 access)");
  if (Rp == 0) return EVC_OK;
  hipLaunchKernelGGL(frames_gather_packed_bn_kernel, dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, num_frames,
                     row_off, B, T, F, every_n, R, Rp, normalize, (const float4*)mean, (const float4*)var, (const float4*)gamma,
                     (const float4*)beta, out, (uint2*)out_bn_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_frames_gather_packed_sel(const float* x, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* row_off,
                                            const int32_t* sel, int B, int Bsel, int T, int F, int every_n, int R, int Rp, int normalize,
                                            float* out, evc_bf16* out_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && Bsel > 0 && Bsel <= B && T > 0 && F > 0 && F % 4 == 0 && every_n >= 1 && R >= 0 && Rp >= R && Rp - R < 32 &&
              (long)R <= (long)Bsel * ((T + every_n - 1) / every_n), EVC_ERR_BAD_SHAPE,
              "evc_frames_gather_packed_sel: needs 1 <= Bsel <= B, F %% 4 == 0, every_n >= 1, R <= Bsel * ceil(T / every_n), R <= Rp < R + 32 "
              "(B=%d Bsel=%d T=%d F=%d every_n=%d R=%d Rp=%d)", B, Bsel, T, F, every_n, R, Rp);
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_frames_gather_packed_sel: exactly one of x / x_u8");
  EVC_REQUIRE(num_frames && row_off && sel && (out || out_bf16), EVC_ERR_BAD_ARG,
              "evc_frames_gather_packed_sel: NULL operand (num_frames, row_off, sel, and at least one of out / out_bf16)");
  EVC_REQUIRE(nx_aligned16(x) && ((uintptr_t)x_u8 % 4) == 0 && nx_aligned16(out) && ((uintptr_t)out_bf16 % 8) == 0, EVC_ERR_BAD_ALIGN,
              "evc_frames_gather_packed_sel: misaligned operand (float4 / uchar4 / 8-byte bf16 access)");
  if (Rp == 0) return EVC_OK;
  hipLaunchKernelGGL(frames_gather_packed_kernel<true>, dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, num_frames,
                     row_off, sel, Bsel, T, F, every_n, R, Rp, normalize, out, (uint2*)out_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// ---- the packed rows of frames that a table names (evc_frames_gather_packed_tab): row row_off[b] + j is frame
// src[b][j] of video b, src [B][S] the source-frame table of evc_student_frame_select / _scored.  A kernel of its own next to
// frames_gather_packed_kernel, whose instantiations stay what they were; the loads, sums and products are that kernel's in the same
// order, so that a table holding j * every_n gives the grid gather's bits.  An entry outside 0 .. T - 1 (the tables' -1), a slot
// j >= S (never read) and, for uint8 input, a frame >= num_frames[b] are exact zero rows and never an address.  Either output is
// optional.  One wave per row, 16-byte loads and stores (8 bytes for the bf16 quarter); no LDS, no atomics.
__global__ __launch_bounds__(256) void frames_gather_packed_tab_kernel(const float* __restrict__ x, const uint8_t* __restrict__ xq,
                                                                       const int* __restrict__ nfr, const int* __restrict__ row_off,
                                                                       const int* __restrict__ src, int B, int T, int F, int S, int R,
                                                                       int Rp, int normalize, float* __restrict__ out,
                                                                       uint2* __restrict__ out_bf) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Rp) return;
  const int F4 = F >> 2;
  float4* dst = out ? (float4*)(out + row * F) : nullptr;
  uint2* dst_bf = out_bf ? out_bf + row * F4 : nullptr;
  if (row >= R) {
    for (int j = lane; j < F4; j += 64) {
      if (dst) dst[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (dst_bf) dst_bf[j] = make_uint2(0u, 0u);
    }
    return;
  }
  int b = 0, hi = B;
  while (hi - b > 1) {
    const int mid = (b + hi) >> 1;
    if (row_off[mid] <= (int)row) b = mid; else hi = mid;
  }
  const int slot = (int)row - row_off[b];
  const int s = (slot >= 0 && slot < S) ? src[(long)b * S + slot] : -1;
  const bool none = s < 0 || s >= T;
  const int idx = none ? 0 : s;
  const int n = nfr[b];
  const bool padded = none || (xq && idx >= n);  // no frame, or uint8 padding (zero after Dequantize)
  auto load = [&](int j) {
    if (padded) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (xq) {
      const uchar4 q = ((const uchar4*)(xq + ((long)b * T + idx) * F))[j];
      const float sc = 4.0f / 255.0f, bi = 4.0f / 512.0f - 2.0f;
      return make_float4(q.x * sc + bi, q.y * sc + bi, q.z * sc + bi, q.w * sc + bi);
    }
    return ((const float4*)(x + ((long)b * T + idx) * F))[j];
  };
  float inv = 1.f;
  if (normalize) {
    float ss = 0.f;
    for (int j = lane; j < F4; j += 64) { const float4 v = load(j); ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
    inv = rsqrtf(fmaxf(wave_sum(ss), 1e-12f));
  }
  for (int j = lane; j < F4; j += 64) {
    float4 v = load(j); v.x *= inv; v.y *= inv; v.z *= inv; v.w *= inv;
    if (dst) dst[j] = v;
    if (dst_bf) dst_bf[j] = make_uint2(pack_bf16x2_hw(v.x, v.y), pack_bf16x2_hw(v.z, v.w));
  }
}
extern "C" int evc_frames_gather_packed_tab(const float* x, const uint8_t* x_u8, const int32_t* num_frames, const int32_t* row_off,
                                            const int32_t* src, int B, int T, int F, int S, int R, int Rp, int normalize, float* out,
                                            evc_bf16* out_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && T > 0 && F > 0 && F % 4 == 0 && S >= 1 && R >= 0 && Rp >= R && Rp - R < 32 && (long)R <= (long)B * S,
              EVC_ERR_BAD_SHAPE, "evc_frames_gather_packed_tab: needs F %% 4 == 0, S >= 1, R <= B * S, R <= Rp < R + 32 "
              "(B=%d T=%d F=%d S=%d R=%d Rp=%d)", B, T, F, S, R, Rp);
  EVC_REQUIRE((x != nullptr) != (x_u8 != nullptr), EVC_ERR_BAD_ARG, "evc_frames_gather_packed_tab: exactly one of x / x_u8");
  EVC_REQUIRE(num_frames && row_off && src && (out || out_bf16), EVC_ERR_BAD_ARG,
              "evc_frames_gather_packed_tab: NULL operand (num_frames, row_off, src, and at least one of out / out_bf16)");
  EVC_REQUIRE(nx_aligned16(x) && ((uintptr_t)x_u8 % 4) == 0 && nx_aligned16(out) && ((uintptr_t)out_bf16 % 8) == 0 &&
              ((uintptr_t)src % 4) == 0 && ((uintptr_t)num_frames % 4) == 0 && ((uintptr_t)row_off % 4) == 0, EVC_ERR_BAD_ALIGN,
              "evc_frames_gather_packed_tab: misaligned operand (float4 / uchar4 / 8-byte bf16 / int32 access)");
  if (Rp == 0) return EVC_OK;
  hipLaunchKernelGGL(frames_gather_packed_tab_kernel, dim3((unsigned)((Rp + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_u8, num_frames,
                     row_off, src, B, T, F, S, R, Rp, normalize, out, (uint2*)out_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- dst[sel[j]][:] = src[j][:] for the n rows of src (f32, C columns): one wave per row, float4 where both rows are 16-byte aligned
// (C % 4 == 0 and aligned bases), scalar columns otherwise and for the tail.  Rows of dst that sel does not name are not touched.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float* __restrict__ src, long ld_src, const int* __restrict__ sel, int n,
                                                           int C, int vec, float* __restrict__ dst, long ld_dst) {
  const int lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const float* s = src + j * ld_src;
  float* d = dst + (long)sel[j] * ld_dst;
  const int C4 = vec ? (C >> 2) : 0;
  for (int c = lane; c < C4; c += 64) ((float4*)d)[c] = ((const float4*)s)[c];
  for (int c = (C4 << 2) + lane; c < C; c += 64) d[c] = s[c];
}
extern "C" int evc_scatter_rows(const float* src, int64_t ld_src, const int32_t* sel, int n, int rows_dst, int C, float* dst, int64_t ld_dst,
                                void* stream) {
  EVC_REQUIRE(n >= 0 && n <= rows_dst && C > 0 && ld_src >= C && ld_dst >= C, EVC_ERR_BAD_SHAPE,
              "evc_scatter_rows: needs 0 <= n <= rows_dst, C > 0, row strides >= C (n=%d rows_dst=%d C=%d ld_src=%ld ld_dst=%ld)", n, rows_dst, C,
              (long)ld_src, (long)ld_dst);
  EVC_REQUIRE(src && sel && dst, EVC_ERR_BAD_ARG, "evc_scatter_rows: NULL operand");
  EVC_REQUIRE(((uintptr_t)src % 4) == 0 && ((uintptr_t)dst % 4) == 0, EVC_ERR_BAD_ALIGN, "evc_scatter_rows: misaligned operand (f32 access)");
  if (n == 0) return EVC_OK;
  const int vec = nx_aligned16(src) && nx_aligned16(dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, sel, n, C, vec, dst,
                     (long)ld_dst);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- per-(video, cluster) l2 normalisation over D: one wave each.  n = max(|V|, 1e-12) is kept for the backward pass.
__global__ __launch_bounds__(256) void nextvlad_normalize_fwd_kernel(const float* __restrict__ V, long BK, int D, float* __restrict__ U,
                                                                     float* __restrict__ nrm) {
  const int lane = threadIdx.x & 63;
  const long bk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bk >= BK) return;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) { const float v = V[bk * D + d]; s += v * v; }
  const float n = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
  const float inv = 1.0f / n;
  for (int d = lane; d < D; d += 64) U[bk * D + d] = V[bk * D + d] * inv;
  if (lane == 0) nrm[bk] = n;
}
extern "C" int evc_nextvlad_normalize_fwd(const float* V, int B, int K, int D, float* U, float* norms, void* stream) {
  EVC_REQUIRE(B > 0 && K > 0 && D > 0 && (long)B * K < (1L << 31), EVC_ERR_BAD_SHAPE, "evc_nextvlad_normalize_fwd: bad shape (B=%d K=%d D=%d)", B, K, D);
  EVC_REQUIRE(V && U && norms, EVC_ERR_BAD_ARG, "evc_nextvlad_normalize_fwd: NULL operand");
  hipLaunchKernelGGL(nextvlad_normalize_fwd_kernel, dim3((unsigned)(((long)B * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, V, (long)B * K, D, U, norms);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// dV = (dU - u (u . dU)) / n with u = V / n; where the clamp was active (|V| <= 1e-12, U = V / 1e-12) dV = dU / n
__global__ __launch_bounds__(256) void nextvlad_normalize_bwd_kernel(const float* __restrict__ V, const float* __restrict__ nrm,
                                                                     const float* __restrict__ dU, long BK, int D, float* __restrict__ dV) {
  const int lane = threadIdx.x & 63;
  const long bk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bk >= BK) return;
  const float n = nrm[bk];
  const float inv = 1.0f / n;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s += V[bk * D + d] * inv * dU[bk * D + d];
  s = (n > 1e-12f) ? wave_sum(s) : 0.f;
  for (int d = lane; d < D; d += 64) dV[bk * D + d] = (dU[bk * D + d] - V[bk * D + d] * inv * s) * inv;
}
extern "C" int evc_nextvlad_normalize_bwd(const float* V, const float* norms, const float* dU, int B, int K, int D, float* dV, void* stream) {
  EVC_REQUIRE(B > 0 && K > 0 && D > 0 && (long)B * K < (1L << 31), EVC_ERR_BAD_SHAPE, "evc_nextvlad_normalize_bwd: bad shape (B=%d K=%d D=%d)", B, K, D);
  EVC_REQUIRE(V && norms && dU && dV, EVC_ERR_BAD_ARG, "evc_nextvlad_normalize_bwd: NULL operand");
  hipLaunchKernelGGL(nextvlad_normalize_bwd_kernel, dim3((unsigned)(((long)B * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, V, norms, dU, (long)B * K, D, dV);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- context gating: out = h * sigmoid(gl);  dh = dout * gate (the direct path), dgl = dout * h * gate * (1 - gate)
__global__ void nextvlad_gate_fwd_kernel(const float* __restrict__ h, const float* __restrict__ gl, long n, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = h[i] * sigmoidf_(gl[i]);
}
extern "C" int evc_nextvlad_gate_fwd(const float* h, const float* gl, int64_t n, float* out, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_gate_fwd: bad shape (n=%ld)", (long)n);
  EVC_REQUIRE(h && gl && out, EVC_ERR_BAD_ARG, "evc_nextvlad_gate_fwd: NULL operand");
  hipLaunchKernelGGL(nextvlad_gate_fwd_kernel, dim3(nx_grid(n)), dim3(256), 0, (hipStream_t)stream, h, gl, (long)n, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
__global__ void nextvlad_gate_bwd_kernel(const float* __restrict__ h, const float* __restrict__ gl, const float* __restrict__ dout, long n,
                                         float* __restrict__ dh, float* __restrict__ dgl, bf16_t* __restrict__ dgl_bf) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float g = sigmoidf_(gl[i]), d = dout[i];
    dh[i] = d * g;
    const float dl = d * h[i] * g * (1.0f - g);
    if (dgl) dgl[i] = dl;
    if (dgl_bf) dgl_bf[i] = f32_to_bf16(dl);
  }
}
extern "C" int evc_nextvlad_gate_bwd(const float* h, const float* gl, const float* dout, int64_t n, float* dh, float* dgl, evc_bf16* dgl_bf16,
                                     void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_gate_bwd: bad shape (n=%ld)", (long)n);
  EVC_REQUIRE(h && gl && dout && dh && (dgl || dgl_bf16), EVC_ERR_BAD_ARG, "evc_nextvlad_gate_bwd: NULL operand (dgl and dgl_bf16 may not both be NULL)");
  hipLaunchKernelGGL(nextvlad_gate_bwd_kernel, dim3(nx_grid(n)), dim3(256), 0, (hipStream_t)stream, h, gl, dout, (long)n, dh, dgl, (bf16_t*)dgl_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// the same with a second incoming gradient (serial distillation: dL_REP/d out joins the MoE head's dout): d = dout + dout2, one f32
// add in that order, then the formulas above unchanged.  dout2 == NULL: the bits of evc_nextvlad_gate_bwd.
__global__ void nextvlad_gate_bwd_add_kernel(const float* __restrict__ h, const float* __restrict__ gl, const float* __restrict__ dout,
                                             const float* __restrict__ dout2, long n, float* __restrict__ dh, float* __restrict__ dgl,
                                             bf16_t* __restrict__ dgl_bf) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float g = sigmoidf_(gl[i]);
    float d = dout[i];
    if (dout2) d = __fadd_rn(d, dout2[i]);
    dh[i] = d * g;
    const float dl = d * h[i] * g * (1.0f - g);
    if (dgl) dgl[i] = dl;
    if (dgl_bf) dgl_bf[i] = f32_to_bf16(dl);
  }
}
extern "C" int evc_nextvlad_gate_bwd_add(const float* h, const float* gl, const float* dout, const float* dout2, int64_t n, float* dh,
                                         float* dgl, evc_bf16* dgl_bf16, void* stream) {
  EVC_REQUIRE(n > 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_gate_bwd_add: bad shape (n=%ld)", (long)n);
  EVC_REQUIRE(h && gl && dout && dh && (dgl || dgl_bf16), EVC_ERR_BAD_ARG,
              "evc_nextvlad_gate_bwd_add: NULL operand (dout2 may be NULL; dgl and dgl_bf16 may not both be)");
  hipLaunchKernelGGL(nextvlad_gate_bwd_add_kernel, dim3(nx_grid(n)), dim3(256), 0, (hipStream_t)stream, h, gl, dout, dout2, (long)n, dh, dgl,
                     (bf16_t*)dgl_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- the bf16 operand of the cluster / attention products, centred: xc = bf16(xe - be).  xe = r.We + be carries the expansion
// bias into every row; rounded to bf16 as it stands, that constant costs 2^-9 of ITS magnitude in every element, although all it
// adds to a logit is the per-column constant be.W, which evc_nextvlad_bias_logits computes in f32 and the product takes as its bias.
__global__ void nextvlad_center_cast_kernel(const float* __restrict__ xe, const float* __restrict__ be, long n4, int E4,
                                            uint32_t* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 x = ((const float4*)xe)[i];
    const float4 b = ((const float4*)be)[i % E4];
    out[2 * i] = pack_bf16x2_hw(x.x - b.x, x.y - b.y);
    out[2 * i + 1] = pack_bf16x2_hw(x.z - b.z, x.w - b.w);
  }
}
extern "C" int evc_nextvlad_center_cast(const float* xe, int R, int E, const float* be, evc_bf16* out, void* stream) {
  EVC_REQUIRE(R > 0 && E > 0 && E % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_center_cast: needs E %% 4 == 0 (R=%d E=%d)", R, E);
  EVC_REQUIRE(xe && be && out && ((uintptr_t)xe % 16) == 0 && ((uintptr_t)be % 16) == 0 && ((uintptr_t)out % 8) == 0, EVC_ERR_BAD_ARG,
              "evc_nextvlad_center_cast: NULL or misaligned operand");
  const long n4 = (long)R * (E / 4);
  hipLaunchKernelGGL(nextvlad_center_cast_kernel, dim3(nx_grid(n4)), dim3(256), 0, (hipStream_t)stream, xe, be, n4, E / 4, (uint32_t*)out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// out[n] = sum_e be[e] * W[n][e] (+ add[n]) for n < N, 0 for N <= n < n_out: one wave per output, lanes over e in a fixed order
__global__ __launch_bounds__(256) void nextvlad_bias_logits_kernel(const float* __restrict__ be, const float* __restrict__ W, int N, int E,
                                                                   const float* __restrict__ add, float* __restrict__ out, int n_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= n_out) return;
  float s = 0.f;
  if (n < N) {
    for (int e = lane; e < E; e += 64) s += be[e] * W[(long)n * E + e];
    s = wave_sum(s) + (add ? add[n] : 0.f);
  }
  if (lane == 0) out[n] = s;
}
extern "C" int evc_nextvlad_bias_logits(const float* be, const float* W, int N, int E, const float* add, float* out, int n_out, void* stream) {
  EVC_REQUIRE(N > 0 && E > 0 && n_out >= N, EVC_ERR_BAD_SHAPE, "evc_nextvlad_bias_logits: bad shape (N=%d E=%d n_out=%d)", N, E, n_out);
  EVC_REQUIRE(be && W && out, EVC_ERR_BAD_ARG, "evc_nextvlad_bias_logits: NULL operand");
  hipLaunchKernelGGL(nextvlad_bias_logits_kernel, dim3((n_out + 3) / 4), dim3(256), 0, (hipStream_t)stream, be, W, N, E, add, out, n_out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
// dW[g][e] = dWc[g][e] + du[g] * be[e]: a weight gradient contracted against the CENTRED operand (dWc = dlogit^T . (xe - be)) plus
// the rank-one term the centring took out (du = column sums of dlogit)
__global__ void nextvlad_wgrad_uncenter_kernel(const float* __restrict__ dWc, const float* __restrict__ du, const float* __restrict__ be,
                                               long n, int E, float* __restrict__ dW) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dW[i] = dWc[i] + du[i / E] * be[i % E];
}
extern "C" int evc_nextvlad_wgrad_uncenter(const float* dWc, const float* du, const float* be, int N, int E, float* dW, void* stream) {
  EVC_REQUIRE(N > 0 && E > 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_wgrad_uncenter: bad shape (N=%d E=%d)", N, E);
  EVC_REQUIRE(dWc && du && be && dW, EVC_ERR_BAD_ARG, "evc_nextvlad_wgrad_uncenter: NULL operand");
  hipLaunchKernelGGL(nextvlad_wgrad_uncenter_kernel, dim3(nx_grid((long)N * E)), dim3(256), 0, (hipStream_t)stream, dWc, du, be, (long)N * E, E, dW);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- out[c] = sum_r x[r][c], rows in a fixed order: a workgroup of 16 waves owns 64 columns, wave w adds rows w, w+16, ... and
// the 16 partial rows are added in wave order (the bias gradients dbe = colsum(dxe), dba = colsum(datt_logit)).
__global__ __launch_bounds__(1024) void nextvlad_colsum_kernel(const float* __restrict__ x, long ld, int R, int C, float* __restrict__ out) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < C)
    for (int r = wave; r < R; r += 16) s += x[(long)r * ld + c];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C) {
    float tsum = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tsum += part[w][lane];
    out[c] = tsum;
  }
}
// Tall inputs: NX_CS_PARTS row ranges per 64 columns, so that the chip is filled, then the partial rows added in range order.
static constexpr int NX_CS_PARTS = 32;
__global__ __launch_bounds__(256) void nextvlad_colsum_part_kernel(const float* __restrict__ x, long ld, int R, int C, int rows_per_part,
                                                                   float* __restrict__ ws) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows_per_part, r1 = min(R, r0 + rows_per_part);
  float s = 0.f;
  if (c < C)
    for (int r = r0 + wave; r < r1; r += 4) s += x[(long)r * ld + c];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C) ws[(long)blockIdx.y * C + c] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}
__global__ void nextvlad_colsum_finish_kernel(const float* __restrict__ ws, int C, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < NX_CS_PARTS; ++p) s += ws[(long)p * C + c];
  out[c] = s;
}
// ws (may be NULL): NX_CS_PARTS * C floats of scratch; with it, inputs of 512 rows or more take the two-pass path
extern "C" int evc_nextvlad_colsum(const float* x, int64_t ld, int R, int C, float* out, float* ws, int64_t ws_floats, void* stream) {
  EVC_REQUIRE(R > 0 && C > 0 && ld >= C, EVC_ERR_BAD_SHAPE, "evc_nextvlad_colsum: bad shape (R=%d C=%d ld=%ld)", R, C, (long)ld);
  EVC_REQUIRE(x && out, EVC_ERR_BAD_ARG, "evc_nextvlad_colsum: NULL operand");
  if (ws && R >= 512) {
    EVC_REQUIRE(ws_floats >= (int64_t)NX_CS_PARTS * C, EVC_ERR_BAD_ARG, "evc_nextvlad_colsum: ws holds %ld floats, %ld needed", (long)ws_floats,
                (long)NX_CS_PARTS * C);
    hipLaunchKernelGGL(nextvlad_colsum_part_kernel, dim3(ceil_div(C, 64), NX_CS_PARTS), dim3(256), 0, (hipStream_t)stream, x, (long)ld, R, C,
                       ceil_div(R, NX_CS_PARTS), ws);
    EVC_LAUNCH_CHECK();
    hipLaunchKernelGGL(nextvlad_colsum_finish_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, ws, C, out);
    EVC_LAUNCH_CHECK();
    return EVC_OK;
  }
  hipLaunchKernelGGL(nextvlad_colsum_kernel, dim3(ceil_div(C, 64)), dim3(1024), 0, (hipStream_t)stream, x, (long)ld, R, C, out);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ---- dropout before the hidden layer: Yd = Y * m / keep, m in {0, 1} a function of (seed, rank, step, element)
// alone - a counter-based generator evaluated where the value is consumed, so the mask is never stored: the backward pass
// regenerates it.  Element e = b*C + j of the [B][C] buffer (C = K*D, j = k*D + d: the INTERNAL cluster-major order) is lane
// l = e & 3 of quad q = e >> 2; w = Philox4x32-10(counter (q_lo, q_hi, step_lo, step_hi), key (seed, rank))[l]; m = (w < T) as
// unsigned 32-bit values, T = floor(keep * 2^32) from the host.  C % 4 == 0: a quad never straddles a row.
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): ten rounds of two 32 x 32 -> 64 bit multiplies, the key bumped by the Weyl
// constants between rounds.
__device__ __forceinline__ uint4 nx_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;                          // (the bump after the tenth round is dead code)
  }
  return make_uint4(c0, c1, c2, c3);
}
__device__ __forceinline__ uint4 nx_dropout_words(long q, uint32_t seed, uint32_t rank, uint64_t step) {
  return nx_philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)step, (uint32_t)(step >> 32), seed, rank);
}

// both launches are streaming passes: at most 2048 workgroups (8 per CU) and a grid-stride loop over the rest
static inline int nx_drop_grid(long nq) { long nb = (nq + 255) / 256; return (int)(nb < 2048 ? nb : 2048); }

// Y_bf16[e] = bf16(vlad_bn(U)[e] * scale) where kept, +0 where dropped: the batch-norm apply (the expression of bn_apply_kernel,
// no relu6), the mask and the bf16 store (f32_to_bf16's conversion, two values at a time) in one pass.  One thread per quad and
// iteration: one Philox call, 16-byte loads of U and of the four per-column vectors, one 8-byte store.
__global__ __launch_bounds__(256) void nextvlad_dropout_fwd_kernel(const float4* __restrict__ U, long nq, uint32_t C4,
                                                                   const float4* __restrict__ mean, const float4* __restrict__ var,
                                                                   const float4* __restrict__ gamma, const float4* __restrict__ beta,
                                                                   uint32_t T, float scale, uint32_t seed, uint32_t rank, uint64_t step,
                                                                   uint2* __restrict__ Y) {
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
    const uint32_t c4 = nq <= 0xffffffffL ? (uint32_t)q % C4 : (uint32_t)(q % C4);
    const uint4 w = nx_dropout_words(q, seed, rank, step);
    const float4 x = U[q], mu = mean[c4], va = var[c4], ga = gamma[c4], be = beta[c4];
    const float y0 = ((x.x - mu.x) * rsqrtf(va.x + 1e-3f) * ga.x + be.x) * scale;
    const float y1 = ((x.y - mu.y) * rsqrtf(va.y + 1e-3f) * ga.y + be.y) * scale;
    const float y2 = ((x.z - mu.z) * rsqrtf(va.z + 1e-3f) * ga.z + be.z) * scale;
    const float y3 = ((x.w - mu.w) * rsqrtf(va.w + 1e-3f) * ga.w + be.w) * scale;
    Y[q] = make_uint2(pack_bf16x2_hw(w.x < T ? y0 : 0.f, w.y < T ? y1 : 0.f), pack_bf16x2_hw(w.z < T ? y2 : 0.f, w.w < T ? y3 : 0.f));
  }
}
// dY[e] = m[e] ? dY[e] * scale : 0, in place: the same quads, the same words
__global__ __launch_bounds__(256) void nextvlad_dropout_bwd_kernel(float4* __restrict__ dY, long nq, uint32_t T, float scale, uint32_t seed,
                                                                   uint32_t rank, uint64_t step) {
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
    const uint4 w = nx_dropout_words(q, seed, rank, step);
    const float4 d = dY[q];
    dY[q] = make_float4(w.x < T ? d.x * scale : 0.f, w.y < T ? d.y * scale : 0.f, w.z < T ? d.z * scale : 0.f, w.w < T ? d.w * scale : 0.f);
  }
}

extern "C" int evc_nextvlad_dropout_fwd(const float* U, int B, int C, const float* mean, const float* var, const float* gamma,
                                        const float* beta, uint32_t T, float scale, uint32_t seed, uint32_t rank, uint64_t step,
                                        evc_bf16* Y_bf16, void* stream) {
  EVC_REQUIRE(B > 0 && C > 0 && C % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_dropout_fwd: needs B > 0, C %% 4 == 0 (B=%d C=%d)", B, C);
  EVC_REQUIRE(T != 0, EVC_ERR_BAD_ARG, "evc_nextvlad_dropout_fwd: threshold 0 keeps nothing (the rate must be below 1)");
  EVC_REQUIRE(U && mean && var && gamma && beta && Y_bf16, EVC_ERR_BAD_ARG, "evc_nextvlad_dropout_fwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(U) && nx_aligned16(mean) && nx_aligned16(var) && nx_aligned16(gamma) && nx_aligned16(beta) &&
              ((uintptr_t)Y_bf16 % 8) == 0, EVC_ERR_BAD_ALIGN,
              "evc_nextvlad_dropout_fwd: U and the four column vectors must be 16-byte aligned, Y_bf16 8-byte aligned");
  const long nq = (long)B * (C / 4);
  hipLaunchKernelGGL(nextvlad_dropout_fwd_kernel, dim3(nx_drop_grid(nq)), dim3(256), 0, (hipStream_t)stream, (const float4*)U, nq, (uint32_t)(C / 4),
                     (const float4*)mean, (const float4*)var, (const float4*)gamma, (const float4*)beta, T, scale, seed, rank, step,
                     (uint2*)Y_bf16);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
extern "C" int evc_nextvlad_dropout_bwd(float* dY, int B, int C, uint32_t T, float scale, uint32_t seed, uint32_t rank, uint64_t step,
                                        void* stream) {
  EVC_REQUIRE(B > 0 && C > 0 && C % 4 == 0, EVC_ERR_BAD_SHAPE, "evc_nextvlad_dropout_bwd: needs B > 0, C %% 4 == 0 (B=%d C=%d)", B, C);
  EVC_REQUIRE(T != 0, EVC_ERR_BAD_ARG, "evc_nextvlad_dropout_bwd: threshold 0 keeps nothing (the rate must be below 1)");
  EVC_REQUIRE(dY, EVC_ERR_BAD_ARG, "evc_nextvlad_dropout_bwd: NULL operand");
  EVC_REQUIRE(nx_aligned16(dY), EVC_ERR_BAD_ALIGN, "evc_nextvlad_dropout_bwd: dY must be 16-byte aligned (float4 access)");
  const long nq = (long)B * (C / 4);
  hipLaunchKernelGGL(nextvlad_dropout_bwd_kernel, dim3(nx_drop_grid(nq)), dim3(256), 0, (hipStream_t)stream, (float4*)dY, nq, T, scale, seed, rank, step);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

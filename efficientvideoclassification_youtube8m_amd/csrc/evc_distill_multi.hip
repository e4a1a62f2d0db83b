// The loss section of the serial distillation step for K students against ONE frozen teacher (SerialStudentsGraph): what
// evc_distill_losses computes for one student, for 1 <= K <= 8 of them in one launch + one finish launch.  The labels, state_t and every
// state_s are read once, every dpred_s / dstate_s is written once; pred_t and every pred_s row are read TWICE by the workgroup that owns the
// row: a first pass takes the row sums in double (see dm_teacher_elem), the second, from cache, does the work - and computes the teacher's
// share of every element once for all K students.
// block_sum and the per-element arithmetic of distill_elem (evc_elementwise.hip) are restated here, so that the kernels of that file stay
// byte for byte what they were.
//
// A student's bits do not depend on its company: every student passes through the SAME loop body - the loops over the students below are
// never unrolled, their accumulators live in LDS slots indexed by the loop variable, so there is one copy of the instructions, whatever K
// is and wherever in the list the student stands - and the path a student takes (16-byte or scalar accesses) is decided by the teacher's
// pointers and its own alone.  Contraction of a * b + c is switched off for the whole file on top of that: no value here depends on which
// multiply-adds the compiler chose to fuse.
#include "evc_common.h"

#pragma clang fp contract(off)

#define DM_MAX_K 8

__device__ __forceinline__ float dm_block_sum(float v, float* sh) {      // block_sum of evc_elementwise.hip at 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < 4; ++i) t += sh[i];
  return t;
}
__device__ __forceinline__ double dm_block_sum_f64(double v, double* sh) {      // the same fixed order, on doubles
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < 4; ++i) t += sh[i];
  return t;
}

// per-student pointers and scales, by value in the launch's arguments (as SmallAdamTable)
struct DistillMultiTable {
  const float* ps[DM_MAX_K];     // pred_s   [B][V]
  const float* ss[DM_MAX_K];     // rowsum_s [B]
  const float* b[DM_MAX_K];      // state_s  [B][D]
  float* dps[DM_MAX_K];          // may be NULL
  float* db[DM_MAX_K];           // may be NULL
  float g_ce[DM_MAX_K], g_kl[DM_MAX_K], g_rep[DM_MAX_K];
};

// The teacher's share of one element - computed once, whatever K is - and a student's share: distill_elem in two halves.
// The KL gradient -P / p_s + 1 / sum(p_s) is a DIFFERENCE of two addends that cancel where teacher and student agree, and it is added to a
// CE term that carries 1 / B: with few classes and a large batch (V = 8, B = 1030) one f32 rounding of an addend - or of a row sum handed
// in as f32 - is larger than 1e-5 of the result.  So the two row sums are taken in double inside the kernel (first pass over the row; the
// rowsum inputs decide the degenerate-row rules only) and this one difference is evaluated in double; everything else stays f32.
struct DmTeacherElem { float ce_t, P, logP; double Pd; };
__device__ __forceinline__ DmTeacherElem dm_teacher_elem(float pt, bool pos, double itd) {
  const float eps = 10e-6f;   // cs/losses.py:92
  const float FMIN = 1.17549435e-38f;
  DmTeacherElem r;
  const float at = pt + eps, bt = 1.f - pt + eps;
  r.ce_t = -(pos ? __logf(at) : __logf(bt));
  r.Pd = (double)pt * itd;
  r.P = (float)r.Pd;
  r.logP = (r.P >= FMIN) ? __logf(r.P) : 0.f;
  return r;
}
struct DmStudentElem { float kl, ce_s, g; };
__device__ __forceinline__ DmStudentElem dm_student_elem(const DmTeacherElem te, float ps, bool pos, float is, double isd, bool t_ok, float g_ce,
                                                         float g_kl) {
  const float eps = 10e-6f;
  const float FMIN = 1.17549435e-38f;
  DmStudentElem r;
  const float a = ps + eps, bq = 1.f - ps + eps;
  r.ce_s = -(pos ? __logf(a) : __logf(bq));
  const float P = te.P, q = fmaxf(ps, FMIN);
  r.kl = (P >= FMIN) ? P * (te.logP - __logf(fmaxf(q * is, FMIN))) : 0.f;
  const float gce = (g_ce != 0.f) ? (pos ? -1.f / a : 1.f / bq) * g_ce : 0.f;
  const double gkl = (t_ok && g_kl != 0.f) ? (-te.Pd / (double)q + isd) * (double)g_kl : 0.0;
  r.g = (float)((double)gce + gkl);
  return r;
}

// Workgroups [0, B): one prediction row each; workgroups [B, B + NS): the [B, D] state part, grid-stride.  Workspace (floats):
//   [0, B)                                teacher CE, per row
//   [B + 2 k B, B + (2 k + 1) B)          L_PRED of student k, per row
//   [B + (2 k + 1) B, B + (2 k + 2) B)    CE of student k, per row
//   [(1 + 2 K) B + 256 k, ... + NS)       L_REP of student k, per state workgroup
__global__ __launch_bounds__(256) void distill_multi_kernel(const float* __restrict__ pt, const float* __restrict__ st,
                                                            const uint8_t* __restrict__ y, const float* __restrict__ a,
                                                            const DistillMultiTable t, int K, int B, int V, long nd, int NS, float inv_b,
                                                            float* __restrict__ ws) {
  __shared__ float sh[4];
  __shared__ float acc[DM_MAX_K][2][256];       // per-thread accumulators of the K students (a register array indexed by k would spill)
  __shared__ float inv_s[DM_MAX_K];
  __shared__ double inv_sd[DM_MAX_K];
  __shared__ double shd[4];
  const int tid = threadIdx.x;
  const float FMIN = 1.17549435e-38f;
#pragma nounroll
  for (int k = 0; k < K; ++k) { acc[k][0][tid] = 0.f; acc[k][1][tid] = 0.f; }
  if ((int)blockIdx.x < B) {
    const int row = blockIdx.x;
    const long base = (long)row * V;
    // first pass: the row sums in double (the rows are read again below, from cache)
    double sum_t = 0.0;
    for (int c = tid; c < V; c += 256) sum_t += (double)pt[base + c];
    sum_t = dm_block_sum_f64(sum_t, shd);
    const bool t_ok = st[row] >= FMIN && sum_t >= (double)FMIN;
    const double itd = t_ok ? 1.0 / sum_t : 0.0;
#pragma nounroll
    for (int k = 0; k < K; ++k) {
      const float* ps = t.ps[k] + base;
      double sum_s = 0.0;
      for (int c = tid; c < V; c += 256) sum_s += (double)ps[c];
      sum_s = dm_block_sum_f64(sum_s, shd);
      if (tid == 0) {
        // rowsum_s decides the degenerate rule as in distill_losses_kernel (a sum below FLT_MIN is clamped there); the value is the double sum
        const double isd = t.ss[k][row] >= FMIN ? 1.0 / fmax(sum_s, (double)FMIN) : 1.0 / (double)FMIN;
        inv_sd[k] = isd;
        inv_s[k] = (float)isd;
      }
    }
    __syncthreads();
    float s_ct = 0.f;
    const bool tv4 = (V & 3) == 0 && ((uintptr_t)pt & 15) == 0 && ((uintptr_t)y & 3) == 0;
    if (tv4) {
      const float4* pt4 = (const float4*)(pt + base);
      const uchar4* y4 = (const uchar4*)(y + base);
      for (int c4 = tid; c4 < (V >> 2); c4 += 256) {
        const float4 tq = pt4[c4];
        const uchar4 yq = y4[c4];
        const float tv[4] = {tq.x, tq.y, tq.z, tq.w};
        const bool pos[4] = {yq.x != 0, yq.y != 0, yq.z != 0, yq.w != 0};
        DmTeacherElem te[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          te[r] = dm_teacher_elem(tv[r], pos[r], itd);
          s_ct += te[r].ce_t;
        }
#pragma nounroll
        for (int k = 0; k < K; ++k) {
          const float* ps = t.ps[k] + base;
          float* dps = t.dps[k];
          // a student whose rows are not 16-byte aligned takes 4-byte accesses to the same four elements: the others keep theirs
          const bool sv4 = ((uintptr_t)t.ps[k] & 15) == 0 && ((uintptr_t)dps & 15) == 0;
          const float is = inv_s[k], g_ce = t.g_ce[k], g_kl = t.g_kl[k];
          const double isd = inv_sd[k];
          float sv[4];
          if (sv4) {
            const float4 sq = ((const float4*)ps)[c4];
            sv[0] = sq.x; sv[1] = sq.y; sv[2] = sq.z; sv[3] = sq.w;
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) sv[r] = ps[4 * c4 + r];
          }
          float s_kl = acc[k][0][tid], s_cs = acc[k][1][tid], g[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const DmStudentElem e = dm_student_elem(te[r], sv[r], pos[r], is, isd, t_ok, g_ce, g_kl);
            s_kl += e.kl; s_cs += e.ce_s; g[r] = e.g;
          }
          acc[k][0][tid] = s_kl; acc[k][1][tid] = s_cs;
          if (dps) {
            if (sv4) ((float4*)(dps + base))[c4] = make_float4(g[0], g[1], g[2], g[3]);
            else {
#pragma unroll
              for (int r = 0; r < 4; ++r) dps[base + 4 * c4 + r] = g[r];
            }
          }
        }
      }
    } else {
      for (int c = tid; c < V; c += 256) {
        const bool pos = y[base + c] != 0;
        const DmTeacherElem te = dm_teacher_elem(pt[base + c], pos, itd);
        s_ct += te.ce_t;
#pragma nounroll
        for (int k = 0; k < K; ++k) {
          float* dps = t.dps[k];
          const DmStudentElem e = dm_student_elem(te, t.ps[k][base + c], pos, inv_s[k], inv_sd[k], t_ok, t.g_ce[k], t.g_kl[k]);
          acc[k][0][tid] += e.kl; acc[k][1][tid] += e.ce_s;
          if (dps) dps[base + c] = e.g;
        }
      }
    }
    s_ct = dm_block_sum(s_ct, sh);
    if (tid == 0) ws[row] = s_ct * inv_b;
#pragma nounroll
    for (int k = 0; k < K; ++k) {
      const float s_kl = dm_block_sum(acc[k][0][tid], sh);
      const float s_cs = dm_block_sum(acc[k][1][tid], sh);
      if (tid == 0) {
        ws[(long)B + (2L * k) * B + row] = s_kl;
        ws[(long)B + (2L * k + 1) * B + row] = s_cs * inv_b;
      }
    }
    return;
  }
  const int blk = (int)blockIdx.x - B;
  const bool tv4 = (nd & 3) == 0 && ((uintptr_t)a & 15) == 0;
  if (tv4) {
    for (long i4 = (long)blk * 256 + tid; i4 < (nd >> 2); i4 += (long)NS * 256) {
      const float4 aq = ((const float4*)a)[i4];
      const float av[4] = {aq.x, aq.y, aq.z, aq.w};
#pragma nounroll
      for (int k = 0; k < K; ++k) {
        const float* b = t.b[k];
        float* db = t.db[k];
        const bool sv4 = ((uintptr_t)b & 15) == 0 && ((uintptr_t)db & 15) == 0;
        const float g_rep = t.g_rep[k];
        float bv[4];
        if (sv4) {
          const float4 bq = ((const float4*)b)[i4];
          bv[0] = bq.x; bv[1] = bq.y; bv[2] = bq.z; bv[3] = bq.w;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) bv[r] = b[4 * i4 + r];
        }
        float s = acc[k][0][tid], g[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = av[r] - bv[r];
          s += d * d;
          g[r] = (g_rep != 0.f) ? -2.f * d * inv_b * g_rep : 0.f;
        }
        acc[k][0][tid] = s;
        if (db) {
          if (sv4) ((float4*)db)[i4] = make_float4(g[0], g[1], g[2], g[3]);
          else {
#pragma unroll
            for (int r = 0; r < 4; ++r) db[4 * i4 + r] = g[r];
          }
        }
      }
    }
  } else {
    for (long i = (long)blk * 256 + tid; i < nd; i += (long)NS * 256) {
      const float av = a[i];
#pragma nounroll
      for (int k = 0; k < K; ++k) {
        float* db = t.db[k];
        const float g_rep = t.g_rep[k];
        const float d = av - t.b[k][i];
        acc[k][0][tid] += d * d;
        if (db) db[i] = (g_rep != 0.f) ? -2.f * d * inv_b * g_rep : 0.f;
      }
    }
  }
#pragma nounroll
  for (int k = 0; k < K; ++k) {
    const float s = dm_block_sum(acc[k][0][tid], sh);
    if (tid == 0) ws[(1 + 2L * K) * B + 256L * k + blk] = s * inv_b;
  }
}

// Workgroup k finishes student k as distill_losses_finish_kernel does for its one: four waves, wave w owns loss slot w; the partials pass
// through LDS in pieces of 1024 and lane 0 of each wave adds its piece in workgroup order.  Every workgroup adds the teacher's list in the
// same order: slot 0 holds the same bits in every row.
__global__ __launch_bounds__(256) void distill_multi_finish_kernel(const float* __restrict__ ws, int K, int B, int NS, float* __restrict__ losses) {
  __shared__ float sh[4][1024];
  const int k = blockIdx.x;
  // loss slot (DistillGraph.LOSS_SLOTS) -> its list of partials: teacher CE, L_REP, L_PRED, student CE
  const long off[4] = {0, (1 + 2L * K) * B + 256L * k, (long)B + (2L * k) * B, (long)B + (2L * k + 1) * B};
  const int cnt[4] = {B, NS, B, B};
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nmax = B > NS ? B : NS;
  float s = 0.f;
  for (int base = 0; base < nmax; base += 1024) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      for (int i = threadIdx.x; i < 1024; i += 256)
        if (base + i < cnt[j]) sh[j][i] = ws[off[j] + base + i];
    __syncthreads();
    if (lane == 0) {
      const int n = cnt[w] - base < 1024 ? cnt[w] - base : 1024;
      for (int i = 0; i < n; ++i) s += sh[w][i];
    }
  }
  if (lane == 0) losses[4 * k + w] += s;
}

extern "C" int evc_distill_losses_multi(const float* pred_t, const float* rowsum_t, const uint8_t* labels, const float* state_t, int K,
                                        const float* const* pred_s, const float* const* rowsum_s, const float* const* state_s,
                                        const float* g_ce, const float* g_kl, const float* g_rep, float* const* dpred_s,
                                        float* const* dstate_s, int B, int V, int D, float* losses, float* workspace, void* stream) {
  EVC_REQUIRE(K >= 1 && K <= DM_MAX_K, EVC_ERR_BAD_ARG, "evc_distill_losses_multi: K=%d students (1 .. %d)", K, DM_MAX_K);
  EVC_REQUIRE(B > 0 && V > 0 && D > 0, EVC_ERR_BAD_SHAPE, "evc_distill_losses_multi: bad shape");
  EVC_REQUIRE(pred_t && rowsum_t && labels && state_t && losses && pred_s && rowsum_s && state_s && g_ce && g_kl && g_rep, EVC_ERR_BAD_ARG,
              "evc_distill_losses_multi: a required pointer is NULL");
  EVC_REQUIRE(workspace, EVC_ERR_BAD_ARG, "evc_distill_losses_multi: workspace ((1 + 2 K) * B + 256 * K floats of scratch) is required");
  DistillMultiTable t;
  memset(&t, 0, sizeof(t));
  for (int k = 0; k < K; ++k) {
    EVC_REQUIRE(pred_s[k] && rowsum_s[k] && state_s[k], EVC_ERR_BAD_ARG, "evc_distill_losses_multi: student %d: a required pointer is NULL", k);
    t.ps[k] = pred_s[k]; t.ss[k] = rowsum_s[k]; t.b[k] = state_s[k];
    t.dps[k] = dpred_s ? dpred_s[k] : nullptr;
    t.db[k] = dstate_s ? dstate_s[k] : nullptr;
    t.g_ce[k] = g_ce[k]; t.g_kl[k] = g_kl[k]; t.g_rep[k] = g_rep[k];
  }
  const long nd = (long)B * D;
  const long want = (nd + 1023) / 1024;                 // 4 elements per thread and trip, as evc_distill_losses
  const int NS = (int)(want < 1 ? 1 : (want < 256 ? want : 256));
  hipLaunchKernelGGL(distill_multi_kernel, dim3(B + NS), dim3(256), 0, (hipStream_t)stream, pred_t, rowsum_t, labels, state_t, t, K, B, V,
                     nd, NS, 1.0f / B, workspace);
  hipLaunchKernelGGL(distill_multi_finish_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, K, B, NS, losses);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

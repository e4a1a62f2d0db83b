// The loss section of the offline distillation step: ONE student against F sparse teacher lists (the (class, confidence) pairs of F
// prediction files for the rows of this batch), 1 <= F <= 8.  No teacher tower runs: the lists are scattered into one dense combined row
// P per video, exactly as evc_ensemble_topk_rows scatters its prior files over one all-zero member (max | weighted mean), and the student
// is trained against P as evc_distill_losses_ensemble trains one against its combined row, without a state (a prediction file holds none).
// One launch + one finish launch, no float atomics, no last-block counters.
//
// A row belongs to one workgroup at a time (the grid strides over the rows).  P is built in LDS: the row is zeroed, then one file after
// another is scattered into it with a barrier between files - the classes of one list are distinct, so no two threads of a file meet in
// one element, and the order across files is fixed.  The workgroup then passes over the row twice, P coming from LDS both times: the
// first pass takes the row sums of P and of the student's row in double (and writes P out where asked for), the second does the work of
// evc_distill_losses_ensemble's second pass.  V <= 32768 (128 KiB of LDS), as evc_label_loss and evc_topk_rows.
//
// Contraction of a * b + c is switched off for the whole file.  ed_block_sum, ed_key, ed_teacher_elem and ed_student_elem of
// evc_distill_ensemble.hip are restated here: that file keeps its bytes.
#include "evc_common.h"

#include <mutex>

#pragma clang fp contract(off)

#define DSP_MAX_F 8
#define DSP_MAX_KP 256
#define DSP_MAX_V 32768
#define DSP_MAX_GRID 2048

__device__ __forceinline__ float dsp_block_sum(float v, float* sh) {      // block_sum of evc_elementwise.hip at 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < 4; ++i) t += sh[i];
  return t;
}
__device__ __forceinline__ double dsp_block_sum_f64(double v, double* sh) {      // the same fixed order, on doubles
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

// topk_key of evc_topk.hip: larger key = larger value, -0 ties with +0, every NaN above +inf
__device__ __forceinline__ uint32_t dsp_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A group of G consecutive elements (G = 4 where the row length allows 16-byte accesses, else 1): one 16-byte access where the pointer is
// aligned, G 4-byte accesses to the same elements otherwise.
template <int G>
__device__ __forceinline__ void dsp_load(const float* p, long g, bool v4, float (&v)[G]) {
  if constexpr (G == 4) {
    if (v4) {
      const float4 q = ((const float4*)p)[g];
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = p[4 * g + r];
    }
  } else {
    v[0] = p[g];
  }
}
template <int G>
__device__ __forceinline__ void dsp_store(float* p, long g, bool v4, const float (&v)[G]) {
  if constexpr (G == 4) {
    if (v4) {
      ((float4*)p)[g] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[4 * g + r] = v[r];
    }
  } else {
    p[g] = v[0];
  }
}
template <int G>
__device__ __forceinline__ void dsp_load_labels(const uint8_t* y, long g, bool v4, bool (&pos)[G]) {
  if constexpr (G == 4) {
    if (v4) {
      const uchar4 q = ((const uchar4*)y)[g];
      pos[0] = q.x != 0; pos[1] = q.y != 0; pos[2] = q.z != 0; pos[3] = q.w != 0;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) pos[r] = y[4 * g + r] != 0;
    }
  } else {
    pos[0] = y[g] != 0;
  }
}
// group g of the combined row in LDS (the row starts 16-byte aligned, so a group of 4 is one 16-byte LDS read)
template <int G>
__device__ __forceinline__ void dsp_load_row(const float* row, int g, float (&v)[G]) {
  if constexpr (G == 4) {
    const float4 q = ((const float4*)row)[g];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = row[g];
  }
}

// ed_teacher_elem / ed_student_elem of evc_distill_ensemble.hip (see there for the double-precision difference of the gradient and the
// log1p path of L_PRED's value)
struct DspTeacherElem { float ce_t, P; double Pd; };
__device__ __forceinline__ DspTeacherElem dsp_teacher_elem(float pt, bool pos, double itd) {
  const float eps = 10e-6f;   // cs/losses.py:92
  DspTeacherElem r;
  const float at = pt + eps, bt = 1.f - pt + eps;
  r.ce_t = -(pos ? __logf(at) : __logf(bt));
  r.Pd = (double)pt * itd;
  r.P = (float)r.Pd;
  return r;
}
struct DspStudentElem { double kl; float ce_s, g; };
// ssd = the student's row sum (clamped at FLT_MIN), isd = 1 / ssd
__device__ __forceinline__ DspStudentElem dsp_student_elem(const DspTeacherElem te, float ps, bool pos, double ssd, double isd, bool t_ok,
                                                           float g_ce, float g_kl) {
  const float eps = 10e-6f;
  const float FMIN = 1.17549435e-38f;
  DspStudentElem r;
  const float a = ps + eps, bq = 1.f - ps + eps;
  r.ce_s = -(pos ? __logf(a) : __logf(bq));
  const float q = fmaxf(ps, FMIN);
  const double pq = te.Pd / (double)q;                     // P / p_s
  const double ratio = pq * ssd;                           // P / Q, Q = p_s / sum(p_s)
  const float lr = (ratio > 0.5 && ratio < 2.0) ? log1pf((float)(ratio - 1.0)) : __logf(fminf(fmaxf((float)ratio, FMIN), 3.0e38f));
  r.kl = (te.P >= FMIN) ? te.Pd * (double)lr : 0.0;
  const float gce = (g_ce != 0.f) ? (pos ? -1.f / a : 1.f / bq) * g_ce : 0.f;
  const double gkl = (t_ok && g_kl != 0.f) ? (-pq + isd) * (double)g_kl : 0.0;
  r.g = (float)((double)gce + gkl);
  return r;
}

struct DspArgs {
  const int32_t* pidx;    // [F][B][kp]
  const float* pval;      // [F][B][kp]
  const uint8_t* y;
  const float* ps;        // pred_s [B][V]
  float* dps;             // may be NULL
  float* pred_comb;       // may be NULL
  float* ws;
  int F, kp, mode, B, V;
  float g_ce, g_kl, inv_b;
  float w[DSP_MAX_F];
};

// Workspace (floats): [0, B) CE of the combined row, per row; [B, 2 B) L_PRED, per row; [2 B, 3 B) student CE, per row.
template <int G>
__device__ __forceinline__ void dsp_row(const DspArgs& a, int row_i, float* row, float* sh, double* shd) {
  const int tid = threadIdx.x, V = a.V;
  const float FMIN = 1.17549435e-38f;
  const long base = (long)row_i * V;
  const int ng = V / G;
  const uint8_t* y = a.y + base;
  const float* ps = a.ps + base;
  float* dps = a.dps ? a.dps + base : nullptr;
  float* pcomb = a.pred_comb ? a.pred_comb + base : nullptr;
  const bool y4 = ((uintptr_t)a.y & 3) == 0, ps4 = ((uintptr_t)a.ps & 15) == 0, dps4 = ((uintptr_t)a.dps & 15) == 0,
             pc4 = ((uintptr_t)a.pred_comb & 15) == 0;
  // the combined row: +0.0 everywhere (the all-zero member), then the files in order
  for (int g = tid; g < ng; g += 256) {
    if constexpr (G == 4) ((float4*)row)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    else row[g] = 0.f;
  }
  __syncthreads();
#pragma nounroll
  for (int f = 0; f < a.F; ++f) {
    const long o = ((long)f * a.B + row_i) * a.kp;
    const float w = a.w[f];
    for (int e = tid; e < a.kp; e += 256) {
      const int32_t c = a.pidx[o + e];
      if (c >= 0 && c < V) {
        const float val = a.pval[o + e];
        if (a.mode == 0) {
          if (dsp_key(__float_as_uint(val)) > dsp_key(__float_as_uint(row[c]))) row[c] = val;
        } else {
          const float pr = w * val;
          row[c] = row[c] + pr;
        }
      }
    }
    __syncthreads();
  }
  // first pass: the row sums of P and of the student's row in double (the student's row is read again below, from cache)
  double sum_t = 0.0, sum_s = 0.0;
  for (int g = tid; g < ng; g += 256) {
    float pc[G], sv[G];
    dsp_load_row<G>(row, g, pc);
    dsp_load<G>(ps, g, ps4, sv);
#pragma unroll
    for (int r = 0; r < G; ++r) { sum_t += (double)pc[r]; sum_s += (double)sv[r]; }
    if (pcomb) dsp_store<G>(pcomb, g, pc4, pc);
  }
  sum_t = dsp_block_sum_f64(sum_t, shd);
  sum_s = dsp_block_sum_f64(sum_s, shd);
  // a combined row whose sum is below FLT_MIN (no list names a class of it) contributes L_PRED 0 and KL gradient 0; a student sum below
  // it is clamped to it
  const bool t_ok = sum_t >= (double)FMIN;
  const double itd = t_ok ? 1.0 / sum_t : 0.0;
  const double ssd = fmax(sum_s, (double)FMIN);
  const double isd = 1.0 / ssd;
  float s_ct = 0.f, s_cs = 0.f;
  double s_kl = 0.0;
  for (int g = tid; g < ng; g += 256) {
    bool pos[G];
    float pc[G], sv[G], gr[G];
    dsp_load_labels<G>(y, g, y4, pos);
    dsp_load_row<G>(row, g, pc);
    dsp_load<G>(ps, g, ps4, sv);
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const DspTeacherElem te = dsp_teacher_elem(pc[r], pos[r], itd);
      const DspStudentElem e = dsp_student_elem(te, sv[r], pos[r], ssd, isd, t_ok, a.g_ce, a.g_kl);
      s_ct += te.ce_t; s_kl += e.kl; s_cs += e.ce_s; gr[r] = e.g;
    }
    if (dps) dsp_store<G>(dps, g, dps4, gr);
  }
  // every thread is past its last read of the LDS row once it is through the first barrier below: the next row may zero it
  s_ct = dsp_block_sum(s_ct, sh);
  s_kl = dsp_block_sum_f64(s_kl, shd);
  s_cs = dsp_block_sum(s_cs, sh);
  if (tid == 0) {
    a.ws[row_i] = s_ct * a.inv_b;
    a.ws[(long)a.B + row_i] = (float)s_kl;
    a.ws[2L * a.B + row_i] = s_cs * a.inv_b;
  }
}

__global__ __launch_bounds__(256) void distill_sparse_kernel(const DspArgs a) {
  extern __shared__ __attribute__((aligned(16))) char dsp_lds[];     // the combined row, V floats
  __shared__ float sh[4];
  __shared__ double shd[4];
  float* row = (float*)dsp_lds;
  for (int r = blockIdx.x; r < a.B; r += gridDim.x) {                // block-uniform
    if ((a.V & 3) == 0) dsp_row<4>(a, r, row, sh, shd);
    else dsp_row<1>(a, r, row, sh, shd);
  }
}

// One workgroup of four waves; wave 0 owns loss slot 0 (CE of the combined row), wave 2 slot 2 (L_PRED), wave 3 slot 3 (student CE); slot 1
// (L_REP) is left alone.  The partials pass through LDS in pieces of 1024 and lane 0 of each wave adds its list in row order, as
// distill_ensemble_finish_kernel does.
__global__ __launch_bounds__(256) void distill_sparse_finish_kernel(const float* __restrict__ ws, int B, float* __restrict__ losses) {
  __shared__ float sh[4][1024];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long off[4] = {0, 0, (long)B, 2L * B};
  const int cnt[4] = {B, 0, B, B};
  float s = 0.f;
  for (int base = 0; base < B; base += 1024) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
      for (int e = threadIdx.x; e < 1024; e += 256)
        if (base + e < cnt[i]) sh[i][e] = ws[off[i] + base + e];
    __syncthreads();
    if (lane == 0) {
      const int n = cnt[w] - base < 1024 ? cnt[w] - base : 1024;
      for (int e = 0; e < n; ++e) s += sh[w][e];
    }
  }
  if (lane == 0 && w != 1) losses[w] += s;
}

extern "C" int evc_distill_losses_sparse(int F, const int32_t* prior_idx, const float* prior_val, int kp, const float* w, int mode,
                                         const uint8_t* labels, const float* pred_s, int B, int V, float g_ce, float g_kl, float* losses,
                                         float* pred_comb, float* dpred_s, float* workspace, void* stream) {
  EVC_REQUIRE(F >= 1 && F <= DSP_MAX_F, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: F=%d lists (1 .. %d)", F, DSP_MAX_F);
  EVC_REQUIRE(kp >= 1 && kp <= DSP_MAX_KP, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: kp=%d entries per list (1 .. %d)", kp, DSP_MAX_KP);
  EVC_REQUIRE(mode == 0 || mode == 1, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: mode=%d (0 = max, 1 = weighted mean)", mode);
  EVC_REQUIRE(B >= 0 && V > 0 && V <= DSP_MAX_V, EVC_ERR_BAD_SHAPE, "evc_distill_losses_sparse: B=%d V=%d (B >= 0, 1 <= V <= %d)", B, V,
              DSP_MAX_V);
  EVC_REQUIRE(mode == 0 || w, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: mode 1 (weighted mean) needs w");
  if (B == 0) return EVC_OK;
  EVC_REQUIRE(prior_idx && prior_val && labels && pred_s && losses, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: a required pointer is NULL");
  EVC_REQUIRE(workspace, EVC_ERR_BAD_ARG, "evc_distill_losses_sparse: workspace (3 * B floats of scratch) is required");
  DspArgs a;
  memset(&a, 0, sizeof(a));
  a.pidx = prior_idx; a.pval = prior_val; a.y = labels; a.ps = pred_s; a.dps = dpred_s; a.pred_comb = pred_comb; a.ws = workspace;
  a.F = F; a.kp = kp; a.mode = mode; a.B = B; a.V = V;
  a.g_ce = g_ce; a.g_kl = g_kl; a.inv_b = 1.0f / B;
  for (int f = 0; f < F; ++f) a.w[f] = mode == 1 ? w[f] : 0.f;
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)distill_sparse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DSP_MAX_V * 4);
  });
  const size_t lds = (size_t)((V + 3) / 4) * 16;               // the row, rounded up to whole 16-byte groups
  hipLaunchKernelGGL(distill_sparse_kernel, dim3(B < DSP_MAX_GRID ? B : DSP_MAX_GRID), dim3(256), lds, (hipStream_t)stream, a);
  hipLaunchKernelGGL(distill_sparse_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, B, losses);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

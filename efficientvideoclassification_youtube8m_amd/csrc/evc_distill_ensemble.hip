// The loss section of the serial distillation step for ONE student against J frozen teachers (EnsembleDistillGraph), 1 <= J <= 8: the
// teachers' prediction rows are combined as the dense exit of evc_ensemble_topk_rows combines them (max | weighted mean), their states as a
// weighted sum, and the student is trained against the combined row and state as evc_distill_losses_multi trains one against a single teacher.
// One launch + one finish launch, no float atomics, no last-block counters.
//
// A prediction row belongs to one workgroup, which passes over it twice.  The first pass combines the J member rows element by element,
// takes the row sums of the combined row and of the student's row in double, optionally writes the combined row out and adds up each
// teacher's own CE; the second pass combines the same elements AGAIN (the member rows come from cache; plain IEEE f32 products and sums
// with contraction off, or a selection of bits: the same bits both times) and does the work of evc_distill_losses_multi's second pass.
// Recomputing needs no LDS row and so sets no limit on V.
//
// For a given combined row and state the outputs do not depend on J or on how the row came about: the members pass through ONE loop body
// - the loops over j below are never unrolled, nothing but LDS slots and the launch's argument block is indexed by j - and everything
// behind the combination reads the combined value alone.  Contraction of a * b + c is switched off for the whole file.
// dm_block_sum, dm_teacher_elem and dm_student_elem of evc_distill_multi.hip are restated here: that file keeps its bytes.
#include "evc_common.h"

#pragma clang fp contract(off)

#define ED_MAX_J 8

__device__ __forceinline__ float ed_block_sum(float v, float* sh) {      // block_sum of evc_elementwise.hip at 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < 4; ++i) t += sh[i];
  return t;
}
__device__ __forceinline__ double ed_block_sum_f64(double v, double* sh) {      // the same fixed order, on doubles
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
__device__ __forceinline__ uint32_t ed_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// per-teacher pointers and weights, by value in the launch's arguments (as DistillMultiTable)
struct EnsDistillTable {
  const float* pt[ED_MAX_J];     // pred_t  [B][V]
  const float* st[ED_MAX_J];     // state_t [B][D]; not read (may be NULL) where r == 0
  float w[ED_MAX_J];             // prediction weights (mode 1)
  float r[ED_MAX_J];             // representation weights
};

// A group of G consecutive elements (G = 4 where the row length allows 16-byte accesses, else 1): one 16-byte access where the pointer is
// aligned, G 4-byte accesses to the same elements otherwise.
template <int G>
__device__ __forceinline__ void ed_load(const float* p, long g, bool v4, float (&v)[G]) {
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
__device__ __forceinline__ void ed_store(float* p, long g, bool v4, const float (&v)[G]) {
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
__device__ __forceinline__ void ed_load_labels(const uint8_t* y, long g, bool v4, bool (&pos)[G]) {
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

// Group g of the combined row from the J member rows.  mode 1: acc = w0 x0; acc = acc + wj xj, j ascending, every product and sum an f32
// operation of its own; mode 0: the value with the largest ed_key, the lowest member on equal keys (its bits).  ce_acc != NULL: each
// member's own CE terms of these elements are added to its LDS slot ce_acc[256 j] on the way.
template <int G>
__device__ __forceinline__ void ed_combine(const EnsDistillTable& t, int J, int mode, long base, long g, const bool (&pos)[G], float* ce_acc,
                                           float (&pc)[G]) {
  const float eps = 10e-6f;   // cs/losses.py:92
  uint32_t bk[G];
#pragma unroll
  for (int r = 0; r < G; ++r) { pc[r] = 0.f; bk[r] = 0u; }
#pragma nounroll
  for (int j = 0; j < J; ++j) {
    float x[G];
    ed_load<G>(t.pt[j] + base, g, ((uintptr_t)t.pt[j] & 15) == 0, x);
    if (mode == 1) {
      const float w = t.w[j];
#pragma unroll
      for (int r = 0; r < G; ++r) {
        const float pr = w * x[r];
        pc[r] = (j == 0) ? pr : pc[r] + pr;
      }
    } else {
#pragma unroll
      for (int r = 0; r < G; ++r) {
        const uint32_t km = ed_key(__float_as_uint(x[r]));
        if (j == 0 || km > bk[r]) { pc[r] = x[r]; bk[r] = km; }
      }
    }
    if (ce_acc) {
      float s = ce_acc[256 * j];
#pragma unroll
      for (int r = 0; r < G; ++r) s += -(pos[r] ? __logf(x[r] + eps) : __logf(1.f - x[r] + eps));
      ce_acc[256 * j] = s;
    }
  }
}

// dm_teacher_elem / dm_student_elem of evc_distill_multi.hip (see there for why the one cancelling difference of the gradient is taken in
// double), with one change to L_PRED's VALUE: a student close to the combined row makes sum_c P log(P / Q) a sum of first-order terms of
// both signs that cancel down to the second order (tiny towers at initialisation: 4e-4 out of 0.07), and log(P) - log(Q) from two f32
// logarithms then leaves 1e-7 absolute on every term.  So the ratio P / Q is formed in double from the quotient the gradient needs anyway,
// its logarithm is log1pf(ratio - 1) where the ratio is near 1, and the row's terms are added up in double (a row's own sum is >= 0: the
// rows are joined in f32 as ever).
struct EdTeacherElem { float ce_t, P; double Pd; };
__device__ __forceinline__ EdTeacherElem ed_teacher_elem(float pt, bool pos, double itd) {
  const float eps = 10e-6f;
  EdTeacherElem r;
  const float at = pt + eps, bt = 1.f - pt + eps;
  r.ce_t = -(pos ? __logf(at) : __logf(bt));
  r.Pd = (double)pt * itd;
  r.P = (float)r.Pd;
  return r;
}
struct EdStudentElem { double kl; float ce_s, g; };
// ssd = the student's row sum (clamped at FLT_MIN), isd = 1 / ssd
__device__ __forceinline__ EdStudentElem ed_student_elem(const EdTeacherElem te, float ps, bool pos, double ssd, double isd, bool t_ok, float g_ce,
                                                         float g_kl) {
  const float eps = 10e-6f;
  const float FMIN = 1.17549435e-38f;
  EdStudentElem r;
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

struct EdArgs {
  const uint8_t* y;
  const float* ps;        // pred_s  [B][V]
  const float* ss;        // state_s [B][D]
  float* dps;             // may be NULL
  float* dss;             // may be NULL
  float* pred_comb;       // may be NULL
  float* ws;
  int J, mode, B, V, NS, want_tce;
  long nd;
  float g_ce, g_kl, g_rep, inv_b;
};

// Workspace (floats), NS <= 256 state workgroups:
//   [0, B)                      CE of the combined row, per row          [B, 2 B)   L_PRED, per row          [2 B, 3 B)   student CE, per row
//   [3 B, 3 B + 256)            L_REP, per state workgroup
//   [3 B + 256 + j B, ... + B)  teacher j's own CE, per row (written when teacher_ce is asked for)
template <int G>
__device__ __forceinline__ void ed_row(const EnsDistillTable& t, const EdArgs& a, float (*tce)[256], float* sh, double* shd) {
  const int tid = threadIdx.x, row = blockIdx.x, J = a.J, mode = a.mode;
  const float FMIN = 1.17549435e-38f;
  const long base = (long)row * a.V;
  const int ng = a.V / G;
  const uint8_t* y = a.y + base;
  const float* ps = a.ps + base;
  float* dps = a.dps ? a.dps + base : nullptr;
  float* pcomb = a.pred_comb ? a.pred_comb + base : nullptr;
  const bool y4 = ((uintptr_t)a.y & 3) == 0, ps4 = ((uintptr_t)a.ps & 15) == 0, dps4 = ((uintptr_t)a.dps & 15) == 0,
             pc4 = ((uintptr_t)a.pred_comb & 15) == 0;
  float* ce_acc = a.want_tce ? &tce[0][tid] : nullptr;
  // first pass: the combined row's and the student's row sums in double (both rows are read again below, from cache)
  double sum_t = 0.0, sum_s = 0.0;
  for (int g = tid; g < ng; g += 256) {
    bool pos[G];
    float pc[G], sv[G];
    ed_load_labels<G>(y, g, y4, pos);
    ed_combine<G>(t, J, mode, base, g, pos, ce_acc, pc);
    ed_load<G>(ps, g, ps4, sv);
#pragma unroll
    for (int r = 0; r < G; ++r) { sum_t += (double)pc[r]; sum_s += (double)sv[r]; }
    if (pcomb) ed_store<G>(pcomb, g, pc4, pc);
  }
  sum_t = ed_block_sum_f64(sum_t, shd);
  sum_s = ed_block_sum_f64(sum_s, shd);
  // a combined row whose sum is below FLT_MIN contributes L_PRED 0 and KL gradient 0; a student sum below it is clamped to it
  const bool t_ok = sum_t >= (double)FMIN;
  const double itd = t_ok ? 1.0 / sum_t : 0.0;
  const double ssd = fmax(sum_s, (double)FMIN);
  const double isd = 1.0 / ssd;
  float s_ct = 0.f, s_cs = 0.f;
  double s_kl = 0.0;
  for (int g = tid; g < ng; g += 256) {
    bool pos[G];
    float pc[G], sv[G], gr[G];
    ed_load_labels<G>(y, g, y4, pos);
    ed_combine<G>(t, J, mode, base, g, pos, nullptr, pc);
    ed_load<G>(ps, g, ps4, sv);
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const EdTeacherElem te = ed_teacher_elem(pc[r], pos[r], itd);
      const EdStudentElem e = ed_student_elem(te, sv[r], pos[r], ssd, isd, t_ok, a.g_ce, a.g_kl);
      s_ct += te.ce_t; s_kl += e.kl; s_cs += e.ce_s; gr[r] = e.g;
    }
    if (dps) ed_store<G>(dps, g, dps4, gr);
  }
  s_ct = ed_block_sum(s_ct, sh);
  s_kl = ed_block_sum_f64(s_kl, shd);
  s_cs = ed_block_sum(s_cs, sh);
  if (tid == 0) {
    a.ws[row] = s_ct * a.inv_b;
    a.ws[(long)a.B + row] = (float)s_kl;
    a.ws[2L * a.B + row] = s_cs * a.inv_b;
  }
  if (a.want_tce) {
#pragma nounroll
    for (int j = 0; j < J; ++j) {
      const float s = ed_block_sum(tce[j][tid], sh);
      if (tid == 0) a.ws[3L * a.B + 256 + (long)j * a.B + row] = s * a.inv_b;
    }
  }
}

// The state part, grid-stride over the B * D elements: the combined state is r_j state_t[j] summed left to right over the entries with
// r_j != 0, every product and sum an f32 operation of its own (no such entry: 0).
template <int G>
__device__ __forceinline__ void ed_state(const EnsDistillTable& t, const EdArgs& a, float* sh) {
  const int tid = threadIdx.x, blk = (int)blockIdx.x - a.B, J = a.J;
  const bool ss4 = ((uintptr_t)a.ss & 15) == 0, dss4 = ((uintptr_t)a.dss & 15) == 0;
  float s = 0.f;
  for (long g = (long)blk * 256 + tid; g < a.nd / G; g += (long)a.NS * 256) {
    float sc[G], bv[G], gr[G];
#pragma unroll
    for (int r = 0; r < G; ++r) sc[r] = 0.f;
    bool first = true;
#pragma nounroll
    for (int j = 0; j < J; ++j) {
      const float rw = t.r[j];
      if (rw == 0.f) continue;
      float x[G];
      ed_load<G>(t.st[j], g, ((uintptr_t)t.st[j] & 15) == 0, x);
#pragma unroll
      for (int r = 0; r < G; ++r) {
        const float pr = rw * x[r];
        sc[r] = first ? pr : sc[r] + pr;
      }
      first = false;
    }
    ed_load<G>(a.ss, g, ss4, bv);
#pragma unroll
    for (int r = 0; r < G; ++r) {
      const float d = sc[r] - bv[r];
      s += d * d;
      gr[r] = (a.g_rep != 0.f) ? -2.f * d * a.inv_b * a.g_rep : 0.f;
    }
    if (a.dss) ed_store<G>(a.dss, g, dss4, gr);
  }
  s = ed_block_sum(s, sh);
  if (tid == 0) a.ws[3L * a.B + blk] = s * a.inv_b;
}

// Workgroups [0, B): one prediction row each; workgroups [B, B + NS): the state part.
__global__ __launch_bounds__(256) void distill_ensemble_kernel(const EnsDistillTable t, const EdArgs a) {
  __shared__ float sh[4];
  __shared__ double shd[4];
  __shared__ float tce[ED_MAX_J][256];          // per-thread CE accumulators of the J teachers (a register array indexed by j would spill)
  if ((int)blockIdx.x < a.B) {
    if (a.want_tce) {
#pragma nounroll
      for (int j = 0; j < a.J; ++j) tce[j][threadIdx.x] = 0.f;
    }
    if ((a.V & 3) == 0) ed_row<4>(t, a, tce, sh, shd);
    else ed_row<1>(t, a, tce, sh, shd);
    return;
  }
  if ((a.nd & 3) == 0) ed_state<4>(t, a, sh);
  else ed_state<1>(t, a, sh);
}

// Workgroup 0: four waves, wave w owns loss slot w (CE of the combined row, L_REP, L_PRED, student CE); workgroup 1 + j / 4 (launched
// when teacher_ce is asked for): wave j % 4 owns teacher j's CE.  The partials pass through LDS in pieces of 1024 and lane 0 of each wave
// adds its list in workgroup order, as distill_multi_finish_kernel does.
__global__ __launch_bounds__(256) void distill_ensemble_finish_kernel(const float* __restrict__ ws, int J, int B, int NS, float* __restrict__ losses,
                                                                      float* __restrict__ teacher_ce) {
  __shared__ float sh[4][1024];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long off[4];
  int cnt[4];
  if (blockIdx.x == 0) {
    off[0] = 0; off[1] = 3L * B; off[2] = B; off[3] = 2L * B;
    cnt[0] = B; cnt[1] = NS; cnt[2] = B; cnt[3] = B;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * ((int)blockIdx.x - 1) + i;
      off[i] = 3L * B + 256 + (long)j * B;
      cnt[i] = j < J ? B : 0;
    }
  }
  const int nmax = B > NS ? B : NS;
  float s = 0.f;
  for (int base = 0; base < nmax; base += 1024) {
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
  if (lane == 0) {
    if (blockIdx.x == 0) losses[w] += s;
    else if (cnt[w] > 0) teacher_ce[4 * ((int)blockIdx.x - 1) + w] += s;
  }
}

extern "C" int evc_distill_losses_ensemble(int J, const float* const* pred_t, const float* const* state_t, const float* w, const float* r,
                                           int mode, const uint8_t* labels, const float* pred_s, const float* state_s, int B, int V, int D,
                                           float g_ce, float g_kl, float g_rep, float* losses, float* teacher_ce, float* pred_comb,
                                           float* dpred_s, float* dstate_s, float* workspace, void* stream) {
  EVC_REQUIRE(J >= 1 && J <= ED_MAX_J, EVC_ERR_BAD_ARG, "evc_distill_losses_ensemble: J=%d teachers (1 .. %d)", J, ED_MAX_J);
  EVC_REQUIRE(mode == 0 || mode == 1, EVC_ERR_BAD_ARG, "evc_distill_losses_ensemble: mode=%d (0 = max, 1 = weighted mean)", mode);
  EVC_REQUIRE(B > 0 && V > 0 && D > 0, EVC_ERR_BAD_SHAPE, "evc_distill_losses_ensemble: bad shape");
  EVC_REQUIRE(pred_t && state_t && r && labels && pred_s && state_s && losses && (mode == 0 || w), EVC_ERR_BAD_ARG,
              "evc_distill_losses_ensemble: a required pointer is NULL");
  EVC_REQUIRE(workspace, EVC_ERR_BAD_ARG, "evc_distill_losses_ensemble: workspace ((3 + J) * B + 256 floats of scratch) is required");
  EnsDistillTable t;
  memset(&t, 0, sizeof(t));
  bool any_r = false;
  for (int j = 0; j < J; ++j) {
    EVC_REQUIRE(pred_t[j], EVC_ERR_BAD_ARG, "evc_distill_losses_ensemble: teacher %d: pred_t is NULL", j);
    EVC_REQUIRE(r[j] == 0.f || state_t[j], EVC_ERR_BAD_ARG, "evc_distill_losses_ensemble: teacher %d: state_t is NULL with r != 0", j);
    t.pt[j] = pred_t[j]; t.st[j] = state_t[j];
    t.w[j] = mode == 1 ? w[j] : 0.f;
    t.r[j] = r[j];
    any_r = any_r || r[j] != 0.f;
  }
  EVC_REQUIRE(any_r || (g_rep == 0.f && dstate_s == nullptr), EVC_ERR_BAD_ARG,
              "evc_distill_losses_ensemble: every r is 0: no combined state for L_REP's gradient (g_rep = 0 and dstate_s = NULL only)");
  EdArgs a;
  memset(&a, 0, sizeof(a));
  a.nd = (long)B * D;
  const long want = (a.nd + 1023) / 1024;                 // 4 elements per thread and trip, as evc_distill_losses
  a.NS = (int)(want < 1 ? 1 : (want < 256 ? want : 256));
  a.y = labels; a.ps = pred_s; a.ss = state_s; a.dps = dpred_s; a.dss = dstate_s; a.pred_comb = pred_comb; a.ws = workspace;
  a.J = J; a.mode = mode; a.B = B; a.V = V; a.want_tce = teacher_ce != nullptr;
  a.g_ce = g_ce; a.g_kl = g_kl; a.g_rep = g_rep; a.inv_b = 1.0f / B;
  hipLaunchKernelGGL(distill_ensemble_kernel, dim3(B + a.NS), dim3(256), 0, (hipStream_t)stream, t, a);
  hipLaunchKernelGGL(distill_ensemble_finish_kernel, dim3(teacher_ce ? 1 + (J + 3) / 4 : 1), dim3(256), 0, (hipStream_t)stream,
                     (const float*)workspace, J, B, a.NS, losses, teacher_ce);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

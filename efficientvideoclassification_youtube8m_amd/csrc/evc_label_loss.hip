// The label losses of cs/losses.py besides CrossEntropyLoss (evc_label_loss; --label_loss): value and dL/dpred in one pass, as
// evc_ce_loss gives them for the default loss.  The definitions table is in include/evc.h and DESIGN.md 7.7.
//
// One 256-thread workgroup per row, the grid strides over the rows; one template instantiation per kind:
//   - WITH_SPARSITY, CLASS_IMBALANCE, POSITIVES, NEW, HINGE stream the row once: 16-byte loads of pred (4-byte of the labels) and 16-byte
//     stores of dpred where this row's pointers allow it, 4-byte accesses otherwise (decided per row: an odd V alternates);
//   - TOP50 and SOFTMAX stage the row in LDS once (V * 4 bytes, V <= 32768).  TOP50 finds the exact 50th largest key with a 4-pass radix
//     select on order-preserving keys (integer LDS histogram, suffix scan over the 256 digits, no early stop) and then makes the masked
//     pass from LDS; SOFTMAX takes the row maximum and the sum of exponentials from LDS, then makes the gradient pass;
//   - NEW has a launch in front that leaves per-workgroup minima of (y ? p : 1) in the workspace; every workgroup of the main launch
//     reduces those in index order to the batch minimum.
// Every workgroup leaves its row's loss in workspace[row]; a one-workgroup finish launch adds the B values in a fixed order and does
// *loss +=.  No float atomics anywhere: two calls on the same inputs give the same bits.  dpred is written (or read-modify-written) exactly
// once per element.
// block_sum of evc_elementwise.hip and the key / scan helpers of evc_topk.hip are restated here, so that the kernels of those files stay
// the code they were.
#include "evc_common.h"

#include <mutex>

namespace {

constexpr int LL_THREADS = 256;
constexpr int LL_MAX_COLS = 32768;
constexpr int LL_MAX_GRID = 2048;
constexpr int LL_MIN_SLOTS = 256;                                    // workspace[B .. B + 256): the minima of NEW's first launch
// dynamic LDS carve of the two staged kinds (every offset a multiple of 16): histogram | scan + selection words | row
constexpr int LL_OFF_MISC = 256 * 4;
constexpr int LL_OFF_ROW = LL_OFF_MISC + 64;
constexpr int LL_MAX_LDS = LL_OFF_ROW + LL_MAX_COLS * 4;

__device__ __forceinline__ float ll_block_sum(float v, float* sh) {      // block_sum of evc_elementwise.hip at 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ float ll_block_max(float v, float* sh) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ float ll_block_min(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}

// topk_key of evc_topk.hip: larger key = larger value, -0 ties with +0, every NaN above +inf
__device__ __forceinline__ uint32_t ll_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ll_key_value(uint32_t key) {           // a value with that key
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// block_incl_scan of evc_topk.hip
__device__ __forceinline__ uint32_t ll_incl_scan(uint32_t v, uint32_t* ws) {
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

// What an element needs besides (p, y): the threshold of the kind (TOP50: the 50th largest value, NEW: mpp, SOFTMAX: the row maximum)
// and SOFTMAX's row constants.
struct LLRow {
  float thr;
  float inv_sum;   // 1 / sum_c exp(p_c - max)
  float sy;        // sum_c yhat_c
  float yhat;      // 1 / max(sum y, 10e-8)
};

// One element: s += its share of the row loss (SOFTMAX: of sum_pos (p - max)), returns d(row loss)/dp.  eps = 10e-6 (cs/losses.py).
template <int KIND>
__device__ __forceinline__ float ll_elem(float p, bool pos, float w, const LLRow& r, float& s) {
  const float eps = 10e-6f;
  if constexpr (KIND == EVC_LOSS_HINGE) {
    const float sg = pos ? 1.f : -1.f;
    const float m = 1.f - sg * p;
    const bool on = m > 0.f;                                         // a tie goes to the zeros (tf.maximum)
    s += on ? m : 0.f;
    return on ? -sg : 0.f;
  } else if constexpr (KIND == EVC_LOSS_SOFTMAX) {
    const float d = p - r.thr;
    s += pos ? d : 0.f;
    return __expf(d) * r.inv_sum * r.sy - (pos ? r.yhat : 0.f);
  } else {
    const float a = p + eps, bq = 1.f - p + eps;
    if constexpr (KIND == EVC_LOSS_WITH_SPARSITY) {
      s += 0.1f * p - (pos ? __logf(a) : __logf(bq));
      return (pos ? -1.f / a : 1.f / bq) + 0.1f;
    } else if constexpr (KIND == EVC_LOSS_TOP50) {
      const float k50 = 4716.0f / 50.0f;
      const bool on = p >= r.thr;
      s -= on ? k50 * (pos ? __logf(a) : __logf(bq)) : 0.f;
      return on ? k50 * (pos ? -1.f / a : 1.f / bq) : 0.f;
    } else if constexpr (KIND == EVC_LOSS_CLASS_IMBALANCE) {
      s -= pos ? w * __logf(a) : __logf(bq);
      return pos ? -w / a : 1.f / bq;
    } else if constexpr (KIND == EVC_LOSS_POSITIVES) {
      s -= pos ? __logf(a) : 0.f;
      return pos ? -1.f / a : 0.f;
    } else {                                                         // EVC_LOSS_NEW
      const bool on = pos ? (p < 0.9f) : (p > r.thr);                // bad positive / bad negative (p (1 - y) > mpp, mpp >= 0.1 > 0)
      s -= on ? (pos ? __logf(a) : __logf(bq)) : 0.f;
      return on ? (pos ? -1.f / a : 1.f / bq) : 0.f;
    }
  }
}

// The pass over one row that writes the gradient: pr is the row in global memory or its copy in LDS.  Returns this thread's share of s.
template <int KIND>
__device__ __forceinline__ float ll_row_pass(const float* pr, const uint8_t* __restrict__ yr, const float* __restrict__ w, float* __restrict__ dr,
                                             int V, float gs, int acc, const LLRow& r) {
  const int tid = threadIdx.x;
  float s = 0.f;
  const bool v4 = (((uintptr_t)pr) & 15) == 0 && (((uintptr_t)yr) & 3) == 0 && (dr == nullptr || (((uintptr_t)dr) & 15) == 0) &&
                  (KIND != EVC_LOSS_CLASS_IMBALANCE || (((uintptr_t)w) & 15) == 0);
  int done = 0;
  if (v4) {
    const int n4 = V >> 2;
    for (int i = tid; i < n4; i += LL_THREADS) {
      const float4 pq = ((const float4*)pr)[i];
      const uchar4 yq = ((const uchar4*)yr)[i];
      float4 wq = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (KIND == EVC_LOSS_CLASS_IMBALANCE) wq = ((const float4*)w)[i];
      const float pv[4] = {pq.x, pq.y, pq.z, pq.w};
      const float wv[4] = {wq.x, wq.y, wq.z, wq.w};
      const bool pos[4] = {yq.x != 0, yq.y != 0, yq.z != 0, yq.w != 0};
      float g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = ll_elem<KIND>(pv[j], pos[j], wv[j], r, s);
        g[j] = gs == 0.f ? 0.f : d * gs;
      }
      if (dr) {
        float4 o = make_float4(g[0], g[1], g[2], g[3]);
        if (acc) { const float4 d = ((const float4*)dr)[i]; o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w; }
        ((float4*)dr)[i] = o;
      }
    }
    done = 4 * n4;
  }
  for (int i = done + tid; i < V; i += LL_THREADS) {
    float wv = 0.f;
    if constexpr (KIND == EVC_LOSS_CLASS_IMBALANCE) wv = w[i];
    const float d = ll_elem<KIND>(pr[i], yr[i] != 0, wv, r, s);
    if (dr) {
      const float g = gs == 0.f ? 0.f : d * gs;
      dr[i] = acc ? dr[i] + g : g;
    }
  }
  return s;
}

// row -> LDS (16-byte loads when the row is 16-byte aligned; the LDS row always is)
__device__ __forceinline__ void ll_stage_row(const float* __restrict__ pr, int V, float* row) {
  const int tid = threadIdx.x;
  int done = 0;
  if ((((uintptr_t)pr) & 15) == 0) {
    const int n4 = V >> 2;
    for (int i = tid; i < n4; i += LL_THREADS) ((float4*)row)[i] = ((const float4*)pr)[i];
    done = 4 * n4;
  }
  for (int i = done + tid; i < V; i += LL_THREADS) row[i] = pr[i];
}

// NEW, first launch: part[block] = min over this workgroup's elements of (y ? p : 1)
__global__ __launch_bounds__(LL_THREADS) void label_loss_min_kernel(const float* __restrict__ p, const uint8_t* __restrict__ y, long n,
                                                                     float* __restrict__ part) {
  __shared__ float sh[4];
  float m = 1.f;
  long done = 0;
  if ((((uintptr_t)p) & 15) == 0 && (((uintptr_t)y) & 3) == 0) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * LL_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * LL_THREADS) {
      const float4 pq = ((const float4*)p)[i];
      const uchar4 yq = ((const uchar4*)y)[i];
      m = fminf(m, fminf(fminf(yq.x ? pq.x : 1.f, yq.y ? pq.y : 1.f), fminf(yq.z ? pq.z : 1.f, yq.w ? pq.w : 1.f)));
    }
    done = 4 * n4;
  }
  for (long i = done + (long)blockIdx.x * LL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * LL_THREADS)
    m = fminf(m, y[i] ? p[i] : 1.f);
  m = ll_block_min(m, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

template <int KIND>
__global__ __launch_bounds__(LL_THREADS) void label_loss_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ labels, int B, int V,
                                                                 float gs, const float* __restrict__ w, float* __restrict__ dpred, int acc,
                                                                 float* __restrict__ ws, int nmin) {
  constexpr bool STAGED = KIND == EVC_LOSS_TOP50 || KIND == EVC_LOSS_SOFTMAX;
  extern __shared__ __attribute__((aligned(16))) char ll_lds[];
  uint32_t* hist = (uint32_t*)ll_lds;                                // [256]        (staged kinds only: no dynamic LDS otherwise)
  uint32_t* scan_ws = (uint32_t*)(ll_lds + LL_OFF_MISC);             // [4]
  uint32_t* sel = scan_ws + 4;                                       // prefix, rank left inside it
  float* row = (float*)(ll_lds + LL_OFF_ROW);                        // [V]
  float* sh;                                                         // [4] wave totals of the block reductions
  if constexpr (STAGED) {
    sh = (float*)(scan_ws + 8);                                      // (no static LDS in front of the dynamic region)
  } else {
    __shared__ float sh_static[4];
    sh = sh_static;
  }
  const int tid = threadIdx.x;
  LLRow r = {0.f, 0.f, 0.f, 0.f};
  if constexpr (KIND == EVC_LOSS_NEW) {                              // the batch minimum from the first launch's partials, in index order
    float m = 1.f;
    for (int i = tid; i < nmin; i += LL_THREADS) m = fminf(m, ws[B + i]);
    m = ll_block_min(m, sh);
    r.thr = fmaxf(m - 0.1f, 0.1f);                                   // mpp
  }
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const float* pr = pred + (long)b * V;
    const uint8_t* yr = labels + (long)b * V;
    float* dr = dpred ? dpred + (long)b * V : nullptr;
    float s;
    if constexpr (!STAGED) {
      s = ll_block_sum(ll_row_pass<KIND>(pr, yr, w, dr, V, gs, acc, r), sh);
    } else {
      __syncthreads();                                               // the previous row's readers of `row` are done
      ll_stage_row(pr, V, row);
      __syncthreads();
      if constexpr (KIND == EVC_LOSS_TOP50) {
        // exact key of the 50th largest element (duplicates counted): 4 radix passes of 8 bits from the top
        uint32_t prefix = 0, mask = 0, krem = 50;
        for (int pass = 0; pass < 4; ++pass) {
          const int shift = 24 - 8 * pass;
          hist[tid] = 0;
          __syncthreads();
          for (int i = tid; i < V; i += LL_THREADS) {
            const uint32_t key = ll_key(__float_as_uint(row[i]));
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
          }
          __syncthreads();
          const uint32_t h = hist[255 - tid];                        // thread t: digit 255 - t
          const uint32_t incl = ll_incl_scan(h, scan_ws);            // candidates with digit >= 255 - t
          const uint32_t excl = incl - h;
          if (excl < krem && incl >= krem) {                         // exactly one thread
            sel[0] = prefix | ((uint32_t)(255 - tid) << shift);
            sel[1] = krem - excl;
          }
          __syncthreads();
          prefix = sel[0];
          krem = sel[1];
          mask |= 255u << shift;
          __syncthreads();                                           // sel and scan_ws are rewritten by the next pass
        }
        r.thr = ll_key_value(prefix);
        s = ll_block_sum(ll_row_pass<KIND>(row, yr, w, dr, V, gs, acc, r), sh);
      } else {                                                       // SOFTMAX
        float mx = -INFINITY, cnt = 0.f;
        for (int i = tid; i < V; i += LL_THREADS) {
          mx = fmaxf(mx, row[i]);
          cnt += yr[i] != 0 ? 1.f : 0.f;
        }
        mx = ll_block_max(mx, sh);
        cnt = ll_block_sum(cnt, sh);                                 // an integer below 2^24: exact
        float se = 0.f;
        for (int i = tid; i < V; i += LL_THREADS) se += __expf(row[i] - mx);
        se = ll_block_sum(se, sh);
        if (cnt > 0.f) {
          r.thr = mx;
          r.inv_sum = 1.f / se;
          r.yhat = 1.f / fmaxf(cnt, 10e-8f);
          r.sy = cnt * r.yhat;
          s = ll_block_sum(ll_row_pass<KIND>(row, yr, w, dr, V, gs, acc, r), sh);
          s = logf(se) * r.sy - r.yhat * s;
        } else {                                                     // a row without positives: loss 0, gradient 0
          s = 0.f;
          if (dr && !acc)
            for (int i = tid; i < V; i += LL_THREADS) dr[i] = 0.f;
        }
      }
    }
    if (tid == 0) ws[b] = s;
  }
}

// *loss += inv_b * (the B row losses, added in a fixed order: thread t takes rows t, t + 256, ..., then the block sum)
__global__ __launch_bounds__(LL_THREADS) void label_loss_finish_kernel(const float* __restrict__ ws, int B, float inv_b, float* __restrict__ loss) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += LL_THREADS) s += ws[i];
  s = ll_block_sum(s, sh);
  if (threadIdx.x == 0) *loss += s * inv_b;
}

template <int KIND>
int ll_launch(const float* pred, const uint8_t* labels, int B, int V, float gs, const float* w, float* dpred, int acc, float* ws, int nmin,
              hipStream_t st) {
  constexpr bool STAGED = KIND == EVC_LOSS_TOP50 || KIND == EVC_LOSS_SOFTMAX;
  const size_t lds = STAGED ? (size_t)LL_OFF_ROW + (size_t)((V + 3) & ~3) * sizeof(float) : 0;
  if (STAGED) {
    static std::once_flag once;
    std::call_once(once, [] {
      (void)hipFuncSetAttribute((const void*)label_loss_kernel<KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, LL_MAX_LDS);
    });
  }
  const int grid = B < LL_MAX_GRID ? B : LL_MAX_GRID;
  hipLaunchKernelGGL(label_loss_kernel<KIND>, dim3(grid), dim3(LL_THREADS), lds, st, pred, labels, B, V, gs, w, dpred, acc, ws, nmin);
  return EVC_OK;
}

}  // namespace

extern "C" int evc_label_loss(int kind, const float* pred, const uint8_t* labels, int B, int V, float grad_scale, const float* class_weights,
                              float* loss, float* dpred, int accumulate_grad, float* workspace, void* stream) {
  EVC_REQUIRE(B > 0 && V > 0, EVC_ERR_BAD_SHAPE, "evc_label_loss: bad shape B=%d V=%d", B, V);
  EVC_REQUIRE(V <= LL_MAX_COLS, EVC_ERR_BAD_SHAPE, "evc_label_loss: V=%d (1 .. %d)", V, LL_MAX_COLS);
  EVC_REQUIRE(kind >= EVC_LOSS_WITH_SPARSITY && kind <= EVC_LOSS_SOFTMAX, EVC_ERR_BAD_ARG, "evc_label_loss: unknown kind %d", kind);
  EVC_REQUIRE(kind != EVC_LOSS_TOP50 || V >= 50, EVC_ERR_BAD_ARG, "evc_label_loss: TOP50 needs V >= 50 (V=%d)", V);
  EVC_REQUIRE((kind == EVC_LOSS_CLASS_IMBALANCE) == (class_weights != nullptr), EVC_ERR_BAD_ARG,
              "evc_label_loss: class_weights ([V]) go with kind CLASS_IMBALANCE and with no other (kind %d)", kind);
  EVC_REQUIRE(workspace != nullptr, EVC_ERR_BAD_ARG, "evc_label_loss: workspace (B + 320 floats of scratch) is required");
  EVC_REQUIRE(pred != nullptr && labels != nullptr && loss != nullptr, EVC_ERR_BAD_ARG, "evc_label_loss: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  int nmin = 0;
  if (kind == EVC_LOSS_NEW) {
    const long n = (long)B * V;
    const long want = (n + 4 * LL_THREADS - 1) / (4 * LL_THREADS);
    nmin = (int)(want < LL_MIN_SLOTS ? want : LL_MIN_SLOTS);
    hipLaunchKernelGGL(label_loss_min_kernel, dim3(nmin), dim3(LL_THREADS), 0, st, pred, labels, n, workspace + B);
  }
  const int acc = accumulate_grad ? 1 : 0;
  switch (kind) {
    case EVC_LOSS_WITH_SPARSITY: ll_launch<EVC_LOSS_WITH_SPARSITY>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    case EVC_LOSS_TOP50: ll_launch<EVC_LOSS_TOP50>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    case EVC_LOSS_CLASS_IMBALANCE: ll_launch<EVC_LOSS_CLASS_IMBALANCE>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    case EVC_LOSS_POSITIVES: ll_launch<EVC_LOSS_POSITIVES>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    case EVC_LOSS_NEW: ll_launch<EVC_LOSS_NEW>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    case EVC_LOSS_HINGE: ll_launch<EVC_LOSS_HINGE>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
    default: ll_launch<EVC_LOSS_SOFTMAX>(pred, labels, B, V, grad_scale, class_weights, dpred, acc, workspace, nmin, st); break;
  }
  hipLaunchKernelGGL(label_loss_finish_kernel, dim3(1), dim3(LL_THREADS), 0, st, (const float*)workspace, B, 1.0f / B, loss);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

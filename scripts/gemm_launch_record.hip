// Recording stand-in for the HIP runtime, for scripts/gemm_launch_record.py: linked with HOST-ONLY builds of csrc/evc_gemm.hip and
// csrc/evc_gemm_tn.hip in place of the runtime, it writes every enqueue the NT / TN product entries make to the file named by SHIM_LOG - memsets,
// LDS attributes and every kernel launch with its geometry and each field of its operand and store structs.  Nothing runs; no GPU is needed.
#include "launch_record_stubs.h"
struct StoreParamsTX {      // the layout of StoreParamsT (defined in evc_gemm_tn.hip itself)
  float* C; long ldc; int M, N; int row_il_H; int accumulate, splits, ksteps_per_split; long slab_stride; int ksteps_per_split2;
};
static void dump_launch_args(const std::string& n, void** a) {
  if (n.find("gemm_nt_kernel") != std::string::npos) {
    const GemmOperands& p = *(GemmOperands*)a[0];
    const StoreParams& s = *(StoreParams*)a[1];
    fprintf(out(), "  tiles_m=%d tiles_n=%d\n", *(int*)a[2], *(int*)a[3]);
    fprintf(out(), "  p A1=%p lda1=%ld nk1=%d A2=%p lda2=%ld nk2=%d B=%p ldb=%ld gs=%ld M=%d Nu=%d A1lo=%p A2lo=%p Blo=%p B2=%p A3=%p lda3=%ld nk3=%d A4=%p lda4=%ld nk4=%d B8=%p ldb8=%ld s8=%d amax=%p a8=%d rs=%p ca=%p g2=%g gap=%ld\n",
            (void*)p.A1, p.lda1, p.nk1, (void*)p.A2, p.lda2, p.nk2, (void*)p.B, p.ldb, p.group_stride, p.M, p.Nu, (void*)p.A1lo, (void*)p.A2lo, (void*)p.Blo, (void*)p.B2,
            (void*)p.A3, p.lda3, p.nk3, (void*)p.A4, p.lda4, p.nk4, (void*)p.B8, p.ldb8, p.scale8_exp, (void*)p.amax_ws, p.a8_hi_exp, (void*)p.row_scale, (void*)p.col_add, p.g2_add, p.b8_gap);
    fprintf(out(), "  s C=%p ldc=%ld M=%d N=%d bias=%p out_bf16=%d accumulate=%d splits=%d ksteps=%d ksteps8=%d sq_p=%p sq_l2=%g sq_out=%p\n", s.C, s.ldc, s.M, s.N, (void*)s.bias,
            s.out_bf16, s.accumulate, s.splits, s.ksteps_per_split, s.ksteps8_per_split, (void*)s.sq_p, s.sq_l2, (void*)s.sq_out);
  } else if (n.find("gemm_tn_kernel") != std::string::npos) {
    const GemmOperandsT& p = *(GemmOperandsT*)a[0];
    const StoreParamsTX& s = *(StoreParamsTX*)a[1];
    fprintf(out(), "  tiles_m=%d tiles_n=%d\n", *(int*)a[2], *(int*)a[3]);
    fprintf(out(), "  p A=%p lda=%ld B=%p ldb=%ld M=%d N=%d nk=%d B2=%p ldb2=%ld N1=%d c_col2=%d nseg=%d seg0=%d seg_off0=%d seg=", (void*)p.A, p.lda, (void*)p.B, p.ldb, p.M, p.N, p.nk,
            (void*)p.B2, p.ldb2, p.N1, p.c_col2, p.nseg, p.seg0, p.seg_off0);
    for (int i = 0; i < 16; ++i) fprintf(out(), "%s%u+%u", i ? "," : "", (unsigned)p.seg_start[i], (unsigned)p.seg_len[i]);
    fprintf(out(), "\n  s C=%p ldc=%ld M=%d N=%d row_il_H=%d accumulate=%d splits=%d ksteps=%d slab_stride=%ld\n", (void*)s.C, s.ldc, s.M, s.N, s.row_il_H, s.accumulate, s.splits,
            s.ksteps_per_split, s.slab_stride);
    if (p.k_skip2) fprintf(out(), "  k_skip2=%d ksteps2=%d\n", p.k_skip2, s.ksteps_per_split2);     // (only the launches that skip: logs of older trees stay comparable)
  } else if (n.find("sum_pairs_kernel") != std::string::npos) {
    fprintf(out(), "  part=%p n=%d sums=%p\n", *(void**)a[0], *(int*)a[1], *(void**)a[2]);
  } else if (n.find("sum_slabs_kernel") != std::string::npos) {
    fprintf(out(), "  slabs=%p slab_stride=%ld nslab=%d M=%d N4=%d ld=%ld C=%p ldc=%ld accumulate=%d\n", *(void**)a[0], *(long*)a[1], *(int*)a[2], *(int*)a[3], *(int*)a[4], *(long*)a[5],
            *(void**)a[6], *(long*)a[7], *(int*)a[8]);
  }
}
extern "C" {
hipError_t hipMemset2DAsync(void* p, size_t pitch, int v, size_t w, size_t h, hipStream_t st) { fprintf(out(), "memset2d %p pitch=%zu %d %zu x %zu\n", p, pitch, v, w, h); return hipSuccess; }
// the f16 product is internal to the library (evc_lstm_fwd.hip calls it): reached from Python through this wrapper only
int shim_gemm_nt_f16(const evc_f16* A, int64_t lda, const evc_f16* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, void* stream) {
  return gemm_nt_f16(A, lda, B, ldb, C, ldc, M, N, K, stream);
}
}

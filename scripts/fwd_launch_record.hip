// Recording stand-in for the HIP runtime, for scripts/fwd_launch_record.py: linked with a HOST-ONLY build of csrc/evc_lstm_fwd.hip in place of the
// runtime, it writes every enqueue the forward entries make to the file named by SHIM_LOG - memsets, LDS attributes, the hoisted products and every
// kernel launch with its geometry and each field of its GemmOperands / LstmFwdParams.  Nothing runs; no GPU is needed.
#include "launch_record_stubs.h"
struct LstmFwdParamsX {      // the layout of LstmFwdParams (defined in evc_lstm_fwd.hip itself)
  const float* zx; long ldzx; const float* bias; const int* len; int t; float* c_state; float* h_state; long ld_state;
  bf16_t* hout; bf16_t* hout_lo; uint2* gates; bf16_t* c_hist; const int* row_map; int M, H; int h_wide;
};
static void dump_p(const char* tag, const GemmOperands& p) {
  fprintf(out(), "  %s.p A1=%p lda1=%ld nk1=%d A2=%p lda2=%ld nk2=%d B=%p ldb=%ld gs=%ld M=%d Nu=%d A1lo=%p A2lo=%p Blo=%p B2=%p A3=%p lda3=%ld nk3=%d A4=%p lda4=%ld nk4=%d B8=%p ldb8=%ld s8=%d amax=%p a8=%d rs=%p ca=%p g2=%g gap=%ld\n",
          tag, (void*)p.A1, p.lda1, p.nk1, (void*)p.A2, p.lda2, p.nk2, (void*)p.B, p.ldb, p.group_stride, p.M, p.Nu, (void*)p.A1lo, (void*)p.A2lo, (void*)p.Blo, (void*)p.B2,
          (void*)p.A3, p.lda3, p.nk3, (void*)p.A4, p.lda4, p.nk4, (void*)p.B8, p.ldb8, p.scale8_exp, (void*)p.amax_ws, p.a8_hi_exp, (void*)p.row_scale, (void*)p.col_add, p.g2_add, p.b8_gap);
}
static void dump_e(const char* tag, const LstmFwdParamsX& e) {
  fprintf(out(), "  %s.e zx=%p ldzx=%ld bias=%p len=%p t=%d c=%p h=%p lds=%ld hout=%p hout_lo=%p gates=%p c_hist=%p row_map=%p M=%d H=%d h_wide=%d\n", tag, (void*)e.zx,
          e.zx ? e.ldzx : -1L, (void*)e.bias, (void*)e.len, e.t, (void*)e.c_state, (void*)e.h_state, e.ld_state, (void*)e.hout, (void*)e.hout_lo, (void*)e.gates, (void*)e.c_hist,
          (void*)e.row_map, e.M, e.H, e.h_wide);
}
static void dump_launch_args(const std::string& n, void** a) {
  if (n.find("walk2") != std::string::npos) {
    const int tma = *(int*)a[2], tmb = *(int*)a[5];
    fprintf(out(), "  tiles_ma=%d tiles_mb=%d tiles_n=%d\n", tma, tmb, *(int*)a[6]);
    if (tma) { dump_p("a", *(GemmOperands*)a[0]); dump_e("a", *(LstmFwdParamsX*)a[1]); }      // (an absent role's arguments are never read)
    if (tmb) { dump_p("b", *(GemmOperands*)a[3]); dump_e("b", *(LstmFwdParamsX*)a[4]); }
  } else if (n.find("pair") != std::string::npos) {
    fprintf(out(), "  tiles_m=%d tiles_n=%d\n", *(int*)a[4], *(int*)a[5]);
    dump_p("a", *(GemmOperands*)a[0]); dump_e("a", *(LstmFwdParamsX*)a[1]); dump_p("b", *(GemmOperands*)a[2]); dump_e("b", *(LstmFwdParamsX*)a[3]);
  } else {
    fprintf(out(), "  tiles_m=%d tiles_n=%d\n", *(int*)a[2], *(int*)a[3]);
    dump_p("s", *(GemmOperands*)a[0]); dump_e("s", *(LstmFwdParamsX*)a[1]);
  }
}
extern "C" {
int evc_gemm_nt(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K, const float* bias, int ob, int acc, void* st) {
  fprintf(out(), "evc_gemm_nt %p %ld %p %ld %p %ld %d %d %d %p %d %d\n", (void*)A, (long)lda, (void*)B, (long)ldb, C, (long)ldc, M, N, K, (void*)bias, ob, acc); return 0; }
int evc_gemm_nt_split(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, const float* bias, void* st) {
  fprintf(out(), "evc_gemm_nt_split %p %ld %p %ld %p %ld %d %d %d %p\n", (void*)A, (long)lda, (void*)B, (long)ldb, (void*)C, (long)ldc, M, N, K, (void*)bias); return 0; }
}
int gemm_nt_f16(const evc_f16* A, int64_t lda, const evc_f16* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, void* stream) {
  fprintf(out(), "gemm_nt_f16 %p %ld %p %ld %p %ld %d %d %d\n", (void*)A, (long)lda, (void*)B, (long)ldb, (void*)C, (long)ldc, M, N, K); return 0; }

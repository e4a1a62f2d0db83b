// TN products (weight gradients without transposes, LAB_NOTEBOOK.md 4.2b) and the fused MoE weight update (4.4b).
#include "gemm_shared.h"

// ===========================================================================
// TN GEMM: C[M,N] (+)= A^T . B with A [K][lda], B [K][ldb] (weight gradients without transposes)
// ===========================================================================
struct StoreParamsT {
  float* C; long ldc; int M, N;
  int row_il_H;                   // > 0: row m = u*4+g of the product is stored at row g*H+u (gate de-interleave)
  int accumulate, splits, ksteps_per_split;
  long slab_stride;               // > 0: split s stores its partial tile plainly at C + s*slab_stride (no atomics; the caller sums the slabs)
  int ksteps_per_split2;          // steps per split of the second column segment's tiles, which start at GemmOperandsT::k_skip2
};

template <class Cfg, bool SEG = false>
__global__ __launch_bounds__(Cfg::NT) void gemm_tn_kernel(GemmOperandsT p, StoreParamsT s, int tiles_m, int tiles_n) {
  const int nwg = tiles_m * tiles_n;
  int bid = blockIdx.x, split = 0;
  if (s.splits > 1) {
    split = bid / nwg;
    bid -= split * nwg;
  }
  const int id = xcd_remap(bid, nwg);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn, s.splits > 1 ? patch_rows(nwg, tiles_n) : 8);
  const int m0 = tm * Cfg::BM;
  int n0 = tn * Cfg::BU;
  int nb = n0;                                                 // first column within the B segment this workgroup reads
  int skip = 0, kps = s.ksteps_per_split;                      // this tile's first K step and its steps per split
  if (p.B2) {                                                  // two column segments (workgroup-uniform choice)
    if (n0 >= p.N1) {
      p.B = p.B2; p.ldb = p.ldb2; nb = n0 - p.N1; p.N = s.N - p.N1;
      s.N = p.c_col2 + p.N;                                    // the segment's columns in C: [c_col2, c_col2 + N2)
      n0 = p.c_col2 + nb;
      skip = p.k_skip2; kps = s.ksteps_per_split2;             // the segment's own (shorter) walk, split evenly over ITS steps: no split is empty
    } else {
      p.N = s.N = p.N1;
    }
  } else {
    skip = p.k_skip2;                                          // one segment (the slab entries; the other entries drop the steps on the host)
  }
  if (SEG) {                                                   // K steps are counted over the LIVE steps of the segments (evc_gemm_tn2_rows)
    int off = skip + split * kps, sg = 0;
    p.nk = min(kps, p.nk - off);
#pragma unroll
    for (int i = 0; i < 15; ++i) {                             // (constant indices: the table stays in scalar registers)
      const bool adv = sg == i && i + 1 < p.nseg && off >= (int)p.seg_len[i];
      off -= adv ? (int)p.seg_len[i] : 0;
      sg += adv ? 1 : 0;
    }
    p.seg0 = sg; p.seg_off0 = off;
  } else if (s.splits > 1 || skip) {
    // atomic joins: the tile's own steps [skip, nk) split evenly (kps of this segment).  Slabs (EVC_DETERMINISTIC): the ranges of the unskipped
    // walk, the skipped steps cut off their front - every slab then holds the bits it held without the skip (the cut products are exact zeros;
    // a range that is cut away whole stores zeros), and the fixed-order sum is bit-identical.
    const bool slabs = s.slab_stride > 0;
    const int k0 = slabs ? max(skip, split * s.ksteps_per_split) : skip + split * kps;
    const int k1 = slabs ? min((split + 1) * s.ksteps_per_split, p.nk) : min(k0 + kps, p.nk);
    p.A += (long)k0 * 32 * p.lda;
    p.B += (long)k0 * 32 * p.ldb;
    p.nk = k1 - k0;
  }
  f32x4 acc[Cfg::MI][1][Cfg::NI];
  gemm_mainloop_tn<Cfg, true, TN_LOOP_MODE, SEG>(p, m0, nb, lds_dyn, acc);      // transposed accumulators: lane = one row, 4 consecutive columns
  // Through the per-wave LDS transpose (store_tile_via_lds): whole sub-tile rows for the plain / slab stores, contiguous
  // row runs for the split-K atomics ("accumulate" is the same join onto what C already holds).
  float* C = s.C + split * s.slab_stride;
  const int wave = threadIdx.x >> 6, wc = wave % Cfg::WC;
  const bool plain = s.slab_stride > 0 || (s.splits == 1 && !s.accumulate);
  const bool aligned = (s.ldc % 4) == 0 && ((uintptr_t)C % 16) == 0 && n0 + wc * Cfg::WU + Cfg::WU <= s.N;
  __syncthreads();                                             // every wave has read its last ring slot
  if (plain && aligned) {
    store_tile_via_lds<Cfg, 4, false>(acc, lds_dyn, C, s.ldc, s.M, s.N, m0, n0, nullptr, s.row_il_H);
  } else if (s.splits == 1 && s.accumulate && aligned) {     // one workgroup per tile: C += tile needs no atomics
    store_tile_via_lds<Cfg, 4, false, true>(acc, lds_dyn, C, s.ldc, s.M, s.N, m0, n0, nullptr, s.row_il_H);
  } else if (plain) {            // ragged right edge / unaligned rows: element-wise
    TileCoordsT<Cfg> tc;
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      const int m = m0 + tc.row0 + mi * 16;
      if (m >= s.M) continue;
      const long mo = s.row_il_H > 0 ? (long)(m & 3) * s.row_il_H + (m >> 2) : m;
#pragma unroll
      for (int ni = 0; ni < Cfg::NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + tc.unit0 + ni * 16 + r;
          if (n < s.N) C[mo * s.ldc + n] = acc[mi][0][ni][r];
        }
    }
  } else {
    store_tile_via_lds<Cfg, 4, true>(acc, lds_dyn, C, s.ldc, s.M, s.N, m0, n0, nullptr, s.row_il_H);
  }
}

// ---- host side: every entry is its own refusals, then tn_operands, the tile / split choice, launch_tn ----
// The refusals the product entries share, in the order every entry has made them, worded with the entry the caller used.  nslab: the K split of
// the slab entries; slabs_ok: their slab image's rule.
static int tn_args_ok(const char* entry, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, int row_interleave_H,
                      int N1, const void* B2, int64_t ldb2, int c_col2, int nslab = 1, bool slabs_ok = true) {
  EVC_REQUIRE(M >= 8 && N >= 8 && K > 0 && M % 8 == 0 && N % 8 == 0 && K % 32 == 0, EVC_ERR_BAD_SHAPE,
              "%s: needs M %% 8 == 0, N %% 8 == 0, K %% 32 == 0 (M=%d N=%d K=%d)", entry, M, N, K);
  EVC_REQUIRE(nslab >= 1 && nslab <= K / 32, EVC_ERR_BAD_SHAPE, "%s: needs 1 <= nslab <= K/32 (K=%d nslab=%d)", entry, K, nslab);
  EVC_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, EVC_ERR_BAD_ALIGN,
              "%s: operands must be 16-byte aligned (lda=%ld ldb=%ld)", entry, (long)lda, (long)ldb);
  EVC_REQUIRE(slabs_ok, EVC_ERR_BAD_ALIGN, "%s: slabs == NULL or slab_stride < M * ldc", entry);
  EVC_REQUIRE(row_interleave_H == 0 || M == 4 * row_interleave_H, EVC_ERR_BAD_SHAPE, "%s: row_interleave_H needs M == 4*H", entry);
  EVC_REQUIRE(!B2 || (N1 > 0 && N1 < N && N1 % 256 == 0 && ldb2 % 8 == 0 && ((uintptr_t)B2 % 16) == 0 && c_col2 >= N1), EVC_ERR_BAD_SHAPE,
              "%s: N1=%d must be a multiple of 256 inside (0, N=%d), B2 16-byte aligned with ldb2 %% 8 == 0, c_col2=%d >= N1", entry, N1, N, c_col2);
  EVC_REQUIRE((long)ceil_div(K / 32, nslab) * (nslab - 1) < K / 32, EVC_ERR_BAD_SHAPE, "%s: nslab=%d leaves an empty slab at K=%d", entry, nslab, K);
  return EVC_OK;
}

// operands of C = A^T . B over K rows, B2 != NULL: with a second column segment behind the first N1 columns
static inline GemmOperandsT tn_operands(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, int M, int N, int K,
                                        int N1 = 0, const evc_bf16* B2 = nullptr, int64_t ldb2 = 0, int c_col2 = 0) {
  GemmOperandsT p{A, lda, B, ldb, M, N, K / 32};
  if (B2) { p.B2 = B2; p.ldb2 = ldb2; p.N1 = N1; p.c_col2 = c_col2; }
  return p;
}

// live rows per time slab (evc_gemm_tn2_rows): the K walk covers ceil(rows / 32) steps of every slab.  Fills p's segment table and sets p.nk to the
// live steps; false with more than 16 non-empty slabs, nothing dead or nothing live: the plain walk over all K rows (the dead rows of A are
// zeros: the same sums), which ignores what the table holds by then.
static bool tn_live_segments(GemmOperandsT& p, int K, int slab_rows, const int32_t* rows_per_slab) {
  if (slab_rows % 32 != 0 || K % slab_rows != 0) return false;
  const int nslabs = K / slab_rows, slab_steps = slab_rows / 32;
  // the segment walk indexes both operands by 32-bit BYTE offsets from their un-advanced bases (gemm_core_tn.h: (start + off) * 64 * ld): the
  // last K row must stay below 4 GiB in the wider operand - beyond that the plain walk (which advances the base pointers per split) runs
  const long ld_max = p.lda > p.ldb ? p.lda : p.ldb;
  if ((long)nslabs * slab_steps >= 65536 || (long)K * (p.B2 && p.ldb2 > ld_max ? p.ldb2 : ld_max) * 2 >= (1L << 32)) return false;
  int n = 0, total = 0;
  for (int t = 0; t < nslabs; ++t) {
    const int r = rows_per_slab[t] < 0 ? 0 : (rows_per_slab[t] > slab_rows ? slab_rows : rows_per_slab[t]);
    const int steps = (r + 31) / 32;
    if (steps == 0) continue;
    if (n == 16) return false;
    p.seg_start[n] = (unsigned short)(t * slab_steps); p.seg_len[n] = (unsigned short)steps;
    ++n; total += steps;
  }
  if (total == 0 || total >= K / 32) return false;
  p.nseg = n; p.nk = total;
  return true;
}

// one launch of tm x tn tiles x s.splits K ranges; seg: on the kernel that walks p's live segments
template <class Cfg>
static int launch_tn(const GemmOperandsT& p, StoreParamsT s, bool seg, int tm, int tn, hipStream_t st) {
  s.ksteps_per_split = ceil_div(p.nk, s.splits);
  s.ksteps_per_split2 = p.k_skip2 && !s.slab_stride ? ceil_div(p.nk - p.k_skip2, s.splits) : s.ksteps_per_split;
  if (seg) launch_cfg<Cfg>(gemm_tn_kernel<Cfg, true>, tm * tn * s.splits, st, p, s, tm, tn);
  else launch_cfg<Cfg>(gemm_tn_kernel<Cfg>, tm * tn * s.splits, st, p, s, tm, tn);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// tile ids of the TN products, as EVC_FORCE_TILE names them
enum TnTileId { TN_TILE_256 = 1, TN_TILE_128 = 11 };
struct TnPlan { int tile, tm, tn, splits; bool seg; };

// The plan of one product: tile, tile grid, K splits, and whether the K walk follows live segments.  A pure function of the shapes, the row table,
// the skip and the two process-wide switches - evc_gemm_tn_plan answers with it, gemm_tn_impl launches by it.  Finishes p: segment table and live
// step count, and the skip - k_skip leading K steps (of 32 operand rows) that the LAST column segment does not walk: as k_skip2 for the second of
// two segments, by dropping the steps from a single segment's walk here.
static TnPlan tn_plan(GemmOperandsT& p, int M, int N, int K, int slab_rows, const int32_t* rows_per_slab, int k_skip) {
  TnPlan pl;
  pl.seg = rows_per_slab && slab_rows > 0 && !evc_deterministic() && tn_live_segments(p, K, slab_rows, rows_per_slab);
  K = p.nk * 32;                                 // (the live rows)
  int skip = k_skip;                             // ... in steps of the walk: the live steps below operand step k_skip
  if (pl.seg) {
    skip = 0;
    for (int i = 0; i < p.nseg; ++i) skip += max(0, min((int)p.seg_len[i], k_skip - (int)p.seg_start[i]));
  }
  int nk_short = p.nk - skip;                    // the shorter walk: it decides the splits (>= 32 steps each in every tile)
  if (p.B2) {
    p.k_skip2 = skip;
  } else if (skip) {
    if (pl.seg) {
      int i = 0, n = 0;
      while (i < p.nseg && skip >= (int)p.seg_len[i]) skip -= p.seg_len[i++];
      for (; i < p.nseg; ++i, ++n, skip = 0) {
        p.seg_start[n] = (unsigned short)(p.seg_start[i] + skip); p.seg_len[n] = (unsigned short)(p.seg_len[i] - skip);
      }
      for (i = n; i < 16; ++i) p.seg_start[i] = p.seg_len[i] = 0;
      p.nseg = n;
    } else {
      p.A += (long)skip * 32 * p.lda;
      p.B += (long)skip * 32 * p.ldb;
    }
    p.nk = nk_short;
  }
  const int tm1 = ceil_div(M, 128), tn1 = ceil_div(N, 128);
  // short contractions (the student's L2: K = 5 x 256 rows) on 128x128 tiles without split-K: the atomic join of
  // 256x256 partial tiles costs more than the product itself there (81 -> 36 us at 4096 x 1024 x 1280); from
  // K ~ 5000 on the 256x256 split-K form is faster again (92 vs 99 us)
  const bool short128 = forced_tile() == 11 || (forced_tile() == 0 && K <= 2048 && (long)tm1 * tn1 >= 192);
  // a narrow strip (N <= 128: the last 128 input columns of an L1 layer-0 kernel gradient, see engine._wgrad_tn): 128x128 tiles,
  // K split until ~256 workgroups exist - a 256-column tile would do half of its MFMAs on columns that do not exist
  const bool strip128 = !short128 && forced_tile() == 0 && N <= 128 && !p.B2;
  const bool tile128 = short128 || strip128;
  const int tm = tile128 ? tm1 : ceil_div(M, CfgPlainV2::BM), tn = short128 ? tn1 : strip128 ? 1 : ceil_div(N, CfgPlainV2::BU);
  // K splits joined by atomics until ~256 workgroups exist, >= 32 K steps each - counted on the shorter walk - and none empty in either
  // walk; none with EVC_DETERMINISTIC
  pl.splits = 1;
  if (!short128 && !evc_deterministic()) {
    pl.splits = split_k(256 / (tm * tn), nk_short, 32);
    while (pl.splits > 1 && (long)ceil_div(p.nk, pl.splits) * (pl.splits - 1) >= p.nk) --pl.splits;
  }
  pl.tile = tile128 ? TN_TILE_128 : TN_TILE_256;
  pl.tm = tm; pl.tn = tn;
  return pl;
}

static int gemm_tn_impl(const char* entry, const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, int N1, const evc_bf16* B2, int64_t ldb2,
                        int c_col2, float* C, int64_t ldc, int M, int N, int K, int row_interleave_H, int accumulate, void* stream,
                        int slab_rows = 0, const int32_t* rows_per_slab = nullptr, int k_skip = 0) {
  EVC_TRY(tn_args_ok(entry, A, lda, B, ldb, M, N, K, row_interleave_H, N1, B2, ldb2, c_col2));
  EVC_REQUIRE(k_skip >= 0 && k_skip <= K / 32, EVC_ERR_BAD_ARG, "%s: k_skip=%d outside [0, K/32=%d]", entry, k_skip, K / 32);
  hipStream_t st = (hipStream_t)stream;
  GemmOperandsT p = tn_operands(A, lda, B, ldb, M, N, K, N1, B2, ldb2, c_col2);
  const TnPlan pl = tn_plan(p, M, N, K, slab_rows, rows_per_slab, k_skip);
  StoreParamsT s{C, ldc, M, N, row_interleave_H, accumulate, pl.splits, 0, 0};
  if (s.splits > 1 && !accumulate) EVC_CHECK_HIP(hipMemset2DAsync(C, ldc * sizeof(float), 0, (size_t)N * sizeof(float), M, st));
  return pl.tile == TN_TILE_128 ? launch_tn<CfgTn128>(p, s, pl.seg, pl.tm, pl.tn, st) : launch_tn<CfgPlainV2>(p, s, pl.seg, pl.tm, pl.tn, st);
}

// evc_gemm_tn / evc_gemm_tn2 over TIME SLABS with a live prefix (round 5): the contraction index runs over K = nslabs * slab_rows rows, slab t
// holding rows_per_slab[t] live rows at its start (row plans: rows sorted by length, the weight-gradient products dW^T = dz^T . [x | h] of a
// row-planned LSTM level) - the K walk covers ceil(rows / 32) steps of every slab and jumps over the rest (the teacher's L1 level: 5 % of
// the rows).  The skipped rows of A must be zeros or the skipped rows of A and B finite garbage that the caller does not want summed; rows
// between rows_per_slab[t] and the next multiple of 32 ARE contracted.  B2 == NULL: one column segment of N1 columns.  rows_per_slab is HOST
// memory (read before the launch).  More than 16 non-empty slabs or EVC_DETERMINISTIC: the plain product over all K rows.
extern "C" int evc_gemm_tn2_rows(const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                                 int N2, int c_col2, float* C, int64_t ldc, int M, int slab_rows, int nslabs, const int32_t* rows_per_slab,
                                 int row_interleave_H, int accumulate, void* stream) {
  EVC_REQUIRE(B1 && N1 > 0 && slab_rows > 0 && nslabs > 0 && rows_per_slab && (long)slab_rows * nslabs < (1L << 31), EVC_ERR_BAD_ARG,
              "evc_gemm_tn2_rows: B1, N1, slab_rows, nslabs, rows_per_slab are required");
  EVC_REQUIRE(!B2 || N2 > 0, EVC_ERR_BAD_ARG, "evc_gemm_tn2_rows: N2=%d", N2);
  EVC_REQUIRE(!B2 || accumulate || c_col2 == N1, EVC_ERR_BAD_ARG, "evc_gemm_tn2_rows: segments that are not adjacent in C (c_col2=%d, N1=%d) need accumulate", c_col2, N1);
  return gemm_tn_impl("evc_gemm_tn2_rows", A, lda, B1, ldb1, B2 ? N1 : 0, B2, ldb2, B2 ? c_col2 : 0, C, ldc, M, N1 + (B2 ? N2 : 0), slab_rows * nslabs,
                      row_interleave_H, accumulate, stream, slab_rows, rows_per_slab);
}

// The products of evc_gemm_tn / evc_gemm_tn2 / evc_gemm_tn2_rows with a SKIP: the last column segment (B2, or B1 when B2 == NULL) does not walk the
// first k_skip K steps of 32 operand rows, because the caller knows those rows of it to be zeros (h_prev's slab 0 = h_-1 of the weight-gradient
// products): the same sums without the products that add nothing.  rows_per_slab == NULL: the plain walk over all slab_rows * nslabs rows.
static int tn_skip_args_ok(const char* entry, const void* B1, int N1, const void* B2, int N2, int c_col2, int slab_rows, int nslabs, int accumulate) {
  EVC_REQUIRE(B1 && N1 > 0 && slab_rows > 0 && nslabs > 0 && (long)slab_rows * nslabs < (1L << 31), EVC_ERR_BAD_ARG, "%s: B1, N1, slab_rows, nslabs are required", entry);
  EVC_REQUIRE(!B2 || N2 > 0, EVC_ERR_BAD_ARG, "%s: N2=%d", entry, N2);
  EVC_REQUIRE(!B2 || accumulate || c_col2 == N1, EVC_ERR_BAD_ARG, "%s: segments that are not adjacent in C (c_col2=%d, N1=%d) need accumulate", entry, c_col2, N1);
  return EVC_OK;
}
extern "C" int evc_gemm_tn2_rows_skip(const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                                      int N2, int c_col2, float* C, int64_t ldc, int M, int slab_rows, int nslabs, const int32_t* rows_per_slab,
                                      int k_skip, int row_interleave_H, int accumulate, void* stream) {
  EVC_TRY(tn_skip_args_ok("evc_gemm_tn2_rows_skip", B1, N1, B2, N2, c_col2, slab_rows, nslabs, accumulate));
  return gemm_tn_impl("evc_gemm_tn2_rows_skip", A, lda, B1, ldb1, B2 ? N1 : 0, B2, ldb2, B2 ? c_col2 : 0, C, ldc, M, N1 + (B2 ? N2 : 0), slab_rows * nslabs,
                      row_interleave_H, accumulate, stream, slab_rows, rows_per_slab, k_skip);
}

// What evc_gemm_tn2_rows_skip (and, with k_skip = 0, evc_gemm_tn / evc_gemm_tn2 / evc_gemm_tn2_rows) would launch for these arguments: *tile = 1 (256 x 256)
// or 11 (128 x 128), *splits = the K ranges joined by atomics, *live_walk = 1 when the K walk follows the live segments of rows_per_slab and reads no row
// of a slab from round_up(rows, 32) on (0: the plain walk over every row).  splits == 1: one workgroup per tile - with accumulate = 0 the launch stores plainly and
// is the sole writer of its columns, which the caller then need not zero.  The launch's own choice (tn_plan), asked without enqueueing anything.
extern "C" int evc_gemm_tn_plan(int64_t lda, int64_t ldb1, int N1, int64_t ldb2, int N2, int M, int slab_rows, int nslabs, const int32_t* rows_per_slab,
                                int k_skip, int* tile, int* splits, int* live_walk) {
  EVC_REQUIRE(tile && splits && live_walk, EVC_ERR_BAD_ARG, "evc_gemm_tn_plan: tile, splits and live_walk are required");
  const bf16_t* const some = (const bf16_t*)(uintptr_t)16;      // operands are never read here: an aligned stand-in address
  const bf16_t* const B2 = N2 > 0 ? some : nullptr;
  EVC_TRY(tn_skip_args_ok("evc_gemm_tn_plan", some, N1, B2, N2, N1, slab_rows, nslabs, 1));
  const int N = N1 + (B2 ? N2 : 0), K = slab_rows * nslabs;
  EVC_TRY(tn_args_ok("evc_gemm_tn_plan", some, lda, some, ldb1, M, N, K, 0, B2 ? N1 : 0, B2, ldb2, B2 ? N1 : 0));
  EVC_REQUIRE(k_skip >= 0 && k_skip <= K / 32, EVC_ERR_BAD_ARG, "evc_gemm_tn_plan: k_skip=%d outside [0, K/32=%d]", k_skip, K / 32);
  GemmOperandsT p = tn_operands(some, lda, some, ldb1, M, N, K, B2 ? N1 : 0, B2, ldb2, B2 ? N1 : 0);
  const TnPlan pl = tn_plan(p, M, N, K, slab_rows, rows_per_slab, k_skip);
  *tile = pl.tile;
  *splits = pl.splits;
  *live_walk = pl.seg ? 1 : 0;
  return EVC_OK;
}

extern "C" int evc_gemm_tn(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, float* C, int64_t ldc,
                           int M, int N, int K, int row_interleave_H, int accumulate, void* stream) {
  return gemm_tn_impl("evc_gemm_tn", A, lda, B, ldb, 0, nullptr, 0, 0, C, ldc, M, N, K, row_interleave_H, accumulate, stream);
}

extern "C" int evc_gemm_tn2(const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                            int N2, int c_col2, float* C, int64_t ldc, int M, int K, int row_interleave_H, int accumulate, void* stream) {
  EVC_REQUIRE(B1 && B2 && N1 > 0 && N2 > 0, EVC_ERR_BAD_ARG, "evc_gemm_tn2: two column segments are required");
  EVC_REQUIRE(accumulate || c_col2 == N1, EVC_ERR_BAD_ARG, "evc_gemm_tn2: segments that are not adjacent in C (c_col2=%d, N1=%d) need accumulate "
              "(the split-K join adds into a C the caller has zeroed)", c_col2, N1);
  return gemm_tn_impl("evc_gemm_tn2", A, lda, B1, ldb1, N1, B2, ldb2, c_col2, C, ldc, M, N1 + N2, K, row_interleave_H, accumulate, stream);
}

// Two column segments into slabs (EVC_DETERMINISTIC=1 weight gradients, round 5): evc_gemm_tn2's product with the K split stored as nslab plain partial
// images instead of joined with atomics - slab s at slabs + s*slab_stride, each an [M][ldc] image like C (rows de-interleaved, the second segment
// at column c_col2) - that evc_sum_slabs adds in slab order.  B2 == NULL: one segment of N1 columns.
static int gemm_tn_slabs_impl(const char* entry, const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                              int N2, int c_col2, float* slabs, int64_t ldc, int64_t slab_stride, int M, int K, int row_interleave_H, int nslab, void* stream,
                              int k_skip = 0) {
  const int N = N1 + (B2 ? N2 : 0);
  EVC_REQUIRE(N1 >= 8, EVC_ERR_BAD_SHAPE, "%s: N1=%d", entry, N1);
  EVC_TRY(tn_args_ok(entry, A, lda, B1, ldb1, M, N, K, row_interleave_H, N1, B2, ldb2, c_col2, nslab, slabs && slab_stride >= (int64_t)M * ldc));
  // the last segment's walk without its first k_skip steps (see evc_gemm_tn2_rows_skip), the slab ranges unchanged (gemm_tn_kernel): same bits
  EVC_REQUIRE(k_skip >= 0 && k_skip <= K / 32, EVC_ERR_BAD_ARG, "%s: k_skip=%d outside [0, K/32=%d]", entry, k_skip, K / 32);
  GemmOperandsT p = tn_operands(A, lda, B1, ldb1, M, N, K, N1, B2, ldb2, c_col2);
  p.k_skip2 = k_skip;
  return launch_tn<CfgPlainV2>(p, StoreParamsT{slabs, ldc, M, N, row_interleave_H, 0, nslab, 0, slab_stride},
                               false, ceil_div(M, CfgPlainV2::BM), ceil_div(N, CfgPlainV2::BU), (hipStream_t)stream);
}
extern "C" int evc_gemm_tn2_slabs_skip(const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                                       int N2, int c_col2, float* slabs, int64_t ldc, int64_t slab_stride, int M, int K, int k_skip, int row_interleave_H,
                                       int nslab, void* stream) {
  return gemm_tn_slabs_impl("evc_gemm_tn2_slabs_skip", A, lda, B1, ldb1, N1, B2, ldb2, N2, c_col2, slabs, ldc, slab_stride, M, K, row_interleave_H, nslab, stream,
                            k_skip);
}
extern "C" int evc_gemm_tn2_slabs(const evc_bf16* A, int64_t lda, const evc_bf16* B1, int64_t ldb1, int N1, const evc_bf16* B2, int64_t ldb2,
                                  int N2, int c_col2, float* slabs, int64_t ldc, int64_t slab_stride, int M, int K, int row_interleave_H,
                                  int nslab, void* stream) {
  return gemm_tn_slabs_impl("evc_gemm_tn2_slabs", A, lda, B1, ldb1, N1, B2, ldb2, N2, c_col2, slabs, ldc, slab_stride, M, K, row_interleave_H, nslab, stream);
}
// Split-K into slabs: slab s (s < nslab) = the partial product over K rows [s*ceil(K/32/nslab)*32, ...), stored plainly at
// slabs + s*M*N (row stride N).  For products whose 256x256 tiles do not fill the chip and whose result is read once by a
// pass that can add the slabs on the way (DBoF cluster-weight gradient: 8192 x 1152 x 16384 = 160 tiles): no atomics, no memset.
extern "C" int evc_gemm_tn_slabs(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, float* slabs, int M, int N, int K,
                                 int nslab, void* stream) {
  return gemm_tn_slabs_impl("evc_gemm_tn_slabs", A, lda, B, ldb, N, nullptr, 0, 0, 0, slabs, N, (int64_t)M * N, M, K, 0, nslab, stream);
}

// C[r][c] (+)= sum over slabs s, in slab order, of slabs[s*slab_stride + r*ld + c] for r < M, c < N (N % 4 == 0, 16-byte aligned rows)
__global__ __launch_bounds__(256) void sum_slabs_kernel(const float* __restrict__ slabs, long slab_stride, int nslab, int M, int N4, long ld,
                                                        float* __restrict__ C, long ldc, int accumulate) {
  const long n = (long)M * N4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / N4, c = (i - r * N4) * 4;
    float4 a = accumulate ? *(const float4*)(C + r * ldc + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < nslab; ++s) {
      const float4 v = *(const float4*)(slabs + s * slab_stride + r * ld + c);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    *(float4*)(C + r * ldc + c) = a;
  }
}
extern "C" int evc_sum_slabs(const float* slabs, int64_t slab_stride, int nslab, int M, int N, int64_t ld, float* C, int64_t ldc, int accumulate,
                             void* stream) {
  EVC_REQUIRE(slabs && C && nslab >= 1 && M > 0 && N > 0 && N % 4 == 0 && ld % 4 == 0 && ldc % 4 == 0 && slab_stride % 4 == 0 &&
              ((uintptr_t)slabs % 16) == 0 && ((uintptr_t)C % 16) == 0, EVC_ERR_BAD_SHAPE, "evc_sum_slabs: N, ld, ldc, slab_stride multiples of 4, 16-byte aligned");
  const long n = (long)M * (N / 4);
  long nb = (n + 255) / 256;
  nb = nb > 2048 ? 2048 : nb;
  hipLaunchKernelGGL(sum_slabs_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, slabs, (long)slab_stride, nslab, M, N / 4, (long)ld, C, (long)ldc,
                     accumulate);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ===========================================================================
// MoE weight update without materialising the gradient.
// The gradient of a MoE weight matrix W [V][K] (stored as the forward GEMM's B operand) is the outer
// product dlogits^T . x over the batch rows: rank = batch.  Writing it (4 B/param), reading it for the
// norm (4+4) and again for Adam, then transposing the updated weights for the backward shadow costs 46
// bytes per parameter of HBM traffic for 96.6 M parameters per tower.  Here the [256 x 256] gradient tile is
// recomputed from the factors (8 K steps of the TN loop) in each of two passes:
//   pass 1: sum (g + l2 p)^2 and sum p^2 per workgroup -> partials (summed in a fixed order afterwards)
//   pass 2: per-tensor clip + TF-Adam in the epilogue: reads p, m, v, writes p, m, v, the bf16 forward
//           shadow and - through an LDS transpose - the bf16 transposed shadow: 30 bytes per parameter.
//           The epilogue runs ROW-MAJOR over the tile (the gradient tile changes layout through the idle ring): every global
//           access of a wave covers whole rows of the tile.  From the transposed accumulator layout one instruction touched 16
//           rows with 64 bytes each (half a 128-byte line): 368 -> 273 us on the gates matrix, 257 -> 188 us on the experts
//           matrix, same bits (profiles/moe_update_lines_ab.txt).
// Under data parallelism the factors of all ranks are all-gathered (14 MB per rank) instead of all-reducing
// the 386 MB gradient; the contraction then simply runs over world x batch rows.
// ===========================================================================
struct MoeUpdateParams {
  float* p; float* m; float* v;        // [V][K] f32, row stride K
  bf16_t* p_bf16;                      // forward shadow [V][K], or NULL (round 5: a "high" tower's forward reads the f16 + e4m3 images, not this one)
  bf16_t* pT_bf16; long ldT;           // transposed shadow [K][ldT], ldT >= V, or NULL (plain bf16 form: the backward reads p_bf16)
  bf16_t* p_wide;                      // or NULL: wide split-bf16 image [V][2K] = [hi | lo] of the new weights (the "split" forward's operand)
  bf16_t* p_f16; uint8_t* p_fp8;       // or NULL: IEEE f16 image [V][K] and e4m3 image [V][2K] = [e4m3((w - f16(w)) lo_scale) | e4m3(w hi_scale)] of the
  float lo_scale, hi_scale;            // new weights (the "high" forward's operands: evc_gemm_nt_f16_fp8)
  float* partial;                      // pass 1 out: [workgroups][2]
  float* wsq_partial;                  // or NULL; pass 2 out: [workgroups][2] = {sum of the new weights squared, 0}
  const float* sums;                   // pass 2 in: sums[0] = sum (g + l2 p)^2 of this tensor
  int V, K;
  float l2, clip, lr_t, b1, b2, eps;
};

// W, m, v of the fused MoE update - read once, written once, 5.9 GB per step - as non-temporal accesses (round 5: same box, alternated three times,
// 10.00 -> 9.93 ms per step); the bf16 shadows stay plain - they are read again soon (non-temporal too: 9.82 -> 9.93)
__device__ __forceinline__ float4 ld_stream_moe(const float* p) {
  const f32x4 v = __builtin_nontemporal_load((const f32x4*)p);
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st_stream_moe(float* p, float a, float b, float c, float d) {
  __builtin_nontemporal_store(f32x4{a, b, c, d}, (f32x4*)p);
}
// (m and v asked for ahead of the factor product like p - 219 VGPRs, still one workgroup per CU - measured 459-462 / 309-316 us against
//  442-456 / 302-305: nothing, the pass is not waiting for those loads)
template <class Cfg, int PASS>
__global__ __launch_bounds__(Cfg::NT, 2) void moe_update_kernel(GemmOperandsT p, MoeUpdateParams u, int tiles_m, int tiles_n) {
  const int nwg = tiles_m * tiles_n;
  const int id = xcd_remap(blockIdx.x, nwg);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * Cfg::BM, n0 = tn * Cfg::BU;
  f32x4 acc[Cfg::MI][1][Cfg::NI];
  TileCoordsT<Cfg> tc;
  const int K = u.K;
  // Epilogue loads first, all of them (the stores of one fragment and the loads of the next go to the same
  // arrays, so hipcc keeps them in program order and every fragment would wait for the previous one's stores:
  // 8 x (load latency + store acknowledge) per workgroup; issued up front they overlap - 3.4 -> see DESIGN.md).
  // The weights themselves are asked for BEFORE the factor product: they do not depend on it, and their HBM
  // latency then runs under the 8-step loop instead of after it.
  // PASS 1 reads them in the accumulator layout (its sums run in that order); PASS 2 reads, computes and writes ROW-MAJOR: thread t
  // owns, in round i, the 4 consecutive k at (row i * RROWS + t / LPR, column (t % LPR) * 4) of the tile, so a wave-instruction covers
  // whole rows of the tile - 512 contiguous bytes of p, m, v, 256 of a bf16 image - instead of 16 rows x 64 bytes.
  constexpr int LPR = Cfg::BU / 4, RROWS = Cfg::NT / LPR, ROUNDS = Cfg::BM / RROWS;   // 32 lanes per row, 16 rows per round, 8 rounds
  static_assert(Cfg::MI * Cfg::NI == ROUNDS && Cfg::NT % LPR == 0 && Cfg::BM % RROWS == 0, "row-major rounds must cover the tile");
  const int rrow = threadIdx.x / LPR, rcol = (threadIdx.x % LPR) * 4;
  float4 pv[Cfg::MI * Cfg::NI];
#pragma unroll
  for (int mi = 0; mi < Cfg::MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < Cfg::NI; ++ni) {
      const int i = mi * Cfg::NI + ni;
      const int vr = PASS == 1 ? m0 + tc.row0 + mi * 16 : m0 + i * RROWS + rrow, k = PASS == 1 ? n0 + tc.unit0 + ni * 16 : n0 + rcol;
      pv[i] = (vr < u.V && k < K) ? ld_stream_moe(u.p + (long)vr * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  gemm_mainloop_tn<Cfg, true>(p, m0, n0, lds_dyn, acc);
  if (PASS == 1) {
    float sg = 0.f, sp = 0.f;
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      const int vr = m0 + tc.row0 + mi * 16;
#pragma unroll
      for (int ni = 0; ni < Cfg::NI; ++ni) {
        const int k = n0 + tc.unit0 + ni * 16;
        if (vr >= u.V || k >= K) continue;
        const float4 pq = pv[mi * Cfg::NI + ni];
        const float pa[4] = {pq.x, pq.y, pq.z, pq.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w = acc[mi][0][ni][r] + u.l2 * pa[r];
          sg += w * w;
          sp += pa[r] * pa[r];
        }
      }
    }
    sg = wave_sum(sg);
    sp = wave_sum(sp);
    __syncthreads();                                   // the LDS ring is free now
    float* red = (float*)lds_dyn;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave * 2] = sg; red[wave * 2 + 1] = sp; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float a = 0.f, b = 0.f;
      for (int w = 0; w < Cfg::NT / 64; ++w) { a += red[w * 2]; b += red[w * 2 + 1]; }
      u.partial[2 * blockIdx.x] = a;
      u.partial[2 * blockIdx.x + 1] = b;
    }
    return;
  }
  float4 mv[ROUNDS], vv[ROUNDS];
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i) {
    const int vr = m0 + i * RROWS + rrow, k = n0 + rcol;
    const bool ok = vr < u.V && k < K;
    mv[i] = ok ? ld_stream_moe(u.m + (long)vr * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    vv[i] = ok ? ld_stream_moe(u.v + (long)vr * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float scale = 1.f;
  if (u.clip > 0.f) scale = u.clip / fmaxf(sqrtf(u.sums[0]), u.clip);      // tf.clip_by_norm
  float wsq = 0.f;                                     // sum of the NEW weights squared (the next update's |W|^2: evc_moe_grad_norms)
  // The gradient tile changes layout through the (idle) ring, one wave row (WM tile rows) at a time: its waves lay their accumulators
  // down as an f32 image gbuf [WM][GP], all waves pick them up row-major, and - for wsq, whose sum keeps its accumulator-layout order -
  // put the new weights back in the same places for the owners to read.  The bf16 transpose image [BU k][BM v] sits behind gbuf.
  constexpr int GP = Cfg::BU + 4;                      // floats per gbuf row (+16 B: bank spread, as in store_tile_via_lds)
  constexpr int TP = Cfg::BM + 2;                      // bf16 per k row of the transpose image: 65 dwords, so the 4 k of a lane and the 32
                                                       // lanes of a row spread over the banks (a multiple of 4 dwords puts them on two)
  constexpr int G_BYTES = Cfg::WM * GP * 4, T_BYTES = Cfg::BU * TP * 2;
  static_assert(G_BYTES % 16 == 0 && T_BYTES % 4 == 0 && G_BYTES + T_BYTES + (Cfg::NT / 64) * 4 <= Cfg::LDS_BYTES, "staging must fit the ring");
  static_assert(Cfg::WM % RROWS == 0 && Cfg::WR * Cfg::WM == Cfg::BM, "a wave row is a whole number of row-major rounds");
  constexpr int RPH = Cfg::WM / RROWS;                 // rounds per wave row
  float* gbuf = (float*)lds_dyn;
  bf16_t* tile = (bf16_t*)(lds_dyn + G_BYTES);
  float* red = (float*)(lds_dyn + G_BYTES + T_BYTES);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / Cfg::WC;
  const int arow = lane & 15;                          // accumulator layout inside gbuf: row mi * 16 + arow, columns tc.unit0 + ni * 16 ..
#pragma unroll
  for (int h = 0; h < Cfg::WR; ++h) {
    __syncthreads();                                   // h == 0: every wave is done with the ring; later: gbuf has been read
    if (wr == h) {
#pragma unroll
      for (int mi = 0; mi < Cfg::MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < Cfg::NI; ++ni) {
          const f32x4 a = acc[mi][0][ni];
          *(float4*)(gbuf + (mi * 16 + arow) * GP + tc.unit0 + ni * 16) = make_float4(a[0], a[1], a[2], a[3]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPH; ++j) {
      const int i = h * RPH + j;
      const int vl = i * RROWS + rrow, vr = m0 + vl, k = n0 + rcol;
      float* gp = gbuf + (j * RROWS + rrow) * GP + rcol;
      bf16_t pb[4] = {0, 0, 0, 0};
      if (vr < u.V && k < K) {
        const long o = (long)vr * K + k;
        const float4 gq = *(const float4*)gp;
        const float ga[4] = {gq.x, gq.y, gq.z, gq.w};
        const float pa[4] = {pv[i].x, pv[i].y, pv[i].z, pv[i].w};
        const float ma[4] = {mv[i].x, mv[i].y, mv[i].z, mv[i].w};
        const float va[4] = {vv[i].x, vv[i].y, vv[i].z, vv[i].w};
        float pn[4], mn[4], vn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                 // same operation order as clip_adam_kernel
          const float gc = (ga[r] + u.l2 * pa[r]) * scale;
          mn[r] = u.b1 * ma[r] + (1.f - u.b1) * gc;
          vn[r] = u.b2 * va[r] + (1.f - u.b2) * gc * gc;
          pn[r] = adam_step_(pa[r], mn[r], vn[r], u.lr_t, u.eps);
          pb[r] = f32_to_bf16(pn[r]);
        }
        st_stream_moe(u.p + o, pn[0], pn[1], pn[2], pn[3]);
        st_stream_moe(u.m + o, mn[0], mn[1], mn[2], mn[3]);
        st_stream_moe(u.v + o, vn[0], vn[1], vn[2], vn[3]);
        if (u.wsq_partial) *(float4*)gp = make_float4(pn[0], pn[1], pn[2], pn[3]);
        if (u.p_bf16) {
          const u32x2_t sb = {(uint32_t)pb[0] | ((uint32_t)pb[1] << 16), (uint32_t)pb[2] | ((uint32_t)pb[3] << 16)};
          *(u32x2_t*)(u.p_bf16 + o) = sb;
        }
        if (u.p_f16) {                                // f16 + e4m3 images: saves the passes over the f32 weights (evc_cast_f32_to_f16 / _fp8_lo) per update
          const uint32_t h01 = pack_f16x2_hw(pn[0], pn[1]), h23 = pack_f16x2_hw(pn[2], pn[3]);
          *(uint2*)(u.p_f16 + o) = make_uint2(h01, h23);
          const float hf[4] = {f16_to_f32((f16_t)(h01 & 0xffffu)), f16_to_f32((f16_t)(h01 >> 16)), f16_to_f32((f16_t)(h23 & 0xffffu)), f16_to_f32((f16_t)(h23 >> 16))};
          float lo8[4], hi8[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            lo8[r] = fminf(fmaxf((pn[r] - hf[r]) * u.lo_scale, -448.f), 448.f);
            hi8[r] = fminf(fmaxf(pn[r] * u.hi_scale, -448.f), 448.f);
          }
          int wl = __builtin_amdgcn_cvt_pk_fp8_f32(lo8[0], lo8[1], 0, false);
          wl = __builtin_amdgcn_cvt_pk_fp8_f32(lo8[2], lo8[3], wl, true);
          int wh = __builtin_amdgcn_cvt_pk_fp8_f32(hi8[0], hi8[1], 0, false);
          wh = __builtin_amdgcn_cvt_pk_fp8_f32(hi8[2], hi8[3], wh, true);
          uint8_t* w8 = u.p_fp8 + (long)vr * 2 * K + k;
          *(int*)w8 = wl;
          *(int*)(w8 + K) = wh;
        }
        if (u.p_wide) {                               // [hi | lo]: saves a pass over the f32 weights (evc_cast_f32_to_bf16_wide) per update
          bf16_t* w = u.p_wide + (long)vr * 2 * K + k;
          *(uint2*)w = make_uint2((uint32_t)pb[0] | ((uint32_t)pb[1] << 16), (uint32_t)pb[2] | ((uint32_t)pb[3] << 16));
          *(uint2*)(w + K) = make_uint2(pack_bf16x2_hw(pn[0] - bf16_to_f32(pb[0]), pn[1] - bf16_to_f32(pb[1])),
                                        pack_bf16x2_hw(pn[2] - bf16_to_f32(pb[2]), pn[3] - bf16_to_f32(pb[3])));
        }
      }
      if (u.pT_bf16) {                                 // (kernel-uniform)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(rcol + r) * TP + vl] = pb[r];
      }
    }
    __syncthreads();                                   // gbuf holds the new weights of this wave row, the transpose image its columns
    if (u.wsq_partial && wr == h) {                    // (kernel-uniform / wave-uniform)
#pragma unroll
      for (int mi = 0; mi < Cfg::MI; ++mi) {
        const int vr = m0 + tc.row0 + mi * 16;
#pragma unroll
        for (int ni = 0; ni < Cfg::NI; ++ni) {
          const int k = n0 + tc.unit0 + ni * 16;
          if (vr >= u.V || k >= K) continue;
          const float4 q = *(const float4*)(gbuf + (mi * 16 + arow) * GP + tc.unit0 + ni * 16);
          const float pn[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) wsq += pn[r] * pn[r];
        }
      }
    }
  }
  // rows k of the transposed shadow: 4 bf16 per lane, BM/4 lanes per row (256 contiguous bytes), 64/(BM/4) rows per wave-instruction
  constexpr int TLPR = Cfg::BM / 4, RPW = 64 / TLPR;
  static_assert(TLPR <= 64 && 64 % TLPR == 0, "row of the transposed image must fit a wave");
  // (pT_bf16 == NULL: a caller whose backward reads the forward image - evc_gemm_kn - keeps no transposed shadow; this phase and the LDS
  //  image behind it are skipped, 2 of the pass's 30 bytes per parameter: profiles/moe_head_fwd_image_ab.txt)
  const int v4 = m0 + (lane % TLPR) * 4;
  for (int kl = wave * RPW + lane / TLPR; u.pT_bf16 && kl < Cfg::BU; kl += (Cfg::NT / 64) * RPW) {
    const int k = n0 + kl;
    if (k >= K || v4 >= u.V) continue;                 // V % 4 == 0: a lane's 4 rows are all valid or all not
    const uint32_t* src = (const uint32_t*)(tile + kl * TP + (lane % TLPR) * 4);     // (4-byte aligned: TP is not a multiple of 4)
    *(uint2*)(u.pT_bf16 + (long)k * u.ldT + v4) = make_uint2(src[0], src[1]);
  }
  if (u.wsq_partial) {                                 // per-workgroup partial, summed in a fixed order by moe_update_finalize_kernel
    wsq = wave_sum(wsq);
    if (lane == 0) red[wave] = wsq;                    // (its own corner of the ring: nothing to wait for)
    __syncthreads();
    if (threadIdx.x == 0) {
      float a = 0.f;
      for (int w = 0; w < Cfg::NT / 64; ++w) a += red[w];
      u.wsq_partial[2 * blockIdx.x] = a;
      u.wsq_partial[2 * blockIdx.x + 1] = 0.f;
    }
  }
}

__global__ __launch_bounds__(1024) void moe_update_finalize_kernel(const float* partial, int n, float* sums, int assign) {
  // one workgroup, fixed summation order (thread-strided partial sums, wave butterflies, then the 16 wave totals
  // in order): run-to-run identical
  __shared__ float wa[16], wb[16];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) { a += partial[2 * i]; b += partial[2 * i + 1]; }
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { wa[threadIdx.x >> 6] = a; wb[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sa = 0.f, sb = 0.f;
    for (int w = 0; w < 16; ++w) { sa += wa[w]; sb += wb[w]; }
    if (assign) { sums[0] = sa; sums[1] = sb; }
    else { sums[0] += sa; sums[1] += sb; }
  }
}

static int moe_grad_update_impl(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16, int64_t ldT,
                                float l2_coeff, float* sums, float* partial_ws, float clip_norm, float lr_t,
                                float beta1, float beta2, float eps, int phase, evc_bf16* p_wide, evc_f16* p_f16, uint8_t* p_fp8, int lo_exp, int hi_exp,
                                void* stream, float* wsq_out = nullptr);

extern "C" int evc_moe_grad_update_wide(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                        int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16, int64_t ldT,
                                        evc_bf16* p_wide_hilo, evc_f16* p_f16, uint8_t* p_fp8, int fp8_lo_exp, int fp8_hi_exp,
                                        float l2_coeff, float* sums, float* partial_ws, float clip_norm, float lr_t,
                                        float beta1, float beta2, float eps, void* stream) {
  EVC_REQUIRE(p_wide_hilo || p_f16, EVC_ERR_BAD_ARG, "evc_moe_grad_update_wide: p_wide_hilo [V][2K] or p_f16 [V][K] + p_fp8 [V][2K] is required");
  EVC_REQUIRE(!p_wide_hilo || ((uintptr_t)p_wide_hilo % 8) == 0, EVC_ERR_BAD_ALIGN, "evc_moe_grad_update_wide: p_wide_hilo must be 8-byte aligned");
  EVC_REQUIRE((p_f16 == nullptr) == (p_fp8 == nullptr) && (!p_f16 || (((uintptr_t)p_f16 % 8) == 0 && ((uintptr_t)p_fp8 % 4) == 0)), EVC_ERR_BAD_ARG,
              "evc_moe_grad_update_wide: p_f16 (8-byte aligned) and p_fp8 (4-byte aligned) go together");
  EVC_REQUIRE(!p_f16 || (fp8_lo_exp >= 0 && fp8_lo_exp <= 60 && fp8_hi_exp >= -30 && fp8_hi_exp <= 30), EVC_ERR_BAD_ARG,
              "evc_moe_grad_update_wide: fp8_lo_exp=%d fp8_hi_exp=%d", fp8_lo_exp, fp8_hi_exp);
  return moe_grad_update_impl(dlogits, ld_dlogits, x, ldx, rows, V, K, p, m, v, p_bf16, pT_bf16, ldT, l2_coeff, sums, partial_ws, clip_norm, lr_t,
                              beta1, beta2, eps, 0, p_wide_hilo, p_f16, p_fp8, fp8_lo_exp, fp8_hi_exp, stream);
}

extern "C" int evc_moe_grad_update_phase(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                         int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16, int64_t ldT,
                                         float l2_coeff, float* sums, float* partial_ws, float clip_norm, float lr_t,
                                         float beta1, float beta2, float eps, int phase, void* stream) {
  return moe_grad_update_impl(dlogits, ld_dlogits, x, ldx, rows, V, K, p, m, v, p_bf16, pT_bf16, ldT, l2_coeff, sums, partial_ws, clip_norm, lr_t,
                              beta1, beta2, eps, phase, nullptr, nullptr, nullptr, 0, 0, stream);
}

static int moe_grad_update_impl(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16,
                                int64_t ldT, float l2_coeff, float* sums, float* partial_ws, float clip_norm,
                                float lr_t, float beta1, float beta2, float eps, int phase, evc_bf16* p_wide, evc_f16* p_f16, uint8_t* p_fp8,
                                int lo_exp, int hi_exp, void* stream, float* wsq_out) {
  EVC_REQUIRE(rows > 0 && rows % 32 == 0 && V > 0 && V % 4 == 0 && K > 0 && K % 8 == 0, EVC_ERR_BAD_SHAPE,
              "evc_moe_grad_update: rows=%d (%%32), V=%d (%%4), K=%d (%%8)", rows, V, K);
  EVC_REQUIRE(phase >= 0 && phase <= 2, EVC_ERR_BAD_ARG, "evc_moe_grad_update_phase: phase=%d (0 both, 1 norms, 2 update)", phase);
  EVC_REQUIRE(ld_dlogits % 8 == 0 && ld_dlogits >= V && ldx % 8 == 0 && (!pT_bf16 || (ldT % 4 == 0 && ldT >= V)) &&
              ((uintptr_t)dlogits % 16) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)p % 16) == 0 && ((uintptr_t)m % 16) == 0 &&
              ((uintptr_t)v % 16) == 0 && ((uintptr_t)p_bf16 % 8) == 0 && ((uintptr_t)pT_bf16 % 8) == 0, EVC_ERR_BAD_ALIGN,
              "evc_moe_grad_update: operand alignment / leading dimensions");
  EVC_REQUIRE(pT_bf16 || (p_bf16 && !p_wide && !p_f16), EVC_ERR_BAD_ARG,
              "evc_moe_grad_update: pT_bf16 == NULL needs the plain bf16 form (p_bf16 written, no wide / f16 + e4m3 images)");
  hipStream_t st = (hipStream_t)stream;
  // 128x128 tiles, two workgroups per CU: the kernel is a stream over W, m, v with an 8-step GEMM in front - what
  // counts is how many epilogue loads are in flight per CU (256x256 tiles, one workgroup per CU: 3.4 TB/s)
  typedef CfgTn128 Cfg;
  const int Vp = (int)(ld_dlogits < ((V + 7) / 8) * 8 ? ld_dlogits : ((V + 7) / 8) * 8);   // A columns the loop may touch (%8)
  GemmOperandsT g{dlogits, ld_dlogits, x, ldx, Vp, K, rows / 32};
  const int tm = ceil_div(V, Cfg::BM), tn = ceil_div(K, Cfg::BU);
  EVC_REQUIRE(wsq_out == nullptr || phase == 2, EVC_ERR_BAD_ARG, "evc_moe_grad_update_apply: wsq_out goes with the update pass alone");
  MoeUpdateParams u{p, m, v, p_bf16, pT_bf16, ldT, p_wide, (bf16_t*)p_f16, p_fp8, ldexpf(1.0f, lo_exp), ldexpf(1.0f, hi_exp),
                    partial_ws, wsq_out ? partial_ws : nullptr, sums, V, K, l2_coeff, clip_norm, lr_t, beta1, beta2, eps};
  if (phase != 2) {
    launch_cfg<Cfg>(moe_update_kernel<Cfg, 1>, tm * tn, st, g, u, tm, tn);
    hipLaunchKernelGGL(moe_update_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)partial_ws, tm * tn, sums, 0);
  }
  if (phase != 1) launch_cfg<Cfg>(moe_update_kernel<Cfg, 2>, tm * tn, st, g, u, tm, tn);
  if (wsq_out) hipLaunchKernelGGL(moe_update_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)partial_ws, tm * tn, wsq_out, 1);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// The update pass alone (clip scale from sums[0], which evc_moe_grad_norms has filled), with any of the forward operand images of
// evc_moe_grad_update_wide (all three may be NULL: plain bf16) and wsq_out[0] = sum of the NEW weights squared (wsq_out[1] = 0):
// the |W|^2 term of the next update's norm.
extern "C" int evc_moe_grad_update_apply(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                         int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16, int64_t ldT,
                                         evc_bf16* p_wide_hilo, evc_f16* p_f16, uint8_t* p_fp8, int fp8_lo_exp, int fp8_hi_exp,
                                         float l2_coeff, const float* sums, float* partial_ws, float clip_norm, float lr_t,
                                         float beta1, float beta2, float eps, float* wsq_out, void* stream) {
  EVC_REQUIRE(wsq_out != nullptr, EVC_ERR_BAD_ARG, "evc_moe_grad_update_apply: wsq_out is required");
  EVC_REQUIRE(!p_wide_hilo || ((uintptr_t)p_wide_hilo % 8) == 0, EVC_ERR_BAD_ALIGN, "evc_moe_grad_update_apply: p_wide_hilo must be 8-byte aligned");
  EVC_REQUIRE((p_f16 == nullptr) == (p_fp8 == nullptr) && (!p_f16 || (((uintptr_t)p_f16 % 8) == 0 && ((uintptr_t)p_fp8 % 4) == 0)), EVC_ERR_BAD_ARG,
              "evc_moe_grad_update_apply: p_f16 (8-byte aligned) and p_fp8 (4-byte aligned) go together");
  EVC_REQUIRE(!p_f16 || (fp8_lo_exp >= 0 && fp8_lo_exp <= 60 && fp8_hi_exp >= -30 && fp8_hi_exp <= 30), EVC_ERR_BAD_ARG,
              "evc_moe_grad_update_apply: fp8_lo_exp=%d fp8_hi_exp=%d", fp8_lo_exp, fp8_hi_exp);
  return moe_grad_update_impl(dlogits, ld_dlogits, x, ldx, rows, V, K, p, m, v, p_bf16, pT_bf16, ldT, l2_coeff, (float*)sums, partial_ws, clip_norm, lr_t,
                              beta1, beta2, eps, 2, p_wide_hilo, p_f16, p_fp8, fp8_lo_exp, fp8_hi_exp, stream, wsq_out);
}

extern "C" int evc_moe_grad_update(const evc_bf16* dlogits, int64_t ld_dlogits, const evc_bf16* x, int64_t ldx, int rows,
                                   int V, int K, float* p, float* m, float* v, evc_bf16* p_bf16, evc_bf16* pT_bf16, int64_t ldT,
                                   float l2_coeff, float* sums, float* partial_ws, float clip_norm, float lr_t,
                                   float beta1, float beta2, float eps, void* stream) {
  return evc_moe_grad_update_phase(dlogits, ld_dlogits, x, ldx, rows, V, K, p, m, v, p_bf16, pT_bf16, ldT, l2_coeff, sums,
                                   partial_ws, clip_norm, lr_t, beta1, beta2, eps, 0, stream);
}


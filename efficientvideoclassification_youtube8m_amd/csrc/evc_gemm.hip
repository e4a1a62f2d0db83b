// Generic NT GEMM entry points (bf16 / f16 / split-bf16 / f16 + e4m3 low-order stages); DESIGN.md 3, LAB_NOTEBOOK.md 4.1-4.2a.
#include "gemm_shared.h"

template <class Cfg, bool F16 = false, bool FP8 = false>
__global__ __launch_bounds__(Cfg::NT) void gemm_nt_kernel(GemmOperands p, StoreParams s, int tiles_m, int tiles_n) {
  static_assert(!FP8 || (F16 && is_v3<Cfg>::value), "the e4m3 tail rides behind f16 stages of the 64-wide ring loop");
  const int nwg = tiles_m * tiles_n;
  int bid = blockIdx.x, split = 0;
  if (s.splits > 1) {               // this workgroup's K range (wave-uniform)
    split = bid / nwg;
    bid -= split * nwg;
    const int k0 = split * s.ksteps_per_split;
    const int kstep = (is_v2<Cfg>::value && !is_v3<Cfg>::value) ? 32 : 64;
    p.A1 += (long)k0 * kstep;
    p.B += (long)k0 * kstep;
    p.nk1 = min(s.ksteps_per_split, p.nk1 - k0);
    if constexpr (FP8) {
      const int k8 = split * s.ksteps8_per_split;
      p.A3 += (long)k8 * 128;
      p.B8 += (long)k8 * 128;
      p.nk3 = min(s.ksteps8_per_split, p.nk3 - k8);
    }
  }
  const int id = xcd_remap(bid, nwg);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn, s.splits > 1 ? patch_rows(nwg, tiles_n) : 8);
  const int m0 = tm * Cfg::BM, u0 = tn * Cfg::BU;
  f32x4 acc[Cfg::MI][Cfg::G][Cfg::NI];
  constexpr bool V2 = is_v2<Cfg>::value;
  // loop options (gemm_core_v2.h): producer waves + LDS-DMA first + no priority flips for every ring tile but the 320-row one
  // (same box: L1 dX 477 -> 431 us, 1280 x 4096 x 4096 63 -> 56.5 us, MoE gates forward 48.3 -> 46 us; 5120 x 4096 x 4096 on
  // the 320-row tile 153 -> 162 us with them)
  // the weight rows of the batch-row products (256 x 64 tiles: every weight row is read by ONE workgroup) as non-temporal LDS-DMA loads
  // (round 5; same box, alternated three times: the MoE gates product ALONE 42.9 -> 49.3 us, the training step 9.96 -> 9.92 ms -
  // 193 MB of weights per product no longer evict what the other streams' kernels re-read)
  constexpr int NT_MODE = (Cfg::BM == 320 ? 0 : (LOOP_PRODUCER | LOOP_DMA_FIRST | LOOP_NO_PRIO)) | (F16 ? LOOP_F16 : 0) | (FP8 ? LOOP_FP8_TAIL : 0) |
                          ((is_v3<Cfg>::value && Cfg::BM == 256 && Cfg::BU == 64) ? LOOP_B_NT : 0);
  run_mainloop<Cfg, Cfg::G, V2, true, NT_MODE>(p, m0, u0, acc);     // ring tiles: transposed accumulators (lane = one row, 4 consecutive columns)
  if constexpr (V2) {
    // plain overwrite with 16-byte-aligned rows, or the split-K join: through LDS (kernel-uniform conditions: one barrier)
    const int es = s.out_bf16 ? 2 : 4;
    const bool via_lds = s.splits == 1 && !s.accumulate && (s.ldc * es) % 16 == 0 && ((uintptr_t)s.C % 16) == 0 &&
                           (!s.bias || ((uintptr_t)s.bias % 16) == 0);
    const int wave = threadIdx.x >> 6, wc = wave % Cfg::WC;
    const bool wave_cols_in = u0 + wc * Cfg::WU + Cfg::WU <= s.N;         // this wave's column span lies inside C
    if constexpr (Cfg::WU <= 64) {                                       // (wider wave tiles are never launched with a K split)
      if (s.splits > 1) {
        __syncthreads();                                                 // every wave has read its last ring slot
        store_tile_via_lds<Cfg, 4, true>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, split == 0 ? s.bias : nullptr);
        return;
      }
    }
    if (via_lds) {
      __syncthreads();
      if (wave_cols_in) {
        if (s.out_bf16) store_tile_via_lds<Cfg, 2>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, s.bias);
        else store_tile_via_lds<Cfg, 4>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, s.bias, 0, s.sq_p, s.sq_l2, s.sq_out);
        return;
      }
    }
    TileCoordsT<Cfg> tc;                               // element-wise: accumulate, unaligned rows, the ragged right edge
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      const int m = m0 + tc.row0 + mi * 16;
      if (m >= s.M) continue;
#pragma unroll
      for (int ni = 0; ni < Cfg::NI; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = u0 + tc.unit0 + ni * 16 + r;
          if (n >= s.N) continue;
          float v = acc[mi][0][ni][r] + ((s.bias && split == 0) ? s.bias[n] : 0.f);
          const long o = (long)m * s.ldc + n;
          if (s.splits > 1) {
            atomicAdd((float*)s.C + o, v);          // one global_atomic_add_f32 per element, executed at the memory side
          } else if (s.out_bf16) {
            ((bf16_t*)s.C)[o] = f32_to_bf16(v);
          } else {
            float* cp = (float*)s.C + o;
            if (s.accumulate) v += *cp;
            *cp = v;
          }
        }
    }
  } else {
    TileCoords<Cfg> tc;
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < Cfg::NI; ++ni) {
        const int n = u0 + tc.unit0 + ni * 16;
        if (n >= s.N) continue;
        const float b = (s.bias && split == 0) ? s.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + tc.row0 + mi * 16 + r;
          if (m >= s.M) continue;
          float v = acc[mi][0][ni][r] + b;
          const long o = (long)m * s.ldc + n;
          if (s.splits > 1) {
            atomicAdd((float*)s.C + o, v);          // one global_atomic_add_f32 per element, executed at the memory side
          } else if (s.out_bf16) {
            ((bf16_t*)s.C)[o] = f32_to_bf16(v);
          } else {
            float* cp = (float*)s.C + o;
            if (s.accumulate) v += *cp;
            *cp = v;
          }
        }
      }
  }
}

// ---- host side: every entry is its own refusals, then nt_operands, choose_nt, launch_nt ----
enum NtForm { NT_BF16, NT_F16, NT_SPLIT, NT_F16_E4M3 };
struct NtPlan { int tile, splits; };        // an NT_TILES id and the number of K splits
struct NtCandidate { int tile, min_k; };    // a tile the cost comparison may take from K = min_k on

// The costed candidates of each operand form IN TIE-BREAK ORDER: the first of the cheapest wins.
// per-flop cost factors measured on MI355X (scripts/gemm_bench.py): v2 ~1000 TF/s, v1 128^2 ~800, v1 64^2 ~400
constexpr int NT_CAND_BF16_RING = 4;       // (the first four of the bf16 list are its ring tiles)
static const NtCandidate NT_CAND_BF16[] = {{NT_RING256, 0}, {NT_RING224, 0}, {NT_RING320, 0}, {NT_RING160, 2048}, {NT_V1_128, 0}, {NT_V1_64, 0}};
static const NtCandidate NT_CAND_F16[] = {{NT_RING320, 0}, {NT_RING256, 0}, {NT_RING160, 0}, {NT_RING128, 0}};
static const NtCandidate NT_CAND_SPLIT[] = {{NT_RING320, 0}, {NT_RING256, 0}, {NT_RING224, 0}, {NT_RING160, 0}, {NT_RING128, 0}};

static inline int cheapest_nt_tile(const NtCandidate* cand, int n, int M, int N, int K) {
  int best = cand[0].tile;
  double best_cost = 1e300;
  for (int i = 0; i < n; ++i) {
    const NtTile& t = nt_tile(cand[i].tile);
    const double c = tile_cost((long)ceil_div(M, t.bm) * ceil_div(N, t.bn), t.bm, t.bn, t.cost);
    if (K >= cand[i].min_k && c < best_cost) { best_cost = c; best = t.id; }
  }
  return best;
}

// Which tile and how many K splits an NT product gets.  forced (EVC_FORCE_TILE) counts for the bf16 form alone; K8: the e4m3 depth of NT_F16_E4M3
// (K is its f16 depth).  Partial tiles of a K split are joined by f32 atomics into a C that launch_nt zeroes unless the caller accumulates.
static NtPlan choose_nt(int M, int N, int K, NtForm form, bool out_bf16, bool sq_out, bool deterministic, int forced, int K8 = 0) {
  if (form == NT_F16) return {cheapest_nt_tile(NT_CAND_F16, 4, M, N, K), 1};       // ring tiles, no K split
  if (form == NT_SPLIT) {                                                          // ring tiles only (B2 lives in the v2 / v3 loops), no K split
    if (M <= 256) return {NT_ROWS256x64, 1};                                       // batch-row products (MoE head): stream the weights once
    return {cheapest_nt_tile(NT_CAND_SPLIT, 5, M, N, K), 1};
  }
  if (form == NT_F16_E4M3) {
    if (M > 512) return {NT_RING256, 1};
    // batch-row products (MoE head, DBoF hidden layer): 256 x 64 tiles stream the weights once; few column tiles and a long K
    // (512 x 1024 x 8192: 32 tiles) are cut along K until ~256 workgroups exist - every split takes the same share of the f16
    // and of the e4m3 stages (>= 4 of each: a full ring)
    const int tiles = ceil_div(M, 256) * ceil_div(N, 64), nk16 = K / 64, nk8 = K8 / 128;
    int splits = 1;
    while (!deterministic && splits < 16 && tiles * splits * 2 <= 256 && nk16 % (splits * 2) == 0 && nk8 % (splits * 2) == 0 &&
           nk16 / (splits * 2) >= 4 && nk8 / (splits * 2) >= 4)
      splits *= 2;
    return {NT_ROWS256x64, splits};
  }
  // M <= 256 (one row tile: the MoE head on a batch of videos, [B, K] x [N, K]^T with N or K ~ 14k): the product
  // streams the weight matrix once from HBM, so it wants ~256 workgroups pulling at the same time and a deep
  // load pipeline rather than a square tile: 256x64 tiles, K split until ~256 workgroups exist (>= 16 K steps of 64 each).
  if (M <= 256 && N >= 1024 && K >= 1024 && forced == 0)
    return {NT_ROWS256x64, (out_bf16 || deterministic) ? 1 : split_k(256 / ceil_div(N, 64), K / 64, 16)};
  if (!out_bf16 && forced == 0 && !deterministic) {
    // A few hundred rows against a long K with few output columns (DBoF: hidden layer [512 x 8192] . [1024 x 8192]^T, the MoE
    // head's dX at batch 512 with K = 14148 / 9432): eight 256x256 tiles cannot be split far enough to fill the chip (K/2048
    // splits = 32-48 workgroups, measured 105 us for 8.6 GFLOP).  128x128 ring tiles at two workgroups per CU instead, K split
    // until ~512 workgroups exist (>= 16 K steps of 32 each).
    // (M <= 512 only: streams.concurrent_streams probes with a 1024 x 1024 x 4096 product that must stay on 64 workgroups.)
    const long t128 = (long)ceil_div(M, 128) * ceil_div(N, 128);
    if (M > 256 && M <= 512 && t128 <= 128 && K >= 4096) {
      const int splits = split_k(512 / t128, K / 32, 16);
      if (splits > 1) return {NT_SPLIT128, splits};
    }
    // Split-K: a long-K product with too few 256x256 tiles to fill the 256 CUs (the weight-gradient
    // GEMMs: M=4H, N~1-2K, K = T*M rows) is cut along K, >= 64 K steps of 32 per split (63 MB of atomic
    // traffic at ~1.3 TB/s << the ~0.7 ms it saves per GEMM).
    const long t256 = (long)ceil_div(M, 256) * ceil_div(N, 256);
    if (t256 <= 128 && K >= 8192) {
      const int splits = split_k(256 / t256, K / 32, 64);
      if (splits > 1) return {NT_SPLIT256, splits};
    }
  }
  if (forced) return {forced >= 1 && forced <= 7 ? forced : NT_V1_64, 1};
  const int ring = cheapest_nt_tile(NT_CAND_BF16, NT_CAND_BF16_RING, M, N, K);
  int pick = cheapest_nt_tile(NT_CAND_BF16, 6, M, N, K);
  // 128x128 ring tiles (LDS-DMA ring instead of the v1 two-stage loop): 20-25 % faster than the v1 128x128 tile while the
  // whole product is one round of <= 256 tiles (measured: 1024 x 4096 x 4096 50 vs 63 us, 2048^3 28 vs 38, 1280 x 1024 x 4096
  // 45 vs 58); beyond that two workgroups share a CU's L2 ingest and the v1 / 256x256 tiles win again
  if (pick == NT_V1_128 && K >= 2048 && (long)ceil_div(M, 128) * ceil_div(N, 128) <= 256) pick = NT_RING128;
  if (sq_out && (pick == NT_V1_128 || pick == NT_V1_64)) pick = ring;            // (the fused norm lives in the ring tiles' LDS store)
  return {pick, 1};
}

// operands of C = A . B^T, one K segment; the forms then set what differs (A2 / B2, the e4m3 tail)
static inline GemmOperands nt_operands(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N) {
  GemmOperands p{};
  p.A1 = p.A2 = (const bf16_t*)A; p.lda1 = p.lda2 = lda;
  p.B = (const bf16_t*)B; p.ldb = ldb; p.M = M; p.Nu = N;
  return p;
}

struct NtDepth { int k1, k2, k8; };         // elements contracted from A1, from A2 and - e4m3 bytes - from A3

template <class Cfg, bool F16, bool FP8>
static int launch_nt(GemmOperands p, StoreParams s, NtDepth k, int splits, hipStream_t st) {
  p.nk1 = k.k1 / kdiv<Cfg>(); p.nk2 = k.k2 / kdiv<Cfg>(); p.nk3 = k.k8 / 128;
  const int tm = ceil_div(s.M, Cfg::BM), tn = ceil_div(s.N, Cfg::BU);
  s.splits = splits;
  s.ksteps_per_split = ceil_div(p.nk1, splits); s.ksteps8_per_split = ceil_div(p.nk3, splits);   // (the e4m3 form's splits divide both)
  if (splits > 1 && !s.accumulate) EVC_CHECK_HIP(hipMemset2DAsync(s.C, s.ldc * sizeof(float), 0, (size_t)s.N * sizeof(float), s.M, st));
  launch_cfg<Cfg>(gemm_nt_kernel<Cfg, F16, FP8>, tm * tn * splits, st, p, s, tm, tn);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}
template <bool F16, bool FP8>
static int launch_nt_plan(const GemmOperands& p, const StoreParams& s, NtDepth k, NtPlan plan, void* stream) {
  return with_nt_tile<F16, FP8>(plan.tile, [&](auto tile) { return launch_nt<typename decltype(tile)::type, F16, FP8>(p, s, k, plan.splits, (hipStream_t)stream); });
}

static int gemm_nt_impl(const char* entry, const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, void* C, int64_t ldc,
                        int M, int N, int K, const float* bias, int out_bf16, int accumulate, void* stream,
                        const float* sq_p = nullptr, float sq_l2 = 0.f, float* sq_out = nullptr) {
  EVC_REQUIRE(M > 0 && N > 0 && K >= 0, EVC_ERR_BAD_SHAPE, "%s: bad shape M=%d N=%d K=%d", entry, M, N, K);
  // fused squared norm: only where the product runs as ONE pass of ring tiles that store whole rows through LDS (no K split, no ragged edge)
  EVC_REQUIRE(!sq_out || (!out_bf16 && !accumulate && !bias && M > 512 && N % 256 == 0 && K < 8192 && ldc % 4 == 0 && ((uintptr_t)C % 16) == 0 &&
                          (!sq_p || ((uintptr_t)sq_p % 16) == 0) && forced_tile() == 0), EVC_ERR_BAD_ARG,
              "evc_gemm_nt_sqnorm: needs a plain f32 product with M > 512, N %% 256 == 0, K < 8192, 16-byte aligned C / P (M=%d N=%d K=%d ldc=%ld)", M, N, K, (long)ldc);
  EVC_REQUIRE(K % 64 == 0, EVC_ERR_BAD_SHAPE, "%s: K=%d must be a multiple of 64", entry, K);
  EVC_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0,
              EVC_ERR_BAD_ALIGN, "%s: operands must be 16-byte aligned (lda=%ld ldb=%ld)", entry, (long)lda, (long)ldb);
  EVC_REQUIRE(!(out_bf16 && accumulate), EVC_ERR_BAD_ARG, "%s: accumulate needs f32 output", entry);
  EVC_REQUIRE(ring_operand_ok(M, lda) && ring_operand_ok(N, ldb), EVC_ERR_BAD_SHAPE,
              "%s: an operand spans 4 GiB or more (M=%d lda=%ld, N=%d ldb=%ld): split the product", entry, M, (long)lda, N, (long)ldb);
  StoreParams s{C, ldc, M, N, bias, out_bf16, accumulate, 1, 0};
  s.sq_p = sq_p; s.sq_l2 = sq_l2; s.sq_out = sq_out;
  return launch_nt_plan<false, false>(nt_operands(A, lda, B, ldb, M, N), s, {K, 0, 0},
                                      choose_nt(M, N, K, NT_BF16, out_bf16, sq_out != nullptr, evc_deterministic(), forced_tile()), stream);
}
extern "C" int evc_gemm_nt(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, void* C, int64_t ldc,
                           int M, int N, int K, const float* bias, int out_bf16, int accumulate, void* stream) {
  return gemm_nt_impl("evc_gemm_nt", A, lda, B, ldb, C, ldc, M, N, K, bias, out_bf16, accumulate, stream);
}
// evc_gemm_nt (plain f32 output) + evc_grad_sqnorm in one pass (round 6): sums[0] += sum of (C + l2_coeff * P)^2, sums[1] += sum of P^2 over the product's elements, from
// the tiles' stores (one f32 atomic per wave; P [M][N] f32 laid out as C, NULL with l2_coeff 0).  A weight gradient that is materialised anyway -
// the MoE head at 1024 rows, cfg 5 - then needs no separate norm pass before its clip + Adam (8 of 40 bytes per parameter).  sums must be zeroed
// by the caller (the launch ADDS to them); every wave stores its partial pair into part_ws (>= 16 * ceil(M/128) * ceil(N/128) floats) and a one-block
// finishing launch adds the slots in index order - no atomics, the same bits every run.
__global__ __launch_bounds__(1024) void sum_pairs_kernel(const float* __restrict__ part, int n, float* __restrict__ sums) {
  __shared__ float sh[2][16];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) { a += part[2 * i]; b += part[2 * i + 1]; }     // fixed order per thread, fixed tree below
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f;
    for (int i = 0; i < 16; ++i) { ta += sh[0][i]; tb += sh[1][i]; }
    sums[0] += ta; sums[1] += tb;
  }
}
extern "C" int evc_gemm_nt_sqnorm(const evc_bf16* A, int64_t lda, const evc_bf16* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
                                  const float* P, float l2_coeff, float* sums, float* part_ws, int64_t part_ws_floats, void* stream) {
  EVC_REQUIRE(sums && part_ws && (P || l2_coeff == 0.f), EVC_ERR_BAD_ARG, "evc_gemm_nt_sqnorm: sums / part_ws must not be NULL; P == NULL needs l2_coeff == 0");
  // every wave of every tile owns one {|C + l2 P|^2, |P|^2} slot: at most ceil(M / 128) * ceil(N / 128) workgroups of 8 waves whatever tile is picked
  const long slots = (long)ceil_div(M, 128) * ceil_div(N, 128) * 8;
  EVC_REQUIRE(part_ws_floats >= 2 * slots, EVC_ERR_BAD_ARG, "evc_gemm_nt_sqnorm: part_ws holds %ld floats, %ld needed", (long)part_ws_floats, 2 * slots);
  EVC_CHECK_HIP(hipMemsetAsync(part_ws, 0, (size_t)(2 * slots) * sizeof(float), (hipStream_t)stream));
  const int rc = gemm_nt_impl("evc_gemm_nt_sqnorm", A, lda, B, ldb, C, ldc, M, N, K, nullptr, 0, 0, stream, P, l2_coeff, part_ws);
  if (rc) return rc;
  hipLaunchKernelGGL(sum_pairs_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, part_ws, (int)slots, sums);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// C[M,N] f32 = A . B^T on IEEE f16 operands (one f16 MFMA product per depth): the hoisted input projection of the "high" mode's L2
// level (evc_lstm_stack2_fwd_f16).
int gemm_nt_f16(const evc_f16* A, int64_t lda, const evc_f16* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K, void* stream) {
  EVC_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0,
              EVC_ERR_BAD_SHAPE, "f16 product: M=%d N=%d K=%d (K %% 64), operands 16-byte aligned", M, N, K);
  EVC_REQUIRE(ring_operand_ok(M, lda) && ring_operand_ok(N, ldb), EVC_ERR_BAD_SHAPE, "f16 product: an operand spans 4 GiB or more");
  return launch_nt_plan<true, false>(nt_operands(A, lda, B, ldb, M, N), StoreParams{C, ldc, M, N, nullptr, 0, 0, 1, 0}, {K, 0, 0},
                                     choose_nt(M, N, K, NT_F16, false, false, evc_deterministic(), 0), stream);
}

// Split-bf16 product C = (A_hi + A_lo) . (B_hi + B_lo)^T (+ bias) to ~2^-16 as ONE launch: the three products
// lo.hi + hi.lo + hi.hi are a K-extension of the plain loop.  A rows are the wide image [lo(K) | hi(K)]
// (evc_cast_f32_to_bf16_wide, lo first), B rows [hi(K) | lo(K)] (hi first): segment 1 walks A's whole row against B's whole row
// (k < K: lo.hi, k >= K: hi.lo), segment 2 walks A's hi half again against B2 = B's hi half (GemmOperands::B2 restarts B's k
// index).  Same accumulator, one epilogue, no split-K join - against three launches that each re-staged both operands and
// joined through C.  Ring tiles only (B2 lives in the v2 / v3 loops).
extern "C" int evc_gemm_nt_split(const evc_bf16* A_lohi, int64_t lda, const evc_bf16* B_hilo, int64_t ldb, float* C, int64_t ldc,
                                 int M, int N, int K, const float* bias, void* stream) {
  EVC_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0, EVC_ERR_BAD_SHAPE, "evc_gemm_nt_split: bad shape M=%d N=%d K=%d (K %% 64)", M, N, K);
  EVC_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && lda >= 2L * K && ldb >= 2L * K && ((uintptr_t)A_lohi % 16) == 0 && ((uintptr_t)B_hilo % 16) == 0,
              EVC_ERR_BAD_ALIGN, "evc_gemm_nt_split: wide operands [2K] per row, 16-byte aligned (lda=%ld ldb=%ld K=%d)", (long)lda, (long)ldb, K);
  EVC_REQUIRE(ring_operand_ok(M, lda) && ring_operand_ok(N, ldb), EVC_ERR_BAD_SHAPE,
              "evc_gemm_nt_split: an operand spans 4 GiB or more (M=%d lda=%ld, N=%d ldb=%ld)", M, (long)lda, N, (long)ldb);
  GemmOperands p = nt_operands(A_lohi, lda, B_hilo, ldb, M, N);     // [lo | hi] against [hi | lo], then ...
  p.A2 = A_lohi + K; p.B2 = B_hilo;                                 // ... hi against hi (B's k index restarts)
  return launch_nt_plan<false, false>(p, StoreParams{C, ldc, M, N, bias, 0, 0, 1, 0}, {2 * K, K, 0},
                                      choose_nt(M, N, K, NT_SPLIT, false, false, evc_deterministic(), 0), stream);
}

// C [M][N] f32 = A16 . B16^T (IEEE f16, K16 deep) + 2^scale_exp A8 . B8^T (OCP e4m3 bytes, K8 deep) + bias in ONE launch: a product whose
// low-order corrections ride behind its f16 stages on the MX-scaled MFMA (gemm_core_v3.h LOOP_FP8_TAIL) - the "high" precision MoE head:
// [f16(x)] . [f16(W)]^T + 2^-24 [e4m3(x 2^6) | e4m3((x - f16(x)) 2^17)] . [e4m3((W - f16(W)) 2^18) | e4m3(W 2^7)]^T leaves ~2.5e-5 on
// logits of magnitude 8 (f16 alone: 8e-4; scripts/precision_budget.py "MOE fine") for 2/3 of the operand bytes of the split-bf16
// K-extension (evc_gemm_nt_split).  lda / ldb in halfwords, lda8 / ldb8 in bytes.
static int gemm_nt_f16_fp8_impl(const char* entry, const evc_f16* A16, int64_t lda, const uint8_t* A8, int64_t lda8, const evc_f16* B16, int64_t ldb,
                                const uint8_t* B8, int64_t ldb8, float* C, int64_t ldc, int M, int N, int K16, int K8, int scale_exp,
                                const float* amax_ws, int a8_hi_exp, const float* bias, void* stream) {
  EVC_REQUIRE(M > 0 && N > 0 && K16 >= 64 && K16 % 64 == 0 && K8 >= 512 && K8 % 128 == 0, EVC_ERR_BAD_SHAPE,
              "%s: bad shape M=%d N=%d K16=%d (%%64, >= 64) K8=%d (%%128, >= 512)", entry, M, N, K16, K8);
  EVC_REQUIRE(A16 && A8 && B16 && B8 && C, EVC_ERR_BAD_ARG, "%s: NULL operand", entry);
  EVC_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && lda8 % 16 == 0 && ldb8 % 16 == 0 && lda >= K16 && ldb >= K16 && lda8 >= K8 && ldb8 >= K8 &&
              ((uintptr_t)A16 % 16) == 0 && ((uintptr_t)B16 % 16) == 0 && ((uintptr_t)A8 % 16) == 0 && ((uintptr_t)B8 % 16) == 0, EVC_ERR_BAD_ALIGN,
              "%s: 16-byte aligned operands and row strides (lda=%ld ldb=%ld lda8=%ld ldb8=%ld)", entry, (long)lda, (long)ldb, (long)lda8, (long)ldb8);
  EVC_REQUIRE(scale_exp >= -60 && scale_exp <= 60, EVC_ERR_BAD_ARG, "%s: scale_exp=%d", entry, scale_exp);
  EVC_REQUIRE(ring_operand_ok(M, lda) && ring_operand_ok(N, ldb) && ring_operand_ok(M, (lda8 + 1) / 2) && ring_operand_ok(N, (ldb8 + 1) / 2), EVC_ERR_BAD_SHAPE,
              "%s: an operand spans 4 GiB or more", entry);
  GemmOperands p = nt_operands(A16, lda, B16, ldb, M, N);
  p.A3 = p.A4 = A8; p.lda3 = p.lda4 = lda8; p.B8 = B8; p.ldb8 = ldb8; p.scale8_exp = scale_exp;
  p.amax_ws = amax_ws; p.a8_hi_exp = a8_hi_exp;
  return launch_nt_plan<true, true>(p, StoreParams{C, ldc, M, N, bias, 0, 0, 1, 0}, {K16, 0, K8},
                                    choose_nt(M, N, K16, NT_F16_E4M3, false, false, evc_deterministic(), 0, K8), stream);
}
extern "C" int evc_gemm_nt_f16_fp8(const evc_f16* A16, int64_t lda, const uint8_t* A8, int64_t lda8, const evc_f16* B16, int64_t ldb,
                                   const uint8_t* B8, int64_t ldb8, float* C, int64_t ldc, int M, int N, int K16, int K8, int scale_exp,
                                   const float* bias, void* stream) {
  return gemm_nt_f16_fp8_impl("evc_gemm_nt_f16_fp8", A16, lda, A8, lda8, B16, ldb, B8, ldb8, C, ldc, M, N, K16, K8, scale_exp, nullptr, 0, bias, stream);
}
// ... with the A8 images written by evc_cast_f32_to_f16_fp8x_dyn from the same amax_ws / hi_exp: every e4m3 product is scaled by
// 2^(scale_exp + d), d = the range shift both kernels derive from the 64 partial maxima (0 while max|x| 2^a8_hi_exp <= 448: the fixed-scale product).
extern "C" int evc_gemm_nt_f16_fp8_dyn(const evc_f16* A16, int64_t lda, const uint8_t* A8, int64_t lda8, const evc_f16* B16, int64_t ldb,
                                       const uint8_t* B8, int64_t ldb8, float* C, int64_t ldc, int M, int N, int K16, int K8, int scale_exp,
                                       const float* amax_ws, int a8_hi_exp, const float* bias, void* stream) {
  EVC_REQUIRE(amax_ws && a8_hi_exp >= -30 && a8_hi_exp <= 30, EVC_ERR_BAD_ARG, "evc_gemm_nt_f16_fp8_dyn: amax_ws=%p a8_hi_exp=%d", (const void*)amax_ws, a8_hi_exp);
  return gemm_nt_f16_fp8_impl("evc_gemm_nt_f16_fp8_dyn", A16, lda, A8, lda8, B16, ldb, B8, ldb8, C, ldc, M, N, K16, K8, scale_exp, amax_ws, a8_hi_exp, bias, stream);
}

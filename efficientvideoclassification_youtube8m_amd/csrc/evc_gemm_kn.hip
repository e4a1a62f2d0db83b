// K-major-B product (evc_gemm_kn): C[M][N] (+)= A[M][K] . B[K][N] with B stored as it is CONTRACTED - the contraction index is B's row, N is
// contiguous.  The MoE head's dX = dlogits . W reads the FORWARD weight image [V][K] through it (contraction over v = the image's rows), so
// the update kernel writes no transposed image for it.
//
// One tile, the batch-row shape of the NT products (CfgRing256x64: 256 rows x 64 columns, 8 waves, 4-deep ring of 64-wide K stages = the
// same 160 KiB of LDS), and the skeleton of gemm_core_v3.h: counted vmcnt, one raw barrier per stage, producer waves, register-double-
// buffered fragments, SWAP accumulators, the same epilogues.  What differs from the NT tile is the B operand alone:
//  * A [M][lda] is staged and read exactly as there (rows of 128 bytes, chunk c of row r at c ^ (r & 7), ds_read_b128 fragments).
//  * B's part of a stage is [64 k rows][64 n] bf16: a row is 128 bytes = one whole cache line, a 1 KiB LDS-DMA piece is 8 k rows.  Its MFMA
//    fragments come from ds_read_b64_tr_b16 as in gemm_core_tn.h (lane 16g + 4q + p supplies the address of row 8g + 4j + q, columns nc + 4p ..
//    and receives column nc + (lane & 15) of rows 8g + 4j .. +3; j = 0, 1 are the fragment's 8 k values) - the element order of the NT
//    tile's 16-byte fragment reads, so with equal K splits the sums are those of evc_gemm_nt on a transposed copy of B, bit for bit.
//  * Swizzle of the B rows, re-derived for 128-byte rows: a 32-lane half of a transposing read covers 8 rows (g & 1, q) x 32 bytes.  A row is
//    half of the 256-byte bank row, rows r and r + 2 start on the same banks, and the rule of gemm_core_tn.h (bits 3 and 0-1 of the row) would
//    leave rows q and q + 2 in one slot.  Here the 32-byte slot index wc of a row is XORed with kn_h(r) = 2 * bit 3 of r + bit 1 of r: the 8 rows
//    of a half land in the 8 slots (r & 1) * 4 + (wc ^ kn_h(r)) of the bank row, all different; r + 4 and r + 32 (the j = 1 read and the second
//    K half of the stage) keep kn_h, so their distances are immediates of the read.  The LDS-DMA source address carries the same XOR.
//  * K need not be a multiple of 64 (K % 8 == 0): the last stage of a segment clamps its A chunks and B rows in bounds, and the A chunks
//    beyond K are overwritten with zeros in LDS before the stage is read (a wave-uniform branch that only that stage takes).
//  * B may have fewer rows than K (b_rows): the rows beyond are read as its last row, and the caller keeps A's columns there zero - the head's
//    factor images are padded to 64 columns with zeros, the weight image has exactly V rows.
//  * two K segments (A1 . B1 then A2 . B2) in one launch: dX = dgl . Wg + del . We without a read-modify-write of dx between them.  The
//    segment of a stage is a pair of scalar selects per stage, as the A1 / A2 switch of the NT loops.
#include "gemm_shared.h"

struct KnOperands {
  const bf16_t* A1; long lda1; const bf16_t* B1; long ldb1; int nk1, kr1, br1;   // stages, contraction length and B rows of segment 1
  const bf16_t* A2; long lda2; const bf16_t* B2; long ldb2; int nk2, kr2, br2;   // ... then segment 2 (nk2 == 0: none)
  int M, N;                                                                      // valid rows of A / columns of B
};

__device__ __forceinline__ constexpr int kn_h(int row) { return (((row >> 3) & 1) << 1) | ((row >> 1) & 1); }

// stages [s_first, s_end) of the concatenated segments (a K split's share)
template <class Cfg, int MODE>
__device__ __forceinline__ void gemm_mainloop_kn(const KnOperands& p, const int m0, const int n0, const int s_first, const int s_end, char* lds,
                                                 f32x4 (&acc)[Cfg::MI][1][Cfg::NI]) {
  static_assert(Cfg::G == 1 && Cfg::BK == 64 && !Cfg::RAGGED && !Cfg::UNEVEN && Cfg::BN % 64 == 0, "K-major B: plain 64-wide-stage tiles, 128-byte B rows");
  static_assert(Cfg::BN == 64, "a B row of a stage is one 128-byte line");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave / Cfg::WC, wc = wave % Cfg::WC;
#pragma unroll
  for (int mi = 0; mi < Cfg::MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < Cfg::NI; ++ni) acc[mi][0][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = __builtin_amdgcn_readfirstlane(s_end - s_first);
  if (nk <= 0) return;

  // ---- staging.  A: piece q (1 KiB) = tile rows 8q .. 8q+7, lane -> row lane>>3, physical chunk lane&7 (gemm_core_v3.h).
  //      B: piece q = k rows 8q .. 8q+7 of the stage, lane -> k row lane>>3, physical chunk lane&7 = logical chunk (lane&7) ^ (kn_h(row) << 1)
  const int lc8 = ((lane & 7) ^ (lane >> 3)) * 8;
  constexpr bool PRODUCERS = (MODE & LOOP_PRODUCER) != 0 && Cfg::NT == 512;
  constexpr int NPW = PRODUCERS ? 4 : Cfg::NT / 64;
  const bool producer = wave < NPW;
  constexpr int ACH = Cfg::BM / 8 / NPW, BCH = 64 / 8 / NPW, PER = ACH + BCH;
  static_assert(ACH * NPW * 8 == Cfg::BM && BCH * NPW * 8 == 64, "pieces must divide over the staging waves");
  int a_row[ACH], b_row[BCH];
  uint32_t b_col[BCH];                   // byte offset of this lane's 16-byte chunk within a B row (clamped in bounds; N % 8 == 0)
#pragma unroll
  for (int i = 0; i < ACH; ++i) {
    const int gr = m0 + ((wave % NPW) + i * NPW) * 8 + (lane >> 3);
    a_row[i] = gr < p.M ? gr : p.M - 1;
  }
#pragma unroll
  for (int i = 0; i < BCH; ++i) {
    const int r = ((wave % NPW) + i * NPW) * 8 + (lane >> 3);
    b_row[i] = r;
    int col = n0 + (((lane & 7) ^ (kn_h(r) << 1)) << 3);
    col = col + 8 <= p.N ? col : p.N - 8;
    b_col[i] = (uint32_t)col * 2u;
  }
  int ks_issue = s_first;
  int slot_issue = 0, slot_read = 0;

  auto stage = [&]() {                 // branch-free (scalar selects only)
    const bool s1 = ks_issue < p.nk1;
    const int kl = (s1 ? ks_issue : ks_issue - p.nk1) * 64;        // first k of the stage within its segment
    const int kr = s1 ? p.kr1 : p.kr2, br = s1 ? p.br1 : p.br2;
    const char* ab = (const char*)(s1 ? p.A1 : p.A2);
    const char* bb = (const char*)(s1 ? p.B1 : p.B2);
    const uint32_t lda_b = (uint32_t)(s1 ? p.lda1 : p.lda2) * 2u, ldb_b = (uint32_t)(s1 ? p.ldb1 : p.ldb2) * 2u;
    const uint32_t chunk_b = (uint32_t)min(kl + lc8, kr - 8) * 2u;   // (a chunk beyond K: re-reads the last one; zeroed in LDS, fix_tail)
    char* sbase = lds + slot_issue * Cfg::STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      const uint32_t vo = __umul24((uint32_t)a_row[i], lda_b) + chunk_b;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ab + vo),
                                       (__attribute__((address_space(3))) void*)(sbase + ((wave % NPW) + i * NPW) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BCH; ++i) {
      const uint32_t vo = __umul24((uint32_t)min(kl + b_row[i], br - 1), ldb_b) + b_col[i];
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bb + vo),
                                       (__attribute__((address_space(3))) void*)(sbase + Cfg::A_BYTES + ((wave % NPW) + i * NPW) * 1024), 16, 0,
                                       (MODE & LOOP_B_NT) ? 2 : 0);
    }
    ++ks_issue;
    slot_issue = (slot_issue + 1 == Cfg::STAGES) ? 0 : slot_issue + 1;
  };

  // Stage ks sits in ring slot slot_read, has landed and is about to be read: if it reaches beyond its segment's K, its A chunks there become
  // zeros (B's rows there are copies of a valid row: finite).  Wave-uniform; only the last stage of a segment with K % 64 != 0 takes it.
  auto fix_tail = [&](const int ks) {
    const bool s1 = ks < p.nk1;
    const int kl = (s1 ? ks : ks - p.nk1) * 64, kr = s1 ? p.kr1 : p.kr2;
    if (__builtin_expect(kl + 64 > kr, 0)) {
      char* sb = lds + slot_read * Cfg::STAGE_BYTES;
      const int c0 = (kr - kl) >> 3;                            // first logical chunk beyond K (1 .. 7)
      for (int idx = tid; idx < Cfg::BM * 8; idx += Cfg::NT) {
        const int r = idx >> 3, c = idx & 7;
        if (c >= c0) *(uint4*)(sb + r * 128 + ((c ^ (r & 7)) << 4)) = make_uint4(0u, 0u, 0u, 0u);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  };

  // ---- fragment reads.  A as in gemm_core_v3.h; B: one address register per fragment (K half 0, j = 0), the rest are immediates
  const int frow = lane & 15, fq = lane >> 4;
  const int fch = (fq ^ (frow & 7)) * 16;
  const int a_rd0 = (wr * Cfg::ROW1 + frow) * 128 + fch, a_rd1 = a_rd0 ^ 64;
  auto a_off = [](const int mi) { return mi * 16 * 128; };
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  constexpr int B_J1 = 4 * 128, B_KB1 = 32 * 128;
  static_assert(kn_h(0) == kn_h(4) && kn_h(11) == kn_h(15) && kn_h(3) == kn_h(35) && kn_h(27) == kn_h(63), "j = 1 and the second K half keep the swizzle");
  uint32_t b_rd[Cfg::NI];
  {
    const int r = 8 * tg + tq, hs = kn_h(r) << 1;
#pragma unroll
    for (int ni = 0; ni < Cfg::NI; ++ni) {
      const int nc = wc * Cfg::WU + ni * 16;
      b_rd[ni] = (uint32_t)(Cfg::A_BYTES + r * 128 + ((((nc >> 3) + (tp >> 1)) ^ hs) << 4) + ((tp & 1) << 3));
    }
  }
  const uint32_t lds_rd = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)lds);
  auto read_half = [&](auto kb_tag, bf16x8 (&af)[Cfg::MI], bf16x8 (&bfr)[Cfg::NI]) {   // half kb of ring slot slot_read
    constexpr int kb = decltype(kb_tag)::value;
    const char* sb = lds + slot_read * Cfg::STAGE_BYTES;
    const uint32_t sbb = lds_rd + slot_read * Cfg::STAGE_BYTES;
#pragma unroll
    for (int ni = 0; ni < Cfg::NI; ++ni) {
      const uint32_t a = sbb + b_rd[ni];
      const s16x4 lo = tn_tr<kb * B_KB1>(a), hi = tn_tr<kb * B_KB1 + B_J1>(a);
      bfr[ni] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    const char* pa = sb + (kb ? a_rd1 : a_rd0);
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) af[mi] = *(const bf16x8*)(pa + a_off(mi));
  };
  using KB0 = std::integral_constant<int, 0>;
  using KB1 = std::integral_constant<int, 1>;
  auto next_slot = [&]() { slot_read = (slot_read + 1 == Cfg::STAGES) ? 0 : slot_read + 1; };
  auto mfma_all = [&](const bf16x8 (&af)[Cfg::MI], const bf16x8 (&bfr)[Cfg::NI]) {     // SWAP: lane = one row, 4 consecutive columns
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < Cfg::NI; ++ni) acc[mi][0][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][0][ni], 0, 0, 0);
  };
  auto end_of_step = [&]() {          // retires the LDS reads - the transposing ones are inline asm, nothing else waits for them
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
  };
  constexpr int AHEAD = Cfg::STAGES - 2;
  auto wait_landed = [&](int outstanding_stages) {
    if (outstanding_stages >= 4) wait_vmcnt<4 * PER>();
    else if (outstanding_stages == 3) wait_vmcnt<3 * PER>();
    else if (outstanding_stages == 2) wait_vmcnt<2 * PER>();
    else if (outstanding_stages == 1) wait_vmcnt<PER>();
    else wait_vmcnt<0>();
  };

  auto run = [&](auto prod_tag) {     // one copy of the loop per role
  constexpr bool PROD = decltype(prod_tag)::value;
  constexpr int PERX = PROD ? PER : 0;
  constexpr int NMFMA = Cfg::MI * Cfg::NI, NREAD = Cfg::MI;      // (the scheduler sees A's reads; B's are asm in program order)
  auto stage_role = [&]() {
    if constexpr (PROD) stage();
  };
  auto interleave = [&](auto ndma_tag) {   // MFMAs with one LDS read / LDS-DMA between them (LOOP_DMA_FIRST order)
    constexpr int ndma = decltype(ndma_tag)::value;
    constexpr int per = NMFMA / (NREAD + ndma) > 0 ? NMFMA / (NREAD + ndma) : 1;
#pragma unroll
    for (int i = 0; i < ndma; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, per, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
#pragma unroll
    for (int i = 0; i < NREAD; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, per, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
  };
  // ---- prologue: every slot of the ring in flight ----
#pragma unroll
  for (int i = 0; i < Cfg::STAGES; ++i)
    if (i < nk) stage_role();
  if constexpr (PROD) wait_landed(min(nk, Cfg::STAGES) - 1);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  fix_tail(s_first);
  bf16x8 afA[Cfg::MI], bfA[Cfg::NI], afB[Cfg::MI], bfB[Cfg::NI];
  read_half(KB0{}, afA, bfA);
  __builtin_amdgcn_s_waitcnt(0xC07F);

  int j = 0;
  for (; j + Cfg::STAGES < nk; ++j) {   // steady state: stage j + STAGES exists, every trip refills the slot it frees
    read_half(KB1{}, afB, bfB);
    mfma_all(afA, bfA);
    interleave(std::integral_constant<int, 0>{});
    end_of_step();
    if constexpr (PROD) wait_vmcnt<AHEAD * PER>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    next_slot();
    fix_tail(s_first + j + 1);          // (in front of the refill: the LDS-DMA, the reads and the MFMAs below stay one block for the scheduler)
    stage_role();
    read_half(KB0{}, afA, bfA);
    mfma_all(afB, bfB);
    interleave(std::integral_constant<int, PERX>{});
    end_of_step();
  }
  for (; j < nk; ++j) {                 // last STAGES stages: no refills
    read_half(KB1{}, afB, bfB);
    mfma_all(afA, bfA);
    end_of_step();
    if (j + 1 < nk) {
      if constexpr (PROD) wait_landed(nk - (j + 2));
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      next_slot();
      fix_tail(s_first + j + 1);
      read_half(KB0{}, afA, bfA);
    }
    mfma_all(afB, bfB);
    end_of_step();
  }
  };   // run
  if constexpr (PRODUCERS) {
    if (producer) run(std::true_type{});
    else run(std::false_type{});
  } else {
    run(std::true_type{});
  }
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::NT) void gemm_kn_kernel(KnOperands p, StoreParams s, int tiles_m, int tiles_n) {
  const int nwg = tiles_m * tiles_n;
  int bid = blockIdx.x, split = 0;
  int s_first = 0, s_end = p.nk1 + p.nk2;
  if (s.splits > 1) {               // this workgroup's stages (wave-uniform)
    split = bid / nwg;
    bid -= split * nwg;
    s_first = split * s.ksteps_per_split;
    s_end = min(s_end, s_first + s.ksteps_per_split);
  }
  const int id = xcd_remap(bid, nwg);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn, s.splits > 1 ? patch_rows(nwg, tiles_n) : 8);
  const int m0 = tm * Cfg::BM, u0 = tn * Cfg::BU;
  f32x4 acc[Cfg::MI][1][Cfg::NI];
  // the loop options of the batch-row NT tile (evc_gemm.hip): producer waves, LDS-DMA first, no priority flips, the weight rows non-temporal
  gemm_mainloop_kn<Cfg, LOOP_PRODUCER | LOOP_DMA_FIRST | LOOP_NO_PRIO | LOOP_B_NT>(p, m0, u0, s_first, s_end, lds_dyn, acc);
  // the epilogue of gemm_nt_kernel's ring tiles
  if (s.splits > 1) {
    __syncthreads();                                                   // every wave has read its last ring slot
    store_tile_via_lds<Cfg, 4, true>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, split == 0 ? s.bias : nullptr);
    return;
  }
  const int es = s.out_bf16 ? 2 : 4;
  const bool via_lds = !s.accumulate && (s.ldc * es) % 16 == 0 && ((uintptr_t)s.C % 16) == 0 && (!s.bias || ((uintptr_t)s.bias % 16) == 0);
  const int wave = threadIdx.x >> 6, wc = wave % Cfg::WC;
  if (via_lds) {
    __syncthreads();
    if (u0 + wc * Cfg::WU + Cfg::WU <= s.N) {                          // this wave's column span lies inside C
      if (s.out_bf16) store_tile_via_lds<Cfg, 2>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, s.bias);
      else store_tile_via_lds<Cfg, 4>(acc, lds_dyn, s.C, s.ldc, s.M, s.N, m0, u0, s.bias);
      return;
    }
  }
  TileCoordsT<Cfg> tc;                                                 // element-wise: accumulate, unaligned rows, the ragged right edge
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
        float v = acc[mi][0][ni][r] + (s.bias ? s.bias[n] : 0.f);
        const long o = (long)m * s.ldc + n;
        if (s.out_bf16) {
          ((bf16_t*)s.C)[o] = f32_to_bf16(v);
        } else {
          float* cp = (float*)s.C + o;
          if (s.accumulate) v += *cp;
          *cp = v;
        }
      }
  }
}

// K splits of the product, as evc_gemm_nt picks them for its batch-row tile: until ~256 workgroups exist, >= 16 stages each, none under
// EVC_DETERMINISTIC (the join is f32 atomics) or for a bf16 output
static int kn_splits(int N, int nk, bool out_bf16) {
  return (out_bf16 || evc_deterministic()) ? 1 : split_k(256 / ceil_div(N, 64) > 0 ? 256 / ceil_div(N, 64) : 1, nk, 16);
}

extern "C" int evc_gemm_kn_plan(int N, int K1, int K2, int out_bf16, int* splits) {
  EVC_REQUIRE(splits && N > 0 && K1 > 0 && K2 >= 0, EVC_ERR_BAD_ARG, "evc_gemm_kn_plan: N=%d K1=%d K2=%d", N, K1, K2);
  *splits = kn_splits(N, ceil_div(K1, 64) + ceil_div(K2, 64), out_bf16 != 0);
  return EVC_OK;
}

extern "C" int evc_gemm_kn(const evc_bf16* A1, int64_t lda1, const evc_bf16* B1, int64_t ldb1, int K1, int b_rows1,
                           const evc_bf16* A2, int64_t lda2, const evc_bf16* B2, int64_t ldb2, int K2, int b_rows2,
                           void* C, int64_t ldc, int M, int N, const float* bias, int out_bf16, int accumulate, int splits, void* stream) {
  EVC_REQUIRE(A1 && B1 && C, EVC_ERR_BAD_ARG, "evc_gemm_kn: NULL operand");
  EVC_REQUIRE(K2 >= 0 && (K2 == 0 || (A2 && B2)), EVC_ERR_BAD_ARG, "evc_gemm_kn: the second K segment needs A2 and B2 (K2=%d)", K2);
  EVC_REQUIRE(M > 0 && N > 0 && K1 > 0, EVC_ERR_BAD_SHAPE, "evc_gemm_kn: bad shape M=%d N=%d K1=%d", M, N, K1);
  EVC_REQUIRE(M <= 256, EVC_ERR_BAD_SHAPE, "evc_gemm_kn: M=%d: only the batch-row tile (M <= 256) is built", M);
  EVC_REQUIRE(K1 % 8 == 0 && K2 % 8 == 0 && N % 8 == 0, EVC_ERR_BAD_SHAPE, "evc_gemm_kn: K1=%d, K2=%d and N=%d must be multiples of 8", K1, K2, N);
  if (b_rows1 == 0) b_rows1 = K1;
  if (b_rows2 == 0) b_rows2 = K2;
  EVC_REQUIRE(b_rows1 > 0 && b_rows1 <= K1 && (K2 == 0 || (b_rows2 > 0 && b_rows2 <= K2)), EVC_ERR_BAD_SHAPE,
              "evc_gemm_kn: b_rows1=%d / b_rows2=%d must lie in 1 .. K", b_rows1, b_rows2);
  EVC_REQUIRE(lda1 % 8 == 0 && ldb1 % 8 == 0 && ((uintptr_t)A1 % 16) == 0 && ((uintptr_t)B1 % 16) == 0 &&
              (K2 == 0 || (lda2 % 8 == 0 && ldb2 % 8 == 0 && ((uintptr_t)A2 % 16) == 0 && ((uintptr_t)B2 % 16) == 0)),
              EVC_ERR_BAD_ALIGN, "evc_gemm_kn: operands must be 16-byte aligned (lda=%ld ldb=%ld lda2=%ld ldb2=%ld)", (long)lda1, (long)ldb1, (long)lda2, (long)ldb2);
  EVC_REQUIRE(ldc >= N, EVC_ERR_BAD_SHAPE, "evc_gemm_kn: ldc=%ld < N=%d", (long)ldc, N);
  EVC_REQUIRE(lda1 >= K1 && ldb1 >= N && (K2 == 0 || (lda2 >= K2 && ldb2 >= N)), EVC_ERR_BAD_SHAPE,
              "evc_gemm_kn: a leading dimension is shorter than its row (lda=%ld K1=%d ldb=%ld N=%d lda2=%ld K2=%d ldb2=%ld)", (long)lda1, K1, (long)ldb1, N,
              (long)lda2, K2, (long)ldb2);
  EVC_REQUIRE(ring_operand_ok(M, lda1) && ring_operand_ok(b_rows1, ldb1) && (K2 == 0 || (ring_operand_ok(M, lda2) && ring_operand_ok(b_rows2, ldb2))),
              EVC_ERR_BAD_SHAPE, "evc_gemm_kn: an operand spans 4 GiB or more: split the product");
  EVC_REQUIRE(!(out_bf16 && accumulate), EVC_ERR_BAD_ARG, "evc_gemm_kn: accumulate needs f32 output");
  typedef CfgRing256x64 Cfg;
  KnOperands p{(const bf16_t*)A1, lda1, (const bf16_t*)B1, ldb1, ceil_div(K1, 64), K1, b_rows1,
               (const bf16_t*)(K2 ? A2 : A1), K2 ? lda2 : lda1, (const bf16_t*)(K2 ? B2 : B1), K2 ? ldb2 : ldb1, ceil_div(K2, 64), K2 ? K2 : K1, K2 ? b_rows2 : b_rows1, M, N};
  const int nk = p.nk1 + p.nk2;
  EVC_REQUIRE(splits >= 0 && (splits <= 1 || (!out_bf16 && (long)ceil_div(nk, splits) * (splits - 1) < nk)), EVC_ERR_BAD_ARG,
              "evc_gemm_kn: splits=%d (0: chosen by shape; f32 output, no empty split of %d stages)", splits, nk);
  if (splits == 0) splits = kn_splits(N, nk, out_bf16 != 0);
  StoreParams s{C, ldc, M, N, bias, out_bf16, accumulate, splits, ceil_div(nk, splits)};
  hipStream_t st = (hipStream_t)stream;
  const int tm = ceil_div(M, Cfg::BM), tn = ceil_div(N, Cfg::BU);
  if (splits > 1 && !accumulate) EVC_CHECK_HIP(hipMemset2DAsync(C, ldc * sizeof(float), 0, (size_t)N * sizeof(float), M, st));
  launch_cfg<Cfg>(gemm_kn_kernel<Cfg>, tm * tn * splits, st, p, s, tm, tn);
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

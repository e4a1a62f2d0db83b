// Fused LSTM forward step, the L2 wavefront pair launches and their entry points.
#include "gemm_shared.h"

// ===========================================================================
// LSTM forward step: z = [x_t, h_{t-1}] . W^T (+ zx) + bias ; gate tail fused
// ===========================================================================
struct LstmFwdParams {
  const float* zx; long ldzx;        // hoisted x-projection rows for this step (or NULL)
  const float* bias;                 // [4H]
  const int* len; int t;
  float* c_state; float* h_state; long ld_state;
  bf16_t* hout;                      // [M][H] slab t+1 (row-major: next step's A operand)
  bf16_t* hout_lo;                   // SPLIT: slab t+1 of the WIDE image [M][2H] = [lo(h_t) | hi(h_t)] (next step's split A operand);
                                     // F16 (hout then holds IEEE f16): the bf16 copy of h_t the backward pass reads; else NULL
  uint2* gates;                      // [M][H] 8-byte records of slab t (or NULL): bf16 {i, j, f, o}
  bf16_t* c_hist;                    // slab t+1 of the bf16 cell-state history [M][H] (c after this step), or NULL
  const int* row_map;                // slot -> row of c_state / h_state (row plan, evc_sort_rows_by_len) or NULL
  int M, H;
  int h_wide = 0;                    // F16 only: 1 = hout rows are WIDE, [M][2H] = [f16(h_t) | f16(h_t)/64] - the activation operand of a
                                     // contraction whose weights are K-extended by their low-order halves (evc_lstm_stack2_fwd_f16);
                                     // 2 = hout rows are [f16(h_t) (H halfwords) | e4m3(h_t * 2^7) (H bytes)], row stride 3H bytes - the
                                     // operands of a step whose low-order weight halves are contracted in fp8 (evc_lstm_layer_fwd_f16_fp8lo);
                                     // 3 (round 6) = 2 + the low-order half of h itself: rows of 4H bytes [f16(h_t) | e4m3(h_t 2^7) |
                                     // e4m3((h_t - f16(h_t)) 2^18)] - contracted against [lo(W) | hi(W)] weight rows (h_lo = 1 of the same entries)
};


// F16: the operands (x_t, h_{t-1}, W) are IEEE f16 and ONE v_mfma_f32_16x16x32_f16 product is issued per depth - the cost of
// the bf16 step with 8x smaller operand rounding; h_t leaves twice, as f16 (next step's / next layer's operand) and as bf16
// (what the BPTT products contract over).
// the accumulators start from bias (+ forget_bias 1.0): its loads fly under the loop's prologue, and the tail
// has no load left that hipcc could re-issue between the fragments' stores
template <class Cfg>
__device__ __forceinline__ void lstm_fwd_acc_bias(const LstmFwdParams& e, const int u0, f32x4 (&acc)[Cfg::MI][4][Cfg::NI]) {
  {
    TileCoordsT<Cfg> tc0;
#pragma unroll
    for (int ni = 0; ni < Cfg::NI; ++ni) {
      const int u = min(u0 + tc0.unit0 + ni * 16, e.H - 4);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b = *(const float4*)(e.bias + (long)g * e.H + u);
        const float fb = (g == 2) ? 1.0f : 0.0f;       // forget_bias
#pragma unroll
        for (int mi = 0; mi < Cfg::MI; ++mi) acc[mi][g][ni] = f32x4{b.x + fb, b.y + fb, b.z + fb, b.w + fb};
      }
    }
  }
}

// gate tail of one tile: sigma / tanh, c' = c f + i j, h' = tanh(c') o, masking, the stores (transposed accumulators: lane = one row, 4 units)
template <class Cfg, bool SPLIT, bool F16, bool FP8>
__device__ __forceinline__ void lstm_fwd_epilogue(const GemmOperands& p, const LstmFwdParams& e, const int m0, const int u0,
                                                  f32x4 (&acc)[Cfg::MI][4][Cfg::NI]) {
  TileCoordsT<Cfg> tc;
  const int H = e.H;     // H % 4 == 0 (checked on the host): a lane's 4 units never straddle H
  // Every load of the tail is issued before the first store: the stores of one fragment and the loads of the next
  // go to the same arrays (c_state is updated in place), so in program order hipcc must finish the stores before
  // the next loads - with 8 fragments per lane that was 8 serial load->store round trips (21 of the 67 us).
#pragma unroll
  for (int ni = 0; ni < Cfg::NI; ++ni) {
    const int u = u0 + tc.unit0 + ni * 16;
    if (u >= H) continue;
    int ln[Cfg::MI], rm[Cfg::MI];
    const int mi_n = wave_row_frags<Cfg>::of(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) / Cfg::WC);   // (uneven row split: the fragments this wave row owns)
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      const int m = m0 + tc.row0 + mi * 16;
      const bool in = m < e.M && mi < mi_n;
      ln[mi] = in ? e.len[m] : -1;                     // -1: row outside the launch (nothing to do, not even zeros)
      rm[mi] = (in && e.row_map) ? e.row_map[m] : m;
    }
    float4 cv[Cfg::MI];
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      cv[mi] = make_float4(0.f, 0.f, 0.f, 0.f);        // zero initial state (no memset of the state buffers)
      if (e.t > 0 && e.t < ln[mi]) cv[mi] = *(const float4*)(e.c_state + (long)rm[mi] * e.ld_state + u);   // running f32 cell state, in place
    }
    // stores: uniform base + 32-bit lane byte offset (a time slab is far below 4 GiB: checked by the launchers), plain cache policy (evc_common.h store16<>) -
    // also for the write-once tapes of the backward pass (gate records, bf16 cell history)
    constexpr int SP = 0, TP = 0;
#pragma unroll
    for (int mi = 0; mi < Cfg::MI; ++mi) {
      const int m = m0 + tc.row0 + mi * 16;
      if (ln[mi] < 0) continue;
      const uint32_t hu = (uint32_t)m * (uint32_t)H + (uint32_t)u;                      // element index in an [M][H] slab
      const uint32_t su4 = ((uint32_t)rm[mi] * (uint32_t)e.ld_state + (uint32_t)u) * 4u;   // byte offset in c_state / h_state
      // byte offset of this lane's 4 units in hout: FP8 rows are [f16(h) (H halfwords) | e4m3 (H bytes)] = 3H bytes, wide f16 rows 2H halfwords
      const bool rows8 = FP8 && e.h_wide >= 2;        // (an FP8 launch with h_wide 0 - evc_lstm_layer_fwd_f16_dith, whose e4m3 stages are the input's only - writes plain f16 rows)
      const bool rows8lo = FP8 && e.h_wide == 3;      // ... + the e4m3 image of h's own low-order half: rows of 4H bytes
      const uint32_t rowb = (uint32_t)m * (uint32_t)((rows8lo ? 4 : 3) * H);
      const uint32_t hw2 = rows8 ? rowb + (uint32_t)u * 2u : (F16 && e.h_wide == 1) ? ((uint32_t)m * (uint32_t)(2 * H) + (uint32_t)u) * 2u : hu * 2u;
      const uint32_t h8o = rowb + (uint32_t)(2 * H) + (uint32_t)u;      // (FP8: the row's e4m3 part)
      const u32x2_t z2 = {0u, 0u};
      if (e.t >= ln[mi]) {          // dynamic_rnn: state copied through, zero output
        store8<SP>(e.hout, hw2, z2);
        if (rows8) store4<SP>(e.hout, h8o, 0u);
        else if (F16 && e.h_wide == 1) store8<SP>(e.hout, hw2 + (uint32_t)H * 2u, z2);
        if (rows8lo) store4<SP>(e.hout, h8o + (uint32_t)H, 0u);
        if (F16) store8<SP>(e.hout_lo, hu * 2u, z2);
        if (SPLIT) {
          const uint32_t wo = ((uint32_t)m * (uint32_t)(2 * H) + (uint32_t)u) * 2u;
          store8<SP>(e.hout_lo, wo, z2);
          store8<SP>(e.hout_lo, wo + (uint32_t)H * 2u, z2);
        }
        if (e.t == 0) {             // zero-length row: its final state is the zero initial state
          const u32x4_t z4 = {0u, 0u, 0u, 0u};
          store16<SP>(e.c_state, su4, z4);
          store16<SP>(e.h_state, su4, z4);
        }
        continue;
      }
      float zi[4], zj[4], zf[4], zo[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {                     // bias and forget_bias are already in the accumulators
        zi[r] = acc[mi][0][ni][r]; zj[r] = acc[mi][1][ni][r]; zf[r] = acc[mi][2][ni][r]; zo[r] = acc[mi][3][ni][r];
      }
      if (e.zx) {                   // hoisted x-projection (small-M stacks: one or two fragments per lane)
        const float* zr = e.zx + (long)m * e.ldzx + u;
        const float4 a = *(const float4*)zr, b = *(const float4*)(zr + H), c = *(const float4*)(zr + 2 * H), d = *(const float4*)(zr + 3 * H);
        zi[0] += a.x; zi[1] += a.y; zi[2] += a.z; zi[3] += a.w;
        zj[0] += b.x; zj[1] += b.y; zj[2] += b.z; zj[3] += b.w;
        zf[0] += c.x; zf[1] += c.y; zf[2] += c.z; zf[3] += c.w;
        zo[0] += d.x; zo[1] += d.y; zo[2] += d.z; zo[3] += d.w;
      }
      const float co[4] = {cv[mi].x, cv[mi].y, cv[mi].z, cv[mi].w};
      float cn[4], hn[4];
      uint2 rec[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gi = sigmoidf_(zi[r]), gj = tanhf_(zj[r]), gf = sigmoidf_(zf[r]), go = sigmoidf_(zo[r]);
        cn[r] = co[r] * gf + gi * gj;
        hn[r] = tanhf_(cn[r]) * go;
        rec[r] = make_uint2(pack_bf16x2(gi, gj), pack_bf16x2(gf, go));
      }
      const u32x4_t cnv = {__float_as_uint(cn[0]), __float_as_uint(cn[1]), __float_as_uint(cn[2]), __float_as_uint(cn[3])};
      store16<SP>(e.c_state, su4, cnv);               // rows stop updating at t = len: what stays is the returned state
      if (e.c_hist) store8<TP>(e.c_hist, hu * 2u, u32x2_t{pack_bf16x2(cn[0], cn[1]), pack_bf16x2(cn[2], cn[3])});
      if (e.t == ln[mi] - 1)
        store16<SP>(e.h_state, su4, u32x4_t{__float_as_uint(hn[0]), __float_as_uint(hn[1]), __float_as_uint(hn[2]), __float_as_uint(hn[3])});
      const u32x2_t hb = {pack_bf16x2(hn[0], hn[1]), pack_bf16x2(hn[2], hn[3])};
      if (F16) {
        const uint32_t p01 = pack_f16x2_hw(hn[0], hn[1]), p23 = pack_f16x2_hw(hn[2], hn[3]);
        store8<SP>(e.hout, hw2, u32x2_t{p01, p23});
        if (rows8) {                // e4m3(h * 2^7): the activation operand of the weights' low-order halves (|h| < 1: no saturation)
          int w8 = __builtin_amdgcn_cvt_pk_fp8_f32(hn[0] * 128.0f, hn[1] * 128.0f, 0, false);
          w8 = __builtin_amdgcn_cvt_pk_fp8_f32(hn[2] * 128.0f, hn[3] * 128.0f, w8, true);
          store4<SP>(e.hout, h8o, (uint32_t)w8);
          if (rows8lo) {            // e4m3((h - f16(h)) 2^18): |h - f16(h)| <= 2^-12, at most 64 - against e4m3(W 2^6), the same 2^-24 as 7 + 17
            const float l0 = (hn[0] - f16_to_f32((f16_t)(p01 & 0xffffu))) * 262144.0f, l1 = (hn[1] - f16_to_f32((f16_t)(p01 >> 16))) * 262144.0f;
            const float l2 = (hn[2] - f16_to_f32((f16_t)(p23 & 0xffffu))) * 262144.0f, l3 = (hn[3] - f16_to_f32((f16_t)(p23 >> 16))) * 262144.0f;
            int v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l0, l1, 0, false);
            v8 = __builtin_amdgcn_cvt_pk_fp8_f32(l2, l3, v8, true);
            store4<SP>(e.hout, h8o + (uint32_t)H, (uint32_t)v8);
          }
        } else if (e.h_wide == 1) { // f16(h)/64: the operand of the weights' low-order halves (scaled by 64)
          const float s0 = f16_to_f32((f16_t)(p01 & 0xffffu)) * (1.0f / 64.0f), s1 = f16_to_f32((f16_t)(p01 >> 16)) * (1.0f / 64.0f);
          const float s2 = f16_to_f32((f16_t)(p23 & 0xffffu)) * (1.0f / 64.0f), s3 = f16_to_f32((f16_t)(p23 >> 16)) * (1.0f / 64.0f);
          store8<SP>(e.hout, hw2 + (uint32_t)H * 2u, u32x2_t{pack_f16x2_hw(s0, s1), pack_f16x2_hw(s2, s3)});
        }
        store8<SP>(e.hout_lo, hu * 2u, hb);
      } else {
        store8<SP>(e.hout, hu * 2u, hb);
      }
      if (SPLIT) {
        float lo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) lo[r] = hn[r] - bf16_to_f32(f32_to_bf16(hn[r]));
        const uint32_t wo = ((uint32_t)m * (uint32_t)(2 * H) + (uint32_t)u) * 2u;
        store8<SP>(e.hout_lo, wo, u32x2_t{pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3])});
        store8<SP>(e.hout_lo, wo + (uint32_t)H * 2u, hb);
      }
      if (e.gates) {                                   // 4 units x 8 bytes
        store16<TP>(e.gates, hu * 8u, u32x4_t{rec[0].x, rec[0].y, rec[1].x, rec[1].y});
        store16<TP>(e.gates, hu * 8u + 16u, u32x4_t{rec[2].x, rec[2].y, rec[3].x, rec[3].y});
      }
    }
  }
#ifdef EVC_STAMPS
  EVC_STAMP(p.stamp_slot, 3);
  wait_vmcnt<0>();                       // this wave's stores acknowledged
  EVC_STAMP(p.stamp_slot, 4);
  __syncthreads();
  EVC_STAMP(p.stamp_slot, 5);
#endif
}

template <class Cfg, bool SPLIT = false, bool F16 = false, bool FP8 = false, bool XINT = false>
__device__ __forceinline__ void lstm_fwd_step_body(const GemmOperands& p, const LstmFwdParams& e, int tiles_m, int tiles_n, int bid) {
  static_assert(!XINT || FP8, "the integer-frame form rides on the f16 + e4m3 loop");
  static_assert(Cfg::G == 4, "LSTM step needs the four gate groups");
  static_assert(!(SPLIT && F16), "split operands are bf16 halves");
  static_assert(!FP8 || (F16 && is_v3<Cfg>::value), "the e4m3 tail rides behind f16 stages of the 64-wide ring loop");
  const int nwg = tiles_m * tiles_n;
  EVC_STAMP(p.stamp_slot, 0);
  const int id = xcd_remap(bid, nwg);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * Cfg::BM, u0 = tn * Cfg::BU;
  f32x4 acc[Cfg::MI][4][Cfg::NI];
  lstm_fwd_acc_bias<Cfg>(e, u0, acc);
  // (SPLIT: the split-bf16 products hi.hi + hi.lo + lo.hi are a K-EXTENSION of the same loop - the caller hands A = [lo | hi] rows
  //  against B = [W_hi | W_lo] rows as segment 1 and A = hi against B2 = W_hi as segment 2, evc_lstm_layer_fwd_hp - so the loop
  //  itself is the plain one; only the epilogue differs: it writes h_t's wide [lo | hi] image for the next step.)
  // (XINT, round 6: e.bias holds (255/256) colsum(f16(Wx)) here - the accumulators start from the constant term of the dequantised frames - and the
  //  loop rescales them by the frame's factor and adds the true bias behind the x-part: LOOP_ROW_SCALE)
  run_mainloop<Cfg, 4, true, false, FWD_LOOP_MODE | (F16 ? LOOP_F16 : 0) | (FP8 ? LOOP_FP8_TAIL : 0) | (XINT ? LOOP_ROW_SCALE : 0)>(p, m0, u0, acc);   // transposed accumulators: lane = one row, 4 consecutive units
  EVC_STAMP(p.stamp_slot, 2);
  lstm_fwd_epilogue<Cfg, SPLIT, F16, FP8>(p, e, m0, u0, acc);
}

// Two tiles per workgroup (round 5; bf16, the 64-wide ring tiles): layer 0's step s and layer 1's step s-1 of a two-layer L1 level are
// independent, so one launch runs both - every workgroup computes tile (tm, tn) of step a, then the same tile of step b.  Once every wave
// has left the ring, the first stages of tile b are issued (gemm_mainloop_v3 PHASE 1) and land under tile a's gate tail (which needs no
// LDS); tile b's loop starts on them (PHASE 2).  Per pair of steps that is one ring fill and one kernel boundary less.
// (round 6, the "high" L1 level: tile a = layer 0 on f16 + e4m3 stages (FP8, XINT: integer frames), tile b = the dithered upper layer on plain f16 stages
//  (FP8B = false) - each tile's loop and gate tail in its own mode, the PHASE split as in bf16)
template <class Cfg, bool F16 = false, bool FP8 = false, bool XINT = false, bool FP8B = FP8>
__global__ __launch_bounds__(Cfg::NT) void lstm_fwd_walk2_kernel(GemmOperands pa, LstmFwdParams ea, int tiles_ma, GemmOperands pb, LstmFwdParams eb,
                                                                 int tiles_mb, int tiles_n) {
  static_assert(is_v3<Cfg>::value && Cfg::G == 4, "tile walk: the 64-wide ring tiles");
  static_assert((!FP8 && !FP8B) || F16, "the e4m3 tail rides behind f16 stages");
  static_assert(!XINT || FP8, "the integer-frame form rides on the f16 + e4m3 loop");
  constexpr int MODE_A = FWD_LOOP_MODE | (F16 ? LOOP_F16 : 0) | (FP8 ? LOOP_FP8_TAIL : 0) | (XINT ? LOOP_ROW_SCALE : 0);
  constexpr int MODE_B = FWD_LOOP_MODE | (F16 ? LOOP_F16 : 0) | (FP8B ? LOOP_FP8_TAIL : 0);
  const int tiles_m = tiles_ma > tiles_mb ? tiles_ma : tiles_mb;
  const int id = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  int tm, tn;
  tile_of(id, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * Cfg::BM, u0 = tn * Cfg::BU;
  const bool has_a = tm < tiles_ma, has_b = tm < tiles_mb;          // workgroup-uniform
  f32x4 acc[Cfg::MI][4][Cfg::NI];
  if (has_a) {
    lstm_fwd_acc_bias<Cfg>(ea, u0, acc);
    gemm_mainloop_v3<Cfg, true, false, MODE_A, 0>(pa, m0, u0, lds_dyn, acc);
    if (has_b) {
      __syncthreads();                                              // every wave has read its last ring slot
      gemm_mainloop_v3<Cfg, true, false, MODE_B, 1>(pb, m0, u0, lds_dyn, acc);
    }
    lstm_fwd_epilogue<Cfg, false, F16, FP8>(pa, ea, m0, u0, acc);
    if (has_b) {
      __builtin_amdgcn_sched_barrier(0);                            // (keep tile b's address set-up out of tile a's tail: register pressure)
      asm volatile("" ::: "memory");
      lstm_fwd_acc_bias<Cfg>(eb, u0, acc);
      gemm_mainloop_v3<Cfg, true, false, MODE_B, 2>(pb, m0, u0, lds_dyn, acc);
      lstm_fwd_epilogue<Cfg, false, F16, FP8B>(pb, eb, m0, u0, acc);
    }
  } else if (has_b) {
    lstm_fwd_acc_bias<Cfg>(eb, u0, acc);
    gemm_mainloop_v3<Cfg, true, false, MODE_B, 0>(pb, m0, u0, lds_dyn, acc);
    lstm_fwd_epilogue<Cfg, false, F16, FP8B>(pb, eb, m0, u0, acc);
  }
}
#ifdef EVC_STAMPS
extern "C" int evc_debug_read_stamps(unsigned long long* out) {     // out: [8][512][8]
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(evc_stamps), sizeof(unsigned long long) * 8 * 512 * 8) == hipSuccess ? 0 : 1;
}
#endif

template <class Cfg, bool SPLIT = false, bool F16 = false, bool FP8 = false, bool XINT = false>
__global__ __launch_bounds__(Cfg::NT) void lstm_fwd_step_kernel(GemmOperands p, LstmFwdParams e, int tiles_m, int tiles_n) {
  lstm_fwd_step_body<Cfg, SPLIT, F16, FP8, XINT>(p, e, tiles_m, tiles_n, blockIdx.x);
}

// Two independent steps of the same geometry in one launch (the first tiles_m*tiles_n workgroups run step a, the
// rest step b): layer 0 at time t+1 and layer 1 at time t of a two-layer stack with M ~ batch rows - those steps are
// latency-bound (12 us for 2 GFLOP), so the pair costs about what one of them does and the stack's chain of
// dependent launches is T+1 long instead of 2T (evc_lstm_stack2_fwd).
template <class Cfg, bool F16 = false, bool FP8 = false>
__global__ __launch_bounds__(Cfg::NT) void lstm_fwd_pair_kernel(GemmOperands pa, LstmFwdParams ea, GemmOperands pb, LstmFwdParams eb,
                                                                int tiles_m, int tiles_n) {
  const int n = tiles_m * tiles_n;
  const bool first = blockIdx.x < n;                   // workgroup-uniform: scalar selects of the two argument sets
  const GemmOperands p = first ? pa : pb;
  const LstmFwdParams e = first ? ea : eb;
  lstm_fwd_step_body<Cfg, false, F16, FP8>(p, e, tiles_m, tiles_n, first ? blockIdx.x : blockIdx.x - n);
}


// ===========================================================================
// Host side: every entry point describes its layers as FwdLayer records, fwd_step() turns (call, layer, t) into the
// arguments of one launch, fwd_layer_loop / fwd_wavefront walk the steps, and the entry's launcher picks the kernel for the tile
// ===========================================================================
typedef TileCfg<128, 4, 32, 2, 2> CfgLstmBig;    // 128 rows x 32 units x 4 gates
typedef TileCfg<64, 4, 16, 4, 1> CfgLstmSmall;   // 64 rows x 16 units x 4 gates (M ~ 256 steps)
// v2 tiles: BM rows x 64 units x 4 gates (256 accumulator columns).  The row count of a step varies with the
// batch (row plans drop the padding rows), so the tile height is chosen per launch to cut the active rows
// into a multiple of 256 workgroups: 5120 rows -> 320, ~3600 -> 224, ...
typedef TileCfg2<320, 4, 64, 2, 4, 4, false> CfgLstmV2a;
typedef TileCfg2<288, 4, 64, 2, 4, 4, false> CfgLstmV2_288;
typedef TileCfg2<256, 4, 64, 2, 4, 5, true> CfgLstmV2b;
typedef TileCfg2<224, 4, 64, 2, 4, 5, true> CfgLstmV2_224;
// The tall forward tiles on 64-wide K stages (gemm_core_v3.h): two stages of 60-64 KB instead of five of 30-32 KB - whole cache
// lines per LDS-DMA piece and one barrier per 64 K columns beat the deeper ring (same-box A/B: 79.0 -> 73.9 us per step)
typedef TileCfg3<256, 4, 64, 2, 4, 2> CfgLstmV3_256;
typedef TileCfg3<224, 4, 64, 2, 4, 2> CfgLstmV3_224;
// 240 rows = 7 row fragments on the producer waves + 8 on their SIMD partners (gemm_core_v3.h, uneven split): 3 585-3 840 live rows are 16 row tiles
// = 256 workgroups of 240 rows instead of 15 x 16 = 240 workgroups of 256 rows (round 4)
typedef TileCfg3<240, 4, 64, 2, 4, 2, 7> CfgLstmV3_240;
typedef TileCfg3<224, 4, 64, 2, 4, 2, 6> CfgLstmV3_224u;      // 6 + 8 instead of 7 + 7: the producer waves issue the LDS-DMA, their partners take the extra row fragment (58.3 -> 58.0 us per launch)
typedef TileCfg3<192, 4, 64, 2, 4, 2> CfgLstmV3_192;
typedef TileCfg3<160, 4, 64, 2, 4, 3> CfgLstmV3_160;
typedef TileCfg2<192, 4, 64, 2, 4, 5, true> CfgLstmV2_192;
typedef TileCfg2<160, 4, 64, 2, 4, 5, true> CfgLstmV2_160;
typedef TileCfg2<128, 4, 64, 2, 4, 5, true> CfgLstmV2_128;
typedef TileCfg2<64, 4, 64, 2, 4, 5, true> CfgLstmV2_64;
typedef TileCfg3<64, 4, 16, 4, 1, 4> CfgLstmV3Small;         // 64 rows x 16 units x 4 gates on 64-wide K stages, 4 waves (64 KB of LDS: still two workgroups per CU): M ~ batch steps

// ---- the call and its layers ------------------------------------------------------------------------------------------------------------
// What the layers of one call share
struct FwdShared {
  const int32_t* len; int T, M, H; long ld_state;
  const int32_t* row_map; const int32_t* rows_per_step;      // row plan (evc_sort_rows_by_len) or NULL
  int rows(int t) const { return rows_per_step ? rows_per_step[t] : M; }      // active rows of step t: the prefix [0, rows)
};

// One layer of a call, in the units the kernels take (16-bit operands in halfwords - bf16_t stands for f16 containers too - e4m3 ones in bytes).
// Step t contracts [x_t | h_{t-1}] against the rows of B, then - e4m3 forms - the e4m3 parts of the same rows against the rows of B8, and writes
// slab t + 1 of the h ring; at t = 0 the h segments are absent (h_{-1} = 0).
struct FwdLayer {
  // x rows of step t at x + t * M * ldx, kx halfwords contracted.  zx != NULL: that product was hoisted out of the steps ([T][M][4H] f32, added
  // in the gate tail); the step's only 16-bit segment is then the h ring itself
  const bf16_t* x = nullptr; long ldx = 0; int kx = 0;
  const float* zx = nullptr;
  bf16_t* h = nullptr; long ldh = 0; int kh = 0;          // h ring [T+1][M][ldh], kh halfwords of a row contracted
  int h_wide = 0;                                        // layout of its rows (LstmFwdParams::h_wide)
  bf16_t* h_copy = nullptr; long ld_copy = 0;            // second ring the tail writes (LstmFwdParams::hout_lo) or NULL
  const bf16_t* B = nullptr; long ldb = 0;               // weight image [4H][ldb]; step t reads the image at B + t * w_step_stride (time-dithered images)
  long w_step_stride = 0;
  // e4m3 segments (B8 != NULL): kx8 bytes at byte x8_off of the x rows, then kh8 bytes behind the H halfwords of the h rows, against B8's rows
  // (b8_gap bytes skipped between the two); kx8 = 0: the h rows' bytes alone
  const uint8_t* B8 = nullptr; long ldb8 = 0, b8_gap = 0; int scale8_exp = 0;
  long x8_off = 0; int kx8 = 0, kh8 = 0;
  // integer frames (row_scale != NULL): behind the x-part acc = acc * row_scale[t][row] + col_add (+ 1 on the forget gate); the accumulators
  // then start from `bias` = the constant term of the dequantised frames and col_add is the true bias
  const float* row_scale = nullptr; const float* col_add = nullptr;
  const float* bias = nullptr; float* c_state = nullptr; float* h_state = nullptr;
  void* gates = nullptr; bf16_t* c_all = nullptr;        // the backward pass's tapes, both or neither
};

// ---- refusals: each returns the error code, the message names the entry -------------------------------------------------------------------
static inline bool aligned_to(const void* p, int a) { return ((uintptr_t)p % a) == 0; }

static inline int fwd_shape_ok(const char* entry, int T, int M, int K, int H, int h_mult = 64, int h_min = 64) {
  EVC_REQUIRE(T > 0 && M > 0 && K > 0 && H >= h_min && K % 64 == 0 && H % h_mult == 0, EVC_ERR_BAD_SHAPE,
              "%s: bad shape T=%d M=%d K=%d (%%64) H=%d (%%%d, >= %d)", entry, T, M, K, H, h_mult, h_min);
  return EVC_OK;
}

// x rows that carry an e4m3 part: kx16 halfwords at the row start, kx8 bytes at byte x8_off, row stride ldx halfwords
static inline int fwd_x8_ok(const char* entry, const void* x, long ldx, int kx16, long x8_off, int kx8) {
  EVC_REQUIRE(kx8 > 0 && kx8 % 128 == 0 && kx8 >= 384, EVC_ERR_BAD_SHAPE,
              "%s: kx8=%d (%%128, >= 384: the ring must be full of e4m3 stages at t = 0)", entry, kx8);
  EVC_REQUIRE(ldx % 8 == 0 && x8_off % 16 == 0 && ldx >= kx16 && ldx * 2 >= x8_off + kx8 && aligned_to(x, 16), EVC_ERR_BAD_ALIGN,
              "%s: ldx=%ld (%%8, >= kx16=%d), x8_off=%ld (%%16), x 16-byte aligned", entry, ldx, kx16, x8_off);
  return EVC_OK;
}

static inline int fwd_xint_ok(const char* entry, const float* x_row_scale, const float* x_col_const, int b8_gap) {
  EVC_REQUIRE((x_row_scale == nullptr) == (x_col_const == nullptr) && b8_gap >= 0 && b8_gap % 128 == 0 && (x_row_scale || b8_gap == 0) &&
              aligned_to(x_col_const, 16), EVC_ERR_BAD_ARG,
              "%s: x_row_scale and x_col_const go together (16-byte aligned), b8_gap=%d (%%128) only with them", entry, b8_gap);
  return EVC_OK;
}

static inline int fwd_shared_ok(const char* entry, const FwdShared& S) {
  EVC_REQUIRE(fwd_tail_ok(S.M, S.H, S.ld_state), EVC_ERR_BAD_SHAPE, "%s: a gate-record / state slab spans 4 GiB or more (M=%d H=%d ld_state=%ld)",
              entry, S.M, S.H, S.ld_state);
  EVC_REQUIRE(S.ld_state % 4 == 0, EVC_ERR_BAD_ALIGN, "%s: ld_state=%ld must be a multiple of 4 (16-byte state rows)", entry, S.ld_state);
  return rows_per_step_ok(entry, S.rows_per_step, S.T, S.M);
}

// h_align: 8 bytes for rings of plain 16-bit rows, 16 for the rows that carry e4m3 parts or a second image
static inline int fwd_layer_ok(const char* entry, const FwdLayer& L, int h_align, int copy_align = 8) {
  EVC_REQUIRE(aligned_to(L.c_state, 16) && aligned_to(L.h_state, 16) && aligned_to(L.bias, 16) && aligned_to(L.col_add, 16) &&
              aligned_to(L.h, h_align) && aligned_to(L.h_copy, copy_align), EVC_ERR_BAD_ALIGN,
              "%s: state / bias must be 16-byte aligned, the h buffers %d- / %d-byte", entry, h_align, copy_align);
  EVC_REQUIRE((L.gates == nullptr) == (L.c_all == nullptr), EVC_ERR_BAD_ARG, "%s: gates and c_all go together", entry);
  EVC_REQUIRE(aligned_to(L.gates, 16) && aligned_to(L.c_all, 8), EVC_ERR_BAD_ALIGN, "%s: gates must be 16-byte, c_all 8-byte aligned", entry);
  return EVC_OK;
}

static inline int fwd_layers2_ok(const char* entry, const FwdLayer& L0, const FwdLayer& L1, int h_align) {
  EVC_TRY(fwd_layer_ok(entry, L0, h_align));
  EVC_TRY(fwd_layer_ok(entry, L1, h_align));
  EVC_REQUIRE((L0.gates == nullptr) == (L1.gates == nullptr), EVC_ERR_BAD_ARG, "%s: gates and c_all go together, for both layers", entry);
  return EVC_OK;
}

// h_{-1} = 0: slab 0 of a layer's rings (the state buffers need no clearing: step 0 treats c_old as 0 and writes the zero state of the
// zero-length rows it covers itself; rows beyond rows_per_step[0] are the caller's)
static inline int fwd_clear_h(const FwdShared& S, const FwdLayer& L, hipStream_t st) {
  EVC_CHECK_HIP(hipMemsetAsync(L.h, 0, (size_t)S.M * L.ldh * sizeof(bf16_t), st));
  return EVC_OK;
}
static inline int fwd_clear_copy(const FwdShared& S, const FwdLayer& L, hipStream_t st) {
  EVC_CHECK_HIP(hipMemsetAsync(L.h_copy, 0, (size_t)S.M * L.ld_copy * sizeof(bf16_t), st));
  return EVC_OK;
}

// ---- one step ---------------------------------------------------------------------------------------------------------------------------
struct FwdStep { GemmOperands p; LstmFwdParams e; int k1, k2; };      // k1, k2: halfwords of the two 16-bit segments (the launchers divide by the tile's K step)

static inline FwdStep fwd_step(const FwdShared& S, const FwdLayer& L, int t) {
  FwdStep s{};
  const int M = S.M, H = S.H;
  const long slab = (long)M * H;
  const bf16_t* hprev = L.h + (long)t * M * L.ldh;
  const bf16_t* xt = L.x ? L.x + (long)t * M * L.ldx : nullptr;
  const int kh = t == 0 ? 0 : L.kh;
  GemmOperands& p = s.p;
  p.M = S.rows(t); p.Nu = H; p.group_stride = H;
  p.B = L.B + (long)t * L.w_step_stride; p.ldb = L.ldb;
  p.A2 = hprev; p.lda2 = L.ldh;
  if (L.zx) { p.A1 = hprev; p.lda1 = L.ldh; s.k1 = kh; s.k2 = 0; }
  else { p.A1 = xt; p.lda1 = L.ldx; s.k1 = L.kx; s.k2 = kh; }
  if (L.B8) {
    const uint8_t* h8 = (const uint8_t*)(hprev + H);
    const int nh8 = (t == 0 ? 0 : L.kh8) / 128;
    if (L.kx8) { p.A3 = (const uint8_t*)xt + L.x8_off; p.lda3 = L.ldx * 2; p.nk3 = L.kx8 / 128; }
    else { p.A3 = h8; p.lda3 = L.ldh * 2; p.nk3 = nh8; }
    if (L.kx8 && L.kh8) { p.A4 = h8; p.lda4 = L.ldh * 2; p.nk4 = nh8; }
    else { p.A4 = p.A3; p.lda4 = p.lda3; p.nk4 = 0; }                  // one e4m3 segment only
    p.B8 = L.B8; p.ldb8 = L.ldb8; p.b8_gap = L.b8_gap; p.scale8_exp = L.scale8_exp;
  }
  if (L.row_scale) { p.row_scale = L.row_scale + (long)t * M; p.col_add = L.col_add; p.g2_add = 1.0f; }
  LstmFwdParams& e = s.e;
  e.zx = L.zx ? L.zx + (long)t * M * 4 * H : nullptr; e.ldzx = 4L * H;
  e.bias = L.bias; e.len = S.len; e.t = t;
  e.c_state = L.c_state; e.h_state = L.h_state; e.ld_state = S.ld_state;
  e.hout = L.h + (long)(t + 1) * M * L.ldh; e.h_wide = L.h_wide;
  e.hout_lo = L.h_copy ? L.h_copy + (long)(t + 1) * M * L.ld_copy : nullptr;
  e.gates = L.gates ? (uint2*)L.gates + t * slab : nullptr;
  e.c_hist = L.c_all ? L.c_all + (t + 1) * slab : nullptr;             // slab t+1 = c after step t
  e.row_map = S.row_map;
  e.M = p.M; e.H = H;
  return s;
}

// A layer alone: one launch per step, until the row plan runs out of rows
template <class Launch>
static inline void fwd_layer_loop(const FwdShared& S, const FwdLayer& L, Launch&& launch) {
  for (int t = 0; t < S.T && S.rows(t) > 0; ++t) launch(fwd_step(S, L, t));
}

// Two layers as a wavefront: launch s = layer 0's step s (a) next to layer 1's step s - 1 (b), T + 1 launches.  A level's first launch has only
// role a, its last only role b, and a row plan may leave a role without rows (layer 1 runs the earlier step: at least as many rows as layer 0);
// the absent role gets a copy of the present one's arguments (never read).  launch(a, has_a, b, has_b) decides one launch or two.
template <class Launch>
static inline void fwd_wavefront(const FwdShared& S, const FwdLayer& L0, const FwdLayer& L1, Launch&& launch) {
  for (int s = 0; s <= S.T; ++s) {
    const bool has_a = s < S.T && S.rows(s) > 0, has_b = s >= 1 && S.rows(s - 1) > 0;
    if (!has_a && !has_b) continue;
    const FwdStep one = has_a ? fwd_step(S, L0, s) : fwd_step(S, L1, s - 1);
    if (has_a && has_b) launch(one, true, fwd_step(S, L1, s - 1), true);
    else launch(one, has_a, one, has_b);
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------------
template <class Cfg, bool SPLIT = false, bool F16 = false, bool FP8 = false, bool XINT = false>
static inline void launch_lstm_fwd(const FwdStep& s, hipStream_t st) {
  GemmOperands p = s.p;
  p.nk1 = s.k1 / kdiv<Cfg>(); p.nk2 = s.k2 / kdiv<Cfg>();
#ifdef EVC_STAMPS
  p.stamp_slot = s.e.t & 7;
#endif
  const int tm = ceil_div(s.e.M, Cfg::BM), tn = ceil_div(s.e.H, Cfg::BU);
  launch_cfg<Cfg>(lstm_fwd_step_kernel<Cfg, SPLIT, F16, FP8, XINT>, tm * tn, st, p, s.e, tm, tn);
}

// both roles in one launch whose workgroups walk both tiles (lstm_fwd_walk2_kernel); with one role, the same kernel: every launch of a level
// carries one kernel name - the per-kernel averages of a profile then cover exactly the launches bench.py times
template <class Cfg, bool F16 = false, bool FP8 = false, bool XINT = false, bool FP8B = FP8>
static inline void launch_lstm_fwd_walk2(const FwdStep& a, bool has_a, const FwdStep& b, bool has_b, hipStream_t st) {
  GemmOperands pa = a.p, pb = b.p;
  pa.nk1 = a.k1 / 64; pa.nk2 = a.k2 / 64;
  pb.nk1 = b.k1 / 64; pb.nk2 = b.k2 / 64;
  const int tma = has_a ? ceil_div(a.e.M, Cfg::BM) : 0, tmb = has_b ? ceil_div(b.e.M, Cfg::BM) : 0, tn = ceil_div(a.e.H, Cfg::BU);
  launch_cfg<Cfg>(lstm_fwd_walk2_kernel<Cfg, F16, FP8, XINT, FP8B>, (tma > tmb ? tma : tmb) * tn, st, pa, a.e, tma, pb, b.e, tmb, tn);
}

// both roles (same geometry) as the two halves of one grid (lstm_fwd_pair_kernel)
template <class Cfg, bool F16 = false, bool FP8 = false>
static inline void launch_lstm_fwd_pair(const FwdStep& a, const FwdStep& b, hipStream_t st) {
  GemmOperands pa = a.p, pb = b.p;
  pa.nk1 = a.k1 / kdiv<Cfg>(); pa.nk2 = a.k2 / kdiv<Cfg>();
  pb.nk1 = b.k1 / kdiv<Cfg>(); pb.nk2 = b.k2 / kdiv<Cfg>();
  const int tm = ceil_div(a.e.M, Cfg::BM), tn = ceil_div(a.e.H, Cfg::BU);
  launch_cfg<Cfg>(lstm_fwd_pair_kernel<Cfg, F16, FP8>, 2 * tm * tn, st, pa, a.e, pb, b.e, tm, tn);
}

// ---- tile choice: two cost-model tables, one dispatcher each -----------------------------------------------------------------------------------
// the tiles lstm_fwd_walk2_kernel is built for
template <class Cfg> struct is_walk2_tile {
  static constexpr bool value = std::is_same<Cfg, CfgLstmV3_256>::value || std::is_same<Cfg, CfgLstmV3_240>::value || std::is_same<Cfg, CfgLstmV3_224u>::value;
};

// forward tile for a step over `rows` rows: index into {320, 288, 256, 224, 192, 160 (v2), 128 (v1), 64 (v1), 128 (v2), 64 (v2), 240}
static inline int pick_fwd_tile(int rows, int H) {
  constexpr int NC = 11;
  static const int bm[NC] = {320, 288, 256, 224, 192, 160, 128, 64, 128, 64, 240};
  static const int bn[NC] = {256, 256, 256, 256, 256, 256, 128, 64, 256, 256, 256};
  static const int bu[NC] = {64, 64, 64, 64, 64, 64, 32, 16, 64, 64, 64};
  static const double cf[NC] = {1.0, 1.0, 1.0, 1.02, 1.04, 1.08, 1.3, 2.6, 1.15, 1.5, 1.01};   // smaller tiles: less efficient per flop
  int best = 0;
  double bc = 1e300;
  for (int i = 0; i < NC; ++i) {
    const double c = tile_cost((long)ceil_div(rows, bm[i]) * ceil_div(H, bu[i]), bm[i], bn[i], cf[i]);
    if (c < bc) { bc = c; best = i; }
  }
  const int f = forced_tile();        // debug: 1 -> 256, 2 -> v1 128, 3 -> v1 64, 4 -> 320, 5 -> 288, 6 -> 224, 7 -> 192, 8 -> 160, 9 -> v2 128, 10 -> v2 64, 11 -> 240
  if (f) { static const int map[12] = {0, 2, 6, 7, 0, 1, 3, 4, 5, 8, 9, 10}; best = map[f < 12 ? f : 0]; }
  return best;
}

// f(TileTag<Cfg>()) for the tile of a pick_fwd_tile() index.  RING32 (evc_lstm_stack2_fwd alone): picks 2-5 on the 32-wide ring tiles instead of
// the 64-wide ones, and no 240-row tile - that pick lands on the 64 x 16 default (open observation)
template <bool RING32 = false, class F>
static inline auto with_fwd_tile(int pick, F&& f) {
  switch (pick) {
    case 0: return f(TileTag<CfgLstmV2a>());
    case 1: return f(TileTag<CfgLstmV2_288>());
    case 2: return f(TileTag<std::conditional_t<RING32, CfgLstmV2b, CfgLstmV3_256>>());
    case 3: return f(TileTag<std::conditional_t<RING32, CfgLstmV2_224, CfgLstmV3_224u>>());
    case 4: return f(TileTag<std::conditional_t<RING32, CfgLstmV2_192, CfgLstmV3_192>>());
    case 5: return f(TileTag<std::conditional_t<RING32, CfgLstmV2_160, CfgLstmV3_160>>());
    case 6: return f(TileTag<CfgLstmBig>());
    case 8: return f(TileTag<CfgLstmV2_128>());
    case 9: return f(TileTag<CfgLstmV2_64>());
    case 10: return f(TileTag<std::conditional_t<RING32, CfgLstmSmall, CfgLstmV3_240>>());
    default: return f(TileTag<CfgLstmSmall>());
  }
}

// forward tile among the 64-wide ring tiles only (the e4m3 tail lives in gemm_core_v3.h): index into {256, 224, 192, 160, 240}
static inline int pick_fwd_tile_v3(int rows, int H) {
  static const int bm[5] = {256, 224, 192, 160, 240};
  static const double cf[5] = {1.0, 1.02, 1.04, 1.08, 1.01};
  int best = 0;
  double bc = 1e300;
  for (int i = 0; i < 5; ++i) {
    const double c = tile_cost((long)ceil_div(rows, bm[i]) * ceil_div(H, 64), bm[i], 256, cf[i]);
    if (c < bc) { bc = c; best = i; }
  }
  const int f = forced_tile();        // debug: 1 -> 256, 6 -> 224, 7 -> 192, 8 -> 160, 11 -> 240
  if (f == 1) best = 0; else if (f == 6) best = 1; else if (f == 7) best = 2; else if (f == 8) best = 3; else if (f == 11) best = 4;
  return best;
}

// f(TileTag<Cfg>()) for the tile of a pick_fwd_tile_v3() index.  C224: the 224-row tile's row split - 6 + 8 (CfgLstmV3_224u) for the f16 and
// two-tile forms, 7 + 7 (CfgLstmV3_224) for the steps with an e4m3 tail
template <class C224, class F>
static inline auto with_fwd_tile_v3(int pick, F&& f) {
  switch (pick) {
    case 0: return f(TileTag<CfgLstmV3_256>());
    case 1: return f(TileTag<C224>());
    case 2: return f(TileTag<CfgLstmV3_192>());
    case 4: return f(TileTag<CfgLstmV3_240>());
    default: return f(TileTag<CfgLstmV3_160>());
  }
}

// one bf16 / f16 step on the tile of `pick` (pick_fwd_tile)
template <bool F16>
static inline void launch_fwd_step(const FwdStep& s, int pick, hipStream_t st) {
  with_fwd_tile(pick, [&](auto tile) { launch_lstm_fwd<typename decltype(tile)::type, false, F16>(s, st); });
}

// one f16 + e4m3 step on the tile of `pick` (pick_fwd_tile_v3); xint: the integer-frame form
static inline void launch_fwd_step_e4m3(const FwdStep& s, int pick, bool xint, hipStream_t st) {
  with_fwd_tile_v3<CfgLstmV3_224>(pick, [&](auto tile) {
    typedef typename decltype(tile)::type Cfg;
    if (xint) launch_lstm_fwd<Cfg, false, true, true, true>(s, st);
    else launch_lstm_fwd<Cfg, false, true, true>(s, st);
  });
}

// ===========================================================================
// One layer, bf16 or IEEE f16
// ===========================================================================
// f16: x, wT, hbuf hold IEEE f16 (16-bit containers) and one v_mfma_f32_16x16x32_f16 product is issued per depth - the cost of the bf16 step
// with 8x smaller operand rounding; hbuf_bf16 receives the bf16 copy of every h_t (what the BPTT products contract over); ldx = row stride of x
// (0: Kin); h_wide: hbuf rows are [h | h/64] (2H) and the kernel's h-part is [Wh | Wh_lo*64] (2H): the recurrent weights K-extended by their
// low-order halves.  w_step_stride (elements; 0 = one image): step t contracts the weight image at wT + t * w_step_stride (time-dithered f16
// images, evc_lstm_layer_fwd_f16_dith).  (The split-bf16 form of a layer is evc_lstm_layer_fwd_hp below.)
static int lstm_layer_fwd_impl(const char* entry, const evc_bf16* x, const evc_bf16* wT, const float* bias, const int32_t* len,
                               int T, int M, int Kin, int H, int hoist, float* zx_ws,
                               evc_bf16* hbuf, float* c_state, float* h_state, int64_t ld_state,
                               void* gates, evc_bf16* c_all, evc_bf16* hbuf_bf16,
                               const int32_t* row_map, const int32_t* rows_per_step, void* stream, int f16 = 0, int64_t ldx = 0, int h_wide = 0,
                               int64_t w_step_stride = 0) {
  if (ldx == 0) ldx = Kin;
  const long ldh = h_wide ? 2L * H : H;            // row stride of hbuf = K of the recurrent part
  const long ldw = Kin + ldh;
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H));
  EVC_REQUIRE(ring_operand_ok(M, ldx > ldh ? ldx : ldh) && ring_operand_ok(4L * H, (long)Kin + ldh), EVC_ERR_BAD_SHAPE,
              "%s: a time slab or the kernel spans 4 GiB or more (M=%d Kin=%d H=%d)", entry, M, Kin, H);
  EVC_REQUIRE(!hoist || (zx_ws && !h_wide && ldx == Kin), EVC_ERR_BAD_ARG, "%s: hoist needs zx_ws (and plain operands)", entry);
  const FwdShared S{len, T, M, H, ld_state, row_map, rows_per_step};
  FwdLayer L;
  L.x = x; L.ldx = ldx; L.kx = Kin;
  L.h = hbuf; L.ldh = ldh; L.kh = (int)ldh;
  L.B = hoist ? wT + Kin : wT; L.ldb = ldw;
  L.bias = bias; L.c_state = c_state; L.h_state = h_state; L.gates = gates; L.c_all = c_all;
  L.zx = hoist ? zx_ws : nullptr; L.h_wide = h_wide; L.w_step_stride = w_step_stride;
  if (f16) { L.h_copy = hbuf_bf16; L.ld_copy = H; }
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layer_ok(entry, L, 8));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L, st));
  if (f16) EVC_TRY(fwd_clear_copy(S, L, st));
  if (hoist) EVC_TRY(evc_gemm_nt(x, Kin, wT, ldw, zx_ws, 4L * H, T * M, 4 * H, Kin, nullptr, 0, 0, stream));
  fwd_layer_loop(S, L, [&](const FwdStep& s) {
    const int pick = pick_fwd_tile(s.e.M, H);
    if (f16) launch_fwd_step<true>(s, pick, st);
    else launch_fwd_step<false>(s, pick, st);
  });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

extern "C" int evc_lstm_layer_fwd(const evc_bf16* x, const evc_bf16* wT, const float* bias, const int32_t* len,
                                  int T, int M, int Kin, int H, int hoist, float* zx_ws,
                                  evc_bf16* hbuf, float* c_state, float* h_state, int64_t ld_state,
                                  void* gates, evc_bf16* c_all, const int32_t* row_map, const int32_t* rows_per_step,
                                  void* stream) {
  return lstm_layer_fwd_impl("evc_lstm_layer_fwd", x, wT, bias, len, T, M, Kin, H, hoist, zx_ws, hbuf, c_state, h_state, ld_state, gates, c_all,
                             nullptr, row_map, rows_per_step, stream);
}

extern "C" int evc_lstm_layer_fwd_f16(const evc_f16* x, int64_t ldx, const evc_f16* wT, const float* bias, const int32_t* len,
                                      int T, int M, int Kin, int H, evc_f16* hbuf, int h_wide, evc_bf16* hbuf_bf16,
                                      float* c_state, float* h_state, int64_t ld_state, void* gates, evc_bf16* c_all,
                                      const int32_t* row_map, const int32_t* rows_per_step, void* stream) {
  EVC_REQUIRE(hbuf_bf16, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16: hbuf_bf16 (the bf16 copy of h for the backward pass) is required");
  EVC_REQUIRE(ldx >= Kin && ldx % 8 == 0 && (h_wide == 0 || h_wide == 1), EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16: ldx=%ld (>= Kin=%d, %%8), h_wide=%d",
              (long)ldx, Kin, h_wide);
  return lstm_layer_fwd_impl("evc_lstm_layer_fwd_f16", (const evc_bf16*)x, (const evc_bf16*)wT, bias, len, T, M, Kin, H, 0, nullptr, (evc_bf16*)hbuf,
                             c_state, h_state, ld_state, gates, c_all, hbuf_bf16, row_map, rows_per_step, stream, 1, ldx, h_wide);
}

// ===========================================================================
// Two-layer L1 level (many rows, row plans), bf16: layer 0's step s and layer 1's step s-1 in ONE launch whose workgroups walk both tiles
// (lstm_fwd_walk2_kernel) - T + 1 launches instead of 2 T, one ring fill and one kernel boundary less per pair of steps; both layers contract
// [x_t | h_{t-1}] . W^T in one K walk (layer 1's x_t is layer 0's output slab).  Same arithmetic as two evc_lstm_layer_fwd calls: bit-identical
// results.  Launches whose tile is not one of the 64-wide ring tiles (224 / 240 / 256 rows) run as two separate launches.
// ===========================================================================
extern "C" int evc_lstm_level2_fwd(const evc_bf16* x, const evc_bf16* wT0, const float* bias0, const evc_bf16* wT1, const float* bias1,
                                   const int32_t* len, int T, int M, int Kin, int H, evc_bf16* hbuf0, evc_bf16* hbuf1,
                                   float* c_state0, float* h_state0, float* c_state1, float* h_state1, int64_t ld_state,
                                   void* gates0, evc_bf16* c_all0, void* gates1, evc_bf16* c_all1,
                                   const int32_t* row_map, const int32_t* rows_per_step, void* stream) {
  const char* entry = "evc_lstm_level2_fwd";
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H));
  EVC_REQUIRE(ring_operand_ok(M, Kin > H ? Kin : H) && ring_operand_ok(4L * H, (long)Kin + H) && ring_operand_ok(4L * H, 2L * H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_level2_fwd: a time slab or a kernel spans 4 GiB or more (M=%d Kin=%d H=%d)", M, Kin, H);
  EVC_REQUIRE(x && wT0 && wT1 && bias0 && bias1 && len && hbuf0 && hbuf1 && c_state0 && h_state0 && c_state1 && h_state1, EVC_ERR_BAD_ARG,
              "evc_lstm_level2_fwd: NULL operand");
  const FwdShared S{len, T, M, H, ld_state, row_map, rows_per_step};
  FwdLayer L0;
  L0.x = x; L0.ldx = Kin; L0.kx = Kin;
  L0.h = hbuf0; L0.ldh = H; L0.kh = H;
  L0.B = wT0; L0.ldb = (long)Kin + H;
  L0.bias = bias0; L0.c_state = c_state0; L0.h_state = h_state0; L0.gates = gates0; L0.c_all = c_all0;
  FwdLayer L1;
  L1.x = hbuf0 + (long)M * H; L1.ldx = H; L1.kx = H;      // x_t = layer 0's output slab t+1
  L1.h = hbuf1; L1.ldh = H; L1.kh = H;
  L1.B = wT1; L1.ldb = 2L * H;
  L1.bias = bias1; L1.c_state = c_state1; L1.h_state = h_state1; L1.gates = gates1; L1.c_all = c_all1;
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layers2_ok(entry, L0, L1, 8));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L0, st));
  EVC_TRY(fwd_clear_h(S, L1, st));
  fwd_wavefront(S, L0, L1, [&](const FwdStep& a, bool has_a, const FwdStep& b, bool has_b) {
    const bool walked = with_fwd_tile(pick_fwd_tile(has_b ? b.e.M : a.e.M, H), [&](auto tile) {
      typedef typename decltype(tile)::type Cfg;
      if constexpr (is_walk2_tile<Cfg>::value) { launch_lstm_fwd_walk2<Cfg>(a, has_a, b, has_b, st); return true; }
      else return false;
    });
    if (walked) return;
    if (has_a) launch_fwd_step<false>(a, pick_fwd_tile(a.e.M, H), st);
    if (has_b) launch_fwd_step<false>(b, pick_fwd_tile(b.e.M, H), st);
  });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ===========================================================================
// "High" precision L1 layers: f16 stages + e4m3 stages
// ===========================================================================
// Layer 0 of the two "high" L1 entries (evc_lstm_layer_fwd_f16_fp8lo, evc_lstm_level2_fwd_high): x rows [kx16 f16 | kx8 e4m3 at byte x8_off],
// h rows [f16(h) | e4m3(h 2^7) (| e4m3((h - f16(h)) 2^18) with h_lo)], wT8 rows [kx8 | b8_gap | kh8]
static inline FwdLayer fwd_layer_fp8lo(const evc_f16* x, int64_t ldx, int kx16, int64_t x8_off, int kx8, const evc_f16* wT16, const uint8_t* wT8,
                                       int w8_scale_exp, int h_lo, const float* bias, const float* x_row_scale, const float* x_col_const,
                                       int b8_gap, int H, evc_f16* hbuf, evc_bf16* hbuf_bf16, float* c_state, float* h_state, void* gates,
                                       evc_bf16* c_all) {
  const long ldh = h_lo ? 2L * H : 3L * H / 2;      // halfwords per hbuf row
  // integer frames: the accumulators start from x_col_const, the true bias is added behind the x-part
  FwdLayer L;
  L.x = x; L.ldx = ldx; L.kx = kx16;
  L.h = hbuf; L.ldh = ldh; L.kh = H;
  L.B = wT16; L.ldb = (long)kx16 + H;
  L.bias = x_col_const ? x_col_const : bias; L.c_state = c_state; L.h_state = h_state; L.gates = gates; L.c_all = c_all;
  L.h_wide = h_lo ? 3 : 2; L.h_copy = hbuf_bf16; L.ld_copy = H;
  L.x8_off = x8_off; L.kx8 = kx8; L.kh8 = h_lo ? 2 * H : H;
  L.B8 = wT8; L.ldb8 = (long)kx8 + b8_gap + L.kh8; L.b8_gap = b8_gap; L.scale8_exp = -(7 + w8_scale_exp);
  if (x_row_scale) { L.row_scale = x_row_scale; L.col_add = bias; }
  return L;
}

// "High" precision L1 layer with the weights' low-order halves contracted in fp8: per step
//   z = [x16 | h16] . [W16x | W16h]^T  (IEEE f16, v_mfma_f32_16x16x32_f16)  +  2^-(7 + w8_scale_exp) [x8 | h8] . [W8x | W8h]^T  (OCP e4m3,
//   v_mfma_scale_f32_16x16x128_f8f6f4: per K element twice the MFMA rate)
// with W8 = e4m3((W - f16(W)) 2^w8_scale_exp) (evc_cast_f32_to_fp8_lo), x8 = e4m3(x 2^7) and h8 = e4m3(h 2^7): the weights are exact to
// ~2^-15 relative instead of f16's 2^-11, for half the MFMA time of K-extending them by f16 low-order halves.  x rows: kx16 halfwords at
// the row start (any K-extension of the input the caller likes, against the first kx16 columns of wT16) and kx8 e4m3 bytes at byte
// offset x8_off of the same row (row stride ldx halfwords); hbuf rows [T+1][M]: [f16(h_t) (H halfwords) | e4m3(h_t 2^7) (H bytes)] (3H
// bytes: what the next layer takes as its x rows with kx16 = H, x8_off = 2H, kx8 = H); wT16 [4H][kx16 + H] f16, wT8 [4H][kx8 + H] bytes.
// h_lo = 1 (round 6): the low-order half of h is corrected too - hbuf rows are 4H bytes [f16(h) | e4m3(h 2^7) | e4m3((h - f16(h)) 2^18)] and the
// h-part of wT8's rows is [lo(Wh) | hi(Wh)] (evc_cast_f32_to_fp8_lo with hi_tail): wT8 [4H][kx8 + 2H]; a layer above reads those rows with
// x8_off = 2H, kx8 = 2H against [lo(Wx) | hi(Wx)].
// x_row_scale (integer frames): acc = acc * rs[row] + bias behind the x-part of the f16 stages; the accumulators start from x_col_const.
extern "C" int evc_lstm_layer_fwd_f16_fp8lo(const evc_f16* x, int64_t ldx, int kx16, int64_t x8_off, int kx8, const evc_f16* wT16,
                                            const uint8_t* wT8, int w8_scale_exp, int h_lo, const float* bias, const int32_t* len,
                                            int T, int M, int H, evc_f16* hbuf, evc_bf16* hbuf_bf16, float* c_state, float* h_state,
                                            int64_t ld_state, void* gates, evc_bf16* c_all, const int32_t* row_map,
                                            const int32_t* rows_per_step, const float* x_row_scale, const float* x_col_const, int b8_gap, void* stream) {
  const char* entry = "evc_lstm_layer_fwd_f16_fp8lo";
  EVC_TRY(fwd_shape_ok(entry, T, M, kx16, H, 128));
  EVC_TRY(fwd_xint_ok(entry, x_row_scale, x_col_const, b8_gap));
  EVC_REQUIRE(x && wT16 && wT8 && hbuf && hbuf_bf16 && bias && len, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_fp8lo: NULL operand");
  EVC_TRY(fwd_x8_ok(entry, x, ldx, kx16, x8_off, kx8));
  EVC_REQUIRE(aligned_to(wT16, 16) && aligned_to(wT8, 16), EVC_ERR_BAD_ALIGN, "evc_lstm_layer_fwd_f16_fp8lo: 16-byte aligned weight images");
  EVC_REQUIRE(w8_scale_exp >= 0 && w8_scale_exp <= 60, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_fp8lo: w8_scale_exp=%d", w8_scale_exp);
  EVC_REQUIRE(h_lo == 0 || h_lo == 1, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_fp8lo: h_lo=%d", h_lo);
  const FwdShared S{len, T, M, H, ld_state, row_map, rows_per_step};
  const FwdLayer L = fwd_layer_fp8lo(x, ldx, kx16, x8_off, kx8, wT16, wT8, w8_scale_exp, h_lo, bias, x_row_scale, x_col_const, b8_gap, H, hbuf,
                                     hbuf_bf16, c_state, h_state, gates, c_all);
  EVC_REQUIRE(ring_operand_ok(M, ldx > L.ldh ? ldx : L.ldh) && ring_operand_ok(4L * H, (long)kx16 + H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_layer_fwd_f16_fp8lo: a time slab or the kernel spans 4 GiB or more");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layer_ok(entry, L, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L, st));                    // (every part of the rows)
  EVC_TRY(fwd_clear_copy(S, L, st));
  fwd_layer_loop(S, L, [&](const FwdStep& s) { launch_fwd_step_e4m3(s, pick_fwd_tile_v3(s.e.M, H), x_row_scale != nullptr, st); });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// "High" precision L1 layer on TIME-DITHERED f16 weight images (round 5; DESIGN.md 7 "dither"): step t contracts
//   z = [x16 | h16] . W16_t^T  (IEEE f16; W16_t = image t of evc_cast_f32_to_f16_dither at wT16 + t * w16_step_stride)
//       + 2^-scale8_exp  x8 . W8^T  (OCP e4m3 stages behind the f16 ones, kx8 > 0: the low-order half of the INPUT frames against an e4m3
//         image of Wx - the one activation term f16 does not cover)
// A weight's f16 rounding error is the same at every step of a chunk, so a recurrence integrates it coherently ("it is the
// weights"); image t rounds every element down or up such that over any run of steps the round-ups match the element's position between
// its two f16 neighbours - the errors cancel over the steps instead of adding up, and the weights' low-order halves need no stages of their
// own (evc_lstm_layer_fwd_f16_fp8lo: 26 + 16 e4m3 stages per step pair of a two-layer level; here 9 + 0).  x rows as in
// evc_lstm_layer_fwd_f16_fp8lo (kx16 halfwords at the row start, kx8 e4m3 bytes at byte offset x8_off; kx8 = 0: none, wT8 unused);
// wT8: rows of ldb8 bytes whose first kx8 bytes are the e4m3 operand; hbuf [T+1][M][H] PLAIN f16 rows (the next layer's x with kx8 = 0),
// hbuf_bf16 the bf16 copy.
extern "C" int evc_lstm_layer_fwd_f16_dith(const evc_f16* x, int64_t ldx, int kx16, int64_t x8_off, int kx8, const evc_f16* wT16,
                                           int64_t w16_step_stride, const uint8_t* wT8, int64_t ldb8, int scale8_exp, const float* bias,
                                           const int32_t* len, int T, int M, int H, evc_f16* hbuf, evc_bf16* hbuf_bf16, float* c_state,
                                           float* h_state, int64_t ld_state, void* gates, evc_bf16* c_all, const int32_t* row_map,
                                           const int32_t* rows_per_step, void* stream) {
  const char* entry = "evc_lstm_layer_fwd_f16_dith";
  EVC_REQUIRE(T > 0 && M > 0 && H > 0 && kx16 > 0 && kx8 >= 0, EVC_ERR_BAD_SHAPE, "evc_lstm_layer_fwd_f16_dith: bad shape");
  EVC_REQUIRE(x && wT16 && hbuf && hbuf_bf16 && bias && len, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_dith: NULL operand");
  EVC_REQUIRE(w16_step_stride >= 0 && w16_step_stride % 8 == 0 && aligned_to(wT16, 16), EVC_ERR_BAD_ALIGN,
              "evc_lstm_layer_fwd_f16_dith: w16_step_stride=%ld (>= 0, %%8: every image 16-byte aligned)", (long)w16_step_stride);
  EVC_REQUIRE(w16_step_stride == 0 || w16_step_stride >= 4L * H * ((long)kx16 + H), EVC_ERR_BAD_ARG,
              "evc_lstm_layer_fwd_f16_dith: w16_step_stride=%ld is smaller than one [4H][kx16 + H] image", (long)w16_step_stride);
  if (kx8 == 0) {                // no e4m3 stages: the plain f16 layer on per-step images
    EVC_REQUIRE(ldx >= kx16 && ldx % 8 == 0, EVC_ERR_BAD_ALIGN, "evc_lstm_layer_fwd_f16_dith: ldx=%ld (>= kx16=%d, %%8)", (long)ldx, kx16);
    return lstm_layer_fwd_impl(entry, (const evc_bf16*)x, (const evc_bf16*)wT16, bias, len, T, M, kx16, H, 0, nullptr, (evc_bf16*)hbuf, c_state, h_state,
                               ld_state, gates, c_all, hbuf_bf16, row_map, rows_per_step, stream, 1, ldx, 0, w16_step_stride);
  }
  EVC_TRY(fwd_shape_ok(entry, T, M, kx16, H, 128));
  EVC_TRY(fwd_x8_ok(entry, x, ldx, kx16, x8_off, kx8));
  EVC_REQUIRE(wT8 && ldb8 >= kx8 && ldb8 % 16 == 0 && aligned_to(wT8, 16), EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_dith: wT8 rows of ldb8=%ld bytes (>= kx8, %%16)", (long)ldb8);
  EVC_REQUIRE(scale8_exp >= 0 && scale8_exp <= 80, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_f16_dith: scale8_exp=%d", scale8_exp);
  const FwdShared S{len, T, M, H, ld_state, row_map, rows_per_step};
  FwdLayer L;
  L.x = x; L.ldx = ldx; L.kx = kx16;
  L.h = hbuf; L.ldh = H; L.kh = H;      // plain f16 h rows: no e4m3 stages of h
  L.B = wT16; L.ldb = (long)kx16 + H;
  L.bias = bias; L.c_state = c_state; L.h_state = h_state; L.gates = gates; L.c_all = c_all;
  L.w_step_stride = w16_step_stride; L.h_copy = hbuf_bf16; L.ld_copy = H;
  L.x8_off = x8_off; L.kx8 = kx8; L.B8 = wT8; L.ldb8 = ldb8; L.scale8_exp = -scale8_exp;
  EVC_REQUIRE(ring_operand_ok(M, ldx > L.ldh ? ldx : L.ldh) && ring_operand_ok(4L * H, (long)kx16 + H) && ring_operand_ok(4L * H, (ldb8 + 1) / 2), EVC_ERR_BAD_SHAPE,
              "evc_lstm_layer_fwd_f16_dith: a time slab or a weight image spans 4 GiB or more");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layer_ok(entry, L, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L, st));
  EVC_TRY(fwd_clear_copy(S, L, st));
  fwd_layer_loop(S, L, [&](const FwdStep& s) { launch_fwd_step_e4m3(s, pick_fwd_tile_v3(s.e.M, H), false, st); });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// The two-layer L1 level of the "high" mode in T + 1 launches (round 6): layer 0 as evc_lstm_layer_fwd_f16_fp8lo (f16 stages + the e4m3 stages of its
// weights' / activations' low-order halves; integer frames with x_row_scale), layer 1 as evc_lstm_layer_fwd_f16_dith with kx8 = 0 (plain f16 stages on the
// time-dithered image of its step), layer 0's step s and layer 1's step s-1 per launch, every workgroup walking both tiles (lstm_fwd_walk2_kernel: the second
// tile's ring fill under the first tile's gate tail, each tile's loop and gate tail in its own mode).  Same arithmetic as the two layer calls: bit-identical
// results.  Argument meaning as in those two entries; hbuf0 rows are layer 1's x rows (row stride 2H halfwords with h_lo, else 3H/2).  Launches whose tile is
// not 224 / 240 / 256 rows run separately, both on the tile picked for the launch.
extern "C" int evc_lstm_level2_fwd_high(const evc_f16* x, int64_t ldx, int kx16, int64_t x8_off, int kx8, const evc_f16* wT16_0, const uint8_t* wT8_0,
                                        int w8_scale_exp, int h_lo, const float* bias0, const float* x_row_scale, const float* x_col_const, int b8_gap,
                                        const evc_f16* wT16_1, int64_t w16_step_stride, const float* bias1, const int32_t* len, int T, int M, int H,
                                        evc_f16* hbuf0, evc_bf16* hbuf0_bf16, evc_f16* hbuf1, evc_bf16* hbuf1_bf16, float* c_state0, float* h_state0,
                                        float* c_state1, float* h_state1, int64_t ld_state, void* gates0, evc_bf16* c_all0, void* gates1, evc_bf16* c_all1,
                                        const int32_t* row_map, const int32_t* rows_per_step, void* stream) {
  const char* entry = "evc_lstm_level2_fwd_high";
  EVC_TRY(fwd_shape_ok(entry, T, M, kx16, H, 128));
  EVC_TRY(fwd_xint_ok(entry, x_row_scale, x_col_const, b8_gap));
  EVC_REQUIRE(x && wT16_0 && wT8_0 && wT16_1 && hbuf0 && hbuf0_bf16 && hbuf1 && hbuf1_bf16 && bias0 && bias1 && len && c_state0 && h_state0 && c_state1 &&
              h_state1, EVC_ERR_BAD_ARG, "evc_lstm_level2_fwd_high: NULL operand");
  EVC_TRY(fwd_x8_ok(entry, x, ldx, kx16, x8_off, kx8));
  EVC_REQUIRE(aligned_to(wT16_0, 16) && aligned_to(wT8_0, 16) && aligned_to(wT16_1, 16), EVC_ERR_BAD_ALIGN, "evc_lstm_level2_fwd_high: 16-byte aligned weight images");
  EVC_REQUIRE(w8_scale_exp >= 0 && w8_scale_exp <= 60 && (h_lo == 0 || h_lo == 1), EVC_ERR_BAD_ARG, "evc_lstm_level2_fwd_high: w8_scale_exp=%d h_lo=%d",
              w8_scale_exp, h_lo);
  EVC_REQUIRE(w16_step_stride >= 0 && w16_step_stride % 8 == 0 && (w16_step_stride == 0 || w16_step_stride >= 4L * H * 2 * H), EVC_ERR_BAD_ARG,
              "evc_lstm_level2_fwd_high: w16_step_stride=%ld (0 or at least one [4H][2H] image, %%8)", (long)w16_step_stride);
  const FwdShared S{len, T, M, H, ld_state, row_map, rows_per_step};
  const FwdLayer L0 = fwd_layer_fp8lo(x, ldx, kx16, x8_off, kx8, wT16_0, wT8_0, w8_scale_exp, h_lo, bias0, x_row_scale, x_col_const, b8_gap, H, hbuf0,
                                      hbuf0_bf16, c_state0, h_state0, gates0, c_all0);
  // layer 1: the plain f16 step on image t; x_t = the f16 part of layer 0's row slab t + 1
  FwdLayer L1;
  L1.x = hbuf0 + (long)M * L0.ldh; L1.ldx = L0.ldh; L1.kx = H;
  L1.h = hbuf1; L1.ldh = H; L1.kh = H;
  L1.B = wT16_1; L1.ldb = 2L * H;
  L1.bias = bias1; L1.c_state = c_state1; L1.h_state = h_state1; L1.gates = gates1; L1.c_all = c_all1;
  L1.w_step_stride = w16_step_stride; L1.h_copy = hbuf1_bf16; L1.ld_copy = H;
  EVC_REQUIRE(ring_operand_ok(M, ldx > L0.ldh ? ldx : L0.ldh) && ring_operand_ok(4L * H, (long)kx16 + H) && ring_operand_ok(4L * H, 2L * H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_level2_fwd_high: a time slab or a kernel spans 4 GiB or more");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layers2_ok(entry, L0, L1, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L0, st));                   // every image of both layers' rows
  EVC_TRY(fwd_clear_copy(S, L0, st));
  EVC_TRY(fwd_clear_h(S, L1, st));
  EVC_TRY(fwd_clear_copy(S, L1, st));
  const bool xint = x_row_scale != nullptr;
  fwd_wavefront(S, L0, L1, [&](const FwdStep& a, bool has_a, const FwdStep& b, bool has_b) {
    const int pick = pick_fwd_tile_v3(has_b ? b.e.M : a.e.M, H);
    const bool walked = with_fwd_tile_v3<CfgLstmV3_224u>(pick, [&](auto tile) {
      typedef typename decltype(tile)::type Cfg;
      if constexpr (is_walk2_tile<Cfg>::value) {     // tile a: f16 + e4m3 stages, tile b: plain f16 stages
        if (xint) launch_lstm_fwd_walk2<Cfg, true, true, true, false>(a, has_a, b, has_b, st);
        else launch_lstm_fwd_walk2<Cfg, true, true, false, false>(a, has_a, b, has_b, st);
        return true;
      } else return false;
    });
    if (walked) return;
    if (has_a) launch_fwd_step_e4m3(a, pick, xint, st);
    if (has_b) with_fwd_tile_v3<CfgLstmV3_224u>(pick, [&](auto tile) { launch_lstm_fwd<typename decltype(tile)::type, false, true>(b, st); });
  });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// "High" precision layer for the M ~ batch stacks (the L2 level): split-bf16 operands, f32-operand accuracy, as K-extensions of
// the plain loops (see evc_gemm_nt_split).  x-projection of all T steps hoisted into one split product; step t contracts
// [lo(h) | hi(h)] . [Wh_hi | Wh_lo]^T + hi(h) . Wh_hi^T (K = 3H) and writes h_t three times: hbuf (plain bf16 = the hi half, what
// the backward products read) and the wide image hbuf_lohi for the next step / the next layer's x-projection.
extern "C" int evc_lstm_layer_fwd_hp(const evc_bf16* x_lohi, const evc_bf16* wx_hilo, int64_t ldwx, const evc_bf16* wh_hilo, int64_t ldwh,
                                     const float* bias, const int32_t* len, int T, int M, int Kin, int H, float* zx_ws,
                                     evc_bf16* hbuf, evc_bf16* hbuf_lohi, float* c_state, float* h_state, int64_t ld_state,
                                     void* gates, evc_bf16* c_all, void* stream) {
  const char* entry = "evc_lstm_layer_fwd_hp";
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H));
  EVC_REQUIRE(x_lohi && wx_hilo && wh_hilo && zx_ws && hbuf && hbuf_lohi, EVC_ERR_BAD_ARG, "evc_lstm_layer_fwd_hp: NULL operand");
  const FwdShared S{len, T, M, H, ld_state, nullptr, nullptr};
  // the tail writes hbuf (plain) and hbuf_lohi (wide); no x rows (hoisted), and the h operands are patched in below
  FwdLayer L;
  L.zx = zx_ws;
  L.h = hbuf; L.ldh = H; L.kh = H; L.h_copy = hbuf_lohi; L.ld_copy = 2L * H;
  L.B = wh_hilo; L.ldb = ldwh;
  L.bias = bias; L.c_state = c_state; L.h_state = h_state; L.gates = gates; L.c_all = c_all;
  EVC_REQUIRE(ldwx >= 2L * Kin && ldwh >= 2L * H && ldwx % 8 == 0 && ldwh % 8 == 0 && aligned_to(wh_hilo, 16), EVC_ERR_BAD_ALIGN,
              "evc_lstm_layer_fwd_hp: weight images are [4H][2Kin] / [4H][2H] (ldwx=%ld ldwh=%ld)", (long)ldwx, (long)ldwh);
  EVC_REQUIRE(ring_operand_ok(M, 2L * H) && ring_operand_ok(4L * H, ldwh), EVC_ERR_BAD_SHAPE, "evc_lstm_layer_fwd_hp: operand spans 4 GiB or more");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layer_ok(entry, L, 8, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L, st));
  EVC_TRY(fwd_clear_copy(S, L, st));
  EVC_TRY(evc_gemm_nt_split(x_lohi, 2L * Kin, wx_hilo, ldwx, zx_ws, 4L * H, T * M, 4 * H, Kin, nullptr, stream));
  // The one entry whose operands fwd_step() does not build: the step's 16-bit segments both come from the SECOND ring - segment 1 = the wide
  // rows [lo | hi] against [Wh_hi | Wh_lo], segment 2 = their hi halves against Wh_hi again (B2 = B) - while the h ring proper (hbuf) is only
  // written.  The common part and the gate tail's arguments are fwd_step()'s.
  fwd_layer_loop(S, L, [&](FwdStep s) {
    const bf16_t* hw = hbuf_lohi + (long)s.e.t * M * 2 * H;
    s.p.A1 = hw; s.p.lda1 = 2L * H; s.p.A2 = hw + H; s.p.lda2 = 2L * H;
    s.p.B2 = wh_hilo;
    s.k1 = s.e.t == 0 ? 0 : 2 * H; s.k2 = s.e.t == 0 ? 0 : H;
    if (M >= 1024) launch_lstm_fwd<CfgLstmV3_256, true>(s, st);
    else launch_lstm_fwd<CfgLstmV3Small, true>(s, st);
  });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// ===========================================================================
// Two-layer stacks with M ~ batch rows (the L2 level): wavefront pair launches
// ===========================================================================
// Layer 0's x-projection of all T steps is hoisted into one GEMM (M ~ batch: a per-step product would be a sliver); layer 1 reads layer 0's
// output slab t+1 as its x_t in a fused [x_t | h_{t-1}] contraction (nothing to hoist: x_t exists only one launch earlier).  The steps are
// latency-bound, so layer 0's step s and layer 1's step s-1 share a launch where the tile has a pair kernel (lstm_fwd_pair_kernel).
extern "C" int evc_lstm_stack2_fwd(const evc_bf16* x, const evc_bf16* wT0, const float* bias0, const evc_bf16* wT1, const float* bias1,
                                   const int32_t* len, int T, int M, int Kin, int H, float* zx_ws,
                                   evc_bf16* hbuf0, evc_bf16* hbuf1, float* c_state0, float* h_state0, float* c_state1,
                                   float* h_state1, int64_t ld_state, void* gates0, evc_bf16* c_all0, void* gates1,
                                   evc_bf16* c_all1, void* stream) {
  const char* entry = "evc_lstm_stack2_fwd";
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H));
  EVC_REQUIRE(ring_operand_ok(M, Kin > H ? Kin : H) && ring_operand_ok(4L * H, (long)Kin + H) && ring_operand_ok(4L * H, 2L * H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_stack2_fwd: a time slab or a kernel spans 4 GiB or more (M=%d Kin=%d H=%d)", M, Kin, H);
  EVC_REQUIRE(zx_ws && hbuf0 && hbuf1, EVC_ERR_BAD_ARG, "evc_lstm_stack2_fwd: zx_ws / hbuf0 / hbuf1 must not be NULL");
  const FwdShared S{len, T, M, H, ld_state, nullptr, nullptr};
  FwdLayer L0;
  L0.x = x; L0.ldx = Kin; L0.kx = Kin;
  L0.h = hbuf0; L0.ldh = H; L0.kh = H;
  L0.B = wT0 + Kin; L0.ldb = (long)Kin + H;
  L0.bias = bias0; L0.c_state = c_state0; L0.h_state = h_state0; L0.gates = gates0; L0.c_all = c_all0;
  L0.zx = zx_ws;
  FwdLayer L1;
  L1.x = hbuf0 + (long)M * H; L1.ldx = H; L1.kx = H;
  L1.h = hbuf1; L1.ldh = H; L1.kh = H;
  L1.B = wT1; L1.ldb = 2L * H;
  L1.bias = bias1; L1.c_state = c_state1; L1.h_state = h_state1; L1.gates = gates1; L1.c_all = c_all1;
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layers2_ok(entry, L0, L1, 8));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L0, st));
  EVC_TRY(fwd_clear_h(S, L1, st));
  EVC_TRY(evc_gemm_nt(x, Kin, wT0, (int64_t)Kin + H, zx_ws, 4L * H, T * M, 4 * H, Kin, nullptr, 0, 0, stream));
  const int tile = pick_fwd_tile(M, H);     // 6: v1 128 rows x 32 units, 7 (M ~ 256): 64 x 16 - the tiles with a pair kernel; others: one step per launch
  fwd_wavefront(S, L0, L1, [&](const FwdStep& a, bool has_a, const FwdStep& b, bool has_b) {
    if (has_a && has_b && tile == 6) return launch_lstm_fwd_pair<CfgLstmBig>(a, b, st);
    if (has_a && has_b && tile == 7) return launch_lstm_fwd_pair<CfgLstmV3Small>(a, b, st);
    const auto one = [&](const FwdStep& s) { with_fwd_tile<true>(tile, [&](auto t) { launch_lstm_fwd<typename decltype(t)::type>(s, st); }); };
    if (has_a) one(a);
    if (has_b) one(b);
  });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// the launcher of the two f16 stacks: one 64 x 16 tile for every launch
template <bool FP8>
static inline void launch_stack2_f16(const FwdStep& a, bool has_a, const FwdStep& b, bool has_b, hipStream_t st) {
  if (has_a && has_b) launch_lstm_fwd_pair<CfgLstmV3Small, true, FP8>(a, b, st);
  else launch_lstm_fwd<CfgLstmV3Small, false, true, FP8>(has_a ? a : b, st);
}

// evc_lstm_stack2_fwd on IEEE f16 operands, with the UPPER layer's weights K-extended by their low-order halves - the "high"
// precision form of the L2 level (M = videos).  The error budget (scripts/precision_budget.py) says what this level needs: f16
// (2^-12) is enough for every activation and for layer 0's weights; the one term it does not cover is the ROUNDING OF THE UPPER
// LAYER'S WEIGHTS, the same error at every one of the 20 steps into a cell state that integrates it (6e-4 on the states).  So
// layer 1 contracts [h0_t | h0_t/64 | h1_{t-1} | h1_{t-1}/64] . [Wx | (Wx - f16(Wx))*64 | Wh | (Wh - f16(Wh))*64]^T (K = 4H instead
// of 2H; split-bf16 would be 6H in three passes), layer 0 runs plain f16 with its x-projection hoisted into one f16 product (its step:
// zx + h0_{s-1} . Wh0^T over K = H of the wide rows; h0_ext: all 2H against [Wh | Wh_lo*64]).
// h rows are WIDE, [f16(h) | f16(h)/64] (2H), written by the step epilogue together with the bf16 copy the backward pass reads.
// Same wavefront as evc_lstm_stack2_fwd: launch s = layer 0 step s next to layer 1 step s-1.
extern "C" int evc_lstm_stack2_fwd_f16(const evc_f16* x, int x_segments, const evc_f16* wT0, int h0_ext, const float* bias0,
                                       const evc_f16* wT1_wlo, const float* bias1,
                                       const int32_t* len, int T, int M, int Kin, int H, float* zx_ws,
                                       evc_f16* h0_wide, evc_f16* h1_wide, evc_bf16* hbuf0, evc_bf16* hbuf1,
                                       float* c_state0, float* h_state0, float* c_state1, float* h_state1, int64_t ld_state,
                                       void* gates0, evc_bf16* c_all0, void* gates1, evc_bf16* c_all1, void* stream) {
  const char* entry = "evc_lstm_stack2_fwd_f16";
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H));
  EVC_REQUIRE(x && wT0 && wT1_wlo && zx_ws && h0_wide && h1_wide && hbuf0 && hbuf1, EVC_ERR_BAD_ARG, "evc_lstm_stack2_fwd_f16: NULL operand");
  EVC_REQUIRE(x_segments >= 1 && x_segments <= 3 && (h0_ext == 0 || h0_ext == 1), EVC_ERR_BAD_ARG, "evc_lstm_stack2_fwd_f16: x_segments=%d h0_ext=%d",
              x_segments, h0_ext);
  const long Kx = (long)x_segments * Kin;              // K of the hoisted x-projection (K-extended input: evc_cast_f32_to_f16_segs)
  const long ldw0 = Kx + (h0_ext ? 2L : 1L) * H;       // row of layer 0's kernel image (evc_cast_f32_to_f16_wide)
  const FwdShared S{len, T, M, H, ld_state, nullptr, nullptr};
  FwdLayer L0;
  L0.x = x; L0.ldx = Kx; L0.kx = (int)Kx;
  L0.h = h0_wide; L0.ldh = 2L * H; L0.kh = h0_ext ? 2 * H : H;
  L0.B = wT0 + Kx; L0.ldb = ldw0;
  L0.bias = bias0; L0.c_state = c_state0; L0.h_state = h_state0; L0.gates = gates0; L0.c_all = c_all0;
  L0.zx = zx_ws; L0.h_wide = 1; L0.h_copy = hbuf0; L0.ld_copy = H;
  FwdLayer L1;
  L1.x = h0_wide + (long)M * 2 * H; L1.ldx = 2L * H; L1.kx = 2 * H;
  L1.h = h1_wide; L1.ldh = 2L * H; L1.kh = 2 * H;
  L1.B = wT1_wlo; L1.ldb = 4L * H;
  L1.bias = bias1; L1.c_state = c_state1; L1.h_state = h_state1; L1.gates = gates1; L1.c_all = c_all1;
  L1.h_wide = 1; L1.h_copy = hbuf1; L1.ld_copy = H;
  EVC_REQUIRE(ring_operand_ok(M, 2L * H) && ring_operand_ok(4L * H, 4L * H) && ring_operand_ok(4L * H, 3L * Kin + 2L * H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_stack2_fwd_f16: an operand spans 4 GiB or more");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layers2_ok(entry, L0, L1, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L0, st));                     // both layers, both images
  EVC_TRY(fwd_clear_h(S, L1, st));
  EVC_TRY(fwd_clear_copy(S, L0, st));
  EVC_TRY(fwd_clear_copy(S, L1, st));
  EVC_TRY(gemm_nt_f16(x, Kx, wT0, ldw0, zx_ws, 4L * H, T * M, 4 * H, (int)Kx, stream));
  fwd_wavefront(S, L0, L1, [&](const FwdStep& a, bool has_a, const FwdStep& b, bool has_b) { launch_stack2_f16<false>(a, has_a, b, has_b, st); });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

// evc_lstm_stack2_fwd_f16 with the low-order halves of the recurrent weights of layer 0 and of all weights of layer 1 contracted as e4m3
// operands behind the f16 stages of the same (pair) launches (LOOP_FP8_TAIL) instead of f16 K-extensions: layer 1 walks 32 f16 + 16 e4m3
// stages instead of 64 f16 ones (H = 1024) - these steps are bound by their chain of dependent stages.  x [T][M][x_segments Kin] f16
// (K-extended input of the hoisted product, as before); wT0 [4H][x_segments Kin + H] f16 = [Wx segments | f16(Wh)], wT0_8 [4H][H] bytes =
// e4m3((Wh - f16(Wh)) 2^w8_scale_exp); wT1 [4H][2H] f16, wT1_8 [4H][2H] bytes; h0_rows / h1_rows [(T+1)][M] rows of 3H bytes = [f16(h) |
// e4m3(h 2^7)].  H % 128 == 0, H >= 512.  Layer 0's step: zx + h0_{s-1} . Wh0^T (f16) + 2^-(7+e) e4m3(h0_{s-1}) . e4m3(lo(Wh0))^T; layer 1's:
// [h0_t | h1_{t-1}] . [Wx | Wh]^T (f16) + the same rows' e4m3 parts against e4m3(lo([Wx | Wh])).
// h_lo = 1 (round 6): the activations' low-order halves are corrected as well - h rows of 4H bytes [f16(h) | e4m3(h 2^7) | e4m3((h - f16(h)) 2^18)],
// wT0_8 [4H][2H] = [lo(Wh0) | hi(Wh0)], wT1_8 [4H][4H] = [lo(Wx1) | hi(Wx1) | lo(Wh1) | hi(Wh1)] (evc_cast_f32_to_fp8_lo with hi_tail): layer 1
// walks 32 f16 + 32 e4m3 stages.
extern "C" int evc_lstm_stack2_fwd_f16_fp8lo(const evc_f16* x, int x_segments, const evc_f16* wT0, const uint8_t* wT0_8, const float* bias0,
                                             const evc_f16* wT1, const uint8_t* wT1_8, int w8_scale_exp, int h_lo, const float* bias1,
                                             const int32_t* len, int T, int M, int Kin, int H, float* zx_ws,
                                             evc_f16* h0_rows, evc_f16* h1_rows, evc_bf16* hbuf0, evc_bf16* hbuf1,
                                             float* c_state0, float* h_state0, float* c_state1, float* h_state1, int64_t ld_state,
                                             void* gates0, evc_bf16* c_all0, void* gates1, evc_bf16* c_all1, void* stream) {
  const char* entry = "evc_lstm_stack2_fwd_f16_fp8lo";
  EVC_TRY(fwd_shape_ok(entry, T, M, Kin, H, 128, 512));
  EVC_REQUIRE(x && wT0 && wT0_8 && wT1 && wT1_8 && zx_ws && h0_rows && h1_rows && hbuf0 && hbuf1, EVC_ERR_BAD_ARG, "evc_lstm_stack2_fwd_f16_fp8lo: NULL operand");
  EVC_REQUIRE(x_segments >= 1 && x_segments <= 3 && w8_scale_exp >= 0 && w8_scale_exp <= 60, EVC_ERR_BAD_ARG,
              "evc_lstm_stack2_fwd_f16_fp8lo: x_segments=%d w8_scale_exp=%d", x_segments, w8_scale_exp);
  EVC_REQUIRE(h_lo == 0 || h_lo == 1, EVC_ERR_BAD_ARG, "evc_lstm_stack2_fwd_f16_fp8lo: h_lo=%d", h_lo);
  const long Kx = (long)x_segments * Kin;
  const long ldw0 = Kx + H, ldh = h_lo ? 2L * H : 3L * H / 2;
  const int kh8 = h_lo ? 2 * H : H;                 // e4m3 bytes per h row: [h8] or [h8 | h_lo8]
  const FwdShared S{len, T, M, H, ld_state, nullptr, nullptr};
  FwdLayer L0;
  L0.x = x; L0.ldx = Kx; L0.kx = (int)Kx;
  L0.h = h0_rows; L0.ldh = ldh; L0.kh = H;
  L0.B = wT0 + Kx; L0.ldb = ldw0;
  L0.bias = bias0; L0.c_state = c_state0; L0.h_state = h_state0; L0.gates = gates0; L0.c_all = c_all0;
  L0.zx = zx_ws; L0.h_copy = hbuf0;
  L0.kh8 = kh8; L0.B8 = wT0_8; L0.ldb8 = kh8;
  FwdLayer L1;
  L1.x = h0_rows + (long)M * ldh; L1.ldx = ldh; L1.kx = H;
  L1.h = h1_rows; L1.ldh = ldh; L1.kh = H;
  L1.B = wT1; L1.ldb = 2L * H;
  L1.bias = bias1; L1.c_state = c_state1; L1.h_state = h_state1; L1.gates = gates1; L1.c_all = c_all1;
  L1.h_copy = hbuf1;
  L1.x8_off = 2L * H; L1.kx8 = kh8; L1.kh8 = kh8; L1.B8 = wT1_8; L1.ldb8 = 2L * kh8;
  L0.h_wide = L1.h_wide = h_lo ? 3 : 2; L0.ld_copy = L1.ld_copy = H; L0.scale8_exp = L1.scale8_exp = -(7 + w8_scale_exp);
  EVC_REQUIRE(ring_operand_ok(M, ldh) && ring_operand_ok(4L * H, ldw0) && ring_operand_ok(4L * H, 2L * H), EVC_ERR_BAD_SHAPE,
              "evc_lstm_stack2_fwd_f16_fp8lo: an operand spans 4 GiB or more");
  EVC_REQUIRE(aligned_to(wT0_8, 16) && aligned_to(wT1_8, 16) && aligned_to(wT0, 16) && aligned_to(wT1, 16), EVC_ERR_BAD_ALIGN,
              "evc_lstm_stack2_fwd_f16_fp8lo: 16-byte aligned weight images");
  EVC_TRY(fwd_shared_ok(entry, S));
  EVC_TRY(fwd_layers2_ok(entry, L0, L1, 16));
  hipStream_t st = (hipStream_t)stream;
  EVC_TRY(fwd_clear_h(S, L0, st));                     // both layers, every image
  EVC_TRY(fwd_clear_h(S, L1, st));
  EVC_TRY(fwd_clear_copy(S, L0, st));
  EVC_TRY(fwd_clear_copy(S, L1, st));
  EVC_TRY(gemm_nt_f16(x, Kx, wT0, ldw0, zx_ws, 4L * H, T * M, 4 * H, (int)Kx, stream));
  fwd_wavefront(S, L0, L1, [&](const FwdStep& a, bool has_a, const FwdStep& b, bool has_b) { launch_stack2_f16<true>(a, has_a, b, has_b, st); });
  EVC_LAUNCH_CHECK();
  return EVC_OK;
}

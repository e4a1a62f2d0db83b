// Launch helpers shared by the GEMM-shaped translation units (evc_gemm.hip, evc_dbof.hip, evc_lstm_fwd.hip, evc_lstm_bwd.hip).
#pragma once
#include "gemm_core_tn.h"
#include "gemm_core_v3.h"
#include <mutex>
#include <vector>
#include <stdlib.h>
#include <type_traits>

// A kernel is instantiated either on a v1 tile (TileCfg: static 2-stage LDS, K steps of 64)
// or a v2 tile (TileCfg2: dynamic 4-stage LDS ring, K steps of 32).
template <class Cfg> struct is_v2 { static constexpr bool value = false; };
template <int a, int b, int c, int d, int e, int f, bool g> struct is_v2<TileCfg2<a, b, c, d, e, f, g>> { static constexpr bool value = true; };
// v3 tiles (TileCfg3: the ring with 64-wide K stages, gemm_core_v3.h) are ring tiles too (dynamic LDS, same epilogues)
template <int a, int b, int c, int d, int e, int f, int g> struct is_v2<TileCfg3<a, b, c, d, e, f, g>> { static constexpr bool value = true; };
template <class Cfg> struct is_v3 { static constexpr bool value = false; };
template <int a, int b, int c, int d, int e, int f, int g> struct is_v3<TileCfg3<a, b, c, d, e, f, g>> { static constexpr bool value = true; };

extern __shared__ __attribute__((aligned(16))) char lds_dyn[];

// The forward step's epilogue addresses its stores as base + 32-bit byte offset: gate records [rows][H] x 8 B, state rows (row_map is a
// permutation of [0, rows)) of ld_state floats, h rows of up to 3H bytes / 2H halfwords (the wide images)
static inline bool fwd_tail_ok(long rows, long H, long ld_state) {
  return rows * H * 8 + 32 < (1L << 32) && rows * ld_state * 4 < (1L << 32);
}
// The ring loops address every LDS-DMA as base + 32-bit byte offset built from a 24-bit row index and a 24-bit row stride
// (gemm_core_v2.h): an operand of `rows` rows with leading dimension `ld` (bf16 elements) must fit that.
static inline bool ring_operand_ok(long rows, long ld) {
  return rows < (1L << 24) && ld * 2 < (1L << 24) && rows * ld * 2 < (1L << 32);
}

// a refusal helper's error code, passed on
#define EVC_TRY(expr)             \
  do {                            \
    const int _rc = (expr);       \
    if (_rc) return _rc;          \
  } while (0)

// row plans (evc_sort_rows_by_len): the active rows of step t are the prefix [0, rows_per_step[t]) of M slots sorted by length
static inline int rows_per_step_ok(const char* entry, const int32_t* rows_per_step, int T, int M) {
  if (rows_per_step)
    for (int t = 0; t < T; ++t)
      EVC_REQUIRE(rows_per_step[t] >= 0 && rows_per_step[t] <= M && (t == 0 || rows_per_step[t] <= rows_per_step[t - 1]), EVC_ERR_BAD_ARG,
                  "%s: rows_per_step[%d]=%d must be non-increasing and within [0, M=%d]", entry, t, rows_per_step[t], M);
  return EVC_OK;
}

// v2 tiles use more dynamic LDS than the 64 KiB default: raise the limit once per kernel (keyed by the
// kernel's address - two kernels of one signature share this template instantiation).
static inline void allow_big_lds(const void* kern, int bytes) {
  static std::mutex mu;
  static std::vector<const void*> done;
  std::lock_guard<std::mutex> lk(mu);
  for (const void* k : done) if (k == kern) return;
  (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done.push_back(kern);
}

template <class Cfg, class Kern, class... Args>
static inline void launch_cfg(Kern kern, int grid, hipStream_t st, Args... args) {
  if (is_v2<Cfg>::value) {
    allow_big_lds((const void*)kern, Cfg::LDS_BYTES);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::NT), Cfg::LDS_BYTES, st, args...);
  } else {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::NT), 0, st, args...);
  }
}

// a tile type handed to a generic callable: f(TileTag<Cfg>()), typename decltype(tile)::type inside (with_nt_tile, with_fwd_tile)
template <class Cfg> struct TileTag { typedef Cfg type; };

// debug/benchmark override of the tile choice, EVC_FORCE_TILE (read once per process; 0 / unset: the choosers decide).  NT products (evc_gemm_nt
// alone; NT_TILES in gemm_shared.h): 1 ring 256x256 | 2 v1 128x128 | 3 v1 64x64 | 4 ring 224x256 | 5 ring 128x128 | 6 ring 320x256 | 7 ring 160x128,
// any other value: 3; a forced tile runs without K split, and the batch-row 256x64 tile and the two split-K tiles are chosen by shape only.  TN products:
// 11 = 128x128 tiles without K split, any other value: 256x256 tiles with the usual K split.  LSTM steps: 1-11 as listed at pick_fwd_tile /
// pick_fwd_tile_v3 (evc_lstm_fwd.hip), 1-7 at the BPTT step's pick (evc_lstm_bwd.hip).
static inline int forced_tile() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("EVC_FORCE_TILE"); v = e ? atoi(e) : 0; }
  return v;
}

// Host side of the GEMM kernel families, shared by their launchers (gemm*.hip): split-K chunking, tile counts, the conv-tap
// mode of a launch, the choice of a kernel instance by operand orientation x tap mode (x operand mode on the fp32 cores)
// as compile-time constants, the CU count, the member table of a grouped launch.  Host-only; the tile ids are in
// gemm_tiles.h.
#pragma once
#include <type_traits>

#include "dispatch.h"
#include "gemm_common.h"
#include "gemm_tiles.h"

// reduction chunk of one split-K slice: whole K-tiles of the core (BK), so the last slices of a split can be empty
inline int fs2_split_chunk(const Fs2GemmArgs& a, int BK) {
  const int chunk = (a.R + a.splitk - 1) / a.splitk;
  return ((chunk + BK - 1) / BK) * BK;
}

// p.tiles_m / p.tiles_n for BM x BN tiles; returns the number of work units of `nz` reduction / tap slices, 0 = more than
// a grid dimension holds (the caller refuses)
template <int BM, int BN>
inline int fs2_set_tiles(GemmP& p, int nz) {
  p.tiles_m = (p.a.Mc + BM - 1) / BM;
  p.tiles_n = (p.a.Nc + BN - 1) / BN;
  const long long units = (long long)p.tiles_m * p.tiles_n * nz;
  return units > 0x7fffffffLL ? 0 : (int)units;
}

// Number of CUs of the current device, asked once per process; 0 = the query failed (the caller refuses).
int fs2_cu_count();  // gemm.hip

// Conv-tap mode of a launch = the TAPS template argument of the cores (TAPS_* in gemm2_core.h, BT_* in gemm_bf16_core.h:
// the launchers assert that the values agree).
enum {
  FS2_TAPS_REFUSED = -1,  // taps that are not uniform per K-tile on a kernel without the generic decode
  FS2_TAPS_NONE = 0,      // plain GEMM
  FS2_TAPS_RED = 1,       // shift_operand == 0, Rper % BK == 0: the tap is a per-K-tile scalar
  FS2_TAPS_ROWS = 2,      // shift_operand == 1 (weight gradient), T >= BK: reduction rows of B shifted by the slice's tap
  FS2_TAPS_GENERIC = 3,   // any Rper / T: per-piece address decode in every K-tile (fp32 cores, FS2_TILE_GENERIC_TAPS)
};
inline int fs2_tap_mode(const GemmP& p, int BK, bool generic) {
  const Fs2GemmArgs& a = p.a;
  if (a.taps <= 1) return FS2_TAPS_NONE;
  const bool uniform = a.shift_operand == 0 ? p.Rper % BK == 0 : a.T >= BK;
  if (!uniform) return generic ? FS2_TAPS_GENERIC : FS2_TAPS_REFUSED;
  return a.shift_operand == 0 ? FS2_TAPS_RED : FS2_TAPS_ROWS;
}

template <int TAPS>
using Fs2TapsC = std::integral_constant<int, TAPS>;

// The one orientation x tap-mode ladder: f(akc, bkc, taps) with std::bool_constant / Fs2TapsC arguments for exactly the
// combinations a core is built for -- NT (forward) and NN (data gradient) plain or FS2_TAPS_RED, TN (weight gradient)
// plain or FS2_TAPS_ROWS, and with GENERIC the three orientations under FS2_TAPS_GENERIC -- else FS2HIP_EINVAL.
template <bool GENERIC, class F>
int fs2_dispatch_orient_taps(const Fs2GemmArgs& a, int mode, F&& f) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  const bool nt = a.a_kcontig && a.b_kcontig, nn = a.a_kcontig && !a.b_kcontig, tn = !a.a_kcontig && !a.b_kcontig;
  if constexpr (GENERIC) {
    if (nt && mode == FS2_TAPS_GENERIC) return f(yes, yes, Fs2TapsC<FS2_TAPS_GENERIC>{});
    if (nn && mode == FS2_TAPS_GENERIC) return f(yes, no, Fs2TapsC<FS2_TAPS_GENERIC>{});
    if (tn && mode == FS2_TAPS_GENERIC) return f(no, no, Fs2TapsC<FS2_TAPS_GENERIC>{});
  }
  if (nt && mode == FS2_TAPS_NONE) return f(yes, yes, Fs2TapsC<FS2_TAPS_NONE>{});
  if (nt && mode == FS2_TAPS_RED) return f(yes, yes, Fs2TapsC<FS2_TAPS_RED>{});
  if (nn && mode == FS2_TAPS_NONE) return f(yes, no, Fs2TapsC<FS2_TAPS_NONE>{});
  if (nn && mode == FS2_TAPS_RED) return f(yes, no, Fs2TapsC<FS2_TAPS_RED>{});
  if (tn && mode == FS2_TAPS_NONE) return f(no, no, Fs2TapsC<FS2_TAPS_NONE>{});
  if (tn && mode == FS2_TAPS_ROWS) return f(no, no, Fs2TapsC<FS2_TAPS_ROWS>{});
  return FS2HIP_EINVAL;
}

// The fp32 cores (BK = 32) on top of it: f(akc, bkc, taps, bf) with bf = Fs2GemmArgs.operand_bf16 as the cores' BF
// template argument -- 0 exact fp32, 1 / 2 operands rounded / split to bf16 in registers, every combination above; 3
// (bf16 in memory) only with STORED3, and then only the NT instances, plain or FS2_TAPS_RED.
template <bool GENERIC, bool STORED3, class F>
int fs2_dispatch_fp32(const GemmP& p, int BK, F&& f) {
  const Fs2GemmArgs& a = p.a;
  return fs2_dispatch_orient_taps<GENERIC>(a, fs2_tap_mode(p, BK, GENERIC), [&](auto akc, auto bkc, auto taps) {
    switch (a.operand_bf16) {
      case 0: return f(akc, bkc, taps, std::integral_constant<int, 0>{});
      case 1: return f(akc, bkc, taps, std::integral_constant<int, 1>{});
      case 2: return f(akc, bkc, taps, std::integral_constant<int, 2>{});
    }
    if constexpr (STORED3 && akc && bkc && taps != FS2_TAPS_GENERIC)
      if (a.operand_bf16 == 3) return f(akc, bkc, taps, std::integral_constant<int, 3>{});
    return (int)FS2HIP_EINVAL;
  });
}

// Grid of a weights-stationary launch: workgroups own column slices of `cols` and walk row streams (tiles of 32 rows); the
// slices of a stream share an XCD, `per_cu` workgroups fit a CU, and few rows get no more streams than row tiles.
// false: more slices than an XCD has slots (the caller refuses).
struct Fs2WsGrid { int n_slices, n_streams, n_row_tiles, blocks; };
inline bool fs2_ws_grid(const Fs2GemmArgs& a, int cols, int per_cu, Fs2WsGrid& g) {
  const int per_xcd = fs2_cu_count() / 8 * per_cu;
  g.n_slices = (a.Nc + cols - 1) / cols;
  if (per_xcd < 1 || g.n_slices > per_xcd) return false;
  g.n_row_tiles = (a.Mc + 31) / 32;
  int streams_per_xcd = per_xcd / g.n_slices;
  while (streams_per_xcd > 1 && (streams_per_xcd - 1) * 8 >= g.n_row_tiles) --streams_per_xcd;
  g.n_streams = streams_per_xcd * 8;
  g.blocks = g.n_streams * g.n_slices;
  return true;
}

// Member table of a grouped launch: each member's tile counts and split-K chunk, and its first workgroup in g.start.
// Returns the grid size, 0 = more workgroups than a grid dimension holds.
template <int BM, int BN>
inline int fs2_group_starts(GemmPG& g, int BK) {
  long long total = 0;
  for (int i = 0; i < g.n; ++i) {
    GemmP& p = g.m[i];
    p.r_chunk = fs2_split_chunk(p.a, BK);
    g.start[i] = (int)total;
    const int units = fs2_set_tiles<BM, BN>(p, p.a.splitk);
    total += units;
    if (!units || total > 0x7fffffffLL) return 0;
  }
  for (int i = g.n; i <= FS2_GEMM_GROUP_MAX; ++i) g.start[i] = (int)total;
  return (int)total;
}

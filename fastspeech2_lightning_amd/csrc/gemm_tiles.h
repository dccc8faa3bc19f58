// Every GEMM tile id (Fs2GemmArgs.tile), written once: which kernel family runs it and with which geometry.  gemm.hip
// routes a launch by the row's family, every family's launcher takes its template arguments from the row
// (fs2_tile_switch), and the binding's GEMM_TILES / GEMM_TILES_B / GROUP_TILES are checked against these rows by
// tests/test_gemm_tiles_cpu.py.  Host-only.
#pragma once
#include "common.h"

enum Fs2TileFamily {
  FS2_TF_STAGED,        // gemm.hip: register-staged BK = 16 core, fp32 only, any of the four orientations
  FS2_TF_LDS,           // gemm2.hip: direct-to-LDS BK = 32 core, one output tile per workgroup
  FS2_TF_PERSIST,       // gemm2p.hip: the same core, one K-tile stream per workgroup across its tiles
  FS2_TF_PERSIST_TAIL,  // gemm2p.hip: + the last partial round of tiles cut along the reduction (needs `workspace`)
  FS2_TF_B,             // gemm_bf16.hip: bf16-storage core (operand_bf16 == 4), one output tile per workgroup
  FS2_TF_BP,            // gemm_bf16p.hip: bf16-storage core, persistent
  FS2_TF_WS_K256,       // gemm_ws.hip: weights-stationary streaming form, 16-bit operands, K = 256, forward orientation
  FS2_TF_WS_K1024,      // gemm_ws4.hip: the same for K = 1024
  FS2_TF_WS32,          // gemm_ws32.hip: the same structure in exact fp32, K = 256
};

struct Fs2Tile {
  int id;
  Fs2TileFamily family;
  int bm, bn;    // output tile of a workgroup (weights-stationary forms: rows per A tile, columns per workgroup)
  int depth;     // one tile per workgroup: stages of the LDS ring; persistent and weights-stationary: workgroups per CU
  bool grouped;  // a grouped instance (fs2hip_gemm_grouped) exists
};

// clang-format off
constexpr Fs2Tile FS2_TILES[] = {
  { 1, FS2_TF_STAGED,       128, 128, 2, false},
  { 2, FS2_TF_STAGED,       128,  64, 2, false},
  { 3, FS2_TF_STAGED,        64,  64, 2, false},
  { 4, FS2_TF_LDS,          128, 128, 3, false},  // 96 KiB ring, 1 workgroup / CU
  { 5, FS2_TF_LDS,          128,  64, 3, false},  // 72 KiB ring, 2 workgroups / CU
  { 6, FS2_TF_LDS,           64,  64, 4, false},  // 64 KiB ring, 2 workgroups / CU
  { 7, FS2_TF_LDS,           64,  64, 2, true },  // 32 KiB, 5 workgroups / CU (occupancy instead of depth); the one tile
                                                  // with the generic conv-tap decode (FS2_TILE_GENERIC_TAPS)
  { 8, FS2_TF_LDS,          128,  64, 2, true },  // 48 KiB, 3 workgroups / CU
  { 9, FS2_TF_LDS,          128, 128, 2, false},  // 64 KiB, 2 workgroups / CU
  {10, FS2_TF_PERSIST,       64,  64, 4, false},  // 128 VGPRs: 4 waves per SIMD
  {11, FS2_TF_PERSIST,      128,  64, 3, false},
  {12, FS2_TF_PERSIST,      128, 128, 2, false},
  {13, FS2_TF_PERSIST_TAIL, 128, 128, 2, false},
  {14, FS2_TF_PERSIST_TAIL, 128,  64, 3, false},
  {15, FS2_TF_PERSIST_TAIL,  64,  64, 4, false},
  {20, FS2_TF_B,            128, 128, 2, false},  // 2 workgroups / CU
  {21, FS2_TF_B,            128,  64, 3, false},  // 72 KiB: 2 workgroups / CU, two K-tiles in flight each
  {22, FS2_TF_B,            128,  64, 2, true },  // 3 workgroups / CU
  {23, FS2_TF_B,             64,  64, 3, true },  // 3 workgroups / CU
  {24, FS2_TF_BP,           128, 128, 2, false},
  {25, FS2_TF_BP,           128,  64, 3, false},
  {26, FS2_TF_B,             64,  64, 2, true },  // 32 KiB: 5 workgroups / CU
  {30, FS2_TF_WS_K256,       32, 512, 1, false},  // 64 output columns per wavefront
  {31, FS2_TF_WS_K256,       32, 256, 1, false},  // 32 per wavefront; with bf16 results 70 KB of LDS: 2 workgroups / CU
  {32, FS2_TF_WS32,          32, 256, 1, false},
  {33, FS2_TF_WS_K1024,      32, 128, 1, false},  // 150 KB of LDS, 512 registers per lane
};
// clang-format on
// [A deep-ring form of the bf16-storage core -- one workgroup per CU, a ring of 4-5 stages with counted waits across tile
// boundaries and epilogues -- was built, is correct, and is slower on every shape (one wavefront per SIMD cannot overlap
// DMA issue, LDS reads, MFMAs and the epilogue): kept as tools/probes/gemm_bf16_deep_ring.hip.txt, see DESIGN.md.]
constexpr int FS2_N_TILES = sizeof(FS2_TILES) / sizeof(FS2_TILES[0]);

// what the library picks when Fs2GemmArgs.tile is 0 (gemm_prepare's heuristic, fs2hip_gemm_grouped)
constexpr int FS2_TILE_STAGED_WIDE = 1, FS2_TILE_STAGED_NARROW = 2, FS2_TILE_STAGED_SMALL = 3;
constexpr int FS2_TILE_LDS_WIDE = 4, FS2_TILE_LDS_NARROW = 5;
constexpr int FS2_TILE_GENERIC_TAPS = 7;  // conv taps that are not uniform per K-tile: this tile's instances only
constexpr int FS2_TILE_B_MANY = 20, FS2_TILE_B_FEW = 23;  // bf16-storage core: 256 work units of 128 x 128 or more / fewer
constexpr int FS2_TILE_GROUP_DEFAULT = 7, FS2_TILE_GROUP_DEFAULT_B = 23;

constexpr const Fs2Tile* fs2_tile(int id) {
  for (int i = 0; i < FS2_N_TILES; ++i)
    if (FS2_TILES[i].id == id) return &FS2_TILES[i];
  return nullptr;
}
// the families that read bf16 operands from memory in any orientation (operand_bf16 == 4); the others take fp32 operands
constexpr bool fs2_family_stored(Fs2TileFamily f) {
  return f == FS2_TF_B || f == FS2_TF_BP || f == FS2_TF_WS_K256 || f == FS2_TF_WS_K1024;
}

template <int I>
struct Fs2Row {  // a row as a type: r.t.bm etc. of an object r are compile-time constants
  static constexpr Fs2Tile t = FS2_TILES[I];
};
// A family's switch over its tile ids: f(Fs2Row<I>{}) for the row of `tile` if it belongs to family FA or FB, else
// FS2HIP_EINVAL.  f is instantiated for the rows of those families only.
template <Fs2TileFamily FA, Fs2TileFamily FB = FA, int I = 0, class F>
int fs2_tile_switch(int tile, F&& f) {
  if constexpr (I == FS2_N_TILES) {
    return FS2HIP_EINVAL;
  } else {
    if constexpr (FS2_TILES[I].family == FA || FS2_TILES[I].family == FB)
      if (FS2_TILES[I].id == tile) return f(Fs2Row<I>{});
    return fs2_tile_switch<FA, FB, I + 1>(tile, f);
  }
}

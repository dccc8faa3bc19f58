// One output tile per workgroup on the bf16-storage GEMM core (gemm_bf16_core.h): the forward and data-gradient GEMMs
// (short reductions, whole-row stores through LDS).  The persistent form is gemm_bf16p.hip.
#include "gemm_bf16_core.h"
#include "gemm_launch.h"

namespace {

static_assert(BT_NONE == FS2_TAPS_NONE && BT_RED == FS2_TAPS_RED && BT_ROWS == FS2_TAPS_ROWS,
              "the launch helpers' tap modes are this core's TAPS arguments");

// ``bid`` of ``nblk``: the workgroup's index inside its launch -- or, in a grouped launch, inside its member's share of it
template <int BM, int BN, bool AKC, bool BKC, int TAPS, int NST, bool COLSUM>
__device__ __forceinline__ void gemmb_body(const GemmP& p, const int bid, const int nblk) {
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  constexpr int L = BM / 32 + BN / 32;  // LDS-DMA instructions per thread per K-tile
  static_assert(NST >= 2 && NST <= 4 && (NST - 2) * L < 64, "ring depth");
  __shared__ __attribute__((aligned(16))) char lds[NST * STAGE];
  const Fs2GemmArgs& a = p.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntile = p.tiles_m * p.tiles_n;
  const int unit = fs2_xcd_remap(bid, nblk);
  const int z = unit / ntile;
  const int wg = unit - z * ntile;
  const int tile_m = wg / p.tiles_n, tile_n = wg - tile_m * p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  int tapz = 0, split = 0;
  if (a.shift_operand == 1 || a.splitk > 1) {  // slice order (split, tap)
    const int ntap = a.shift_operand == 1 ? a.taps : 1;
    split = z / ntap;
    tapz = z - split * ntap;
  }
  const int r_begin = split * p.r_chunk;
  const int r_end = min(a.R, r_begin + p.r_chunk);
  // (the chunk is rounded up to whole K-tiles, so the last slices of a split can be empty: they write zero slabs)
  const int nkt = r_end > r_begin ? (r_end - r_begin + BKE - 1) / BKE : 0;
  const int shift_z = tapz * a.tap_mul + a.tap_add;

  f32x16 acc[TM][TN];
  f32x16 cs[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) cs[i][r] = 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }
  // the bias gradient comes from the workgroups of the first tile column (and, for a convolution, of the centre-most
  // tap only: every tap slice sees the same A rows)
  const bool do_cs = COLSUM && a.colsum != nullptr && tile_n == 0 && tapz == 0;

  PiecesB<BM> pa;
  PiecesB<BN> pb;
  StreamB<AKC, BKC, TAPS> st;
  setup_pieces_b<BM, AKC, true, TAPS>(pa, p, m0, r_begin, tid);
  setup_pieces_b<BN, BKC, false, TAPS>(pb, p, n0, r_begin, tid);
  st.begin(p, r_begin, r_end, shift_z);
  auto issue = [&](int stage) {
#ifdef FS2_PROBES
    if (p.probe & 2) return;
#endif
    char* At = lds + stage * STAGE;
    st.template issue<BM, BN>(p, At, At + A_BYTES, pa, pb, wave, tid);
  };

  const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)lds;
  RdB<BM, AKC> rda;
  RdB<BN, BKC> rdb;
  rda.setup(wm * (BM / 2), lane);
  rdb.setup(wn * (BN / 2), lane);

  for (int kt = 0; kt < NST - 1 && kt < nkt; ++kt) issue(kt);
  int stage = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int newer = min(NST - 2, nkt - 1 - kt);
    if (NST >= 4 && newer == 2) b_wait_vmcnt_barrier<2 * L>();
    else if (NST >= 3 && newer == 1) b_wait_vmcnt_barrier<L>();
    else b_wait_vmcnt_barrier<0>();
    if (kt + NST - 1 < nkt) issue(stage == 0 ? NST - 1 : stage - 1);  // the stage read in iteration kt - 1
    const unsigned sa = lds0 + stage * STAGE, sb = sa + A_BYTES;
#ifdef FS2_PROBES
    if (!(p.probe & 1))
#endif
    compute_ktile_b<BM, BN, AKC, BKC, COLSUM>(acc, cs, rda, rdb, sa, sb, do_cs);
    stage = stage + 1 == NST ? 0 : stage + 1;
  }
  // the stages are free once every wavefront has left the last K-tile: each takes a region of them for its stores
  static_assert(4 * Stager<(BN / 2) * 4>::BYTES <= NST * STAGE, "staging regions fit in the ring");
  __builtin_amdgcn_s_barrier();
#ifdef FS2_PROBES
  if (p.probe & 4) return;
#endif
  epilogue_dispatch_b<BM, BN, true>(p, acc, m0, n0, wm, wn, lane, split, tapz, lds + wave * Stager<(BN / 2) * 4>::BYTES);
  if (COLSUM && do_cs && wn == 0 && lane < 32) {  // every row of cs[i] is the same sum: take the lane's first register
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * (BM / 2) + 32 * i + lane;
      if (m < a.Mc) a.colsum[(long long)split * a.Mc + m] = cs[i][0];
    }
  }
}

template <int BM, int BN, bool AKC, bool BKC, int TAPS, int NST, bool COLSUM>
__global__ __launch_bounds__(256) void gemmb_kernel(GemmP p) {
  gemmb_body<BM, BN, AKC, BKC, TAPS, NST, COLSUM>(p, blockIdx.x, gridDim.x);
}

// grouped launch (GemmPG, gemm_common.h): the member that owns this workgroup, then the same code on ITS arguments
template <int BM, int BN, bool AKC, bool BKC, int NST, bool COLSUM>
__global__ __launch_bounds__(256) void gemmbg_kernel(GemmPG g) {
  const int i = fs2_group_member(g, blockIdx.x);
  gemmb_body<BM, BN, AKC, BKC, BT_NONE, NST, COLSUM>(g.m[i], blockIdx.x - g.start[i], g.start[i + 1] - g.start[i]);
}

template <int BM, int BN, int NST>
int launch_b(GemmP& p, int nz, hipStream_t s) {
  const int units = fs2_set_tiles<BM, BN>(p, nz);
  if (!units) return FS2HIP_EINVAL;
  // (forward; data gradient: the weight as it is stored, read by rows of the reduction; weight gradient + bias gradient)
  return fs2_dispatch_orient_taps<false>(p.a, fs2_tap_mode(p, BKE, false), [&](auto akc, auto bkc, auto taps) {
    gemmb_kernel<BM, BN, akc, bkc, taps, NST, !akc && !bkc><<<dim3(units), dim3(256), 0, s>>>(p);
    return fs2_launched();
  });
}

template <int BM, int BN, int NST>
int launch_b_grouped(GemmPG& g, hipStream_t s) {
  const int total = fs2_group_starts<BM, BN>(g, BKE);
  if (!total) return FS2HIP_EINVAL;
  return fs2_dispatch_orient_taps<false>(g.m[0].a, FS2_TAPS_NONE, [&](auto akc, auto bkc, auto) {
    gemmbg_kernel<BM, BN, akc, bkc, NST, !akc && !bkc><<<dim3((unsigned)total), dim3(256), 0, s>>>(g);
    return fs2_launched();
  });
}

}  // namespace

int fs2_gemmb_launch_grouped(GemmPG& g, int tile, hipStream_t s) {
  return fs2_tile_switch<FS2_TF_B>(tile, [&](auto r) {
    if constexpr (r.t.grouped) return launch_b_grouped<r.t.bm, r.t.bn, r.t.depth>(g, s);
    else return (int)FS2HIP_EINVAL;
  });
}

int fs2_gemmb_launch(GemmP& p, int tile, int nz, hipStream_t s) {
  p.r_chunk = fs2_split_chunk(p.a, BKE);
  return fs2_tile_switch<FS2_TF_B>(tile, [&](auto r) { return launch_b<r.t.bm, r.t.bn, r.t.depth>(p, nz, s); });
}

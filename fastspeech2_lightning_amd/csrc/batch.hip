// Device-side feed of a batch with padding (fs2hip_pad_batch): every tensor of a collated batch copied into the
// top-left corner of a larger, otherwise zero tensor -- the padding half of the reference's collate_method
// (fs2/dataset.py:257-293) done on the GPU for a bucket geometry, all tensors in ONE launch.  The member table travels
// as the kernel argument (as fs2hip_gemm_grouped's does): nothing is uploaded, a launch plan replays it as it stands.
// Byte-wise: token ids, durations and fp32 features go through the same code.
#include "common.h"

namespace {

constexpr int PAD_THREADS = 256;
constexpr int PAD_UNITS_PER_LANE = 4;
constexpr int PAD_BLOCK_UNITS = PAD_THREADS * PAD_UNITS_PER_LANE;

// A member in the kernel's terms: the destination is [B][d0][d1][row units], the source [B][s0][s1][row units], a unit
// being 1 << log_unit bytes (the widest power of two up to 16 that divides the row and both base addresses).
struct PadDev {
  const unsigned char* src;
  unsigned char* dst;
  long long units;   // B * d0 * d1 * row_units
  int s0, s1, d0, d1;
  int row_units;
  int log_unit;
  unsigned first_block;  // prefix count: this member's workgroups are [first_block, next member's first_block)
  int pad_;
};
struct PadTable {
  PadDev m[FS2_PAD_MAX_MEMBERS];
  int n;
};

template <typename V>
__device__ __forceinline__ void pad_units(const PadDev& m, long long u0) {
  const V* __restrict__ src = reinterpret_cast<const V*>(m.src);
  V* __restrict__ dst = reinterpret_cast<V*>(m.dst);
#pragma unroll
  for (int k = 0; k < PAD_UNITS_PER_LANE; ++k) {
    const long long u = u0 + (long long)k * PAD_THREADS + threadIdx.x;  // consecutive lanes, consecutive units
    if (u >= m.units) return;
    const int c = (int)(u % m.row_units);
    long long r = u / m.row_units;
    const int i1 = (int)(r % m.d1);
    r /= m.d1;
    const int i0 = (int)(r % m.d0);
    const long long b = r / m.d0;
    V v = {};
    if (i0 < m.s0 && i1 < m.s1) v = src[((b * m.s0 + i0) * m.s1 + i1) * (long long)m.row_units + c];
    dst[u] = v;
  }
}

__global__ __launch_bounds__(PAD_THREADS) void pad_batch_kernel(const PadTable tab) {
  int i = 0;  // (uniform over the workgroup: the member whose block range holds blockIdx.x)
  while (i + 1 < tab.n && blockIdx.x >= tab.m[i + 1].first_block) ++i;
  const PadDev& m = tab.m[i];
  const long long u0 = (long long)(blockIdx.x - m.first_block) * PAD_BLOCK_UNITS;
  switch (m.log_unit) {
    case 4: pad_units<uint4>(m, u0); break;
    case 3: pad_units<uint2>(m, u0); break;
    case 2: pad_units<unsigned int>(m, u0); break;
    case 1: pad_units<unsigned short>(m, u0); break;
    default: pad_units<unsigned char>(m, u0); break;
  }
}

}  // namespace

extern "C" int fs2hip_pad_batch(const Fs2PadMember* members, int n, void* stream) {
  if (!members || n <= 0 || n > FS2_PAD_MAX_MEMBERS) return FS2HIP_EINVAL;
  PadTable tab = {};
  unsigned long long blocks = 0;
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const Fs2PadMember& a = members[i];
    if (!a.src || !a.dst) return FS2HIP_EINVAL;
    if (a.B <= 0 || a.src0 <= 0 || a.src1 <= 0 || a.dst0 <= 0 || a.dst1 <= 0 || a.row_bytes <= 0) return FS2HIP_EINVAL;
    if (a.dst0 < a.src0 || a.dst1 < a.src1) return FS2HIP_EINVAL;
    const long long src_bytes = (long long)a.B * a.src0 * a.src1 * a.row_bytes;
    const long long dst_bytes = (long long)a.B * a.dst0 * a.dst1 * a.row_bytes;
    const uintptr_t s = (uintptr_t)a.src, d = (uintptr_t)a.dst;
    if (s == d && src_bytes == dst_bytes) continue;                  // the tensor is already where it belongs
    if (s < d + (uintptr_t)dst_bytes && d < s + (uintptr_t)src_bytes) return FS2HIP_EINVAL;  // overlapping boxes
    // fold axes that are not padded into the row: longer contiguous runs, wider units
    long long row = a.row_bytes;
    int s0 = a.src0, s1 = a.src1, d0 = a.dst0, d1 = a.dst1;
    for (int pass = 0; pass < 2; ++pass) {
      if (s1 == d1 && row * d1 <= 0x7fffffffLL) {
        row *= d1;
        s1 = s0; d1 = d0;
        s0 = d0 = 1;
      }
    }
    int log_unit = 4;
    while (log_unit > 0 && ((row | (long long)s | (long long)d) & ((1LL << log_unit) - 1))) --log_unit;
    PadDev& m = tab.m[k++];
    m.src = (const unsigned char*)a.src;
    m.dst = (unsigned char*)a.dst;
    m.s0 = s0; m.s1 = s1; m.d0 = d0; m.d1 = d1;
    m.row_units = (int)(row >> log_unit);
    m.log_unit = log_unit;
    m.units = dst_bytes >> log_unit;
    m.first_block = (unsigned)blocks;
    blocks += (unsigned long long)((m.units + PAD_BLOCK_UNITS - 1) / PAD_BLOCK_UNITS);
    if (blocks > 0x7fffffffULL) return FS2HIP_EINVAL;
  }
  if (k == 0) return 0;
  tab.n = k;
  pad_batch_kernel<<<dim3((unsigned)blocks), dim3(PAD_THREADS), 0, (hipStream_t)stream>>>(tab);
  FS2_LAUNCH_CHECK();
  return 0;
}

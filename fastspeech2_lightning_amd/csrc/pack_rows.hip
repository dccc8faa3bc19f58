// Ragged pack of several small [B][T] tensors in one call (fs2hip_pack_rows): the per-token and per-frame quantities of
// a synthesized batch -- rounded durations, pitch and energy predictions -- every utterance's row cut to its own length
// and written back to back, so that they leave the GPU inside the copy that carries the spectrograms.  The member table
// travels as the kernel argument (as fs2hip_pad_batch's does): nothing is uploaded.  Byte-wise on 4-byte elements:
// int32 durations and fp32 predictions go through the same code.
// HBM-trivial (a few kilobytes per batch): lane i reads element t0 + i of a row and writes element offsets[b] + t0 + i
// of the packed member, 256 B per wavefront either way; a destination is only 4-byte aligned, so nothing wider is used.
#include "common.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_PER_LANE = 4;
constexpr int PR_BLOCK_ELEMS = PR_THREADS * PR_PER_LANE;  // elements of one row a workgroup copies

struct PackRowsTable {
  Fs2PackMember m[FS2_PACK_MAX_MEMBERS];
  unsigned first_block[FS2_PACK_MAX_MEMBERS + 1];  // member i's copy workgroups are [first_block[i], first_block[i + 1])
  int n;
  int B;
};

__device__ __forceinline__ int pr_clamp_len(int n, int T) { return n < 0 ? 0 : (n > T ? T : n); }

// One workgroup per member: offsets[b] = len_0 + ... + len_{b-1}, offsets[B] = the total; lens clamped to 0..T.  Every
// thread sums a contiguous chunk of utterances, the 256 chunk sums are scanned in LDS, the chunk is walked again
// (pack_spec_offsets_kernel's scheme).
__global__ __launch_bounds__(PR_THREADS) void pack_rows_offsets_kernel(const PackRowsTable tab) {
  __shared__ long long part[PR_THREADS];
  const Fs2PackMember& m = tab.m[blockIdx.x];
  const int* __restrict__ lens = m.lens;
  long long* __restrict__ offsets = m.offsets;
  const int B = tab.B, T = m.T, tid = threadIdx.x;
  const int chunk = (B + PR_THREADS - 1) / PR_THREADS;
  const int lo = min(tid * chunk, B), hi = min(lo + chunk, B);
  long long s = 0;
  for (int b = lo; b < hi; ++b) s += pr_clamp_len(lens[b], T);
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < PR_THREADS; o <<= 1) {  // inclusive Hillis-Steele scan
    const long long v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - s;  // exclusive prefix of this thread's chunk
  for (int b = lo; b < hi; ++b) {
    offsets[b] = run;
    run += pr_clamp_len(lens[b], T);
  }
  if (tid == PR_THREADS - 1) offsets[B] = part[tid];
}

// One workgroup = PR_BLOCK_ELEMS consecutive elements of one row of one member.  Elements at and beyond the row's length
// are neither read nor written; a row's workgroups that start there return at once.
__global__ __launch_bounds__(PR_THREADS) void pack_rows_kernel(const PackRowsTable tab) {
  int i = 0;  // (uniform over the workgroup: the member whose block range holds blockIdx.x)
  while (i + 1 < tab.n && blockIdx.x >= tab.first_block[i + 1]) ++i;
  const Fs2PackMember& m = tab.m[i];
  const int T = m.T;
  const unsigned tiles = (unsigned)((T + PR_BLOCK_ELEMS - 1) / PR_BLOCK_ELEMS);
  const unsigned local = blockIdx.x - tab.first_block[i];
  const int b = (int)(local / tiles);
  const int t0 = (int)(local % tiles) * PR_BLOCK_ELEMS;
  const int len = pr_clamp_len(m.lens[b], T);
  if (t0 >= len) return;
  const unsigned int* __restrict__ src = reinterpret_cast<const unsigned int*>(m.src) + (long long)b * T;
  unsigned int* __restrict__ dst = reinterpret_cast<unsigned int*>(m.dst) + m.offsets[b];
#pragma unroll
  for (int k = 0; k < PR_PER_LANE; ++k) {
    const int t = t0 + k * PR_THREADS + (int)threadIdx.x;  // consecutive lanes, consecutive elements
    if (t < len) dst[t] = src[t];
  }
}

}  // namespace

extern "C" int fs2hip_pack_rows(const Fs2PackMember* members, int n, int B, void* stream) {
  if (!members || n <= 0 || n > FS2_PACK_MAX_MEMBERS || B <= 0) return FS2HIP_EINVAL;
  PackRowsTable tab = {};
  unsigned long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const Fs2PackMember& a = members[i];
    if (!a.src || !a.lens || !a.dst || !a.offsets || a.T <= 0) return FS2HIP_EINVAL;
    tab.m[i] = a;
    tab.first_block[i] = (unsigned)blocks;
    blocks += (unsigned long long)B * (unsigned long long)((a.T + PR_BLOCK_ELEMS - 1) / PR_BLOCK_ELEMS);
    if (blocks > 0x7fffffffULL) return FS2HIP_EINVAL;
  }
  tab.first_block[n] = (unsigned)blocks;
  tab.n = n;
  tab.B = B;
  hipStream_t s = (hipStream_t)stream;
  pack_rows_offsets_kernel<<<dim3((unsigned)n), dim3(PR_THREADS), 0, s>>>(tab);
  FS2_LAUNCH_CHECK();
  pack_rows_kernel<<<dim3((unsigned)blocks), dim3(PR_THREADS), 0, s>>>(tab);
  FS2_LAUNCH_CHECK();
  return 0;
}

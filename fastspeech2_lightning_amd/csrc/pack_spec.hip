// Packing a batch of predicted spectrograms for the way out of the GPU: every utterance's valid frames, transposed to
// the [bands][frames] layout the spectrogram files hold (fs2/prediction_writing_callback.py:257-262), written back to
// back into one buffer, so that a batch leaves through ONE device-to-host copy instead of one per utterance.
// HBM-bound and tiny: the only care taken is that both the reads (along the bands) and the writes (along the frames) are
// coalesced, which is what the LDS tile is for.
#include "common.h"

namespace {

constexpr int PS_TF = 64;       // frames per tile = lanes of one output row (a 256-B write per wavefront)
constexpr int PS_TC = 32;       // bands per tile  = lanes of one input row (a 128-B read per half wavefront)
constexpr int PS_LD = PS_TC + 1;  // LDS row stride in floats.  Stores: a 32-lane half writes one row, 32 consecutive
                                  // banks.  Loads: lane f reads tile[f][c], bank (33 f + c) % 32 = (f + c) % 32, distinct
                                  // over the 32 lanes of a half (ds_read_b32 / ds_write_b32 bank per 32-lane half).
constexpr int PS_THREADS = 256;

__device__ __forceinline__ int ps_clamp_len(int n, int Tm) { return n < 0 ? 0 : (n > Tm ? Tm : n); }

// offsets[b] = C * (len_0 + ... + len_{b-1}), offsets[B] = the total; lens clamped to 0..Tm.  One workgroup: every
// thread sums a contiguous chunk of utterances, the 256 chunk sums are scanned in LDS, the chunk is walked again.
__global__ __launch_bounds__(PS_THREADS) void pack_spec_offsets_kernel(const int* __restrict__ lens,
                                                                        long long* __restrict__ offsets, int B, int Tm,
                                                                        int C) {
  __shared__ long long part[PS_THREADS];
  const int tid = threadIdx.x;
  const int chunk = (B + PS_THREADS - 1) / PS_THREADS;
  const int lo = min(tid * chunk, B), hi = min(lo + chunk, B);
  long long s = 0;
  for (int b = lo; b < hi; ++b) s += ps_clamp_len(lens[b], Tm);
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < PS_THREADS; o <<= 1) {  // inclusive Hillis-Steele scan
    const long long v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - s;  // exclusive prefix of this thread's chunk, in frames
  for (int b = lo; b < hi; ++b) {
    offsets[b] = run * C;
    run += ps_clamp_len(lens[b], Tm);
  }
  if (tid == PS_THREADS - 1) offsets[B] = part[tid] * C;
}

// One block = one PS_TF x PS_TC tile of one utterance.  blockIdx.x = (b * tiles_t + tile_t) * tiles_c + tile_c.
// Frames at and beyond len_b are neither read nor written; an utterance's tiles that start there return at once.
__global__ __launch_bounds__(PS_THREADS) void pack_spec_kernel(const float* __restrict__ y, const int* __restrict__ lens,
                                                                const long long* __restrict__ offsets,
                                                                float* __restrict__ packed, int Tm, int C, int tiles_t,
                                                                int tiles_c) {
  __shared__ float tile[PS_TF * PS_LD];
  const int tc = blockIdx.x % tiles_c;
  const int rest = blockIdx.x / tiles_c;
  const int tt = rest % tiles_t, b = rest / tiles_t;
  const int len = ps_clamp_len(lens[b], Tm);
  const int t0 = tt * PS_TF, c0 = tc * PS_TC;
  if (t0 >= len) return;  // (uniform over the block: no barrier is skipped by a part of it)
  const int tid = threadIdx.x;
  {  // read along the bands: lane -> band, 8 frames per pass
    const int c = tid % PS_TC, f = tid / PS_TC;
    const float* src = y + ((long long)b * Tm + t0) * C + c0;
#pragma unroll
    for (int k = 0; k < PS_TF; k += PS_THREADS / PS_TC) {
      const int t = f + k;
      if (t0 + t < len && c0 + c < C) tile[t * PS_LD + c] = src[(long long)t * C + c];
    }
  }
  __syncthreads();
  {  // write along the frames: lane -> frame, 4 bands per pass
    const int f = tid % PS_TF, c = tid / PS_TF;
    float* dst = packed + offsets[b] + t0;
#pragma unroll
    for (int k = 0; k < PS_TC; k += PS_THREADS / PS_TF) {
      const int cc = c + k;
      if (t0 + f < len && c0 + cc < C) dst[(long long)(c0 + cc) * len + f] = tile[f * PS_LD + cc];
    }
  }
}

}  // namespace

extern "C" int fs2hip_pack_spec(const float* y, const int* lens, float* packed, long long* offsets, int B, int Tm, int C,
                                void* stream) {
  if (!y || !lens || !packed || !offsets || B <= 0 || Tm <= 0 || C <= 0) return -22;
  const long long tiles_t = (Tm + PS_TF - 1) / PS_TF, tiles_c = (C + PS_TC - 1) / PS_TC;
  const long long blocks = (long long)B * tiles_t * tiles_c;
  if (blocks > 0x7fffffffLL) return -22;
  hipStream_t s = (hipStream_t)stream;
  pack_spec_offsets_kernel<<<1, PS_THREADS, 0, s>>>(lens, offsets, B, Tm, C);
  FS2_LAUNCH_CHECK();
  pack_spec_kernel<<<(unsigned)blocks, PS_THREADS, 0, s>>>(y, lens, offsets, packed, Tm, C, (int)tiles_t, (int)tiles_c);
  FS2_LAUNCH_CHECK();
  return 0;
}

// Zeroes the padded rows of a dense [B][T][row] activation in place (fs2hip_zero_tail_rows): what exact-length inference
// puts in front of every operator that reads a neighbour in time (the depthwise and k-tap convolutions), so that an
// utterance's result does not depend on what the batch's padding rows hold.  Write-only and byte-wise: the rows at and
// beyond lens[b] of utterance b are one contiguous byte range, filled with zero stores of the widest unit that divides
// the row and the base address -- fp32 and bf16 activations go through the same code, and a NaN in the tail is simply
// overwritten.  The lengths are read from device memory: nothing here waits for the host.
#include "common.h"

namespace {

constexpr int ZT_THREADS = 256;
constexpr int ZT_UNITS_PER_LANE = 4;  // sizes the grid only: a workgroup strides over whatever its utterance's tail holds
constexpr unsigned ZT_MAX_BLOCKS_X = 1024;

// grid (x, B): the workgroups of column b share utterance b's tail, units [(b * T + len) * row_units, (b + 1) * T * row_units)
template <typename V>
__global__ __launch_bounds__(ZT_THREADS) void zero_tail_rows_kernel(V* __restrict__ x, long long row_units,
                                                                     const int* __restrict__ lens, int T) {
  const int b = blockIdx.y;
  int len = lens[b];
  len = len < 0 ? 0 : (len > T ? T : len);
  const long long n = (long long)(T - len) * row_units;  // 0 for a full-length utterance: nothing is touched
  V* __restrict__ tail = x + ((long long)b * T + len) * row_units;
  const V zero = {};
  for (long long u = (long long)blockIdx.x * ZT_THREADS + threadIdx.x; u < n; u += (long long)gridDim.x * ZT_THREADS)
    tail[u] = zero;
}

template <typename V>
void launch_zero_tail(void* x, long long row_bytes, const int* lens, int B, int T, hipStream_t s) {
  const long long row_units = row_bytes / (long long)sizeof(V);
  const long long per_block = (long long)ZT_THREADS * ZT_UNITS_PER_LANE;
  long long gx = ((long long)T * row_units + per_block - 1) / per_block;
  gx = gx < 1 ? 1 : (gx > ZT_MAX_BLOCKS_X ? ZT_MAX_BLOCKS_X : gx);
  zero_tail_rows_kernel<V><<<dim3((unsigned)gx, (unsigned)B), dim3(ZT_THREADS), 0, s>>>(reinterpret_cast<V*>(x), row_units,
                                                                                      lens, T);
}

}  // namespace

extern "C" int fs2hip_zero_tail_rows(void* x, long long row_bytes, const int* lens, int B, int T, void* stream) {
  if (!x || !lens || row_bytes <= 0 || B <= 0 || B > 65535 || T <= 0) return FS2HIP_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned long long both = (unsigned long long)row_bytes | (unsigned long long)(uintptr_t)x;
  if ((both & 15) == 0)
    launch_zero_tail<uint4>(x, row_bytes, lens, B, T, s);
  else if ((both & 3) == 0)
    launch_zero_tail<unsigned int>(x, row_bytes, lens, B, T, s);
  else if ((both & 1) == 0)
    launch_zero_tail<unsigned short>(x, row_bytes, lens, B, T, s);
  else
    launch_zero_tail<unsigned char>(x, row_bytes, lens, B, T, s);
  FS2_LAUNCH_CHECK();
  return 0;
}

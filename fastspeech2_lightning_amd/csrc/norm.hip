// LayerNorm forward/backward: one 64-lane wavefront per row, float4 loads, wavefront-shuffle
// reductions (no LDS on the row statistics).  HBM-bound: forward reads x once and writes y once.
#include <cstdlib>

#include "common.h"
#include "dispatch.h"

namespace {

constexpr int LN_MAX_CH = 4;           // C <= 1024: at most 4 float4 chunks per lane
constexpr int LN_BWD_ROWS = 32;        // rows per workgroup in the backward (4 waves x 8 rows) -- of LONG matrices:
// a wavefront walks its rows one after the other (load, two wave reductions, store: a dependent chain of ~1.5 us per row),
// so with 32 rows per workgroup the 4 096 rows of the encoder / the variance predictors are 128 workgroups on 256 CUs,
// each wavefront 8 rows deep: 13 us for a kernel whose bytes take 3.  Short matrices take fewer rows per workgroup
// (more workgroups, shallower chains); the price is more partial rows for the batched second stage: at most 512 with 8
// rows per workgroup (M <= 4 096), at most 1 024 with 16 (M <= 16 384), M / 32 above that (648 for the model's 20 736 rows).
// FS2_LN_BWD_ROWS=8|16|32 (measurement aid): one value for every row count
static inline int ln_bwd_rows(int M) {
  static const int forced = getenv("FS2_LN_BWD_ROWS") ? atoi(getenv("FS2_LN_BWD_ROWS")) : 0;
  if (forced == 8 || forced == 16 || forced == 32) return forced;
  return M > 16384 ? LN_BWD_ROWS : (M > 4096 ? 16 : 8);
}

__device__ __forceinline__ uint2 ln_pack_bf16(float4 o) {
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  typedef float f32v4 __attribute__((ext_vector_type(4)));
  const f32v4 v = {o.x, o.y, o.z, o.w};
  return __builtin_bit_cast(uint2, __builtin_convertvector(v, bf16x4));  // round to nearest even
}
__device__ __forceinline__ float4 ln_unpack_bf16(uint2 u) {
  return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
}

// YB: y is bf16 (the operand a bf16-storage GEMM reads: the normalised activations exist only in that form)
// DROP: y = dropout(LayerNorm(x)) -- the variance predictors' Conv -> ReLU -> LayerNorm -> Dropout layers
// (fs2/layers.py:30-48): the mask is drawn at the element index row * C + c, as the separate pass over y drew it
template <int NCH, bool YB, bool DROP = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, void* __restrict__ y,
                                                      float* __restrict__ mean, float* __restrict__ rstd, int M,
                                                      int C, float eps, Fs2Drop drop_in = Fs2Drop{}) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  Fs2Drop drop = drop_in;
  if constexpr (DROP) drop = fs2_resolve_drop(drop_in);
  const int c4 = C >> 2;
  float4 v[NCH];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int i = lane + 64 * j;
    v[j] = i < c4 ? reinterpret_cast<const float4*>(x + (long long)row * C)[i] : make_float4(0, 0, 0, 0);
    s += v[j].x + v[j].y + v[j].z + v[j].w;
  }
  const float mu = fs2_wave_sum(s) / C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int i = lane + 64 * j;
    if (i < c4) {
      float a = v[j].x - mu, b = v[j].y - mu, c = v[j].z - mu, d = v[j].w - mu;
      q += a * a + b * b + c * c + d * d;
    }
  }
  const float rs = rsqrtf(fs2_wave_sum(q) / C + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int i = lane + 64 * j;
    if (i < c4) {
      float4 g = reinterpret_cast<const float4*>(gamma)[i];
      float4 b = reinterpret_cast<const float4*>(beta)[i];
      float4 o;
      o.x = (v[j].x - mu) * rs * g.x + b.x;
      o.y = (v[j].y - mu) * rs * g.y + b.y;
      o.z = (v[j].z - mu) * rs * g.z + b.z;
      o.w = (v[j].w - mu) * rs * g.w + b.w;
      if constexpr (DROP) {
        float f[4];  // (C is a multiple of 4: row * C + 4 i is even, the quad is two whole hash pairs)
        fs2_drop_quad(drop, (unsigned)(row * C + 4 * i), f);
        o.x *= f[0]; o.y *= f[1]; o.z *= f[2]; o.w *= f[3];
      }
      if constexpr (YB) reinterpret_cast<uint2*>((unsigned short*)y + (long long)row * C)[i] = ln_pack_bf16(o);
      else reinterpret_cast<float4*>((float*)y + (long long)row * C)[i] = o;
    }
  }
}

// dx = rstd * (g*dy - mean(g*dy) - xhat * mean(g*dy*xhat)) (+ dx_add);
// partial[blk][0][C] = sum_rows dy*xhat, partial[blk][1][C] = sum_rows dy
// DZ: a second output dz = dz_scale * dropmask * dx (the gradient entering the sub-module below through its output
// dropout and residual scale: what would otherwise be an axpby launch over dx) and partial[blk][2][C] = sum_rows dz
// (the gradient of that sub-module's last bias: what would otherwise be a column-sum launch over dz)
// DYB: dy is bf16 (the result of a bf16-storage data-gradient GEMM); ZB: dz is written as bf16 (the operand of the next
// data-gradient and weight-gradient GEMMs; its column sums are those of the rounded values)
// PRED: the backward of such a predictor layer in one pass -- dy is first multiplied by the layer's dropout mask
// (`drop_in`), and dx by relu'(pre-activation) = (x > 0), x being the ReLU's output that the LayerNorm normalised
// (what were an axpby launch in front of this kernel and a dact_mul launch behind it)
// XOB (with PRED): dx is written as bf16 -- the operand of the predictor layer's bf16-storage weight- and data-gradient GEMMs
template <int NCH, bool DZ, bool DYB = false, bool ZB = false, bool PRED = false, bool XOB = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ gamma, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ dx_add,
                                                      void* __restrict__ dx, float* __restrict__ partial, int M, int C,
                                                      void* __restrict__ dz, float dz_scale, Fs2Drop drop_in,
                                                      const int rows_per_wg) {
  constexpr int NP = DZ ? 3 : 2;
  __shared__ float red[4][NP][LN_MAX_CH * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c4 = C >> 2;
  const Fs2Drop drop = fs2_resolve_drop(drop_in);
  float4 g[NCH], dg[NCH], db[NCH], dzs[DZ ? NCH : 1];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int i = lane + 64 * j;
    g[j] = i < c4 ? reinterpret_cast<const float4*>(gamma)[i] : make_float4(0, 0, 0, 0);
    dg[j] = make_float4(0, 0, 0, 0);
    db[j] = make_float4(0, 0, 0, 0);
    if constexpr (DZ) dzs[j] = make_float4(0, 0, 0, 0);
  }
  const int row0 = blockIdx.x * rows_per_wg;
  for (int rr = wave; rr < rows_per_wg; rr += 4) {
    const int row = row0 + rr;
    if (row >= M) break;
    const float mu = mean[row], rs = rstd[row];
    float4 xh[NCH], d[NCH];
    unsigned pos[PRED ? NCH : 1];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int i = lane + 64 * j;
      if (i < c4) {
        float4 xv = reinterpret_cast<const float4*>(x + (long long)row * C)[i];
        if constexpr (DYB) d[j] = ln_unpack_bf16(reinterpret_cast<const uint2*>((const unsigned short*)dy + (long long)row * C)[i]);
        else d[j] = reinterpret_cast<const float4*>((const float*)dy + (long long)row * C)[i];
        xh[j] = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
        if constexpr (PRED) {
          float f[4];
          fs2_drop_quad(drop, (unsigned)(row * C + 4 * i), f);
          d[j].x *= f[0]; d[j].y *= f[1]; d[j].z *= f[2]; d[j].w *= f[3];
          pos[j] = (xv.x > 0.f ? 1u : 0u) | (xv.y > 0.f ? 2u : 0u) | (xv.z > 0.f ? 4u : 0u) | (xv.w > 0.f ? 8u : 0u);
        }
      } else {
        d[j] = make_float4(0, 0, 0, 0);
        xh[j] = make_float4(0, 0, 0, 0);
      }
      dg[j].x += d[j].x * xh[j].x; dg[j].y += d[j].y * xh[j].y; dg[j].z += d[j].z * xh[j].z; dg[j].w += d[j].w * xh[j].w;
      db[j].x += d[j].x; db[j].y += d[j].y; db[j].z += d[j].z; db[j].w += d[j].w;
      d[j].x *= g[j].x; d[j].y *= g[j].y; d[j].z *= g[j].z; d[j].w *= g[j].w;
      s1 += d[j].x + d[j].y + d[j].z + d[j].w;
      s2 += d[j].x * xh[j].x + d[j].y * xh[j].y + d[j].z * xh[j].z + d[j].w * xh[j].w;
    }
    s1 = fs2_wave_sum(s1) / C;
    s2 = fs2_wave_sum(s2) / C;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int i = lane + 64 * j;
      if (i < c4) {
        float4 o;
        o.x = rs * (d[j].x - s1 - xh[j].x * s2);
        o.y = rs * (d[j].y - s1 - xh[j].y * s2);
        o.z = rs * (d[j].z - s1 - xh[j].z * s2);
        o.w = rs * (d[j].w - s1 - xh[j].w * s2);
        if (dx_add) {
          float4 r = reinterpret_cast<const float4*>(dx_add + (long long)row * C)[i];
          o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        if constexpr (PRED) {
          if (!(pos[j] & 1u)) o.x = 0.f;
          if (!(pos[j] & 2u)) o.y = 0.f;
          if (!(pos[j] & 4u)) o.z = 0.f;
          if (!(pos[j] & 8u)) o.w = 0.f;
        }
        if constexpr (XOB) reinterpret_cast<uint2*>((unsigned short*)dx + (long long)row * C)[i] = ln_pack_bf16(o);
        else reinterpret_cast<float4*>((float*)dx + (long long)row * C)[i] = o;
        if constexpr (DZ) {
          const unsigned long long e = ((unsigned long long)row * C) + 4ull * i;  // element index in the [M, C] tensor
          float4 z;
          z.x = o.x * dz_scale * fs2_drop_factor(drop, e + 0);
          z.y = o.y * dz_scale * fs2_drop_factor(drop, e + 1);
          z.z = o.z * dz_scale * fs2_drop_factor(drop, e + 2);
          z.w = o.w * dz_scale * fs2_drop_factor(drop, e + 3);
          if constexpr (ZB) {
            const uint2 zb = ln_pack_bf16(z);
            reinterpret_cast<uint2*>((unsigned short*)dz + (long long)row * C)[i] = zb;
            z = ln_unpack_bf16(zb);
          } else {
            reinterpret_cast<float4*>((float*)dz + (long long)row * C)[i] = z;
          }
          dzs[j].x += z.x; dzs[j].y += z.y; dzs[j].z += z.z; dzs[j].w += z.w;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int i = lane + 64 * j;
    reinterpret_cast<float4*>(&red[wave][0][0])[i] = dg[j];
    reinterpret_cast<float4*>(&red[wave][1][0])[i] = db[j];
    if constexpr (DZ) reinterpret_cast<float4*>(&red[wave][2][0])[i] = dzs[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
#pragma unroll
    for (int k = 0; k < NP; ++k)
      partial[((long long)blockIdx.x * NP + k) * C + c] = red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c];
  }
}

// NCH of a launch: the float4 chunks per lane that cover C channels -- 1, 2, or (three included) the 4-chunk instance
template <class F>
int ln_pick_nch(int C, F&& f) {
  return fs2_pick_int<4, 1, 2>((C / 4 + 63) / 64, f);
}

template <bool YB, bool DROP>
int ln_fwd_launch(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M, int C,
                  float eps, Fs2Drop drop, void* stream) {
  return ln_pick_nch(C, [&](auto nch) {
    ln_fwd_kernel<nch, YB, DROP><<<dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream>>>(x, gamma, beta, y, mean, rstd, M,
                                                                                          C, eps, drop);
    return fs2_launched();
  });
}

template <bool DZ, bool DYB, bool ZB, bool PRED, bool XOB>
int ln_bwd_launch(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                  const float* dx_add, void* dx, float* partial, int M, int C, void* dz, float dz_scale, Fs2Drop drop,
                  void* stream) {
  return ln_pick_nch(C, [&](auto nch) {
    ln_bwd_kernel<nch, DZ, DYB, ZB, PRED, XOB><<<dim3(fs2hip_layernorm_bwd_blocks(M)), dim3(256), 0, (hipStream_t)stream>>>(
        dy, x, gamma, mean, rstd, dx_add, dx, partial, M, C, dz, dz_scale, drop, ln_bwd_rows(M));
    return fs2_launched();
  });
}

// what every entry point refuses: the shape, and tensors the float4 accesses cannot take
bool ln_shape_ok(int M, int C) { return M > 0 && C > 0 && (C % 4) == 0 && C <= LN_MAX_CH * 256; }
bool ln_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

extern "C" int fs2hip_layernorm_bwd_blocks(int M) {
  const int rows = ln_bwd_rows(M);
  return (M + rows - 1) / rows;
}

extern "C" int fs2hip_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y,
                                    float* mean, float* rstd, int M, int C, float eps, void* stream) {
  if (!ln_shape_ok(M, C) || !ln_al16(x) || !ln_al16(y) || !ln_al16(gamma) || !ln_al16(beta)) return FS2HIP_EINVAL;
  return ln_fwd_launch<false, false>(x, gamma, beta, y, mean, rstd, M, C, eps, Fs2Drop{}, stream);
}

extern "C" int fs2hip_layernorm_fwd_drop(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                         float* rstd, int M, int C, float eps, float drop_p, unsigned long long drop_seed,
                                         const unsigned long long* drop_step, void* stream) {
  if (!ln_shape_ok(M, C) || (long long)M * C >= 0x7fffffffLL) return FS2HIP_EINVAL;
  if (!ln_al16(x) || !ln_al16(y) || !ln_al16(gamma) || !ln_al16(beta)) return FS2HIP_EINVAL;
  if (!(drop_p > 0.f)) return fs2hip_layernorm_fwd(x, gamma, beta, y, mean, rstd, M, C, eps, stream);
  return ln_fwd_launch<false, true>(x, gamma, beta, y, mean, rstd, M, C, eps, fs2_make_drop(drop_p, drop_seed, drop_step),
                                    stream);
}

extern "C" int fs2hip_layernorm_fwd_b(const float* x, const float* gamma, const float* beta, void* y_bf16,
                                      float* mean, float* rstd, int M, int C, float eps, void* stream) {
  if (!ln_shape_ok(M, C) || !ln_al16(x) || ((uintptr_t)y_bf16 % 8) || !ln_al16(gamma) || !ln_al16(beta)) return FS2HIP_EINVAL;
  return ln_fwd_launch<true, false>(x, gamma, beta, y_bf16, mean, rstd, M, C, eps, Fs2Drop{}, stream);
}

// partial is [nblk][2][C]: dgamma | dbeta partial sums, finished by fs2hip_reduce_rows_multi
extern "C" int fs2hip_layernorm_bwd_pred(const float* dy, const float* x, const float* gamma, const float* mean,
                                         const float* rstd, void* dx, int dx_bf16, float* partial, int M, int C, float drop_p,
                                         unsigned long long drop_seed, const unsigned long long* drop_step, void* stream) {
  if (!ln_shape_ok(M, C) || !partial || (long long)M * C >= 0x7fffffffLL) return FS2HIP_EINVAL;
  if (!ln_al16(x) || !ln_al16(dy) || !ln_al16(dx) || !ln_al16(gamma)) return FS2HIP_EINVAL;
  const Fs2Drop drop = fs2_make_drop(drop_p, drop_seed, drop_step);  // (p = 0: every factor is 1)
  return fs2_pick_bool(dx_bf16 != 0, [&](auto xob) {
    return ln_bwd_launch<false, false, false, true, xob>(dy, x, gamma, mean, rstd, nullptr, dx, partial, M, C, nullptr, 0.f,
                                                         drop, stream);
  });
}

extern "C" int fs2hip_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                                    const float* rstd, const float* dx_add, float* dx, float* partial,
                                    float* dgamma, float* dbeta, int M, int C, void* stream) {
  if (!ln_shape_ok(M, C) || !partial) return FS2HIP_EINVAL;
  if (!ln_al16(x) || !ln_al16(dy) || !ln_al16(dx) || !ln_al16(gamma) || !ln_al16(dx_add)) return FS2HIP_EINVAL;
  const int rc = ln_bwd_launch<false, false, false, false, false>(dy, x, gamma, mean, rstd, dx_add, dx, partial, M, C, nullptr,
                                                                  0.f, fs2_make_drop(0.f, 0), stream);
  // partial is [nblk][2][C]: columns [0, C) -> dgamma, [C, 2C) -> dbeta
  if (rc || (!dgamma && !dbeta)) return rc;  // (neither: the caller finishes the partial sums with fs2hip_reduce_rows_multi)
  return fs2_reduce_rows(partial, fs2hip_layernorm_bwd_blocks(M), 2 * C, 2LL * C, dgamma, C, dbeta, (hipStream_t)stream);
}

// partial is [nblk][3][C]; the caller finishes it with fs2hip_reduce_rows_multi
extern "C" int fs2hip_layernorm_bwd_dz(const float* dy, const float* x, const float* gamma, const float* mean,
                                       const float* rstd, const float* dx_add, float* dx, float* dz, float dz_scale,
                                       float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                       float* partial, int M, int C, void* stream) {
  if (!ln_shape_ok(M, C) || !dz || !partial) return FS2HIP_EINVAL;
  if (!ln_al16(x) || !ln_al16(dy) || !ln_al16(dx) || !ln_al16(dz) || !ln_al16(gamma) || !ln_al16(dx_add)) return FS2HIP_EINVAL;
  return ln_bwd_launch<true, false, false, false, false>(dy, x, gamma, mean, rstd, dx_add, dx, partial, M, C, dz, dz_scale,
                                                         fs2_make_drop(drop_p, drop_seed, drop_step), stream);
}

// The same backward with bf16 on either side of it.  flags bit 0: dy is bf16; bit 1: dz is bf16.  dz == NULL: no
// second output (partial is [nblk][2][C]), else partial is [nblk][3][C].  The caller finishes the partial sums.
extern "C" int fs2hip_layernorm_bwd_x(const void* dy, const float* x, const float* gamma, const float* mean,
                                      const float* rstd, const float* dx_add, float* dx, void* dz, float dz_scale,
                                      float drop_p, unsigned long long drop_seed, const unsigned long long* drop_step,
                                      float* partial, int M, int C, int flags, void* stream) {
  if (!ln_shape_ok(M, C) || !partial) return FS2HIP_EINVAL;
  const bool dyb = flags & 1, zb = flags & 2;
  if (!ln_al16(x) || ((uintptr_t)dy % (dyb ? 8 : 16)) || !ln_al16(dx) || !ln_al16(gamma)) return FS2HIP_EINVAL;
  if (((uintptr_t)dz % (zb ? 8 : 16)) || !ln_al16(dx_add)) return FS2HIP_EINVAL;
  const Fs2Drop drop = fs2_make_drop(dz ? drop_p : 0.f, drop_seed, drop_step);
  return fs2_pick_bool(dyb, [&](auto dyb_c) {
    if (!dz)  // no second output: its type does not matter
      return ln_bwd_launch<false, dyb_c, false, false, false>(dy, x, gamma, mean, rstd, dx_add, dx, partial, M, C, dz,
                                                              dz_scale, drop, stream);
    return fs2_pick_bool(zb, [&](auto zb_c) {
      return ln_bwd_launch<true, dyb_c, zb_c, false, false>(dy, x, gamma, mean, rstd, dx_add, dx, partial, M, C, dz, dz_scale,
                                                            drop, stream);
    });
  });
}

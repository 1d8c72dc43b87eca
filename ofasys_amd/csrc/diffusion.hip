// Motion diffusion training: the three memory-bound row passes around the stack (adaptor/motion_6d.py:84-107, module/diffusion.py:156-173,
// engine/criterion/diffusion_loss.py:50-57).  No float atomics; every sum has a fixed order, so equal inputs give equal bits on every
// launch and every graph replay; levels, masks and the backward seed are read from device memory.
//   q_sample_kernel        x0, noise fp32 [B, T, Dd] -> the adaptor's input rows [B, T, W] in the model dtype: q-sample, the in-betweening
//                          mix with the known frames and the zero padding to W = max_data_dim columns in one pass.  One thread per
//                          16-byte output vector.  The fp32 rows are Dd wide -- 6 + 6 * joints, rarely a multiple of 4 -- so their rows are
//                          not 16-byte aligned: float4 loads when Dd % 4 == 0 (every row then starts aligned), one element per load else.
//   film_fwd_kernel        out = (scale + 1) * h + shift with (scale | shift) = rows[row_of[b, t] or b]: the noise-level modulation.
//   film_bwd_kernel        workgroup (chunk, b): dh for its FILM_CHUNK frames and the fp32 sums of dout * h and dout over them, in ascending t,
//                          per slot (0: the sentence's own row; 1: the shared level-0 row) -> partial [B, chunks, slots, 2D].
//   film_rows_kernel       drows[r]: the chunks of sentence r in ascending order; the shared row: sentences, then chunks, ascending.
//   diffusion_loss_kernel  workgroup (i, b) owns `fpb` frames of sentence b: per-thread fp32 sums of |w_b (pred - target)| over a few
//                          elements, a DPP wave sum, the waves in wave order in fp64 -> partial[b][i]; it counts the sentence's unmasked
//                          frames itself (integers: the same count in every workgroup), so the gradient's divisor is known in the one pass.
//   diffusion_fold_kernel  ONE workgroup: thread j folds sentences j, j + 256, ... (blocks ascending, / count_b), then a fixed LDS tree.
#include "common.h"

namespace ofa {

constexpr int DF_THREADS = 256;
constexpr int DL_BLOCK_ELEMS = 2048;      // pred elements (columns < Dd) a loss workgroup owns, rounded down to whole frames (at least one)

static inline int64_t dl_frames_per_block(int Dd) { return Dd >= DL_BLOCK_ELEMS ? 1 : DL_BLOCK_ELEMS / Dd; }

// N consecutive fp32 of a row whose `nvalid` remaining columns start at p; columns past the row's end read as 0 (never loaded)
template <int N, bool F32VEC> __device__ __forceinline__ void ld_f32_row(const float* __restrict__ p, int nvalid, float* out) {
  if constexpr (F32VEC && N % 4 == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
      if (k + 4 <= nvalid) {
        const float4 q = *reinterpret_cast<const float4*>(p + k);
        out[k] = q.x; out[k + 1] = q.y; out[k + 2] = q.z; out[k + 3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[k + j] = k + j < nvalid ? p[k + j] : 0.f;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = j < nvalid ? p[j] : 0.f;
  }
}

__device__ __forceinline__ int clamp_level(int64_t lv, int n_levels) { return lv < 0 ? 0 : (lv >= n_levels ? n_levels - 1 : (int)lv); }

template <typename T, bool VEC, bool F32VEC>
__global__ __launch_bounds__(DF_THREADS) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ t, const float* __restrict__ known_w,
                                                              const uint8_t* __restrict__ masks, const float* __restrict__ sqrt_acp,
                                                              const float* __restrict__ sqrt_1m_acp, int n_levels, int64_t rows, int Tn,
                                                              int Dd, int W, T* __restrict__ out) {
  constexpr int N = VEC ? Vec<T>::N : 1;
  const int vpr = W / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x; v < total; v += (int64_t)gridDim.x * DF_THREADS) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = 0.f;
    if (c < Dd && !(masks && masks[r])) {
      const int lv = clamp_level(t[r / Tn], n_levels);
      const float a = sqrt_acp[lv], s = sqrt_1m_acp[lv];
      float x[N], z[N];
      const int nvalid = Dd - c;
      ld_f32_row<N, F32VEC>(x0 + r * Dd + c, nvalid, x);
      ld_f32_row<N, F32VEC>(noise + r * Dd + c, nvalid, z);
      if (known_w) {
        const float kw = known_w[r], ukw = 1.f - kw;
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = j < nvalid ? fmaf(kw, x[j], ukw * fmaf(a, x[j], s * z[j])) : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = j < nvalid ? fmaf(a, x[j], s * z[j]) : 0.f;
      }
    }
    if (VEC) store_vec<T>(out + r * W + c, o);
    else st1<T>(out + r * W + c, o[0]);
  }
}

template <typename T>
__global__ __launch_bounds__(DF_THREADS) void film_fwd_kernel(const T* __restrict__ h, const T* __restrict__ rows,
                                                              const int32_t* __restrict__ row_of, int64_t nrows, int Tn, int D, int R,
                                                              T* __restrict__ out) {
  constexpr int N = Vec<T>::N;
  const int vpr = D / N;
  const int64_t total = nrows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * DF_THREADS + threadIdx.x; v < total; v += (int64_t)gridDim.x * DF_THREADS) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    int64_t rr = row_of ? (int64_t)row_of[r] : r / Tn;
    rr = rr < 0 ? 0 : (rr >= R ? R - 1 : rr);                 // (a row outside the table is never read)
    float x[N], sc[N], sh[N], o[N];
    load_vec<T>(h + r * D + c, x);
    load_vec<T>(rows + rr * 2 * D + c, sc);
    load_vec<T>(rows + rr * 2 * D + D + c, sh);
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = fmaf(sc[j] + 1.f, x[j], sh[j]);
    store_vec<T>(out + r * D + c, o);
  }
}

template <typename T, int SLOTS>
__global__ __launch_bounds__(DF_THREADS) void film_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ h, const T* __restrict__ rows,
                                                              const int32_t* __restrict__ row_of, int B, int Tn, int D, T* __restrict__ dh,
                                                              float* __restrict__ partial) {
  constexpr int N = Vec<T>::N;
  const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
  const int f0 = ch * OFA_FILM_CHUNK;
  const int f1 = f0 + OFA_FILM_CHUNK < Tn ? f0 + OFA_FILM_CHUNK : Tn;
  for (int c = threadIdx.x * N; c < D; c += blockDim.x * N) {
    float sc_own[N], sc_sh[N];
    load_vec<T>(rows + (int64_t)b * 2 * D + c, sc_own);
    if (SLOTS == 2) load_vec<T>(rows + (int64_t)B * 2 * D + c, sc_sh);
    float as0[N], ab0[N], as1[N], ab1[N];
#pragma unroll
    for (int j = 0; j < N; ++j) as0[j] = ab0[j] = as1[j] = ab1[j] = 0.f;
    for (int f = f0; f < f1; ++f) {
      const int64_t r = (int64_t)b * Tn + f;
      const bool shared = SLOTS == 2 && row_of[r] != b;      // (the same for every thread of the workgroup)
      float g[N], x[N], o[N];
      load_vec<T>(dout + r * D + c, g);
      load_vec<T>(h + r * D + c, x);
      if (shared) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          o[j] = (sc_sh[j] + 1.f) * g[j];
          as1[j] = fmaf(g[j], x[j], as1[j]);
          ab1[j] += g[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          o[j] = (sc_own[j] + 1.f) * g[j];
          as0[j] = fmaf(g[j], x[j], as0[j]);
          ab0[j] += g[j];
        }
      }
      store_vec<T>(dh + r * D + c, o);
    }
    float* p = partial + ((int64_t)b * nch + ch) * SLOTS * 2 * D;
    store_vec<float>(p + c, as0);
    store_vec<float>(p + D + c, ab0);
    if constexpr (N == 8) {
      store_vec<float>(p + c + 4, as0 + 4);
      store_vec<float>(p + D + c + 4, ab0 + 4);
    }
    if (SLOTS == 2) {
      store_vec<float>(p + 2 * D + c, as1);
      store_vec<float>(p + 3 * D + c, ab1);
      if constexpr (N == 8) {
        store_vec<float>(p + 2 * D + c + 4, as1 + 4);
        store_vec<float>(p + 3 * D + c + 4, ab1 + 4);
      }
    }
  }
}

template <typename T, int SLOTS>
__global__ __launch_bounds__(DF_THREADS) void film_rows_kernel(const float* __restrict__ partial, int B, int nch, int D, T* __restrict__ drows) {
  const int r = blockIdx.y;
  const int col = blockIdx.x * DF_THREADS + threadIdx.x;
  if (col >= 2 * D) return;
  const int64_t stride = (int64_t)SLOTS * 2 * D;              // one (sentence, chunk) record
  float s = 0.f;
  if (r < B) {
    const float* p = partial + (int64_t)r * nch * stride + col;
    for (int ch = 0; ch < nch; ++ch) s += p[ch * stride];
  } else if (SLOTS == 2 && r == B) {
    const float* p = partial + 2 * D + col;
    for (int64_t i = 0; i < (int64_t)B * nch; ++i) s += p[i * stride];
  }
  st1<T>(drows + (int64_t)r * 2 * D + col, s);
}

__device__ __forceinline__ double dl_block_sum(float v, double* sh) {        // the waves in wave order; thread 0 reads the result
  const float w = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (double)w;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < DF_THREADS / WAVE; ++i) s += sh[i];
  return s;
}

template <typename T, bool VEC, bool F32VEC, bool GRAD>
__global__ __launch_bounds__(DF_THREADS) void diffusion_loss_kernel(const T* __restrict__ pred, const float* __restrict__ tgt,
                                                                    const int64_t* __restrict__ t, const uint8_t* __restrict__ masks,
                                                                    const float* __restrict__ w, int n_levels, float scale,
                                                                    const float* __restrict__ seed, int B, int Tn, int Dd, int W, int fpb,
                                                                    double* __restrict__ partial, double* __restrict__ counts,
                                                                    T* __restrict__ dpred) {
  constexpr int N = VEC ? Vec<T>::N : 1;
  __shared__ int shn[DF_THREADS];
  __shared__ double shd[DF_THREADS / WAVE];
  const int tid = threadIdx.x, b = blockIdx.y, nblk = gridDim.x;
  int cnt = Tn;
  if (masks) {                                                // the sentence's unmasked frames: every workgroup computes the same integer
    int c = 0;
    for (int f = tid; f < Tn; f += DF_THREADS) c += masks[(int64_t)b * Tn + f] ? 0 : 1;
    shn[tid] = c;
    __syncthreads();
    for (int o = DF_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) shn[tid] += shn[tid + o];
      __syncthreads();
    }
    cnt = shn[0];
  }
  const float wb = w ? w[clamp_level(t[b], n_levels)] : 1.f;
  const float sd = GRAD ? (seed ? seed[0] : 1.f) : 0.f;
  const float g = GRAD ? (float)((double)sd * (double)scale * (double)wb / ((double)Dd * (double)cnt * (double)B)) : 0.f;
  const int f0 = blockIdx.x * fpb;
  const int f1 = f0 + fpb < Tn ? f0 + fpb : Tn;
  // (the same partition with and without the gradient: the two forms return the same bits)
  const int vpr = (Dd + N - 1) / N;
  const int nv = (f1 - f0) * vpr;
  float acc = 0.f;
  for (int v = tid; v < nv; v += DF_THREADS) {
    const int64_t r = (int64_t)b * Tn + f0 + v / vpr;
    const int c = (v % vpr) * N;
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = 0.f;
    if (c < Dd && !(masks && masks[r])) {
      float p[N], q[N];
      const int nvalid = Dd - c;
      if (VEC) load_vec<T>(pred + r * W + c, p);             // (W is a whole number of vectors: the load stays inside the row)
      else p[0] = ld1<T>(pred + r * W + c);
      ld_f32_row<N, F32VEC>(tgt + r * Dd + c, nvalid, q);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        if (j < nvalid) {
          const float d = p[j] - q[j];
          acc += fabsf(wb * d);
          if (GRAD) o[j] = d > 0.f ? g : (d < 0.f ? -g : 0.f);
        }
      }
    }
    if (GRAD) {
      if (VEC) store_vec<T>(dpred + r * W + c, o);
      else st1<T>(dpred + r * W + c, o[0]);
    }
  }
  if (GRAD) {                                                 // the padding columns of the gradient rows: zeros
    const int zpr = W / N - vpr;
    float z[N];
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = 0.f;
    for (int v = tid; v < (f1 - f0) * zpr; v += DF_THREADS) {
      const int64_t r = (int64_t)b * Tn + f0 + v / zpr;
      const int c = (vpr + v % zpr) * N;
      if (VEC) store_vec<T>(dpred + r * W + c, z);
      else st1<T>(dpred + r * W + c, 0.f);
    }
  }
  const double s = dl_block_sum(acc, shd);
  if (tid == 0) {
    partial[(int64_t)b * nblk + blockIdx.x] = s;
    if (blockIdx.x == 0) counts[b] = (double)cnt;
  }
}

__global__ __launch_bounds__(DF_THREADS) void diffusion_fold_kernel(const double* __restrict__ partial, const double* __restrict__ counts,
                                                                    int B, int nblk, int Dd, float scale, float* __restrict__ out) {
  __shared__ double sh[DF_THREADS];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int b = tid; b < B; b += DF_THREADS) {
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += partial[(int64_t)b * nblk + i];
    a += s / counts[b];
  }
  sh[tid] = a;
  __syncthreads();
  for (int o = DF_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)((double)scale * sh[0] / ((double)B * (double)Dd));
}

static inline unsigned df_grid(int64_t work_items) {            // memory-bound row passes: at most 2048 workgroups, the rest grid-strided
  const int64_t n = (work_items + DF_THREADS - 1) / DF_THREADS;
  return (unsigned)(n < 1 ? 1 : (n > 2048 ? 2048 : n));
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_diffusion_q_sample(const float* x0, const float* noise, const int64_t* t, const float* known_w, const void* masks,
                                      const float* sqrt_acp, const float* sqrt_1m_acp, int n_levels, int B, int T, int Dd, int W,
                                      void* out, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "diffusion_q_sample: bad dtype %d", dtype);
  OFA_REQUIRE(B >= 0 && T >= 0 && Dd > 0 && W >= Dd && n_levels > 0, OFA_ERR_INVALID,
              "diffusion_q_sample: B=%d T=%d Dd=%d W=%d levels=%d (W >= Dd > 0)", B, T, Dd, W, n_levels);
  if (B == 0 || T == 0) return OFA_OK;
  OFA_REQUIRE(x0 && noise && t && sqrt_acp && sqrt_1m_acp && out, OFA_ERR_INVALID, "diffusion_q_sample: bad argument");
  const int64_t rows = (int64_t)B * T;
  const bool vec = W % dt_vecn(dtype) == 0 && aligned16(out);
  const bool f32vec = vec && Dd % 4 == 0 && aligned16(x0) && aligned16(noise);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    const dim3 grid(df_grid(rows * (vec ? W / Vec<T_>::N : W))), block(DF_THREADS);
#define OFA_QS_LAUNCH(V, F)                                                                                                         \
  hipLaunchKernelGGL((q_sample_kernel<T_, V, F>), grid, block, 0, st, x0, noise, t, known_w, (const uint8_t*)masks, sqrt_acp,        \
                     sqrt_1m_acp, n_levels, rows, T, Dd, W, (T_*)out)
    if (f32vec) OFA_QS_LAUNCH(true, true);
    else if (vec) OFA_QS_LAUNCH(true, false);
    else OFA_QS_LAUNCH(false, false);
#undef OFA_QS_LAUNCH
  });
  return check_launch("diffusion_q_sample");
}

static int film_check(const char* who, int dtype, int B, int T, int D, int R, bool has_row_of, const void* a, const void* b,
                      const void* c, const void* d) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(B >= 0 && T >= 0 && D > 0 && D % 8 == 0, OFA_ERR_UNSUPPORTED, "%s: D=%d must be a positive multiple of 8 (B=%d T=%d)", who, D,
              B, T);
  OFA_REQUIRE(has_row_of ? R == B + 1 : R >= B, OFA_ERR_INVALID, "%s: R=%d rows for B=%d sentences (row_of: B + 1, else >= B)", who, R, B);
  OFA_REQUIRE(aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d), OFA_ERR_INVALID, "%s: buffers must be 16-byte aligned", who);
  return OFA_OK;
}

extern "C" int ofa_film_fwd(const void* h, const void* rows, const int32_t* row_of, int B, int T, int D, int R, void* out, int dtype,
                            void* stream) {
  const int rc = film_check("film_fwd", dtype, B, T, D, R, row_of != nullptr, h, rows, out, nullptr);
  if (rc != OFA_OK) return rc;
  if (B == 0 || T == 0) return OFA_OK;
  OFA_REQUIRE(h && rows && out, OFA_ERR_INVALID, "film_fwd: bad argument");
  const int64_t nrows = (int64_t)B * T;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    hipLaunchKernelGGL((film_fwd_kernel<T_>), dim3(df_grid(nrows * (D / Vec<T_>::N))), dim3(DF_THREADS), 0, st, (const T_*)h,
                       (const T_*)rows, row_of, nrows, T, D, R, (T_*)out);
  });
  return check_launch("film_fwd");
}

extern "C" int ofa_film_bwd(const void* dout, const void* h, const void* rows, const int32_t* row_of, int B, int T, int D, int R,
                            void* dh, float* partial, void* drows, int dtype, void* stream) {
  int rc = film_check("film_bwd", dtype, B, T, D, R, row_of != nullptr, dout, h, rows, dh);
  if (rc != OFA_OK) return rc;
  if (R == 0) return OFA_OK;
  OFA_REQUIRE(drows && aligned16(partial), OFA_ERR_INVALID, "film_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int nch = (T + OFA_FILM_CHUNK - 1) / OFA_FILM_CHUNK;
  if (B > 0 && T > 0) {
    OFA_REQUIRE(dout && h && rows && dh && partial, OFA_ERR_INVALID, "film_bwd: bad argument");
    OFA_REQUIRE(B <= 65535, OFA_ERR_UNSUPPORTED, "film_bwd: B=%d sentences exceed the grid", B);
    dispatch_dtype(dtype, [&](auto tag) {
      using T_ = typename decltype(tag)::type;
      int threads = (D / Vec<T_>::N + WAVE - 1) / WAVE * WAVE;
      threads = threads > DF_THREADS ? DF_THREADS : threads;
      const dim3 grid(nch, B), block(threads);
      if (row_of)
        hipLaunchKernelGGL((film_bwd_kernel<T_, 2>), grid, block, 0, st, (const T_*)dout, (const T_*)h, (const T_*)rows, row_of, B, T, D,
                           (T_*)dh, partial);
      else
        hipLaunchKernelGGL((film_bwd_kernel<T_, 1>), grid, block, 0, st, (const T_*)dout, (const T_*)h, (const T_*)rows, row_of, B, T, D,
                           (T_*)dh, partial);
    });
    rc = check_launch("film_bwd");
    if (rc != OFA_OK) return rc;
  }
  OFA_REQUIRE(R <= 65535, OFA_ERR_UNSUPPORTED, "film_bwd: R=%d rows exceed the grid", R);
  const int nchunks = B > 0 && T > 0 ? nch : 0;
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    const dim3 grid((2 * D + DF_THREADS - 1) / DF_THREADS, R), block(DF_THREADS);
    if (row_of) hipLaunchKernelGGL((film_rows_kernel<T_, 2>), grid, block, 0, st, (const float*)partial, B, nchunks, D, (T_*)drows);
    else hipLaunchKernelGGL((film_rows_kernel<T_, 1>), grid, block, 0, st, (const float*)partial, B, nchunks, D, (T_*)drows);
  });
  return check_launch("film_bwd_rows");
}

extern "C" int64_t ofa_diffusion_loss_frames(int Dd) { return Dd > 0 ? dl_frames_per_block(Dd) : 0; }

extern "C" int ofa_diffusion_loss(const void* pred, const float* target, const int64_t* t, const void* masks, const float* w, int n_levels,
                                  float scale, const float* seed, int B, int T, int Dd, int W, double* partial, double* counts,
                                  float* out, void* dpred, int grad, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "diffusion_loss: bad dtype %d", dtype);
  OFA_REQUIRE(B > 0 && T > 0 && Dd > 0 && W >= Dd, OFA_ERR_INVALID, "diffusion_loss: B=%d T=%d Dd=%d W=%d (W >= Dd > 0, no empty batch)", B, T,
              Dd, W);
  OFA_REQUIRE(pred && target && partial && counts && out && (!w || (t && n_levels > 0)), OFA_ERR_INVALID, "diffusion_loss: bad argument");
  OFA_REQUIRE(!grad || dpred, OFA_ERR_INVALID, "diffusion_loss: the gradient form needs its output");
  OFA_REQUIRE(B <= 65535, OFA_ERR_UNSUPPORTED, "diffusion_loss: B=%d sentences exceed the grid", B);
  const int fpb = (int)dl_frames_per_block(Dd);
  const int nblk = (T + fpb - 1) / fpb;
  const bool vec = W % dt_vecn(dtype) == 0 && aligned16(pred) && (!grad || aligned16(dpred));
  const bool f32vec = vec && Dd % 4 == 0 && aligned16(target);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nblk, B), block(DF_THREADS);
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
#define OFA_DL_LAUNCH(V, F, G)                                                                                                       \
  hipLaunchKernelGGL((diffusion_loss_kernel<T_, V, F, G>), grid, block, 0, st, (const T_*)pred, target, t, (const uint8_t*)masks, w,  \
                     n_levels, scale, seed, B, T, Dd, W, fpb, partial, counts, (T_*)dpred)
    if (grad) {
      if (f32vec) OFA_DL_LAUNCH(true, true, true);
      else if (vec) OFA_DL_LAUNCH(true, false, true);
      else OFA_DL_LAUNCH(false, false, true);
    } else {
      if (f32vec) OFA_DL_LAUNCH(true, true, false);
      else if (vec) OFA_DL_LAUNCH(true, false, false);
      else OFA_DL_LAUNCH(false, false, false);
    }
#undef OFA_DL_LAUNCH
  });
  const int rc = check_launch("diffusion_loss");
  if (rc != OFA_OK) return rc;
  hipLaunchKernelGGL(diffusion_fold_kernel, dim3(1), block, 0, st, (const double*)partial, (const double*)counts, B, nblk, Dd, scale, out);
  return check_launch("diffusion_loss_fold");
}

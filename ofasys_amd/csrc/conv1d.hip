// Conv1d over time on batch-major channels-last rows, and the row kernel of the Tacotron postnet's inner layers
// (adaptor/audio.py:735-763: Conv1d(k, padding (k-1)/2) -> BatchNorm1d -> [Tanh] -> Dropout on [B, C, T]).
// A convolution is ofa_unfold1d + ofa_gemm against the weight in (k, c) order; its input gradient is ofa_gemm + ofa_fold1d.
//   unfold1d_kernel   x [B*T, C] -> col [B*T, Kpad]:  col[b*T + t][j*C + c] = x[b*T + t + j - (k-1)/2][c] when that time step lies in
//                     [0, T) of sample b, else 0 (never a neighbouring sample's row); columns k*C .. Kpad-1 are zero.  Only moves values.
//   fold1d_kernel     dcol [B*T, Kpad] -> dx [B*T, C], the adjoint as a GATHER: dx[b*T + s][c] = sum_j dcol[b*T + s - j + (k-1)/2][j*C + c]
//                     over the taps j = 0 .. k-1 (ascending: a fixed order) whose row lies in sample b; fp32 sum, one rounding.  No atomics.
//   tanh_dropout      y = dropout_p(tanh(x)); backward from (dy, y) alone: dx = dy * keep/(1-p) * (1 - t^2), t = y (1-p) where kept.
//                     tanh in fp32 (tanhf); the mask is ofa_dropout_add_fwd's: element e draws halfword e%8 of Philox counter
//                     offset (+ *offset_base) + e/8, so backward regenerates it and nothing is stored.  p = 0 keeps everything: exact tanh.
// 16-byte accesses when C (for tanh_dropout: the group of 8) allows and the buffers are 16-byte aligned, one element per access
// otherwise.  Nothing reads a length: the postnet runs over the padded layout, padded frames included, as the reference does.
// Traffic of a convolution layer: (1 + k) rows*C elements for the unfold on top of the GEMM's own reads -- the known cost of not
// having a tap-loop GEMM.
#include "common.h"

namespace ofa {

static inline int grid_1d(int64_t work) {
  int64_t g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void unfold1d_kernel(const T* __restrict__ x, T* __restrict__ col, int64_t rows, int Tn, int C, int k,
                                                       int Kpad) {
  constexpr int N = VEC ? Vec<T>::N : 1;
  const int K = k * C, half = (k - 1) / 2;
  const int vpr = Kpad / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int kc = (int)(v % vpr) * N;
    const int64_t r = v / vpr;
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = 0.f;
    if (kc < K) {
      const int tap = kc / C, c = kc % C;
      const int t = (int)(r % Tn) + tap - half;
      if (t >= 0 && t < Tn) {
        const T* src = x + (r + tap - half) * C + c;
        if (VEC) load_vec<T>(src, o);
        else o[0] = ld1<T>(src);
      }
    }
    if (VEC) store_vec<T>(col + r * Kpad + kc, o);
    else st1<T>(col + r * Kpad + kc, o[0]);
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void fold1d_kernel(const T* __restrict__ dcol, T* __restrict__ dx, int64_t rows, int Tn, int C, int k,
                                                     int Kpad) {
  constexpr int N = VEC ? Vec<T>::N : 1;
  const int half = (k - 1) / 2;
  const int vpr = C / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int c = (int)(v % vpr) * N;
    const int64_t r = v / vpr;
    const int s = (int)(r % Tn);
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (int tap = 0; tap < k; ++tap) {
      const int t = s - tap + half;                            // the output row whose tap `tap` read row s
      if (t < 0 || t >= Tn) continue;
      const T* src = dcol + (r - tap + half) * Kpad + tap * C + c;
      float g[N];
      if (VEC) load_vec<T>(src, g);
      else g[0] = ld1<T>(src);
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += g[j];
    }
    if (VEC) store_vec<T>(dx + r * C + c, acc);
    else st1<T>(dx + r * C + c, acc[0]);
  }
}

// 8 consecutive elements starting at e (a whole Philox group) as floats; FAST: two / one 16-byte accesses
template <typename T, bool FAST> __device__ __forceinline__ void load8(const T* p, int64_t e, int64_t n, float* o) {
  if (FAST) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int i = 0; i < 8 / N; ++i) load_vec<T>(p + e + i * N, o + i * N);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = e + j < n ? ld1<T>(p + e + j) : 0.f;
  }
}
template <typename T, bool FAST> __device__ __forceinline__ void store8(T* p, int64_t e, int64_t n, const float* o) {
  if (FAST) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int i = 0; i < 8 / N; ++i) store_vec<T>(p + e + i * N, o + i * N);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (e + j < n) st1<T>(p + e + j, o[j]);
  }
}

// BWD: a = dy, b = y -> out = dx;  else a = x -> out = y.  ALIGNED: the buffers are 16-byte aligned (whole groups take the fast path).
template <typename T, bool BWD, bool ALIGNED>
__global__ __launch_bounds__(256) void tanh_dropout_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, int64_t n,
                                                           float p, uint64_t seed, uint64_t offset,
                                                           const int64_t* __restrict__ offset_base) {
  if (offset_base) offset += (uint64_t)offset_base[0];     // device-resident stream position (hipGraph replays advance it)
  const Philox rng(seed);
  const float keep = 1.0f - p, keep_scale = 1.0f / keep;
  const uint32_t thresh = philox_thresh(p);
  const int64_t nq = (n + 7) / 8;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    const int64_t e = q * 8;
    const bool whole = ALIGNED && e + 8 <= n;
    float va[8], vb[8], o[8];
    if (whole) load8<T, true>(a, e, n, va);
    else load8<T, false>(a, e, n, va);
    if (BWD) {
      if (whole) load8<T, true>(b, e, n, vb);
      else load8<T, false>(b, e, n, vb);
    }
    if (thresh == 0) {                                      // p == 0: no draw
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = BWD ? va[j] * (1.0f - vb[j] * vb[j]) : tanhf(va[j]);
    } else {
      const uint4 r = rng(offset + (uint64_t)q);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool kept = philox_keep(r, j, thresh);
        if (BWD) {
          const float t = vb[j] * keep;
          o[j] = kept ? va[j] * keep_scale * (1.0f - t * t) : 0.f;
        } else {
          o[j] = kept ? tanhf(va[j]) * keep_scale : 0.f;
        }
      }
    }
    if (whole) store8<T, true>(out, e, n, o);
    else store8<T, false>(out, e, n, o);
  }
}

static int tanh_dropout_launch(const char* who, const void* a, const void* b, void* out, int64_t n, float p, uint64_t seed, uint64_t offset,
                               const int64_t* offset_base, int dtype, void* stream, bool bwd) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(n >= 0 && p >= 0.f && p < 1.f && (n == 0 || (a && out && (!bwd || b))), OFA_ERR_INVALID, "%s: bad argument", who);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool al = aligned16(a) && aligned16(out) && (!bwd || aligned16(b));
  dim3 grid(grid_1d((n + 7) / 8)), block(256);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (bwd) {
      if (al) hipLaunchKernelGGL((tanh_dropout_kernel<T, true, true>), grid, block, 0, st, (const T*)a, (const T*)b, (T*)out, n, p, seed, offset, offset_base);
      else hipLaunchKernelGGL((tanh_dropout_kernel<T, true, false>), grid, block, 0, st, (const T*)a, (const T*)b, (T*)out, n, p, seed, offset, offset_base);
    } else {
      if (al) hipLaunchKernelGGL((tanh_dropout_kernel<T, false, true>), grid, block, 0, st, (const T*)a, (const T*)nullptr, (T*)out, n, p, seed, offset, offset_base);
      else hipLaunchKernelGGL((tanh_dropout_kernel<T, false, false>), grid, block, 0, st, (const T*)a, (const T*)nullptr, (T*)out, n, p, seed, offset, offset_base);
    }
  });
  return check_launch(who);
}

static int conv1d_check(const char* who, const void* a, const void* b, int64_t B, int Tn, int C, int k, int Kpad, int dtype) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(B >= 0 && Tn > 0 && C > 0 && k > 0 && (B == 0 || (a && b)), OFA_ERR_INVALID, "%s: bad argument", who);
  OFA_REQUIRE(k % 2 == 1, OFA_ERR_UNSUPPORTED, "%s: kernel size %d is even (padding (k-1)/2 keeps the length for odd k only)", who, k);
  OFA_REQUIRE((int64_t)k * C <= 0x7fffffff - 8 && Kpad >= k * C && Kpad % 8 == 0, OFA_ERR_INVALID,
              "%s: Kpad=%d must be a multiple of 8 and at least k*C=%lld", who, Kpad, (long long)k * C);
  return OFA_OK;
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_unfold1d(const void* x, void* col, int64_t B, int T, int C, int k, int Kpad, int dtype, void* stream) {
  const int rc = conv1d_check("unfold1d", x, col, B, T, C, k, Kpad, dtype);
  if (rc != OFA_OK) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = B * T;
  const int n = dt_vecn(dtype);
  const bool vec = C % n == 0 && aligned16(x) && aligned16(col);        // (then k*C and Kpad are whole vectors too)
  dim3 grid(grid_1d(rows * (Kpad / (vec ? n : 1)))), block(256);
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    if (vec) hipLaunchKernelGGL((unfold1d_kernel<T_, true>), grid, block, 0, st, (const T_*)x, (T_*)col, rows, T, C, k, Kpad);
    else hipLaunchKernelGGL((unfold1d_kernel<T_, false>), grid, block, 0, st, (const T_*)x, (T_*)col, rows, T, C, k, Kpad);
  });
  return check_launch("unfold1d");
}

extern "C" int ofa_fold1d(const void* dcol, void* dx, int64_t B, int T, int C, int k, int Kpad, int dtype, void* stream) {
  const int rc = conv1d_check("fold1d", dcol, dx, B, T, C, k, Kpad, dtype);
  if (rc != OFA_OK) return rc;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = B * T;
  const int n = dt_vecn(dtype);
  const bool vec = C % n == 0 && aligned16(dcol) && aligned16(dx);
  dim3 grid(grid_1d(rows * (C / (vec ? n : 1)))), block(256);
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    if (vec) hipLaunchKernelGGL((fold1d_kernel<T_, true>), grid, block, 0, st, (const T_*)dcol, (T_*)dx, rows, T, C, k, Kpad);
    else hipLaunchKernelGGL((fold1d_kernel<T_, false>), grid, block, 0, st, (const T_*)dcol, (T_*)dx, rows, T, C, k, Kpad);
  });
  return check_launch("fold1d");
}

extern "C" int ofa_tanh_dropout_fwd(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset, const int64_t* offset_base,
                                    int dtype, void* stream) {
  return tanh_dropout_launch("tanh_dropout_fwd", x, nullptr, y, n, p, seed, offset, offset_base, dtype, stream, false);
}

extern "C" int ofa_tanh_dropout_bwd(const void* dy, const void* y, void* dx, int64_t n, float p, uint64_t seed, uint64_t offset,
                                    const int64_t* offset_base, int dtype, void* stream) {
  return tanh_dropout_launch("tanh_dropout_bwd", dy, y, dx, n, p, seed, offset, offset_base, dtype, stream, true);
}

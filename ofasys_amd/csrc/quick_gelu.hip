// QuickGELU of the CLIP-style ViT blocks (module/vit.py: x * sigmoid(1.702 x)) for gfx950: streaming kernels, 16-byte vector loads and
// stores, fp32 math, one rounding of the result.  The backward also leaves the column sums of dh -- the gradient of c_fc.bias -- as fp32
// partial rows [slots][cols] for ofa_fold_batched (no float atomics, fixed summation order: two replays give equal bits).
#include "common.h"

namespace ofa {

// s = sigmoid(a) and q = 1 - s from ONE exponential of -|a| (z in (0, 1]: no overflow, and both come out with full relative precision:
// neither is formed as 1 - the other).  EXACT (fp32 kernels): libm expf and an IEEE division.  Otherwise v_exp_f32 + v_rcp_f32, whose
// ~2 ulp of fp32 are three orders of magnitude below the 16-bit output rounding; their results are flushed where z is an fp32
// denormal (|a| > 87.3, i.e. |h| > 51.3), where the exact output is below 2^-120.
template <bool EXACT> __device__ __forceinline__ void sigmoid_pair(float a, float& s, float& q) {
  const float z = EXACT ? expf(-fabsf(a)) : __expf(-fabsf(a));
  const float r = EXACT ? 1.0f / (1.0f + z) : __builtin_amdgcn_rcpf(1.0f + z);
  const float zr = z * r;
  s = a >= 0.f ? r : zr;
  q = a >= 0.f ? zr : r;
}

constexpr float kQuickGelu = 1.702f;

template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_fwd_kernel(const T* __restrict__ h, T* __restrict__ y, int64_t nvec) {
  constexpr int N = Vec<T>::N;
  constexpr bool EXACT = sizeof(T) == 4;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float a[N], o[N];
    load_vec<T>(h + v * N, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float s, q;
      sigmoid_pair<EXACT>(kQuickGelu * a[j], s, q);
      o[j] = a[j] * s;
    }
    store_vec<T>(y + v * N, o);
  }
}

// dh = dy * s * (1 + 1.702 h (1 - s)).  Block: 4 waves; lane l of every wave owns vector column blockIdx.x * 64 + l (a wave reads 1 KiB
// of a row at a time), wave w the rows w, w + 4, ... of the block's slab of `rpb` rows (blockIdx.y).  Column sums: each lane adds its
// rows in row order, the four waves' sums meet in LDS and wave 0 adds them in wave order and writes the slab's partial row.
constexpr int QG_WAVES = 4;
template <typename T>
__global__ __launch_bounds__(64 * QG_WAVES) void quick_gelu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                                        T* __restrict__ dh, float* __restrict__ ws, int64_t rows,
                                                                        int cols, int rpb) {
  constexpr int N = Vec<T>::N;
  constexpr bool EXACT = sizeof(T) == 4;
  __shared__ float red[QG_WAVES][64][N + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + lane) * N;
  const int64_t r0 = (int64_t)blockIdx.y * rpb;
  const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
  float acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = 0.f;
  if (c < cols) {
#pragma unroll 2
    for (int64_t r = r0 + w; r < r1; r += QG_WAVES) {
      float a[N], g[N], o[N];
      load_vec<T>(h + r * cols + c, a);
      load_vec<T>(dy + r * cols + c, g);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        float s, q;
        const float t = kQuickGelu * a[j];
        sigmoid_pair<EXACT>(t, s, q);
        o[j] = g[j] * s * (1.0f + t * q);
        acc[j] += o[j];
      }
      store_vec<T>(dh + r * cols + c, o);
    }
  }
  if (ws == nullptr) return;                 // (the same in every thread of the launch)
#pragma unroll
  for (int j = 0; j < N; ++j) red[w][lane][j] = acc[j];
  __syncthreads();
  if (w == 0 && c < cols) {
    float t[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      t[j] = red[0][lane][j];
#pragma unroll
      for (int k = 1; k < QG_WAVES; ++k) t[j] += red[k][lane][j];
    }
    float* out = ws + (int64_t)blockIdx.y * cols + c;
#pragma unroll
    for (int j = 0; j < N; j += 4) *reinterpret_cast<float4*>(out + j) = make_float4(t[j], t[j + 1], t[j + 2], t[j + 3]);
  }
}

// rows per block of the backward: 32 up to 8192 rows, then as many (a multiple of the 4 waves) as keep the slab count at 256
static inline int qg_rows_per_block(int64_t rows) {
  const int64_t per = (rows + 255) / 256;
  const int64_t rpb = (per + QG_WAVES - 1) / QG_WAVES * QG_WAVES;
  return (int)(rpb < 32 ? 32 : rpb);
}

static int qg_check(const char* who, int64_t rows, int cols, int dtype) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(rows >= 0 && cols > 0, OFA_ERR_INVALID, "%s: bad shape (rows=%lld cols=%d)", who, (long long)rows, cols);
  OFA_REQUIRE(cols % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "%s: cols=%d is not a multiple of the 16-byte vector (%d elements)", who,
              cols, dt_vecn(dtype));
  return OFA_OK;
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_quick_gelu_bwd_slots(int64_t rows, int cols, int dtype) {
  (void)cols;
  (void)dtype;
  if (rows <= 0) return 0;
  return cdiv(rows, qg_rows_per_block(rows));
}

extern "C" int ofa_quick_gelu_fwd(const void* h, void* a, int64_t rows, int cols, int dtype, void* stream) {
  if (int rc = qg_check("quick_gelu_fwd", rows, cols, dtype)) return rc;
  if (rows == 0) return OFA_OK;
  OFA_REQUIRE(h && a, OFA_ERR_INVALID, "quick_gelu_fwd: null pointer");
  OFA_REQUIRE(aligned16(h) && aligned16(a), OFA_ERR_UNSUPPORTED, "quick_gelu_fwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const int64_t nvec = rows * (cols / Vec<T>::N);
    const int64_t g = (nvec + 255) / 256;
    hipLaunchKernelGGL((quick_gelu_fwd_kernel<T>), dim3((int)(g > 2048 ? 2048 : g)), dim3(256), 0, st, (const T*)h, (T*)a, nvec);
  });
  return check_launch("quick_gelu_fwd");
}

extern "C" int ofa_quick_gelu_bwd(const void* dy, const void* h, void* dh, float* ws, int64_t rows, int cols, int dtype,
                                  void* stream) {
  if (int rc = qg_check("quick_gelu_bwd", rows, cols, dtype)) return rc;
  if (rows == 0) return OFA_OK;
  OFA_REQUIRE(dy && h && dh, OFA_ERR_INVALID, "quick_gelu_bwd: null pointer");
  OFA_REQUIRE(aligned16(dy) && aligned16(h) && aligned16(dh) && aligned16(ws), OFA_ERR_UNSUPPORTED,
              "quick_gelu_bwd: buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int rpb = qg_rows_per_block(rows);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    dim3 grid(cdiv(cols / Vec<T>::N, 64), cdiv(rows, rpb));
    hipLaunchKernelGGL((quick_gelu_bwd_kernel<T>), grid, dim3(64 * QG_WAVES), 0, st, (const T*)dy, (const T*)h, (T*)dh, ws, rows, cols,
                       rpb);
  });
  return check_launch("quick_gelu_bwd");
}

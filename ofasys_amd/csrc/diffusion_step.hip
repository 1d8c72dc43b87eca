// One sampling step of motion diffusion (generator/diffusion_generator.py, module/diffusion.py:130-152, preprocessor/default/
// motion_6d.py:394-419, adaptor/motion_6d.py:90-97) in ONE launch for gfx950: classifier-free guidance, the rot6d rectification, the
// in-betweening infill, the clip, the scheduler step, and the next denoiser input with its level.  See include/ofasys_amd.h
// (ofa_diffusion_sample_step) for the contract.
//
// Shape of the work: frames [B, T] of Dd = 6 * U columns, U = 1 + joints "units" of six values (unit 0: the hip's position and velocity,
// passed through; unit u > 0: one joint's a1 | a2).  A unit is what one thread owns from the prediction to the three stores: the
// Gram-Schmidt step needs all six values and nothing of another unit, so no value ever crosses a lane.  A workgroup owns DS_FRAMES
// consecutive frames of ONE sentence; item i of its DS_FRAMES * U items is (frame i / U, unit i % U), so consecutive lanes walk the
// fp32 rows ([B, T, Dd], contiguous: one unit is 24 bytes, 8-byte aligned -> three float2 accesses) without a gap, across frame borders
// too.  The prediction and the next denoiser input sit at a W-wide stride in the model dtype: a unit is three 32-bit words there (six
// 16-bit values, 4-byte aligned whenever W is even), never a 16-byte vector -- 276-byte rows have no 16-byte grid.
//
// In-betweening reads the RECTIFIED prediction of up to two other frames per frame.  It goes through LDS: pass 1 rectifies the tile's
// frames (and two halo frames, below) into an fp32 [DS_FRAMES + 2, Dd] tile, pass 2 mixes from it.  A run of unknown frames shares its
// two known neighbours, so all a tile needs from outside are the lower neighbour of its first frame and the upper neighbour of its last:
// the two halo rows.  Tables that are not of that form (any two frames per row are legal) are served too -- a neighbour that is neither in
// the tile nor a halo row is rectified again by the thread that needs it -- only slower.  Without in-betweening nothing is staged.
//
// Under guidance workgroup (tile, 2k) owns the pair's state: it reads both predictions, and writes x_t and the denoiser input of rows
// 2k AND 2k + 1 (the reference's x_t[1::2] = x_t[0::2]); workgroup (tile, 2k + 1) only writes its row's own x0_hat to img.
//
// The step index lives on the device: every workgroup reads counter[0] before anything else; the LAST workgroup to finish -- found by an
// integer ticket, counter[1] -- stores the incremented index with a plain store from one thread and puts the ticket back to 0.  No float
// atomics, no cross-lane sums: equal inputs give equal bits on every launch and every graph replay.
#include "common.h"

namespace ofa {
namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_FRAMES = 16;          // frames of a workgroup's tile
constexpr int DS_LDS_MAX = 65536;
constexpr float DS_EPS = 1e-12f;       // F.normalize's floor

static_assert(sizeof(ofa_diffusion_step_args) == 152,"ofa_diffusion_step_args: kernels._DiffusionStepArgs mirrors this layout");

// six consecutive values of a row as floats: packed when the address allows it, one element per access otherwise
template <typename T> __device__ __forceinline__ void ld6(const T* p, float* o) {
  if (((uintptr_t)p & 3) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const uint32_t w = q[j];
      T lo, hi;
      lo = __builtin_bit_cast(T, (uint16_t)(w & 0xffffu));
      hi = __builtin_bit_cast(T, (uint16_t)(w >> 16));
      o[2 * j] = ld1<T>(&lo);
      o[2 * j + 1] = ld1<T>(&hi);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = ld1<T>(p + j);
  }
}
template <> __device__ __forceinline__ void ld6<float>(const float* p, float* o) {
  if (((uintptr_t)p & 7) == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float2 v = reinterpret_cast<const float2*>(p)[j];
      o[2 * j] = v.x;
      o[2 * j + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = p[j];
  }
}
template <typename T> __device__ __forceinline__ void st6(T* p, const float* v) {
  if (((uintptr_t)p & 3) == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) reinterpret_cast<uint32_t*>(p)[j] = pack2<T>(v[2 * j], v[2 * j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < 6; ++j) st1<T>(p + j, v[j]);
  }
}
template <> __device__ __forceinline__ void st6<float>(float* p, const float* v) {
  if (((uintptr_t)p & 7) == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) reinterpret_cast<float2*>(p)[j] = make_float2(v[2 * j], v[2 * j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < 6; ++j) p[j] = v[j];
  }
}

// a1 | a2 -> b1 | b2: the two columns rotmat_to_rot6d(rot6d_to_rotmat(x)) keeps (F.normalize: v / max(|v|, 1e-12))
__device__ __forceinline__ void rectify6(float* x) {
  const float n1 = sqrtf(fmaf(x[0], x[0], fmaf(x[1], x[1], x[2] * x[2])));
  const float i1 = 1.f / fmaxf(n1, DS_EPS);
  const float b0 = x[0] * i1, b1 = x[1] * i1, b2 = x[2] * i1;
  const float d = fmaf(b0, x[3], fmaf(b1, x[4], b2 * x[5]));
  const float r0 = fmaf(-d, b0, x[3]), r1 = fmaf(-d, b1, x[4]), r2 = fmaf(-d, b2, x[5]);
  const float i2 = 1.f / fmaxf(sqrtf(fmaf(r0, r0, fmaf(r1, r1, r2 * r2))), DS_EPS);
  x[0] = b0; x[1] = b1; x[2] = b2;
  x[3] = r0 * i2; x[4] = r1 * i2; x[5] = r2 * i2;
}

// the guided, rectified prediction of unit u of frame (b, f)
template <typename T>
__device__ __forceinline__ void predict6(const ofa_diffusion_step_args& a, int b, int f, int u, float* x) {
  const T* p = (const T*)a.pred + ((int64_t)b * a.T + f) * a.W + 6 * u;
  ld6<T>(p, x);
  if (a.guidance != 0.f && (b & 1) == 0) {
    float y[6];
    ld6<T>(p + (int64_t)a.T * a.W, y);
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = fmaf(1.f + a.guidance, x[j], -a.guidance * y[j]);
  }
  if (u > 0) rectify6(x);
}

template <typename T, bool INFILL>
__global__ __launch_bounds__(DS_THREADS) void diffusion_step_kernel(const ofa_diffusion_step_args a) {
  extern __shared__ float tile[];                              // INFILL: [DS_FRAMES + 2, Dd]
  const int tid = threadIdx.x, b = blockIdx.y;
  const int U = a.Dd / 6;
  const int f0 = blockIdx.x * DS_FRAMES;
  const int nf = a.T - f0 < DS_FRAMES ? a.T - f0 : DS_FRAMES;
  const bool guided = a.guidance != 0.f;
  int s = a.first ? 0 : a.counter[0];                          // (read before this workgroup's ticket: see the end)
  s = s < 0 ? 0 : (s >= a.n_steps ? a.n_steps - 1 : s);
  const uint8_t* masks = (const uint8_t*)a.masks;

  int halo[2] = {-1, -1};
  if (INFILL && !a.first) {
    halo[0] = a.nbr[((int64_t)b * a.T + f0) * 2];
    halo[1] = a.nbr[((int64_t)b * a.T + f0 + nf - 1) * 2 + 1];
    for (int i = tid; i < (DS_FRAMES + 2) * U; i += DS_THREADS) {
      const int slot = i / U, u = i % U;
      const int f = slot < DS_FRAMES ? (slot < nf ? f0 + slot : -1) : halo[slot - DS_FRAMES];
      if (f < 0 || f >= a.T) continue;
      float x[6];
      predict6<T>(a, b, f, u, x);
#pragma unroll
      for (int j = 0; j < 6; ++j) tile[slot * a.Dd + 6 * u + j] = x[j];
    }
    __syncthreads();
  }

  if (!(guided && (b & 1) && a.first)) {                        // (the odd row of a pair has nothing to do in the first mode)
    const float c0 = a.coef[3 * s], c1 = a.coef[3 * s + 1], sg = a.coef[3 * s + 2];
    const float* noise = a.noise ? a.noise + (int64_t)s * a.noise_stride : nullptr;
    for (int i = tid; i < nf * U; i += DS_THREADS) {
      const int fl = i / U, u = i % U, f = f0 + fl;
      const int64_t r = (int64_t)b * a.T + f;
      const int64_t e = r * a.Dd + 6 * u;
      const bool masked = masks && masks[r];
      float x[6], xt[6], v0[6];
      float kw = 0.f;
      if (INFILL) {
        kw = a.known_w[r];
        ld6<float>(a.value_0 + e, v0);
      }
      ld6<float>(a.x_t + e, xt);
      if (!a.first) {
        if (INFILL) {
#pragma unroll
          for (int j = 0; j < 6; ++j) x[j] = tile[fl * a.Dd + 6 * u + j];
          float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int n = a.nbr[r * 2 + k];
            const float wn = a.nbw[r * 2 + k];
            if (wn == 0.f || n < 0 || n >= a.T) continue;
            float xn[6], vn[6];
            const int slot = n >= f0 && n < f0 + nf ? n - f0 : (n == halo[0] ? DS_FRAMES : (n == halo[1] ? DS_FRAMES + 1 : -1));
            if (slot >= 0) {
#pragma unroll
              for (int j = 0; j < 6; ++j) xn[j] = tile[slot * a.Dd + 6 * u + j];
            } else {
              predict6<T>(a, b, n, u, xn);
            }
            ld6<float>(a.value_0 + ((int64_t)b * a.T + n) * a.Dd + 6 * u, vn);
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[j] = fmaf(wn, vn[j] - xn[j], acc[j]);
          }
#pragma unroll
          for (int j = 0; j < 6; ++j) x[j] = fmaf(kw, v0[j], (1.f - kw) * (x[j] + acc[j]));
        } else {
          predict6<T>(a, b, f, u, x);
        }
        if (a.clip) {
#pragma unroll
          for (int j = 0; j < 6; ++j) x[j] = fminf(fmaxf(x[j], -1.f), 1.f);
        }
        if (masked) {
#pragma unroll
          for (int j = 0; j < 6; ++j) x[j] = 0.f;
        }
        st6<float>(a.img + e, x);
        if (guided && (b & 1)) continue;                         // its state is the even row's
        float z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (noise) ld6<float>(noise + e, z);
#pragma unroll
        for (int j = 0; j < 6; ++j) xt[j] = masked ? 0.f : fmaf(c0, x[j], fmaf(c1, xt[j], sg * z[j]));
        st6<float>(a.x_t + e, xt);
      }
      // the adaptor's in-betweening mix of the new state, rounded once: the next denoiser input (unmasked frames, columns < Dd only)
      for (int k = 0; k < (guided ? 2 : 1); ++k) {
        const int64_t rk = r + (int64_t)k * a.T;
        const int64_t ek = rk * a.Dd + 6 * u;
        float o[6];
        if (k == 1) {
          st6<float>(a.x_t + ek, xt);
          if (INFILL) {
            kw = a.known_w[rk];
            ld6<float>(a.value_0 + ek, v0);
          }
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) o[j] = INFILL ? fmaf(kw, v0[j], (1.f - kw) * xt[j]) : xt[j];
        if (!(masks && masks[rk])) st6<T>((T*)a.xin + rk * a.W + 6 * u, o);
      }
    }
  }

  if (tid == 0) {
    if (blockIdx.x == 0) {
      const int nx = a.first ? 0 : (s + 1 < a.n_steps ? s + 1 : a.n_steps - 1);
      a.level[b] = a.timesteps[nx];
    }
    __threadfence();
    const int total = gridDim.x * gridDim.y;
    if (atomicAdd(a.counter + 1, 1) == total - 1) {              // every workgroup has read counter[0] before its ticket
      a.counter[1] = 0;
      a.counter[0] = a.first ? 0 : s + 1;
    }
  }
}

}  // namespace
}  // namespace ofa
using namespace ofa;

extern "C" int ofa_diffusion_step_frames(void) { return DS_FRAMES; }

extern "C" int ofa_diffusion_sample_step(const ofa_diffusion_step_args* a, int dtype, void* stream) {
  OFA_REQUIRE(a != nullptr, OFA_ERR_INVALID, "diffusion_sample_step: null descriptor");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "diffusion_sample_step: bad dtype %d", dtype);
  OFA_REQUIRE(a->B >= 0 && a->T >= 0 && a->Dd >= 12 && (a->Dd - 6) % 6 == 0, OFA_ERR_INVALID,
              "diffusion_sample_step: B=%d T=%d Dd=%d (rot6d frames: Dd = 6 + 6 * joints, joints >= 1)", a->B, a->T, a->Dd);
  OFA_REQUIRE(a->W >= a->Dd, OFA_ERR_INVALID, "diffusion_sample_step: rows of W=%d columns cannot hold Dd=%d", a->W, a->Dd);
  OFA_REQUIRE(a->guidance == 0.f || a->B % 2 == 0, OFA_ERR_INVALID,
              "diffusion_sample_step: guidance pairs rows (2k: the condition, 2k + 1: the null condition), B=%d is odd", a->B);
  OFA_REQUIRE(a->n_steps >= 1, OFA_ERR_INVALID, "diffusion_sample_step: n_steps=%d", a->n_steps);
  if (a->B == 0 || a->T == 0) return OFA_OK;
  OFA_REQUIRE(a->x_t && a->xin && a->level && a->counter && a->coef && a->timesteps && (a->first || (a->pred && a->img)), OFA_ERR_INVALID,
              "diffusion_sample_step: null pointer");
  const int given = (a->value_0 != nullptr) + (a->known_w != nullptr) + (a->nbr != nullptr) + (a->nbw != nullptr);
  OFA_REQUIRE(given == 0 || given == 4, OFA_ERR_INVALID,
              "diffusion_sample_step: in-betweening takes value_0, known_w and both neighbour tables, or none of them");
  OFA_REQUIRE(a->noise == nullptr || a->noise_stride >= 0, OFA_ERR_INVALID, "diffusion_sample_step: noise_stride=%lld", (long long)a->noise_stride);
  OFA_REQUIRE(a->B <= 65535, OFA_ERR_UNSUPPORTED, "diffusion_sample_step: B=%d sentences exceed the grid", a->B);
  const bool infill = given == 4;
  const size_t lds = infill ? (size_t)(DS_FRAMES + 2) * a->Dd * sizeof(float) : 0;
  OFA_REQUIRE(lds <= (size_t)DS_LDS_MAX, OFA_ERR_UNSUPPORTED, "diffusion_sample_step: Dd=%d needs %zu bytes of LDS for the in-betweening tile (max %d)",
              a->Dd, lds, DS_LDS_MAX);
  const dim3 grid((a->T + DS_FRAMES - 1) / DS_FRAMES, a->B), block(DS_THREADS);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
    if (infill) hipLaunchKernelGGL((diffusion_step_kernel<T_, true>), grid, block, lds, st, *a);
    else hipLaunchKernelGGL((diffusion_step_kernel<T_, false>), grid, block, 0, st, *a);
  });
  return check_launch("diffusion_sample_step");
}

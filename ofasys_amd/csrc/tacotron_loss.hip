// The Tacotron2 criterion of the text-to-speech task (engine/criterion/tacotron2_loss.py:169-198 `compute_loss`), loss and gradients in
// one pass over feat_out, post, target [B, T, F] and eos_out [B, T], without float atomics and without a host sync.
// Frame (b, t) is valid iff t < lengths[b] (lengths: int64 on the device, clamped to [0, T]); N = the number of valid frames.
//   l1  = sum |feat - tgt| + sum |post - tgt|,  mse = the same sums of squares          (valid frames; mean: each / (N F))
//   eos = sum_t bce_with_logits(eos_t, y_t = [t == len - 1], pos_weight)                 (valid frames; mean: / N)
//         in the stable form (1 - y) x + w (max(-x, 0) + log1p(exp(-|x|))),  w = 1 + (pos_weight - 1) y
//   loss = l1 + mse + eos
// With `grad` the same pass writes seed * d loss / d (feat_out, post, eos_out) -- seed: a device fp32 scalar (the loss scale; NULL: 1) --
// and padded frames get exact zeros; d|d|/dd at d == 0 is 0, as torch's.  Without it nothing but the scalars is written (validation).
//   tacotron2_loss_kernel   workgroup i owns FPB consecutive frames (FPB from the shape alone).  Every workgroup sums the B lengths itself
//                           (integers: the same N everywhere), so the mean's divisors are known in the one pass.  Per thread fp32 sums of
//                           a few elements, a DPP wave sum, the four waves in wave order in fp64: partial[i] = (l1, mse, eos) fp64.
//   tacotron2_fold_kernel   ONE workgroup, a second launch (the choice the criterion kernels make where no ticket is needed: no
//                           counter to reset, no fence): thread j adds partials j, j + 256, ... in ascending order, then a fixed LDS tree;
//                           writes out = (loss, l1, mse, eos) in fp32.
// Equal inputs give equal bits: the partition, the order of every sum and N depend on the shape and the lengths alone.
// 16-byte accesses when F is a whole number of vectors and the buffers are aligned, one element per access otherwise.
// N == 0 under "mean" divides by zero like torch (NaN scalars); the gradients are then all padded frames: zeros.
#include "common.h"

namespace ofa {

constexpr int TL_THREADS = 256;
constexpr int TL_BLOCK_ELEMS = 8192;      // elements of [B*T, F] a workgroup owns, rounded down to whole frames (at least one)

static inline int64_t tl_frames_per_block(int F) { return F >= TL_BLOCK_ELEMS ? 1 : TL_BLOCK_ELEMS / F; }

__device__ __forceinline__ double tl_block_sum(float v, double* sh) {        // every thread receives the sum; waves in wave order
  const float w = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (double)w;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < TL_THREADS / WAVE; ++i) s += sh[i];
  return s;
}

template <typename T, bool VEC, bool GRAD>
__global__ __launch_bounds__(TL_THREADS) void tacotron2_loss_kernel(const T* __restrict__ feat, const T* __restrict__ post,
                                                                    const T* __restrict__ tgt, const T* __restrict__ eos,
                                                                    const int64_t* __restrict__ lengths, int B, int Tn, int F,
                                                                    int64_t fpb, float pos_weight, int mean, const float* __restrict__ seed,
                                                                    double* __restrict__ partial, T* __restrict__ dfeat,
                                                                    T* __restrict__ dpost, T* __restrict__ deos) {
  constexpr int N = VEC ? Vec<T>::N : 1;
  __shared__ long long shn[TL_THREADS];
  __shared__ double shd[TL_THREADS / WAVE];
  const int tid = threadIdx.x;
  // N = sum of the clamped lengths: every workgroup computes the same integer
  long long cnt = 0;
  for (int b = tid; b < B; b += TL_THREADS) {
    const int64_t l = lengths[b];
    cnt += l < 0 ? 0 : (l > Tn ? Tn : l);
  }
  shn[tid] = cnt;
  __syncthreads();
  for (int o = TL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) shn[tid] += shn[tid + o];
    __syncthreads();
  }
  const double nvalid = (double)shn[0];
  const float sd = GRAD ? (seed ? seed[0] : 1.0f) : 0.f;
  const float gscale = GRAD ? (mean ? (float)((double)sd / (nvalid * (double)F)) : sd) : 0.f;      // d l1 / d mse per element
  const float escale = GRAD ? (mean ? (float)((double)sd / nvalid) : sd) : 0.f;                    // d eos per frame

  const int64_t rows = (int64_t)B * Tn;
  const int64_t r0 = (int64_t)blockIdx.x * fpb;
  const int64_t r1 = r0 + fpb < rows ? r0 + fpb : rows;
  float s_l1 = 0.f, s_mse = 0.f, s_eos = 0.f;
  const int vpf = F / N;
  const int64_t nv = (r1 - r0) * vpf;
  for (int64_t v = tid; v < nv; v += TL_THREADS) {
    const int64_t r = r0 + v / vpf;
    const int c = (int)(v % vpf) * N;
    const int64_t e = r * F + c;
    const int64_t len = lengths[r / Tn];
    const bool valid = (r % Tn) < len;                     // (len <= 0: nothing; len > T: every frame)
    if (valid) {
      float a[N], p[N], t[N], ga[N], gp[N];
      if (VEC) {
        load_vec<T>(feat + e, a);
        load_vec<T>(post + e, p);
        load_vec<T>(tgt + e, t);
      } else {
        a[0] = ld1<T>(feat + e);
        p[0] = ld1<T>(post + e);
        t[0] = ld1<T>(tgt + e);
      }
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const float da = a[j] - t[j], dp = p[j] - t[j];
        s_l1 += fabsf(da) + fabsf(dp);
        s_mse += da * da + dp * dp;
        if (GRAD) {
          ga[j] = gscale * ((da > 0.f ? 1.f : (da < 0.f ? -1.f : 0.f)) + 2.f * da);
          gp[j] = gscale * ((dp > 0.f ? 1.f : (dp < 0.f ? -1.f : 0.f)) + 2.f * dp);
        }
      }
      if (GRAD) {
        if (VEC) {
          store_vec<T>(dfeat + e, ga);
          store_vec<T>(dpost + e, gp);
        } else {
          st1<T>(dfeat + e, ga[0]);
          st1<T>(dpost + e, gp[0]);
        }
      }
    } else if (GRAD) {
      float z[N];
#pragma unroll
      for (int j = 0; j < N; ++j) z[j] = 0.f;
      if (VEC) {
        store_vec<T>(dfeat + e, z);
        store_vec<T>(dpost + e, z);
      } else {
        st1<T>(dfeat + e, 0.f);
        st1<T>(dpost + e, 0.f);
      }
    }
  }
  for (int64_t r = r0 + tid; r < r1; r += TL_THREADS) {
    const int64_t len = lengths[r / Tn];
    const int64_t t = r % Tn;
    float g = 0.f;
    if (t < len) {
      const float x = ld1<T>(eos + r);
      const float y = t == len - 1 ? 1.f : 0.f;            // (a length beyond T has its last frame outside the tensor)
      const float w = 1.f + (pos_weight - 1.f) * y;
      const float en = expf(-fabsf(x));
      s_eos += (1.f - y) * x + w * (fmaxf(-x, 0.f) + log1pf(en));
      if (GRAD) {
        // (1 - y) - w sigmoid(-x) = (1 - y) sigmoid(x) - y pos_weight sigmoid(-x): no 1 - (1 - tiny) at a confident logit
        const float big = 1.f / (1.f + en), small = en * big;                    // sigmoid(|x|), sigmoid(-|x|)
        const float sig = x >= 0.f ? big : small, sig_neg = x >= 0.f ? small : big;
        g = escale * ((1.f - y) * sig - y * pos_weight * sig_neg);
      }
    }
    if (GRAD) st1<T>(deos + r, g);
  }
  const double b_l1 = tl_block_sum(s_l1, shd);
  const double b_mse = tl_block_sum(s_mse, shd);
  const double b_eos = tl_block_sum(s_eos, shd);
  if (tid == 0) {
    partial[(int64_t)blockIdx.x * 3 + 0] = b_l1;
    partial[(int64_t)blockIdx.x * 3 + 1] = b_mse;
    partial[(int64_t)blockIdx.x * 3 + 2] = b_eos;
  }
}

__global__ __launch_bounds__(TL_THREADS) void tacotron2_fold_kernel(const double* __restrict__ partial, int64_t nblocks,
                                                                    const int64_t* __restrict__ lengths, int B, int Tn, int F, int mean,
                                                                    float* __restrict__ out) {
  __shared__ double sh[3][TL_THREADS];
  __shared__ long long shn[TL_THREADS];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int64_t i = tid; i < nblocks; i += TL_THREADS) {
    a0 += partial[i * 3 + 0];
    a1 += partial[i * 3 + 1];
    a2 += partial[i * 3 + 2];
  }
  long long cnt = 0;
  for (int b = tid; b < B; b += TL_THREADS) {
    const int64_t l = lengths[b];
    cnt += l < 0 ? 0 : (l > Tn ? Tn : l);
  }
  sh[0][tid] = a0; sh[1][tid] = a1; sh[2][tid] = a2; shn[tid] = cnt;
  __syncthreads();
  for (int o = TL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sh[0][tid] += sh[0][tid + o];
      sh[1][tid] += sh[1][tid + o];
      sh[2][tid] += sh[2][tid + o];
      shn[tid] += shn[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double l1 = sh[0][0], mse = sh[1][0], eos = sh[2][0];
    if (mean) {
      const double n = (double)shn[0];
      l1 /= n * (double)F;
      mse /= n * (double)F;
      eos /= n;
    }
    out[0] = (float)(l1 + mse + eos);
    out[1] = (float)l1;
    out[2] = (float)mse;
    out[3] = (float)eos;
  }
}

}  // namespace ofa
using namespace ofa;

extern "C" int64_t ofa_tacotron2_loss_blocks(int64_t rows, int F) {
  if (rows <= 0 || F <= 0) return 0;
  const int64_t fpb = tl_frames_per_block(F);
  return (rows + fpb - 1) / fpb;
}

extern "C" int ofa_tacotron2_loss(const void* feat_out, const void* post, const void* target, const void* eos_out, const int64_t* lengths,
                                  int B, int T, int F, float bce_pos_weight, int reduction, const float* seed, double* partial,
                                  float* out, void* dfeat, void* dpost, void* deos, int grad, int dtype, int target_dtype,
                                  void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype) && OFA_DT_OK(target_dtype), OFA_ERR_INVALID, "tacotron2_loss: bad dtype %d / %d", dtype, target_dtype);
  OFA_REQUIRE(F > 0, OFA_ERR_INVALID, "tacotron2_loss: F=%d frames have no features", F);
  OFA_REQUIRE(reduction == OFA_REDUCE_MEAN || reduction == OFA_REDUCE_SUM, OFA_ERR_INVALID,
              "tacotron2_loss: unknown reduction %d (0: mean, 1: sum)", reduction);
  OFA_REQUIRE(dtype == target_dtype, OFA_ERR_UNSUPPORTED, "tacotron2_loss: the target's dtype %d differs from the outputs' %d", target_dtype,
              dtype);
  OFA_REQUIRE(B > 0 && T > 0 && feat_out && post && target && eos_out && lengths && partial && out, OFA_ERR_INVALID,
              "tacotron2_loss: bad argument");
  OFA_REQUIRE(!grad || (dfeat && dpost && deos), OFA_ERR_INVALID, "tacotron2_loss: the gradient form needs its three outputs");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * T;
  const int64_t fpb = tl_frames_per_block(F);
  const int64_t nblocks = (rows + fpb - 1) / fpb;
  OFA_REQUIRE(nblocks <= 0x7fffffff, OFA_ERR_UNSUPPORTED, "tacotron2_loss: %lld workgroups", (long long)nblocks);
  const int mean = reduction == OFA_REDUCE_MEAN;
  const bool vec = F % dt_vecn(dtype) == 0 && aligned16(feat_out) && aligned16(post) && aligned16(target) &&
                   (!grad || (aligned16(dfeat) && aligned16(dpost)));
  dim3 grid((unsigned)nblocks), block(TL_THREADS);
  dispatch_dtype(dtype, [&](auto tag) {
    using T_ = typename decltype(tag)::type;
#define OFA_TL_LAUNCH(V, G)                                                                                                              \
  hipLaunchKernelGGL((tacotron2_loss_kernel<T_, V, G>), grid, block, 0, st, (const T_*)feat_out, (const T_*)post, (const T_*)target,     \
                     (const T_*)eos_out, lengths, B, T, F, fpb, bce_pos_weight, mean, seed, partial, (T_*)dfeat, (T_*)dpost, (T_*)deos)
    if (vec) {
      if (grad) OFA_TL_LAUNCH(true, true);
      else OFA_TL_LAUNCH(true, false);
    } else {
      if (grad) OFA_TL_LAUNCH(false, true);
      else OFA_TL_LAUNCH(false, false);
    }
#undef OFA_TL_LAUNCH
  });
  const int rc = check_launch("tacotron2_loss");
  if (rc != OFA_OK) return rc;
  hipLaunchKernelGGL(tacotron2_fold_kernel, dim3(1), block, 0, st, (const double*)partial, nblocks, lengths, B, T, F, mean, out);
  return check_launch("tacotron2_loss_fold");
}

// The policy of one autoregressive speech-generation step (generator/speech_generator.py:143-166) in ONE launch for gfx950 (wave64):
// the fbank head on the decoder's new position (feat_proj, eos_proj), sigmoid, the finish rule on device state, the next position's
// key-padding flag, the finished-row count, and the prenet (adaptor/audio.py:721-732) + projection on the new frame -- the next step's
// input embedding.  See include/ofasys_amd.h (ofa_speech_step) for the contract.
//
// Shape of the work: B rows (tens) against ~0.7 MB of weights (D = 768: 768x80 + 80x256 + 256x256 + 256x768 elements).  A workgroup
// owns SS_ROWS rows from the head through to the embedding and streams every weight row ONCE for all of them, straight from global
// memory into registers (each weight element is used by one lane only: an LDS round trip would add nothing); the rows' activations live
// in LDS as fp32 between the layers.  No workgroup waits for another; the only cross-workgroup word is the finished count, an integer
// atomic add (order-independent, so the state is reproducible).
//
// Rounding follows the unfused composition (ops.linear / ops.relu / ops.dropout_add): fp32 accumulation, + bias in fp32, ONE rounding
// to the model dtype per Linear output, ReLU on the rounded value, the dropout's scaled value rounded again.  What differs is the
// summation order inside a dot product: a lane sums every G-th 8-element chunk, the G lanes are folded by DPP.
#include "common.h"

namespace ofa {
namespace {

constexpr int SS_ROWS = 4;          // rows per workgroup
constexpr int SS_THREADS = 512;     // 8 waves (256 VGPRs each: a lane keeps up to 8 weight vectors in flight without spilling)
constexpr int SS_COLS = 4;          // output columns a lane group works on at a time
constexpr int SS_MAXL = 4;          // prenet layers
constexpr int SS_LDS_MAX = 65536;

static_assert(sizeof(ofa_speech_step_args) == 264, "ofa_speech_step_args: kernels._SpeechStepArgs mirrors this layout");

template <typename T> __device__ __forceinline__ float ss_round(float v);
template <> __device__ __forceinline__ float ss_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float ss_round<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <> __device__ __forceinline__ float ss_round<f16_t>(float v) { return (float)(f16_t)v; }

// 8 consecutive elements (16-byte aligned start; fp32: two vectors) as floats
template <typename T> __device__ __forceinline__ void ss_load8(const T* p, float* out) { load_vec<T>(p, out); }
template <> __device__ __forceinline__ void ss_load8<float>(const float* p, float* out) {
  load_vec<float>(p, out);
  load_vec<float>(p + 4, out + 4);
}
template <typename T> __device__ __forceinline__ void ss_store8(T* p, const float* in) { store_vec<T>(p, in); }
template <> __device__ __forceinline__ void ss_store8<float>(float* p, const float* in) {
  store_vec<float>(p, in);
  store_vec<float>(p + 4, in + 4);
}

template <int G> __device__ __forceinline__ float ss_group_sum(float v);
template <> __device__ __forceinline__ float ss_group_sum<16>(float v) { return row16_sum(v); }
template <> __device__ __forceinline__ float ss_group_sum<64>(float v) { return wave_sum(v); }

// 8 consecutive weights as raw 16-byte vectors (unpacked at their use: a lane keeps SS_COLS x KS of them in flight)
template <typename T> struct Raw8 {
  static constexpr int NV = 8 * sizeof(T) / 16;              // 1 (16-bit) or 2 (fp32)
  uint4 v[NV];
  __device__ __forceinline__ void load(const T* p) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = reinterpret_cast<const uint4*>(p)[i];
  }
  __device__ __forceinline__ void floats(float* out) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) unpack16<T>(v[i], out + i * (8 / NV));
  }
};

// out[r][n] = round(act(sum_k in[r][k] * W[n][k] + bias[n])) for r < SS_ROWS, n < N.  in / out: LDS, fp32, row strides ldi / ldo.
// G lanes share an output column (G = 16: four columns per wave at a time; G = 64: one) and a group works on SS_COLS columns at a
// time.  KS > 0: K <= KS * G * 8 and all SS_COLS * KS weight vectors of a lane are requested before the first is used (a chunk past K
// reads chunk 0 and multiplies zeros); KS == 0: any K, SS_COLS vectors per trip.
template <typename T, int G, int KS>
__device__ __forceinline__ void ss_linear_g(const float* __restrict__ in, int ldi, const T* __restrict__ W, const T* __restrict__ bias,
                                            int N, int K, float* __restrict__ out, int ldo, bool relu) {
  constexpr int NG = SS_THREADS / G;                         // column groups of the workgroup
  constexpr int C = SS_COLS;
  const int g = threadIdx.x / G, li = threadIdx.x % G;
  for (int n0 = 0; n0 < N; n0 += C * NG) {                  // (uniform trip count: every lane takes part in the folds)
    float acc[C][SS_ROWS];
    const T* w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int n = n0 + c * NG + g;
      w[c] = W + (int64_t)(n < N ? n : N - 1) * K;           // (a column past the end reads the last row and is not stored)
#pragma unroll
      for (int r = 0; r < SS_ROWS; ++r) acc[c][r] = 0.f;
    }
    auto fma8 = [&](const Raw8<T> (&raw)[C], int k, bool valid) {
      float wv[C][8];
#pragma unroll
      for (int c = 0; c < C; ++c) raw[c].floats(wv[c]);
#pragma unroll
      for (int r = 0; r < SS_ROWS; ++r) {
        const float4 x0 = *reinterpret_cast<const float4*>(in + r * ldi + k);
        const float4 x1 = *reinterpret_cast<const float4*>(in + r * ldi + k + 4);
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = valid ? xv[j] : 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c][r] = fmaf(x, wv[c][j], acc[c][r]);
        }
      }
    };
    if constexpr (KS > 0) {
      Raw8<T> raw[KS][C];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = li * 8 + s * G * 8;
#pragma unroll
        for (int c = 0; c < C; ++c) raw[s][c].load(w[c] + (k < K ? k : 0));
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = li * 8 + s * G * 8;
        fma8(raw[s], k < K ? k : 0, k < K);
      }
    } else {
      for (int k = li * 8; k < K; k += G * 8) {
        Raw8<T> raw[C];
#pragma unroll
        for (int c = 0; c < C; ++c) raw[c].load(w[c] + k);
        fma8(raw, k, true);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int n = n0 + c * NG + g;
#pragma unroll
      for (int r = 0; r < SS_ROWS; ++r) acc[c][r] = ss_group_sum<G>(acc[c][r]);
      if (li == 0 && n < N) {
        const float bv = ld1<T>(bias + n);
#pragma unroll
        for (int r = 0; r < SS_ROWS; ++r) {
          float v = ss_round<T>(acc[c][r] + bv);
          if (relu) v = fmaxf(v, 0.f);
          out[r * ldo + n] = v;
        }
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ void ss_linear(const float* in, int ldi, const T* W, const T* bias, int N, int K, float* out, int ldo,
                                          bool relu) {
  if (K <= 128) ss_linear_g<T, 16, 1>(in, ldi, W, bias, N, K, out, ldo, relu);        // short rows: 16 lanes cover them
  else if (K <= 256) ss_linear_g<T, 16, 2>(in, ldi, W, bias, N, K, out, ldo, relu);
  else if (K <= 1024) ss_linear_g<T, 64, 2>(in, ldi, W, bias, N, K, out, ldo, relu);
  else ss_linear_g<T, 64, 0>(in, ldi, W, bias, N, K, out, ldo, relu);
}

template <typename T>
__global__ __launch_bounds__(SS_THREADS) void speech_step_kernel(const ofa_speech_step_args a) {
  extern __shared__ __attribute__((aligned(16))) char ss_smem[];
  const int D = a.D, F = a.out_dim, P = a.P, E = a.E;
  int ld = D > F ? D : F;
  ld = ld > P ? ld : P;
  ld = ld > E ? ld : E;
  float* buf0 = reinterpret_cast<float*>(ss_smem);           // [SS_ROWS][ld]
  float* buf1 = buf0 + SS_ROWS * ld;                         // [SS_ROWS][ld]
  float* eosz = buf1 + SS_ROWS * ld;                         // [SS_ROWS]
  const int row0 = blockIdx.x * SS_ROWS;
  const int nr = a.B - row0 < SS_ROWS ? a.B - row0 : SS_ROWS;
  const int tid = threadIdx.x;

  // the rows' decoder outputs -> LDS (fp32); rows past the batch are zeros and are never stored
  for (int v = tid; v < SS_ROWS * (D / 8); v += SS_THREADS) {
    const int r = v / (D / 8), c = (v % (D / 8)) * 8;
    float x[8];
    if (r < nr) ss_load8<T>((const T*)a.x + (int64_t)(row0 + r) * a.ldx + c, x);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) buf0[r * ld + c + j] = x[j];
  }
  __syncthreads();

  // the head: feat (rounded to the model dtype, as the stored tensor is) and the eos logit
  ss_linear<T>(buf0, ld, (const T*)a.feat_w, (const T*)a.feat_b, F, D, buf1, ld, false);
  ss_linear<T>(buf0, ld, (const T*)a.eos_w, (const T*)a.eos_b, 1, D, eosz, 1, false);
  __syncthreads();

  for (int v = tid; v < nr * (F / 8); v += SS_THREADS) {
    const int r = v / (F / 8), c = (v % (F / 8)) * 8;
    ss_store8<T>((T*)a.feats + ((int64_t)(row0 + r) * a.T_cap + a.step) * F + c, buf1 + r * ld + c);
  }
  if (tid < WAVE) {                                          // the state of the rows: one lane per row, ordinary vector stores
    bool newly = false;
    if (tid < nr) {
      const int b = row0 + tid;
      const float p = 1.0f / (1.0f + expf(-eosz[tid]));
      a.eos_prob[(int64_t)b * a.T_cap + a.step] = p;
      const int was = a.finished[b];
      const bool cross = p > a.threshold[0];                    // strict
      newly = !was && cross;
      if (newly) a.out_lens[b] = a.step + 1;
      const int fin = (was || cross) ? 1 : 0;
      a.finished[b] = fin;
      a.pad_next[b] = (uint8_t)fin;                          // position step + 1 of a row that has finished is a padded key
    }
    const unsigned long long m = __ballot(newly);
    if (tid == 0 && m != 0ull) atomicAdd(a.nfin, (int)__popcll(m));
  }

  // the prenet on the new frame
  float* cur = buf1;
  float* nxt = buf0;
  int K = F;
  const float keep_scale = 1.0f / (1.0f - a.p_drop);
  const uint32_t thresh = philox_thresh(a.p_drop);
  for (int l = 0; l < a.layers; ++l) {
    ss_linear<T>(cur, ld, (const T*)a.pre_w[l], (const T*)a.pre_b[l], P, K, nxt, ld, true);
    __syncthreads();
    if (a.p_drop > 0.f) {                                    // ofa_dropout_add_fwd's mask of a [B, P] tensor
      const Philox rng(a.seed);
      const uint64_t off = a.offset + (uint64_t)l * a.offset_stride + (a.offset_base ? (uint64_t)a.offset_base[0] : 0ull);
      for (int v = tid; v < nr * (P / 8); v += SS_THREADS) {
        const int r = v / (P / 8), c8 = v % (P / 8);
        const uint4 rnd = rng(off + (uint64_t)(row0 + r) * (uint64_t)(P / 8) + (uint64_t)c8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float* e = nxt + r * ld + c8 * 8 + j;
          *e = philox_keep(rnd, j, thresh) ? ss_round<T>(*e * keep_scale) : 0.f;
        }
      }
      __syncthreads();
    }
    float* t = cur; cur = nxt; nxt = t;
    K = P;
  }
  ss_linear<T>(cur, ld, (const T*)a.proj_w, (const T*)a.proj_b, E, K, nxt, ld, false);
  __syncthreads();
  for (int v = tid; v < nr * (E / 8); v += SS_THREADS) {
    const int r = v / (E / 8), c = (v % (E / 8)) * 8;
    ss_store8<T>((T*)a.embed + (int64_t)(row0 + r) * E + c, nxt + r * ld + c);
  }
}

size_t ss_lds_bytes(int D, int F, int P, int E) {
  int ld = D > F ? D : F;
  ld = ld > P ? ld : P;
  ld = ld > E ? ld : E;
  return ((size_t)2 * SS_ROWS * ld + SS_ROWS) * sizeof(float);
}

bool ss_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace ofa

using namespace ofa;

extern "C" int ofa_speech_step_rows(void) { return SS_ROWS; }

extern "C" int ofa_speech_step_route(int D, int out_dim, int P, int E, int layers, int dtype) {
  if (!OFA_DT_OK(dtype)) return -1;
  if (D <= 0 || out_dim <= 0 || P <= 0 || E <= 0 || layers < 1 || layers > SS_MAXL) return 0;
  if ((D | out_dim | P | E) & 7) return 0;
  return ss_lds_bytes(D, out_dim, P, E) <= (size_t)SS_LDS_MAX ? 1 : 0;
}

extern "C" int ofa_speech_step(const ofa_speech_step_args* a, int dtype, void* stream) {
  OFA_REQUIRE(a, OFA_ERR_INVALID, "ofa_speech_step: null descriptor");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ofa_speech_step: bad dtype %d", dtype);
  OFA_REQUIRE(a->B > 0 && a->step >= 0 && a->step < a->T_cap, OFA_ERR_INVALID, "ofa_speech_step: B=%d step=%d T_cap=%d", a->B, a->step,
              a->T_cap);
  OFA_REQUIRE(ofa_speech_step_route(a->D, a->out_dim, a->P, a->E, a->layers, dtype) == 1, OFA_ERR_UNSUPPORTED,
              "ofa_speech_step: D=%d out_dim=%d prenet_dim=%d embed_dim=%d prenet_layers=%d is not served (multiples of 8, 1..%d layers, "
              "%d rows of the widest in LDS)", a->D, a->out_dim, a->P, a->E, a->layers, SS_MAXL, SS_ROWS);
  OFA_REQUIRE(a->p_drop >= 0.f && a->p_drop < 1.f, OFA_ERR_INVALID, "ofa_speech_step: p_drop=%g", (double)a->p_drop);
  OFA_REQUIRE(a->ldx >= a->D && (a->ldx & 7) == 0, OFA_ERR_INVALID, "ofa_speech_step: ldx=%lld must be a multiple of 8 covering D=%d",
              (long long)a->ldx, a->D);
  bool ok = a->x && a->feat_w && a->feat_b && a->eos_w && a->eos_b && a->proj_w && a->proj_b && a->feats && a->eos_prob && a->finished &&
            a->out_lens && a->nfin && a->pad_next && a->embed && a->threshold;
  for (int l = 0; l < a->layers; ++l) ok = ok && a->pre_w[l] && a->pre_b[l];
  OFA_REQUIRE(ok, OFA_ERR_INVALID, "ofa_speech_step: null pointer");
  bool al = ss_aligned16(a->x) && ss_aligned16(a->feat_w) && ss_aligned16(a->eos_w) && ss_aligned16(a->proj_w) && ss_aligned16(a->feats) &&
            ss_aligned16(a->embed);
  for (int l = 0; l < a->layers; ++l) al = al && ss_aligned16(a->pre_w[l]);
  OFA_REQUIRE(al, OFA_ERR_INVALID, "ofa_speech_step: x, the weights, feats and embed must be 16-byte aligned");
  const size_t smem = ss_lds_bytes(a->D, a->out_dim, a->P, a->E);
  const dim3 grid((a->B + SS_ROWS - 1) / SS_ROWS), block(SS_THREADS);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(speech_step_kernel<typename decltype(tag)::type>, grid, block, smem, st, *a);
  });
  return check_launch("ofa_speech_step");
}

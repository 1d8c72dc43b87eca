// The VQGAN image decoder's kernels (taming's Decoder: GroupNorm(32) -> swish -> 3 x 3 convolution res blocks, nearest x2 upsampling) on
// NHWC rows [B, H, W, C] in fp16 / bf16, fp32 accumulation.
//   vq_gn_partial_kernel / vq_gn_final_kernel
//                     GroupNorm statistics per (sample, group) without E[x^2] - mean^2: a workgroup holds a chunk of VQ_GN_ITER * npl
//                     pixels in registers, sums it, centres it on the chunk's own group means and sums the squares -- (mean, M2) per
//                     (chunk, group) to a workspace.  The finalise kernel combines the chunks pairwise (Chan et al.) in a fixed order --
//                     eight strided chains per group, then those eight in order -- and writes scale[b, c] = gamma rstd and
//                     shift[b, c] = beta - mean rstd gamma.  No atomics: equal inputs give equal bits.
//   vq_conv3x3_kernel one launch of a 3 x 3 / stride 1 / padding 1 convolution as a tap-loop implicit GEMM on the 32x32x16 MFMA.  A
//                     workgroup (4 waves) owns a 16 x 16 tile of output pixels of one sample and 32 NF NT output channels.  It loops over
//                     Cin in slices of KS channels; per slice it stages the 18 x 18 halo image (with the x2 upsample: the 10 x 10 SOURCE
//                     pixels under it) ONCE into LDS -- swish(x scale + shift) applied on the way in, pixels outside the image zeros
//                     AFTER that -- and runs the nine taps as pixel offsets into that image.  Nothing unfolded or upsampled exists in HBM.
//                     An MFMA column fragment is 2 rows x 16 columns of output pixels: lanes 0..15 read 16 neighbouring LDS pixels whose
//                     rows are KS + 8 elements apart (16 bytes of padding: an odd number of 16-byte bank groups, so they never meet).
//                     With the upsample, output pixel (y, x) under tap (dy, dx) reads source pixel ((y + dy + 1) >> 1, (x + dx + 1) >> 1)
//                     of the staged image: the shift is folded into the fragment's row addresses, per tap.
//                     A wave owns NF = 2 fragments of output channels and MT fragments of pixels: every LDS fragment feeds NF MFMAs and
//                     every weight fragment MT.  Weights are [tap][Cout][Cin]: lane (i, hi) reads the 8 input channels kc + 8 hi .. + 7
//                     of channel n0 + i with one 16-byte load from L2 straight into the A fragment, a group of K-steps ahead; the first
//                     group of a slice is requested before the slice is staged.  Epilogue as voc_conv_kernel's: a lane holds 4 consecutive
//                     channels of a pixel per register quad -- bias, optional residual, one rounding, 8-byte stores.
//                     Tiling starts at each sample's (0, 0) and no sum crosses a workgroup: a sample's bits do not depend on its batch.
//   vq_conv_out_kernel the last layer: norm + swish (kept in fp32) -> 3 x 3 convolution to <= 4 channels -> fp32 NCHW.  VALU; 16 x 16
//                     outputs per workgroup from an fp32 LDS image of 18 x 18 pixels x 32 channels (pitch 33 floats), sliced over C.
//   vq_norm_rows_kernel x scale + shift into 16-bit rows (AttnBlock's q / k / v read the normalised map without the swish).
#include <type_traits>

#include "common.h"

namespace ofa {

typedef __attribute__((ext_vector_type(8))) short vq_bf16x8;
typedef __attribute__((ext_vector_type(16))) float vq_f32x16;

constexpr int VQ_TILE = 16;                    // output pixels per workgroup: VQ_TILE x VQ_TILE, as 8 fragments of 2 rows x 16 columns
constexpr int VQ_FRAGS = 8;
constexpr int VQ_LDS_TARGET = 80 * 1024;       // two workgroups per CU
constexpr int VQ_GROUPS = 32;
constexpr int VQ_GN_ITER = 8;                  // pixels a thread of the statistics kernel holds
constexpr int VQ_GN_CHAINS = 8;                // strided chains per group in the finalise kernel
constexpr int VQ_OUT_MAX = 4, VQ_OUT_KS = 32;
constexpr float VQ_EPS = 1e-6f;

template <bool F16> __device__ __forceinline__ vq_f32x16 vq_mfma(const uint4& a, const uint4& b, const vq_f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vq_bf16x8, a), __builtin_bit_cast(vq_bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float vq_swish(float v) { return v / (1.0f + __expf(-v)); }

// ---------------------------------------------------------------- GroupNorm statistics
// Chan et al.: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb), counts as floats (at most 2^20 * 16: exact)
__device__ __forceinline__ void vq_chan(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  const float n = na + nb, d = mb - ma;
  ma += d * (nb / n);
  qa += qb + d * d * (na * nb / n);
  na = n;
}

// pixels per chunk of the statistics kernel at C channels: npl pixel lanes (256 / (C / 8), whole) times VQ_GN_ITER
static __host__ __device__ inline int vq_gn_chunk(int C) { return (256 / (C / 8)) * VQ_GN_ITER; }

template <typename T>
__global__ __launch_bounds__(256) void vq_gn_partial_kernel(const T* __restrict__ x, float* __restrict__ ws, int HW, int C, int nchunk) {
  __shared__ float part[256 * 8];              // [pixel lane][channel]
  __shared__ float gmean[VQ_GROUPS];
  const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
  const int vpr = C / 8, npl = 256 / vpr, cpg = C / VQ_GROUPS;
  const int cv = tid % vpr, pl = tid / vpr;
  const bool live = pl < npl;
  const int p0 = chunk * npl * VQ_GN_ITER;
  const int rows = min(npl * VQ_GN_ITER, HW - p0);                 // pixels of this chunk that exist
  const T* xb = x + ((int64_t)b * HW + p0) * C + cv * 8;
  float v[VQ_GN_ITER][8], s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
#pragma unroll
  for (int i = 0; i < VQ_GN_ITER; ++i) {
    const int p = pl + i * npl;
    const bool ok = live && p < rows;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
    if (ok) load_vec<T>(xb + (int64_t)p * C, v[i]);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += v[i][e];
  }
  if (live)
#pragma unroll
    for (int e = 0; e < 8; ++e) part[pl * C + cv * 8 + e] = s[e];
  __syncthreads();
  const float cnt = (float)rows * (float)cpg;
  if (tid < VQ_GROUPS) {                                            // fixed order: pixel lanes outer, the group's channels inner
    float t = 0.f;
    for (int l = 0; l < npl; ++l)
      for (int c = 0; c < cpg; ++c) t += part[l * C + tid * cpg + c];
    gmean[tid] = t / cnt;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = gmean[(cv * 8 + e) / cpg];
#pragma unroll
  for (int i = 0; i < VQ_GN_ITER; ++i) {
    const bool ok = live && pl + i * npl < rows;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = ok ? v[i][e] - m[e] : 0.f;
      s[e] = fmaf(d, d, s[e]);
    }
  }
  if (live)
#pragma unroll
    for (int e = 0; e < 8; ++e) part[pl * C + cv * 8 + e] = s[e];
  __syncthreads();
  if (tid < VQ_GROUPS) {
    float t = 0.f;
    for (int l = 0; l < npl; ++l)
      for (int c = 0; c < cpg; ++c) t += part[l * C + tid * cpg + c];
    float* o = ws + (((int64_t)b * nchunk + chunk) * VQ_GROUPS + tid) * 2;
    o[0] = gmean[tid];
    o[1] = t;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vq_gn_final_kernel(const float* __restrict__ ws, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                          float* __restrict__ scale, float* __restrict__ shift, int HW, int C, int nchunk) {
  __shared__ float cn[256], cm[256], cq[256];
  __shared__ float mean[VQ_GROUPS], rstd[VQ_GROUPS];
  const int tid = threadIdx.x, b = blockIdx.x, g = tid / VQ_GN_CHAINS, s = tid % VQ_GN_CHAINS;
  const int cpg = C / VQ_GROUPS, per = vq_gn_chunk(C);
  float n = 0.f, m = 0.f, q = 0.f;
  for (int ch = s; ch < nchunk; ch += VQ_GN_CHAINS) {
    const float* p = ws + (((int64_t)b * nchunk + ch) * VQ_GROUPS + g) * 2;
    vq_chan(n, m, q, (float)min(per, HW - ch * per) * (float)cpg, p[0], p[1]);
  }
  cn[tid] = n; cm[tid] = m; cq[tid] = q;
  __syncthreads();
  if (s == 0) {
    for (int i = 1; i < VQ_GN_CHAINS; ++i) vq_chan(n, m, q, cn[tid + i], cm[tid + i], cq[tid + i]);
    mean[g] = m;
    rstd[g] = 1.0f / sqrtf(q / n + VQ_EPS);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const float ga = ld1<T>(gamma + c), r = rstd[c / cpg], sc = ga * r;
    scale[(int64_t)b * C + c] = sc;
    shift[(int64_t)b * C + c] = ld1<T>(beta + c) - mean[c / cpg] * sc;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vq_norm_rows_kernel(const T* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                           T* __restrict__ y, int64_t per_sample, int C, int64_t total) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= total) return;
  const int64_t b = i / per_sample;
  const int c = (int)(i % C);
  float v[8], sc[8], sh[8];
  load_vec<T>(x + i, v);
  load_vec<float>(scale + b * C + c, sc); load_vec<float>(scale + b * C + c + 4, sc + 4);
  load_vec<float>(shift + b * C + c, sh); load_vec<float>(shift + b * C + c + 4, sh + 4);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
  *reinterpret_cast<uint4*>(y + i) = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
}

// ---------------------------------------------------------------- the 3 x 3 convolution
struct VqConvArgs {
  const void *x, *w, *bias, *res;
  const float *scale, *shift;                  // [B, Cin] or NULL: no prologue
  void* y;
  int B, H, W, Cin, Cout, KS;                  // H, W: the OUTPUT's (with the upsample: twice the source's)
};

template <bool F16, bool UP, int NF, int NT>
__global__ __launch_bounds__(256, 2) void vq_conv3x3_kernel(VqConvArgs a) {
  typedef typename std::conditional<F16, f16_t, bf16_t>::type T;
  constexpr int MG = 4 / NT, MT = VQ_FRAGS / MG, G = 2;
  constexpr int PW = UP ? VQ_TILE / 2 + 2 : VQ_TILE + 2;           // staged pixels per side
  extern __shared__ __attribute__((aligned(16))) unsigned char vq_smem[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(vq_smem);           // [PW * PW][KS + 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, KS = a.KS, LD = KS + 8;
  const int tiles_w = (W + VQ_TILE - 1) / VQ_TILE;
  const int b = blockIdx.z, h0 = (blockIdx.x / tiles_w) * VQ_TILE, w0 = (blockIdx.x % tiles_w) * VQ_TILE;
  const int Hs = UP ? H >> 1 : H, Ws = UP ? W >> 1 : W;            // the stored map's size
  const int sh0 = (UP ? h0 >> 1 : h0) - 1, sw0 = (UP ? w0 >> 1 : w0) - 1;   // its pixel under staged pixel (0, 0)
  const uint16_t* xb = reinterpret_cast<const uint16_t*>(a.x) + (int64_t)b * Hs * Ws * Cin;

  const int ng = wave % NT, mg = wave / NT;
  const int n0 = blockIdx.y * (32 * NF * NT) + ng * (32 * NF);
  const int li = lane & 31, hi = lane >> 5;
  const int oy = li >> 4, ox = li & 15;                             // this lane's pixel inside a 2 x 16 fragment
  bool f_ok[NF];
  const uint16_t* wp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f_ok[f] = n0 + 32 * f < Cout;                                   // Cout is a multiple of 32: a fragment exists whole or not at all
    wp[f] = reinterpret_cast<const uint16_t*>(a.w) + (int64_t)(f_ok[f] ? n0 + 32 * f + li : 0) * Cin + hi * 8;
  }
  const int64_t tap_stride = (int64_t)Cout * Cin;

  vq_f32x16 acc[NF][MT];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[f][mt][i] = 0.f;

  for (int c0 = 0; c0 < Cin; c0 += KS) {
    const int kc = min(KS, Cin - c0), nk = kc / 16, total = 9 * nk;
    // K-steps it = tap * nk + kk of this slice, in groups of G; the first group is requested before the slice is staged
    uint4 cur[G][NF], nxt[G][NF];
    auto load_group = [&](int it0, uint4 (*dst)[NF]) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int it = it0 + g, tap = it / nk, kk = it - tap * nk;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          dst[g][f] = make_uint4(0, 0, 0, 0);
          if (it < total && f_ok[f]) dst[g][f] = *reinterpret_cast<const uint4*>(wp[f] + tap * tap_stride + c0 + kk * 16);
        }
      }
    };
    load_group(0, cur);

    if (c0) __syncthreads();                                        // the previous slice's image has been read by every wave
    {
      const int vpr = kc / 8;
      const float* scb = a.scale ? a.scale + (int64_t)b * Cin + c0 : nullptr;
      const float* shb = a.scale ? a.shift + (int64_t)b * Cin + c0 : nullptr;
      for (int v = tid; v < PW * PW * vpr; v += 256) {
        const int p = v / vpr, c = (v - p * vpr) * 8, py = p / PW, px = p - py * PW;
        const int sy = sh0 + py, sx = sw0 + px;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) {
          val = *reinterpret_cast<const uint4*>(xb + ((int64_t)sy * Ws + sx) * Cin + c0 + c);
          if (scb) {
            float f[8], sc[8], sh[8];
            unpack16<T>(val, f);
            load_vec<float>(scb + c, sc); load_vec<float>(scb + c + 4, sc + 4);
            load_vec<float>(shb + c, sh); load_vec<float>(shb + c + 4, sh + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = vq_swish(fmaf(f[e], sc[e], sh[e]));
            val = make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
          }
        }
        *reinterpret_cast<uint4*>(tile + p * LD + c) = val;
      }
    }
    __syncthreads();

    int tap_now = -1;
    const uint16_t* src[MT];
    for (int it0 = 0; it0 < total; it0 += G) {
      load_group(it0 + G, nxt);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int it = it0 + g;
        if (it < total) {
          const int tap = it / nk, kk = it - tap * nk;
          if (tap != tap_now) {                                     // (wave-uniform) this tap's pixel of every fragment of the lane
            tap_now = tap;
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const int y = (mg * MT + mt) * 2 + oy + dy, x = ox + dx;          // in the 18 x 18 halo frame of the output tile
              const int pix = UP ? ((y + 1) >> 1) * PW + ((x + 1) >> 1) : y * PW + x;
              src[mt] = tile + pix * LD + hi * 8;
            }
          }
          uint4 bf[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) bf[mt] = *reinterpret_cast<const uint4*>(src[mt] + kk * 16);
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[f][mt] = vq_mfma<F16>(cur[g][f], bf[mt], acc[f][mt]);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int f = 0; f < NF; ++f) cur[g][f] = nxt[g][f];
    }
  }

  // ---- epilogue: register quad q of a lane = channels n + 8 q + 4 hi .. + 3 of the lane's pixel in fragment mt
  const uint16_t* bias = reinterpret_cast<const uint16_t*>(a.bias);
  const uint16_t* resb = a.res ? reinterpret_cast<const uint16_t*>(a.res) + (int64_t)b * H * W * Cout : nullptr;
  uint16_t* yb = reinterpret_cast<uint16_t*>(a.y) + (int64_t)b * H * W * Cout;
  auto dec = [](uint16_t u) -> float {
    if constexpr (F16) return (float)__builtin_bit_cast(f16_t, u);
    else return bf2f(u);
  };
  auto add4 = [&](float* v, const uint16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] += dec((uint16_t)(u.x & 0xffffu)); v[1] += dec((uint16_t)(u.x >> 16));
    v[2] += dec((uint16_t)(u.y & 0xffffu)); v[3] += dec((uint16_t)(u.y >> 16));
  };
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int h = h0 + (mg * MT + mt) * 2 + oy, w = w0 + ox;
    if (h >= H || w >= W) continue;
    const int64_t row = ((int64_t)h * W + w) * Cout;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (!f_ok[f]) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = n0 + 32 * f + 8 * q + 4 * hi;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[f][mt][4 * q + e];
        add4(v, bias + c);
        if (resb) add4(v, resb + row + c);
        *reinterpret_cast<uint2*>(yb + row + c) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
      }
    }
  }
}

// ---------------------------------------------------------------- conv_out
template <typename T>
__global__ __launch_bounds__(256) void vq_conv_out_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ bias,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          float* __restrict__ out, int H, int W, int C, int OC) {
  constexpr int PW = VQ_TILE + 2, LD = VQ_OUT_KS + 1;
  __shared__ float img[PW * PW * LD];
  __shared__ float wf[9 * VQ_OUT_KS * VQ_OUT_MAX];                   // [tap][c][oc]
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tiles_w = (W + VQ_TILE - 1) / VQ_TILE;
  const int h0 = (blockIdx.x / tiles_w) * VQ_TILE, w0 = (blockIdx.x % tiles_w) * VQ_TILE;
  const int oy = tid >> 4, ox = tid & 15;
  const T* xb = x + (int64_t)b * H * W * C;
  float acc[VQ_OUT_MAX];
#pragma unroll
  for (int o = 0; o < VQ_OUT_MAX; ++o) acc[o] = o < OC ? ld1<T>(bias + o) : 0.f;
  for (int c0 = 0; c0 < C; c0 += VQ_OUT_KS) {
    if (c0) __syncthreads();
    for (int v = tid; v < PW * PW * (VQ_OUT_KS / 8); v += 256) {
      const int p = v / (VQ_OUT_KS / 8), c = (v - p * (VQ_OUT_KS / 8)) * 8, py = p / PW, px = p - py * PW;
      const int sy = h0 - 1 + py, sx = w0 - 1 + px;
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = 0.f;
      if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
        float sc[8], sh[8];
        load_vec<T>(xb + ((int64_t)sy * W + sx) * C + c0 + c, f);
        load_vec<float>(scale + (int64_t)b * C + c0 + c, sc); load_vec<float>(scale + (int64_t)b * C + c0 + c + 4, sc + 4);
        load_vec<float>(shift + (int64_t)b * C + c0 + c, sh); load_vec<float>(shift + (int64_t)b * C + c0 + c + 4, sh + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = vq_swish(fmaf(f[e], sc[e], sh[e]));
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) img[p * LD + c + e] = f[e];
    }
    // w is [tap][OC][C]
    for (int i = tid; i < 9 * VQ_OUT_KS * VQ_OUT_MAX; i += 256) {
      const int o = i % VQ_OUT_MAX, c = (i / VQ_OUT_MAX) % VQ_OUT_KS, tap = i / (VQ_OUT_MAX * VQ_OUT_KS);
      wf[i] = o < OC ? ld1<T>(w + ((int64_t)tap * OC + o) * C + c0 + c) : 0.f;
    }
    __syncthreads();
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - dy * 3;
      const float* row = img + ((oy + dy) * PW + ox + dx) * LD;
      const float* wt = wf + tap * VQ_OUT_KS * VQ_OUT_MAX;
      for (int c = 0; c < VQ_OUT_KS; ++c) {
        const float xv = row[c];
#pragma unroll
        for (int o = 0; o < VQ_OUT_MAX; ++o) acc[o] = fmaf(wt[c * VQ_OUT_MAX + o], xv, acc[o]);
      }
    }
  }
  const int h = h0 + oy, wc = w0 + ox;
  if (h >= H || wc >= W) return;
#pragma unroll
  for (int o = 0; o < VQ_OUT_MAX; ++o)
    if (o < OC) out[(((int64_t)b * OC + o) * H + h) * W + wc] = acc[o];
}

// ---------------------------------------------------------------- host side
struct VqPlan { int nf, nt, ks, lds; };
// The tiling of a (Cin, Cout) convolution: NF channel fragments per wave, NT waves side by side over the channels, and the Cin slice --
// the fewest slices whose halo image stays under VQ_LDS_TARGET, evened out to multiples of 32 channels.
static VqPlan vq_plan(int Cin, int Cout, int up) {
  VqPlan p;
  p.nf = Cout >= 64 ? 2 : 1;
  p.nt = Cout >= 128 ? 2 : 1;
  const int pw = up ? VQ_TILE / 2 + 2 : VQ_TILE + 2;
  const int ks_max = (VQ_LDS_TARGET / (2 * (VQ_TILE + 2) * (VQ_TILE + 2)) - 8) / 32 * 32;      // 96: the same slices with and without the upsample
  const int ns = cdiv(Cin, ks_max);
  p.ks = cdiv(cdiv(Cin, ns), 32) * 32;
  p.lds = pw * pw * (p.ks + 8) * 2;
  return p;
}

static int vq_rows_check(const char* who, int dtype, int B, int H, int W, int C) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(dtype != OFA_F32, OFA_ERR_UNSUPPORTED, "%s: fp16 or bf16 only (the kernels read 16-bit NHWC rows)", who);
  OFA_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 20) && (int64_t)B * H * W <= (1 << 30), OFA_ERR_INVALID,
              "%s: bad B=%d H=%d W=%d (a map of at most 2^20 pixels, a batch of at most 2^30)", who, B, H, W);
  OFA_REQUIRE(C >= 32 && C <= 512 && C % 32 == 0, OFA_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of 32 in 32..512", who, C);
  return OFA_OK;
}

template <bool F16, bool UP> static void vq_conv_launch(const VqPlan& p, const VqConvArgs& a, hipStream_t st) {
  const dim3 grid(cdiv(a.H, VQ_TILE) * cdiv(a.W, VQ_TILE), cdiv(a.Cout, 32 * p.nf * p.nt), a.B), block(256);
  auto go = [&](auto kern) {
    if (p.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
    hipLaunchKernelGGL(kern, grid, block, p.lds, st, a);
  };
  if (p.nt == 2) go(vq_conv3x3_kernel<F16, UP, 2, 2>);
  else if (p.nf == 2) go(vq_conv3x3_kernel<F16, UP, 2, 1>);
  else go(vq_conv3x3_kernel<F16, UP, 1, 1>);
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_vqgan_conv_plan(int Cin, int Cout, int upsample, int* out4) {
  if (Cin < 32 || Cin > 512 || Cin % 32 || Cout < 32 || Cout > 512 || Cout % 32 || !out4) return OFA_ERR_UNSUPPORTED;
  const VqPlan p = vq_plan(Cin, Cout, upsample);
  out4[0] = VQ_TILE; out4[1] = p.ks; out4[2] = 32 * p.nf * p.nt; out4[3] = p.lds;
  return OFA_OK;
}

extern "C" int ofa_vqgan_gn_chunks(int HW, int C) {
  if (HW < 1 || C < 32 || C > 512 || C % 32) return 0;
  return cdiv(HW, vq_gn_chunk(C));
}

extern "C" int ofa_vqgan_groupnorm_stats(const void* x, const void* gamma, const void* beta, float* scale, float* shift, float* ws,
                                         int64_t ws_bytes, int B, int H, int W, int C, int dtype, void* stream) {
  const int rc = vq_rows_check("vqgan_groupnorm_stats", dtype, B, H, W, C);
  if (rc != OFA_OK) return rc;
  const int HW = H * W, nchunk = cdiv(HW, vq_gn_chunk(C));
  OFA_REQUIRE(ws_bytes >= (int64_t)B * nchunk * VQ_GROUPS * 2 * 4, OFA_ERR_INVALID, "vqgan_groupnorm_stats: the workspace needs %lld bytes (%d chunks)",
              (long long)B * nchunk * VQ_GROUPS * 2 * 4, nchunk);
  OFA_REQUIRE(B == 0 || (x && gamma && beta && scale && shift && ws), OFA_ERR_INVALID, "vqgan_groupnorm_stats: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(x) && aligned16(scale) && aligned16(shift)), OFA_ERR_UNSUPPORTED, "vqgan_groupnorm_stats: operands must be 16-byte aligned");
  if (B == 0) return OFA_OK;
  dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((vq_gn_partial_kernel<T>), dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, (const T*)x, ws, HW, C, nchunk);
    hipLaunchKernelGGL((vq_gn_final_kernel<T>), dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)ws, (const T*)gamma, (const T*)beta, scale,
                       shift, HW, C, nchunk);
  });
  return check_launch("vqgan_groupnorm_stats");
}

extern "C" int ofa_vqgan_norm_rows(const void* x, const float* scale, const float* shift, void* y, int B, int H, int W, int C, int dtype,
                                   void* stream) {
  const int rc = vq_rows_check("vqgan_norm_rows", dtype, B, H, W, C);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(B == 0 || (x && scale && shift && y), OFA_ERR_INVALID, "vqgan_norm_rows: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(x) && aligned16(y) && aligned16(scale) && aligned16(shift)), OFA_ERR_UNSUPPORTED,
              "vqgan_norm_rows: operands must be 16-byte aligned");
  if (B == 0) return OFA_OK;
  const int64_t per = (int64_t)H * W * C, total = per * B;
  dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((vq_norm_rows_kernel<T>), dim3(cdiv(total / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, scale, shift, (T*)y, per, C,
                       total);
  });
  return check_launch("vqgan_norm_rows");
}

extern "C" int ofa_vqgan_conv3x3(const void* x, const void* w, const void* bias, const void* res, const float* scale, const float* shift, void* y,
                                 int B, int H, int W, int Cin, int Cout, int upsample, int dtype, void* stream) {
  int rc = vq_rows_check("vqgan_conv3x3", dtype, B, H, W, Cin);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(Cout >= 32 && Cout <= 512 && Cout % 32 == 0, OFA_ERR_UNSUPPORTED, "vqgan_conv3x3: Cout=%d must be a multiple of 32 in 32..512", Cout);
  OFA_REQUIRE(!upsample || (H % 2 == 0 && W % 2 == 0), OFA_ERR_INVALID, "vqgan_conv3x3: with the x2 upsample H=%d and W=%d are the output's, twice the source's", H, W);
  OFA_REQUIRE((scale == nullptr) == (shift == nullptr), OFA_ERR_INVALID, "vqgan_conv3x3: scale and shift come together");
  OFA_REQUIRE(B == 0 || (x && w && bias && y), OFA_ERR_INVALID, "vqgan_conv3x3: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias) && aligned16(res) && aligned16(scale) && aligned16(shift)),
              OFA_ERR_UNSUPPORTED, "vqgan_conv3x3: operands must be 16-byte aligned");
  OFA_REQUIRE(B == 0 || (y != x && y != res), OFA_ERR_INVALID, "vqgan_conv3x3: y must not alias x or res (other workgroups read their halo)");
  if (B == 0) return OFA_OK;
  const VqPlan p = vq_plan(Cin, Cout, upsample);
  const VqConvArgs a = {x, w, bias, res, scale, shift, y, B, H, W, Cin, Cout, p.ks};
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype16(dtype, [&](auto tag) {
    constexpr bool F16 = std::is_same<typename decltype(tag)::type, f16_t>::value;
    if (upsample) vq_conv_launch<F16, true>(p, a, st);
    else vq_conv_launch<F16, false>(p, a, st);
  });
  return check_launch("vqgan_conv3x3");
}

extern "C" int ofa_vqgan_conv_out(const void* x, const void* w, const void* bias, const float* scale, const float* shift, float* out, int B, int H,
                                  int W, int C, int out_ch, int dtype, void* stream) {
  const int rc = vq_rows_check("vqgan_conv_out", dtype, B, H, W, C);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(out_ch >= 1 && out_ch <= VQ_OUT_MAX, OFA_ERR_UNSUPPORTED, "vqgan_conv_out: out_ch=%d must be 1..%d", out_ch, VQ_OUT_MAX);
  OFA_REQUIRE(B == 0 || (x && w && bias && scale && shift && out), OFA_ERR_INVALID, "vqgan_conv_out: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(x) && aligned16(scale) && aligned16(shift)), OFA_ERR_UNSUPPORTED, "vqgan_conv_out: operands must be 16-byte aligned");
  if (B == 0) return OFA_OK;
  const dim3 grid(cdiv(H, VQ_TILE) * cdiv(W, VQ_TILE), B), block(256);
  dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((vq_conv_out_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, (const T*)w, (const T*)bias, scale, shift, out, H, W, C,
                       out_ch);
  });
  return check_launch("vqgan_conv_out");
}

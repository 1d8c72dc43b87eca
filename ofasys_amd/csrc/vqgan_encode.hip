// The VQGAN image encoder's kernels that the decoder (vqgan.hip) does not have: taming's Encoder conv_in and Downsample, and the Gumbel
// quantizer's projection + arg-max.  fp16 / bf16 operands, fp32 accumulation on the 32x32x16 MFMA, NHWC rows, no atomics, no sum across
// workgroups; tiling starts at each sample's (0, 0): a sample's bits do not depend on its batch (but see the quantizer's noise counter).
//   vq_downsample_kernel  pad (0, 1, 0, 1) + 3 x 3 / stride 2 / no padding: output (y, x) under tap (dy, dx) reads source pixel
//                     (2 y + dy, 2 x + dx), zeros at source row H and column W; there is no row or column -1.  The tap loop, the weight
//                     prefetch ([tap][Cout][Cin] from L2, a group of K-steps ahead) and the epilogue are vq_conv3x3_kernel's.  A workgroup
//                     owns VQD_TH x VQD_TW = 8 x 16 output pixels (four fragments of 2 rows x 16 columns) and stages the 17 x 33 source
//                     pixels under them per Cin slice.  At stride 2 the sixteen lanes of a fragment column would read pixels TWO apart:
//                     2 (KS + 8) elements = an EVEN number of 16-byte bank groups, so lanes i and i + 8 would meet.  The image is therefore
//                     staged de-interleaved by (row parity, column parity) into four planes -- 9 x 17, 9 x 16, 8 x 17, 8 x 16 pixels, 561 in
//                     all -- and tap (dy, dx) reads plane (dy & 1, dx & 1) at offset (dy >> 1, dx >> 1): inside a plane the lanes read
//                     NEIGHBOURING pixels at the odd pitch KS + 8, as the stride-1 kernel does.
//   vq_conv_in_kernel  Conv2d(3, Cout, 3, padding 1) on the fp32 NCHW image as ONE implicit GEMM of K = 27 padded to 32 (two K-steps),
//                     k = 3 tap + c.  The workgroup stages the 18 x 18 x 3 halo of its 16 x 16 tile in LDS as [pixel][3], rounded once to
//                     the 16-bit type, zeros outside the image; a lane gathers the 8 elements of its B fragment from it (the element of k
//                     sits 3 (18 dy + dx) + c past the lane's pixel; k >= 27 is zero).  A wave owns two pixel fragments, builds their four
//                     B fragments once and loops over the Cout / 32 channel fragments of the host-arranged [Cout][32] weight.
//   vq_quantize_kernel  ind[r] = argmax_n (W[n] . h[r] + bias[n] + g[r, n]) without the logits.  grid (row tiles, code splits).  The four
//                     waves stage the tile's R = 32 MT rows of h ONCE in LDS at pitch K + 8 and then each sweeps its share of the split's
//                     codes, two 32-code fragments at a time: the weight rows are the A operand (16-byte loads from L2, a group of K-steps
//                     ahead), the staged rows the B operand -- every LDS fragment feeds two MFMAs.  In the 32 x 32 accumulator lane
//                     (i, hi) holds ROW i of the tile against codes 8 q + 4 hi + e: the running (best, index) per row is a compare in the
//                     lane's own registers.  After the sweep the two lane halves are exchanged (v_permlane32_swap), the four waves merge
//                     through LDS and the workgroup writes one (value, index) pair per row and split; vq_quantize_fold_kernel folds the
//                     splits in index order.  One rule everywhere: start at (-inf, none); a candidate replaces the best iff
//                     v > best || (v == best && n < best_n) -- the lowest index wins a tie and a NaN never wins.
//                     Noise (seed >= 0): g = -log(-log(u)), u = ((word >> 8) + 0.5) 2^-24, word n % 4 of Philox(counter r n_embed / 4 +
//                     n / 4, key seed): one generator call serves the four codes of a register quad.  For u >= 1/2 log(u) is
//                     log1p(-(2^24 - (word >> 8) - 0.5) 2^-24), whose argument is exact in fp32 (u itself would round to 1 there).
#include <type_traits>

#include "common.h"

namespace ofa {

typedef __attribute__((ext_vector_type(8))) short vqe_bf16x8;
typedef __attribute__((ext_vector_type(16))) float vqe_f32x16;

constexpr int VQE_LDS_TARGET = 80 * 1024;      // two workgroups per CU, as vqgan.hip
constexpr int VQD_TH = 8, VQD_TW = 16;         // the downsample's output tile: four fragments of 2 rows x 16 columns
constexpr int VQD_FRAGS = VQD_TH / 2;
constexpr int VQD_SH = 2 * VQD_TH + 1, VQD_SW = 2 * VQD_TW + 1;    // staged source pixels
constexpr int VQD_PIX = VQD_SH * VQD_SW;
constexpr int VQI_TILE = 16, VQI_PW = VQI_TILE + 2;                // conv_in: output tile and its halo
constexpr int VQQ_CUS = 256;                   // the code split fills this many CUs (MI355X)
constexpr int VQQ_NF = 2;                      // code fragments per wave and pass
constexpr int VQQ_NONE = 0x7fffffff;           // "no candidate yet": loses every tie

template <bool F16> __device__ __forceinline__ vqe_f32x16 vqe_mfma(const uint4& a, const uint4& b, const vqe_f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(vqe_bf16x8, a), __builtin_bit_cast(vqe_bf16x8, b), c, 0, 0, 0);
}
template <bool F16> __device__ __forceinline__ float vqe_dec(uint16_t u) {
  if constexpr (F16) return (float)__builtin_bit_cast(f16_t, u);
  else return bf2f(u);
}
// acc quad q of a lane = channels c .. c + 3 of one pixel: bias, one rounding, an 8-byte store
template <bool F16> __device__ __forceinline__ void vqe_store4(uint16_t* y, const uint16_t* bias, const vqe_f32x16& acc, int q) {
  typedef typename std::conditional<F16, f16_t, bf16_t>::type T;
  const uint2 u = *reinterpret_cast<const uint2*>(bias);
  const float v0 = acc[4 * q] + vqe_dec<F16>((uint16_t)(u.x & 0xffffu)), v1 = acc[4 * q + 1] + vqe_dec<F16>((uint16_t)(u.x >> 16));
  const float v2 = acc[4 * q + 2] + vqe_dec<F16>((uint16_t)(u.y & 0xffffu)), v3 = acc[4 * q + 3] + vqe_dec<F16>((uint16_t)(u.y >> 16));
  *reinterpret_cast<uint2*>(y) = make_uint2(pack2<T>(v0, v1), pack2<T>(v2, v3));
}

// ---------------------------------------------------------------- Downsample
// pixel index of (r, c) of parity plane (py, px) in the staged image: planes in (0,0), (0,1), (1,0), (1,1) order
__device__ __forceinline__ int vqd_pix(int py, int px, int r, int c) {
  const int base = py ? (VQD_TH + 1) * VQD_SW + (px ? VQD_TH * (VQD_TW + 1) : 0) : (px ? (VQD_TH + 1) * (VQD_TW + 1) : 0);
  return base + r * (px ? VQD_TW : VQD_TW + 1) + c;
}

struct VqDownArgs {
  const void *x, *w, *bias;
  void* y;
  int B, H, W, Cin, Cout, KS;                  // H, W: the SOURCE map's; the output is H / 2 x W / 2
};

template <bool F16, int NF, int NT>
__global__ __launch_bounds__(256, 2) void vq_downsample_kernel(VqDownArgs a) {
  constexpr int MG = 4 / NT, MT = VQD_FRAGS / MG, G = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char vqe_smem[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(vqe_smem);          // [VQD_PIX][KS + 8], four parity planes
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, Ho = H >> 1, Wo = W >> 1, Cin = a.Cin, Cout = a.Cout, KS = a.KS, LD = KS + 8;
  const int tiles_w = (Wo + VQD_TW - 1) / VQD_TW;
  const int b = blockIdx.z, h0 = (blockIdx.x / tiles_w) * VQD_TH, w0 = (blockIdx.x % tiles_w) * VQD_TW;
  const uint16_t* xb = reinterpret_cast<const uint16_t*>(a.x) + (int64_t)b * H * W * Cin;

  const int ng = wave % NT, mg = wave / NT;
  const int n0 = blockIdx.y * (32 * NF * NT) + ng * (32 * NF);
  const int li = lane & 31, hi = lane >> 5;
  const int oy = li >> 4, ox = li & 15;
  bool f_ok[NF];
  const uint16_t* wp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f_ok[f] = n0 + 32 * f < Cout;
    wp[f] = reinterpret_cast<const uint16_t*>(a.w) + (int64_t)(f_ok[f] ? n0 + 32 * f + li : 0) * Cin + hi * 8;
  }
  const int64_t tap_stride = (int64_t)Cout * Cin;

  vqe_f32x16 acc[NF][MT];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[f][mt][i] = 0.f;

  for (int c0 = 0; c0 < Cin; c0 += KS) {
    const int kc = min(KS, Cin - c0), nk = kc / 16, total = 9 * nk;
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

    if (c0) __syncthreads();
    {
      const int vpr = kc / 8;
      for (int v = tid; v < VQD_PIX * vpr; v += 256) {
        const int p = v / vpr, c = (v - p * vpr) * 8, sy = p / VQD_SW, sx = p - sy * VQD_SW;
        const int gy = 2 * h0 + sy, gx = 2 * w0 + sx;                // never negative: the padding is on the bottom and right only
        uint4 val = make_uint4(0, 0, 0, 0);
        if (gy < H && gx < W) val = *reinterpret_cast<const uint4*>(xb + ((int64_t)gy * W + gx) * Cin + c0 + c);
        *reinterpret_cast<uint4*>(tile + vqd_pix(sy & 1, sx & 1, sy >> 1, sx >> 1) * LD + c) = val;
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
          if (tap != tap_now) {
            tap_now = tap;
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              src[mt] = tile + vqd_pix(dy & 1, dx & 1, (mg * MT + mt) * 2 + oy + (dy >> 1), ox + (dx >> 1)) * LD + hi * 8;
          }
          uint4 bf[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) bf[mt] = *reinterpret_cast<const uint4*>(src[mt] + kk * 16);
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[f][mt] = vqe_mfma<F16>(cur[g][f], bf[mt], acc[f][mt]);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int f = 0; f < NF; ++f) cur[g][f] = nxt[g][f];
    }
  }

  const uint16_t* bias = reinterpret_cast<const uint16_t*>(a.bias);
  uint16_t* yb = reinterpret_cast<uint16_t*>(a.y) + (int64_t)b * Ho * Wo * Cout;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int h = h0 + (mg * MT + mt) * 2 + oy, w = w0 + ox;
    if (h >= Ho || w >= Wo) continue;
    const int64_t row = ((int64_t)h * Wo + w) * Cout;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (!f_ok[f]) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = n0 + 32 * f + 8 * q + 4 * hi;
        vqe_store4<F16>(yb + row + c, bias + c, acc[f][mt], q);
      }
    }
  }
}

// ---------------------------------------------------------------- conv_in
template <bool F16>
__global__ __launch_bounds__(256) void vq_conv_in_kernel(const float* __restrict__ image, const uint16_t* __restrict__ w32,
                                                         const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int H, int W, int Cout) {
  typedef typename std::conditional<F16, f16_t, bf16_t>::type T;
  constexpr int NPIX = VQI_PW * VQI_PW;
  __shared__ uint16_t img[NPIX * 3 + 2];                            // [pixel][3]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_w = (W + VQI_TILE - 1) / VQI_TILE;
  const int b = blockIdx.y, h0 = (blockIdx.x / tiles_w) * VQI_TILE, w0 = (blockIdx.x % tiles_w) * VQI_TILE;
  const float* xb = image + (int64_t)b * 3 * H * W;
  for (int i = tid; i < NPIX * 3; i += 256) {                       // channel-major: neighbouring threads read neighbouring columns
    const int c = i / NPIX, p = i - c * NPIX, py = p / VQI_PW, px = p - py * VQI_PW;
    const int gy = h0 - 1 + py, gx = w0 - 1 + px;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[((int64_t)c * H + gy) * W + gx];
    img[p * 3 + c] = (uint16_t)(pack2<T>(v, 0.f) & 0xffffu);
  }
  __syncthreads();

  const int li = lane & 31, hi = lane >> 5, oy = li >> 4, ox = li & 15;
  // the lane's 8 + 8 elements of K: k = 16 s + 8 hi + e sits off[s][e] halfwords past the lane's pixel (k >= 27: none)
  uint4 bf[2][2];                                                    // [pixel fragment][K-step]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const uint16_t* base = img + (((wave * 2 + mt) * 2 + oy) * VQI_PW + ox) * 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      uint32_t e8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 16 * s + 8 * hi + e, tap = k / 3, c = k - tap * 3, dy = tap / 3, dx = tap - dy * 3;
        e8[e] = k < 27 ? base[(dy * VQI_PW + dx) * 3 + c] : 0u;
      }
      bf[mt][s] = make_uint4(e8[0] | e8[1] << 16, e8[2] | e8[3] << 16, e8[4] | e8[5] << 16, e8[6] | e8[7] << 16);
    }
  }
  uint16_t* yb = y + (int64_t)b * H * W * Cout;
  for (int n0 = 0; n0 < Cout; n0 += 32) {
    const uint4 a0 = *reinterpret_cast<const uint4*>(w32 + (n0 + li) * 32 + hi * 8);
    const uint4 a1 = *reinterpret_cast<const uint4*>(w32 + (n0 + li) * 32 + 16 + hi * 8);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      vqe_f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      acc = vqe_mfma<F16>(a0, bf[mt][0], acc);
      acc = vqe_mfma<F16>(a1, bf[mt][1], acc);
      const int h = h0 + (wave * 2 + mt) * 2 + oy, w = w0 + ox;
      if (h >= H || w >= W) continue;
      const int64_t row = ((int64_t)h * W + w) * Cout;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = n0 + 8 * q + 4 * hi;
        vqe_store4<F16>(yb + row + c, bias + c, acc, q);
      }
    }
  }
}

// ---------------------------------------------------------------- projection + arg-max
__device__ __forceinline__ void vqq_take(float& best, int& best_n, float v, int n) {
  if (v > best || (v == best && n < best_n)) { best = v; best_n = n; }
}

// Gumbel noise of one 32-bit word (see the head of the file)
__device__ __forceinline__ float vqq_gumbel(uint32_t word) {
  const uint32_t x = word >> 8;
  const float t = x < (1u << 23) ? -logf(((float)x + 0.5f) * 0x1p-24f) : -log1pf(-((float)((1u << 24) - x) - 0.5f) * 0x1p-24f);
  return -logf(t);
}

struct VqQuantArgs {
  const void *h, *w, *bias;
  int* out;
  float* ws_v;                                 // [splits][N]
  int* ws_n;
  int64_t N;
  int K, n_embed, splits, frags_per_split;
  int64_t seed;                                // < 0: no noise
};

template <bool F16, int MT, bool NOISY>
__global__ __launch_bounds__(256, 2) void vq_quantize_kernel(VqQuantArgs a) {
  constexpr int R = 32 * MT, NF = VQQ_NF, G = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char vqe_smem[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(vqe_smem);          // [R][K + 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, LD = K + 8, nk = K / 16, li = lane & 31, hi = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const uint16_t* hb = reinterpret_cast<const uint16_t*>(a.h);
  {
    const int vpr = K / 8;
    for (int v = tid; v < R * vpr; v += 256) {
      const int r = v / vpr, c = (v - r * vpr) * 8;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (r0 + r < a.N) val = *reinterpret_cast<const uint4*>(hb + (r0 + r) * K + c);
      *reinterpret_cast<uint4*>(tile + r * LD + c) = val;
    }
  }
  __syncthreads();

  const int nfr = a.n_embed / 32, f_begin = blockIdx.y * a.frags_per_split, f_end = min(nfr, f_begin + a.frags_per_split);
  const uint16_t* wb = reinterpret_cast<const uint16_t*>(a.w);
  const uint16_t* bias = reinterpret_cast<const uint16_t*>(a.bias);
  const Philox rng((uint64_t)a.seed);
  const int quads = a.n_embed / 4;
  float best[MT];
  int best_n[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) { best[mt] = -INFINITY; best_n[mt] = VQQ_NONE; }

  for (int f0 = f_begin + wave * NF; f0 < f_end; f0 += 4 * NF) {      // (wave-uniform)
    bool f_ok[NF];
    const uint16_t* wp[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      f_ok[f] = f0 + f < f_end;
      wp[f] = wb + (int64_t)(f_ok[f] ? (f0 + f) * 32 + li : 0) * K + hi * 8;
    }
    vqe_f32x16 acc[NF][MT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[f][mt][i] = 0.f;
    uint4 cur[G][NF], nxt[G][NF];
    auto load_group = [&](int it0, uint4 (*dst)[NF]) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          dst[g][f] = make_uint4(0, 0, 0, 0);
          if (it0 + g < nk && f_ok[f]) dst[g][f] = *reinterpret_cast<const uint4*>(wp[f] + (it0 + g) * 16);
        }
    };
    load_group(0, cur);
    for (int it0 = 0; it0 < nk; it0 += G) {                          // K is a multiple of 32: nk is a multiple of G
      load_group(it0 + G, nxt);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        uint4 bf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bf[mt] = *reinterpret_cast<const uint4*>(tile + (mt * 32 + li) * LD + (it0 + g) * 16 + hi * 8);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[f][mt] = vqe_mfma<F16>(cur[g][f], bf[mt], acc[f][mt]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int f = 0; f < NF; ++f) cur[g][f] = nxt[g][f];
    }
    // register quad q of fragment f = codes n .. n + 3, n = 32 (f0 + f) + 8 q + 4 hi, against row r0 + 32 mt + li
    auto finish = [&](auto fc) {                                      // (a compile-time f: acc stays in registers)
      constexpr int f = decltype(fc)::value;
      if (!f_ok[f]) return;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = (f0 + f) * 32 + 8 * q + 4 * hi;
        const uint2 u = *reinterpret_cast<const uint2*>(bias + n);
        const float bv[4] = {vqe_dec<F16>((uint16_t)(u.x & 0xffffu)), vqe_dec<F16>((uint16_t)(u.x >> 16)), vqe_dec<F16>((uint16_t)(u.y & 0xffffu)),
                             vqe_dec<F16>((uint16_t)(u.y >> 16))};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[f][mt][4 * q + e] + bv[e];
          if constexpr (NOISY) {
            const uint4 rw = rng((uint64_t)(r0 + mt * 32 + li) * (uint64_t)quads + (uint64_t)(n >> 2));
            v[0] += vqq_gumbel(rw.x); v[1] += vqq_gumbel(rw.y); v[2] += vqq_gumbel(rw.z); v[3] += vqq_gumbel(rw.w);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) vqq_take(best[mt], best_n[mt], v[e], n + e);
        }
      }
    };
    static_assert(NF == 2, "two code fragments per pass");
    finish(std::integral_constant<int, 0>{});
    finish(std::integral_constant<int, 1>{});
  }

  // the two lane halves hold the same row against different codes: exchange and take
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const auto sv = __builtin_amdgcn_permlane32_swap(__float_as_uint(best[mt]), __float_as_uint(best[mt]), false, false);
    const auto sn = __builtin_amdgcn_permlane32_swap((uint32_t)best_n[mt], (uint32_t)best_n[mt], false, false);
    vqq_take(best[mt], best_n[mt], __uint_as_float(hi ? sv[0] : sv[1]), (int)(hi ? sn[0] : sn[1]));
  }
  __syncthreads();                                                   // every wave has finished reading the tile
  float* mv = reinterpret_cast<float*>(vqe_smem);                    // [4][R]
  int* mn = reinterpret_cast<int*>(vqe_smem) + 4 * R;
  if (hi == 0)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { mv[wave * R + mt * 32 + li] = best[mt]; mn[wave * R + mt * 32 + li] = best_n[mt]; }
  __syncthreads();
  if (tid < R && r0 + tid < a.N) {
    float bv = mv[tid];
    int bn = mn[tid];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) vqq_take(bv, bn, mv[wv * R + tid], mn[wv * R + tid]);
    if (a.splits == 1) a.out[r0 + tid] = bn == VQQ_NONE ? 0 : bn;
    else { a.ws_v[(int64_t)blockIdx.y * a.N + r0 + tid] = bv; a.ws_n[(int64_t)blockIdx.y * a.N + r0 + tid] = bn; }
  }
}

__global__ __launch_bounds__(256) void vq_quantize_fold_kernel(const float* __restrict__ ws_v, const int* __restrict__ ws_n, int* __restrict__ out,
                                                               int64_t N, int splits) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  float bv = -INFINITY;
  int bn = VQQ_NONE;
  for (int s = 0; s < splits; ++s) vqq_take(bv, bn, ws_v[s * N + r], ws_n[s * N + r]);
  out[r] = bn == VQQ_NONE ? 0 : bn;
}

// ---------------------------------------------------------------- host side
struct VqDownPlan { int nf, nt, ks, lds; };
// NF / NT as vq_plan's; the Cin slice: the fewest slices whose four planes stay under VQE_LDS_TARGET (64 channels at most), evened out
static VqDownPlan vq_down_plan(int C) {
  VqDownPlan p;
  p.nf = C >= 64 ? 2 : 1;
  p.nt = C >= 128 ? 2 : 1;
  const int ks_max = (VQE_LDS_TARGET / (2 * VQD_PIX) - 8) / 32 * 32;
  p.ks = cdiv(cdiv(C, cdiv(C, ks_max)), 32) * 32;
  p.lds = VQD_PIX * (p.ks + 8) * 2;
  return p;
}

struct VqQuantPlan { int rows, splits, fps, lds; int64_t ws; };
// The row tile: 128 rows while they fit under VQE_LDS_TARGET at pitch K + 8, else 64.  The split: until row tiles x splits fills the chip,
// but a split keeps at least one pass of every wave (4 waves x VQQ_NF fragments = 256 codes).
static VqQuantPlan vq_quant_plan(int64_t N, int K, int n_embed) {
  VqQuantPlan p;
  p.rows = 128 * (K + 8) * 2 <= VQE_LDS_TARGET ? 128 : 64;
  p.lds = p.rows * (K + 8) * 2;
  const int nfr = n_embed / 32, tiles = cdiv(N, p.rows);
  int splits = tiles > 0 ? cdiv(VQQ_CUS, tiles) : 1;
  splits = max(1, min(splits, nfr / (4 * VQQ_NF)));
  p.fps = cdiv(nfr, splits);
  p.splits = cdiv(nfr, p.fps);                                       // no empty split
  p.ws = p.splits > 1 ? (int64_t)p.splits * N * 8 : 0;
  return p;
}

static int vqe_rows_check(const char* who, int dtype, int B, int H, int W) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(dtype != OFA_F32, OFA_ERR_UNSUPPORTED, "%s: fp16 or bf16 only (the kernels write 16-bit NHWC rows)", who);
  OFA_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 20) && (int64_t)B * H * W <= (1 << 30), OFA_ERR_INVALID,
              "%s: bad B=%d H=%d W=%d (a map of at most 2^20 pixels, a batch of at most 2^30)", who, B, H, W);
  return OFA_OK;
}
static bool vqe_chan_ok(int C) { return C >= 32 && C <= 512 && C % 32 == 0; }

template <typename K> static void vqe_launch(K kern, dim3 grid, int lds, hipStream_t st, const VqDownArgs& a) {
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_vqgan_downsample_plan(int C, int* out5) {
  if (!vqe_chan_ok(C) || !out5) return OFA_ERR_UNSUPPORTED;
  const VqDownPlan p = vq_down_plan(C);
  out5[0] = VQD_TH; out5[1] = VQD_TW; out5[2] = p.ks; out5[3] = 32 * p.nf * p.nt; out5[4] = p.lds;
  return OFA_OK;
}

extern "C" int ofa_vqgan_downsample(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin, int Cout, int dtype,
                                    void* stream) {
  const int rc = vqe_rows_check("vqgan_downsample", dtype, B, H, W);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(vqe_chan_ok(Cin) && Cin == Cout, OFA_ERR_UNSUPPORTED, "vqgan_downsample: Cin=%d = Cout=%d must be a multiple of 32 in 32..512", Cin, Cout);
  OFA_REQUIRE(H >= 2 && W >= 2, OFA_ERR_INVALID, "vqgan_downsample: the source map H=%d W=%d must be at least 2 x 2 (the output is H/2 x W/2)", H, W);
  OFA_REQUIRE(B == 0 || (x && w && bias && y), OFA_ERR_INVALID, "vqgan_downsample: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias)), OFA_ERR_UNSUPPORTED,
              "vqgan_downsample: operands must be 16-byte aligned");
  OFA_REQUIRE(B == 0 || y != x, OFA_ERR_INVALID, "vqgan_downsample: y must not alias x");
  if (B == 0) return OFA_OK;
  const VqDownPlan p = vq_down_plan(Cin);
  const VqDownArgs a = {x, w, bias, y, B, H, W, Cin, Cout, p.ks};
  const dim3 grid(cdiv(H / 2, VQD_TH) * cdiv(W / 2, VQD_TW), cdiv(Cout, 32 * p.nf * p.nt), B);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype16(dtype, [&](auto tag) {
    constexpr bool F16 = std::is_same<typename decltype(tag)::type, f16_t>::value;
    if (p.nt == 2) vqe_launch(vq_downsample_kernel<F16, 2, 2>, grid, p.lds, st, a);
    else if (p.nf == 2) vqe_launch(vq_downsample_kernel<F16, 2, 1>, grid, p.lds, st, a);
    else vqe_launch(vq_downsample_kernel<F16, 1, 1>, grid, p.lds, st, a);
  });
  return check_launch("vqgan_downsample");
}

extern "C" int ofa_vqgan_conv_in(const float* image, const void* w32, const void* bias, void* y, int B, int in_channels, int H, int W, int Cout,
                                 int dtype, void* stream) {
  const int rc = vqe_rows_check("vqgan_conv_in", dtype, B, H, W);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(in_channels == 3, OFA_ERR_UNSUPPORTED, "vqgan_conv_in: in_channels=%d must be 3 (K = 27 padded to 32)", in_channels);
  OFA_REQUIRE(vqe_chan_ok(Cout), OFA_ERR_UNSUPPORTED, "vqgan_conv_in: Cout=%d must be a multiple of 32 in 32..512", Cout);
  OFA_REQUIRE(B == 0 || (image && w32 && bias && y), OFA_ERR_INVALID, "vqgan_conv_in: null operand");
  OFA_REQUIRE(B == 0 || (aligned16(w32) && aligned16(y) && aligned16(bias)), OFA_ERR_UNSUPPORTED, "vqgan_conv_in: w32, bias and y must be 16-byte aligned");
  if (B == 0) return OFA_OK;
  const dim3 grid(cdiv(H, VQI_TILE) * cdiv(W, VQI_TILE), B);
  dispatch_dtype16(dtype, [&](auto tag) {
    constexpr bool F16 = std::is_same<typename decltype(tag)::type, f16_t>::value;
    hipLaunchKernelGGL((vq_conv_in_kernel<F16>), grid, dim3(256), 0, (hipStream_t)stream, image, (const uint16_t*)w32, (const uint16_t*)bias, (uint16_t*)y,
                       H, W, Cout);
  });
  return check_launch("vqgan_conv_in");
}

static int vqq_shape_check(const char* who, int64_t N, int K, int n_embed) {
  OFA_REQUIRE(N >= 0 && N <= (1ll << 30), OFA_ERR_INVALID, "%s: bad N=%lld (at most 2^30 rows)", who, (long long)N);
  OFA_REQUIRE(vqe_chan_ok(K), OFA_ERR_UNSUPPORTED, "%s: K=%d must be a multiple of 32 in 32..512", who, K);
  OFA_REQUIRE(n_embed >= 32 && n_embed <= (1 << 24) && n_embed % 32 == 0, OFA_ERR_UNSUPPORTED, "%s: n_embed=%d must be a multiple of 32 (at most 2^24)", who,
              n_embed);
  return OFA_OK;
}

extern "C" int ofa_vqgan_quantize_plan(int64_t N, int K, int n_embed, int64_t* out4) {
  const int rc = vqq_shape_check("vqgan_quantize_plan", N, K, n_embed);
  if (rc != OFA_OK) return rc;
  OFA_REQUIRE(out4, OFA_ERR_INVALID, "vqgan_quantize_plan: null out4");
  const VqQuantPlan p = vq_quant_plan(N, K, n_embed);
  out4[0] = p.rows; out4[1] = p.splits; out4[2] = p.ws; out4[3] = p.lds;
  return OFA_OK;
}

extern "C" int ofa_vqgan_quantize(const void* h, const void* w, const void* bias, int* out, void* ws, int64_t ws_bytes, int64_t N, int K, int n_embed,
                                  int64_t seed, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "vqgan_quantize: bad dtype %d", dtype);
  OFA_REQUIRE(dtype != OFA_F32, OFA_ERR_UNSUPPORTED, "vqgan_quantize: fp16 or bf16 only");
  const int rc = vqq_shape_check("vqgan_quantize", N, K, n_embed);
  if (rc != OFA_OK) return rc;
  const VqQuantPlan p = vq_quant_plan(N, K, n_embed);
  OFA_REQUIRE(ws_bytes >= p.ws, OFA_ERR_INVALID, "vqgan_quantize: the workspace needs %lld bytes (%d code splits)", (long long)p.ws, p.splits);
  OFA_REQUIRE(N == 0 || (h && w && bias && out && (ws || !p.ws)), OFA_ERR_INVALID, "vqgan_quantize: null operand");
  OFA_REQUIRE(N == 0 || (aligned16(h) && aligned16(w) && aligned16(bias) && aligned16(ws)), OFA_ERR_UNSUPPORTED,
              "vqgan_quantize: operands must be 16-byte aligned");
  if (N == 0) return OFA_OK;
  VqQuantArgs a = {h, w, bias, out, (float*)ws, (int*)ws + (int64_t)p.splits * N, N, K, n_embed, p.splits, p.fps, seed};
  const dim3 grid(cdiv(N, p.rows), p.splits);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype16(dtype, [&](auto tag) {
    constexpr bool F16 = std::is_same<typename decltype(tag)::type, f16_t>::value;
    auto go = [&](auto kern) {
      if (p.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
      hipLaunchKernelGGL(kern, grid, dim3(256), p.lds, st, a);
    };
    if (p.rows == 128) seed >= 0 ? go(vq_quantize_kernel<F16, 4, true>) : go(vq_quantize_kernel<F16, 4, false>);
    else seed >= 0 ? go(vq_quantize_kernel<F16, 2, true>) : go(vq_quantize_kernel<F16, 2, false>);
  });
  if (p.splits > 1) hipLaunchKernelGGL(vq_quantize_fold_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, (const float*)a.ws_v, (const int*)a.ws_n, out, N, p.splits);
  return check_launch("vqgan_quantize");
}

// The HiFi-GAN generator's kernels (module/hifigan.py:24-162) on channels-last rows [B, L, C] in fp16 / bf16, fp32 accumulation.
//   voc_conv_kernel   one launch of a dilated Conv1d as a tap-loop GEMM on the 32x32x16 MFMA:
//                       y[b, t] = (bias + sum_j W_j . act(x[b, t + (j - (k-1)/2) d]) + res[b, t] + y[b, t]) * out_scale
//                     (res, the += into y and the scale are optional; act = leaky ReLU, slope 1 = none).  A workgroup (4 waves) owns TM
//                     time rows of one sample and 32 * NT output channels.  The TM + 2 * halo input rows (halo = d (k-1)/2 <= 25) are
//                     staged ONCE into LDS, activated on the way in, rows outside [0, lens[b] * len_scale) as zeros -- a tap shift is then
//                     a row offset j * d into that one image and nothing unfolded ever exists in HBM.  LDS rows are Cin + 8 elements apart
//                     (16 bytes of padding: the 32 lanes of a fragment read 32 different rows at one column and would otherwise meet in
//                     the same banks).  The weight is [k][Cout][Cin] (tap-major, Cin contiguous): lane (i, hi) of a wave reads the 8
//                     input channels kc + 8 hi .. + 7 of output channel n0 + i with one 16-byte load straight from L2 into the A fragment,
//                     four K-steps ahead of the MFMAs that use them, and keeps it for the wave's MT time tiles.  The MFMA's rows are the
//                     output channels and its columns the time rows, so a lane ends up holding 4 consecutive channels of one time row per
//                     register quad: the epilogue reads res / y and writes y in 8-byte pieces.
//                     NT waves side by side over the channels (4 when Cout >= 128, 2 from 64, else 1), the other 4 / NT over time;
//                     MT in {4, 2, 1} the largest whose image fits 80 KiB (two workgroups per CU), so TM = 32 MT 4 / NT.
//                     A tile that lies wholly past its sample's end writes zeros and never touches the MFMA: a ragged batch pays for
//                     its frames, not for its padding.  The tiling of a sample starts at its own row 0 and no sum crosses a workgroup,
//                     so a sample's bits do not depend on its neighbours in the batch; no atomics.
//   ConvTranspose1d(k = 2u, stride u, padding u/2) runs through the SAME kernel as a 3-tap convolution with u * Cout output columns
//                     (the host arranges the weight once, module/hifigan.py `polyphase_weight`): row q of [L, u * Cout] is rows
//                     q u .. q u + u - 1 of [L u, Cout].  A third of those weight blocks are zeros; the upsamplers are ~1 % of the flops.
//   voc_post_kernel   conv_post: out[b, t] = tanh(bias + sum_{j, c} w[j][c] act(x[b, t + j - (k-1)/2][c])), fp32 out.  256 outputs per
//                     workgroup from an fp32 LDS image of 256 + k - 1 rows (row pitch C + 1 floats), one thread per output, VALU.
#include <type_traits>

#include "common.h"

namespace ofa {

typedef __attribute__((ext_vector_type(8))) short voc_bf16x8;
typedef __attribute__((ext_vector_type(16))) float voc_f32x16;

constexpr int VOC_LDS_TARGET = 80 * 1024;      // two workgroups per CU
constexpr int VOC_LDS_MAX = 160 * 1024;
constexpr int VOC_MAX_HALO = 25;
constexpr int VOC_POST_TILE = 256, VOC_POST_MAX_C = 32, VOC_POST_MAX_K = 7;

struct VocConvArgs {
  const void *x, *w, *bias, *res;
  void* y;
  const int32_t* lens;
  int B, L, Cin, Cout, k, d, len_scale, accum;
  float slope, out_scale;
};

template <bool F16> __device__ __forceinline__ voc_f32x16 voc_mfma(const uint4& a, const uint4& b, const voc_f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(voc_bf16x8, a), __builtin_bit_cast(voc_bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ float voc_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// rows of sample b that exist at this stage: lens[b] * len_scale clamped into [0, L]
__device__ __forceinline__ int voc_valid(const int32_t* lens, int b, int len_scale, int L) {
  if (!lens) return L;
  const int64_t v = (int64_t)lens[b] * len_scale;
  return (int)(v < 0 ? 0 : (v > L ? L : v));
}

template <bool F16, int MT, int NT>
__global__ __launch_bounds__(256) void voc_conv_kernel(VocConvArgs a) {
  typedef typename std::conditional<F16, f16_t, bf16_t>::type T;
  constexpr int MG = 4 / NT, TM = 32 * MT * MG, G = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char voc_smem[];
  uint16_t* tile = reinterpret_cast<uint16_t*>(voc_smem);                 // [TM + 2 halo][Cin + 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z, t0 = blockIdx.x * TM, n_wg = blockIdx.y * (32 * NT);
  const int L = a.L, Cin = a.Cin, Cout = a.Cout;
  const int halo = a.d * ((a.k - 1) / 2), LD = Cin + 8;
  const int valid = voc_valid(a.lens, b, a.len_scale, L);
  const uint16_t* xb = reinterpret_cast<const uint16_t*>(a.x) + (int64_t)b * L * Cin;
  uint16_t* yb = reinterpret_cast<uint16_t*>(a.y) + (int64_t)b * L * Cout;

  if (t0 >= valid) {                                                      // wholly past the sample's end: zeros, no arithmetic
    const int rows = min(TM, L - t0), cols = min(32 * NT, Cout - n_wg) / 4;
    for (int v = tid; v < rows * cols; v += 256)
      *reinterpret_cast<uint2*>(yb + (int64_t)(t0 + v / cols) * Cout + n_wg + (v % cols) * 4) = make_uint2(0, 0);
    return;
  }

  // ---- the input image: rows t0 - halo .. t0 + TM + halo - 1, activated, zeros outside [0, valid)
  {
    const int vpr = Cin / 8, nrow = TM + 2 * halo;
    const float slope = a.slope;
    for (int v = tid; v < nrow * vpr; v += 256) {
      const int r = v / vpr, c = (v - r * vpr) * 8, t = t0 - halo + r;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (t >= 0 && t < valid) {
        val = *reinterpret_cast<const uint4*>(xb + (int64_t)t * Cin + c);
        if (slope != 1.0f) {
          float f[8];
          unpack16<T>(val, f);
          val = make_uint4(pack2<T>(voc_lrelu(f[0], slope), voc_lrelu(f[1], slope)), pack2<T>(voc_lrelu(f[2], slope), voc_lrelu(f[3], slope)),
                           pack2<T>(voc_lrelu(f[4], slope), voc_lrelu(f[5], slope)), pack2<T>(voc_lrelu(f[6], slope), voc_lrelu(f[7], slope)));
        }
      }
      *reinterpret_cast<uint4*>(tile + r * LD + c) = val;
    }
  }
  __syncthreads();

  const int ng = wave % NT, mg = wave / NT;
  const int n0 = n_wg + ng * 32;
  if (n0 >= Cout) return;                                                 // (after the only barrier)
  const int li = lane & 31, hi = lane >> 5;
  const bool a_ok = n0 + li < Cout;                                       // Cout is a multiple of 16: the upper half of a tile may not exist
  const int nk = Cin / 16, total = a.k * nk;
  const uint16_t* wp = reinterpret_cast<const uint16_t*>(a.w) + (int64_t)(a_ok ? n0 + li : n0) * Cin + hi * 8;
  const int64_t tap_stride = (int64_t)Cout * Cin;
  const uint16_t* lp = tile + (mg * MT * 32 + li) * LD + hi * 8;
  const int tap_rows = a.d * LD;

  voc_f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

  // K-steps it = j * nk + kk (tap j, input channels 16 kk .. + 15), in groups of G: the next group's weight fragments are in flight
  // while this group's MFMAs run
  uint4 cur[G], nxt[G];
  auto load_group = [&](int it0, uint4* dst) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int it = it0 + g;
      dst[g] = make_uint4(0, 0, 0, 0);
      if (it < total && a_ok) {
        const int j = it / nk, kk = it - j * nk;
        dst[g] = *reinterpret_cast<const uint4*>(wp + j * tap_stride + kk * 16);
      }
    }
  };
  load_group(0, cur);
  for (int it0 = 0; it0 < total; it0 += G) {
    load_group(it0 + G, nxt);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int it = it0 + g;
      if (it < total) {
        const int j = it / nk, kk = it - j * nk;
        const uint16_t* src = lp + j * tap_rows + kk * 16;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const uint4 bf = *reinterpret_cast<const uint4*>(src + mt * 32 * LD);
          acc[mt] = voc_mfma<F16>(cur[g], bf, acc[mt]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) cur[g] = nxt[g];
  }

  // ---- epilogue: register quad q of a lane = channels n0 + 8 q + 4 hi .. + 3 of time row (tile mt, column li)
  const uint16_t* bias = reinterpret_cast<const uint16_t*>(a.bias);
  const uint16_t* resb = a.res ? reinterpret_cast<const uint16_t*>(a.res) + (int64_t)b * L * Cout : nullptr;
  const float out_scale = a.out_scale;
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
    const int t = t0 + (mg * MT + mt) * 32 + li;
    if (t >= L) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = n0 + 8 * q + 4 * hi;
      if (c >= Cout) continue;
      uint2 o = make_uint2(0, 0);
      if (t < valid) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[mt][4 * q + e];
        add4(v, bias + c);
        const int64_t off = (int64_t)t * Cout + c;
        if (resb) add4(v, resb + off);
        if (a.accum) add4(v, yb + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= out_scale;
        o = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
      }
      *reinterpret_cast<uint2*>(yb + (int64_t)t * Cout + c) = o;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(VOC_POST_TILE) void voc_post_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ bias,
                                                                 float* __restrict__ out, const int32_t* __restrict__ lens, int L, int C,
                                                                 int k, int len_scale, float slope) {
  __shared__ float img[(VOC_POST_TILE + VOC_POST_MAX_K - 1) * (VOC_POST_MAX_C + 1)];
  __shared__ float wf[VOC_POST_MAX_K * VOC_POST_MAX_C];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * VOC_POST_TILE;
  const int valid = voc_valid(lens, b, len_scale, L);
  const int t = t0 + tid;
  if (t0 >= valid) {
    if (t < L) out[(int64_t)b * L + t] = 0.f;
    return;
  }
  const int half = (k - 1) / 2, LD = C + 1, vpr = C / 8, nrow = VOC_POST_TILE + k - 1;
  const T* xb = x + (int64_t)b * L * C;
  for (int v = tid; v < nrow * vpr; v += VOC_POST_TILE) {
    const int r = v / vpr, c = (v - r * vpr) * 8, ts = t0 - half + r;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0.f;
    if (ts >= 0 && ts < valid) load_vec<T>(xb + (int64_t)ts * C + c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) img[r * LD + c + e] = voc_lrelu(f[e], slope);
  }
  for (int i = tid; i < k * C; i += VOC_POST_TILE) wf[i] = ld1<T>(w + i);
  __syncthreads();
  if (t >= L) return;
  float acc = ld1<T>(bias);
  for (int j = 0; j < k; ++j) {
    const float* row = img + (tid + j) * LD;
    const float* wj = wf + j * C;
    for (int c = 0; c < C; ++c) acc = fmaf(wj[c], row[c], acc);
  }
  out[(int64_t)b * L + t] = t < valid ? tanhf(acc) : 0.f;
}

// ---------------------------------------------------------------- host side
struct VocPlan { int mt, nt, tm, lds; };
// The tiling of a (Cin, Cout, k, d) convolution; tm == 0: the image of even the smallest tile does not fit the LDS.
static VocPlan voc_plan(int Cin, int Cout, int k, int d) {
  VocPlan p;
  p.nt = Cout >= 128 ? 4 : (Cout >= 64 ? 2 : 1);
  const int halo = d * ((k - 1) / 2);
  auto lds = [&](int mt) { return (32 * mt * (4 / p.nt) + 2 * halo) * (Cin + 8) * 2; };
  p.mt = 1;
  for (int mt = 4; mt >= 1; mt >>= 1)
    if (lds(mt) <= VOC_LDS_TARGET) { p.mt = mt; break; }
  p.lds = lds(p.mt);
  p.tm = p.lds <= VOC_LDS_MAX ? 32 * p.mt * (4 / p.nt) : 0;
  return p;
}

static int voc_conv_check(const char* who, const VocConvArgs& a, int max_cout, int dtype) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(dtype != OFA_F32, OFA_ERR_UNSUPPORTED, "%s: fp16 or bf16 only (the kernel is an MFMA loop over 16-bit operands)", who);
  OFA_REQUIRE(a.B >= 0 && a.B <= 65535 && a.L > 0 && a.len_scale >= 1, OFA_ERR_INVALID, "%s: bad B=%d L=%d len_scale=%d", who, a.B, a.L,
              a.len_scale);
  OFA_REQUIRE(a.Cin % 16 == 0 && a.Cin >= 16 && a.Cin <= 512 && a.Cout % 16 == 0 && a.Cout >= 16 && a.Cout <= max_cout, OFA_ERR_UNSUPPORTED,
              "%s: Cin=%d must be a multiple of 16 in 16..512 and Cout=%d one in 16..%d", who, a.Cin, a.Cout, max_cout);
  OFA_REQUIRE(a.k >= 1 && a.k % 2 == 1 && a.d >= 1 && a.d * ((a.k - 1) / 2) <= VOC_MAX_HALO, OFA_ERR_UNSUPPORTED,
              "%s: k=%d must be odd and the halo d (k-1)/2 = %d at most %d rows", who, a.k, a.d * ((a.k - 1) / 2), VOC_MAX_HALO);
  OFA_REQUIRE((int64_t)a.L * (a.Cin > a.Cout ? a.Cin : a.Cout) <= 0x7fffffff, OFA_ERR_UNSUPPORTED, "%s: a sample of L=%d rows is too long", who,
              a.L);
  OFA_REQUIRE(a.B == 0 || (a.x && a.w && a.bias && a.y), OFA_ERR_INVALID, "%s: null operand", who);
  OFA_REQUIRE(a.B == 0 || (aligned16(a.x) && aligned16(a.w) && aligned16(a.y) && aligned16(a.bias) && aligned16(a.res)), OFA_ERR_UNSUPPORTED,
              "%s: operands must be 16-byte aligned", who);
  OFA_REQUIRE(a.B == 0 || (a.y != a.x && a.y != a.res), OFA_ERR_INVALID, "%s: y must not alias x or res (other workgroups read their halo)", who);
  return OFA_OK;
}

template <bool F16, int MT> static void voc_conv_launch_nt(const VocPlan& p, const VocConvArgs& a, hipStream_t st) {
  const dim3 grid(cdiv(a.L, p.tm), cdiv(a.Cout, 32 * p.nt), a.B), block(256);
  auto go = [&](auto kern) {
    if (p.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds);
    hipLaunchKernelGGL(kern, grid, block, p.lds, st, a);
  };
  if (p.nt == 4) go(voc_conv_kernel<F16, MT, 4>);
  else if (p.nt == 2) go(voc_conv_kernel<F16, MT, 2>);
  else go(voc_conv_kernel<F16, MT, 1>);
}

static int voc_conv_launch(const char* who, const VocConvArgs& a, int max_cout, int dtype, void* stream) {
  const int rc = voc_conv_check(who, a, max_cout, dtype);
  if (rc != OFA_OK) return rc;
  const VocPlan p = voc_plan(a.Cin, a.Cout, a.k, a.d);
  OFA_REQUIRE(p.tm > 0, OFA_ERR_UNSUPPORTED, "%s: the input image of Cin=%d k=%d d=%d (%d bytes) exceeds the LDS", who, a.Cin, a.k, a.d, p.lds);
  if (a.B == 0) return OFA_OK;
  hipStream_t st = (hipStream_t)stream;
  auto by_mt = [&](auto f16) {
    constexpr bool F16 = decltype(f16)::value;
    if (p.mt == 4) voc_conv_launch_nt<F16, 4>(p, a, st);
    else if (p.mt == 2) voc_conv_launch_nt<F16, 2>(p, a, st);
    else voc_conv_launch_nt<F16, 1>(p, a, st);
  };
  if (dtype == OFA_F16) by_mt(std::true_type{});
  else by_mt(std::false_type{});
  return check_launch(who);
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_vocoder_conv_tile(int Cin, int Cout, int k, int d) {
  if (Cin < 16 || Cin % 16 || Cout < 16 || Cout % 16 || k < 1 || k % 2 == 0 || d < 1) return 0;
  return voc_plan(Cin, Cout, k, d).tm;
}

extern "C" int ofa_vocoder_post_tile(void) { return VOC_POST_TILE; }

extern "C" int ofa_vocoder_conv(const void* x, const void* w, const void* bias, const void* res, void* y, const int32_t* lens, int B, int L,
                                int Cin, int Cout, int k, int d, int len_scale, float slope, int accum, float out_scale, int dtype,
                                void* stream) {
  const VocConvArgs a = {x, w, bias, res, y, lens, B, L, Cin, Cout, k, d, len_scale, accum, slope, out_scale};
  return voc_conv_launch("vocoder_conv", a, 512, dtype, stream);
}

extern "C" int ofa_vocoder_upsample(const void* x, const void* w, const void* bias, void* y, const int32_t* lens, int B, int L, int Cin,
                                    int Cout, int u, int len_scale, float slope, int dtype, void* stream) {
  OFA_REQUIRE(u >= 2 && u % 2 == 0 && u <= 16, OFA_ERR_UNSUPPORTED, "vocoder_upsample: stride u=%d must be even, 2..16 (kernel size 2u)", u);
  OFA_REQUIRE(Cout >= 16 && Cout <= 512 && Cout % 16 == 0, OFA_ERR_UNSUPPORTED, "vocoder_upsample: Cout=%d must be a multiple of 16 in 16..512", Cout);
  const VocConvArgs a = {x, w, bias, nullptr, y, lens, B, L, Cin, u * Cout, 3, 1, len_scale, 0, slope, 1.0f};
  return voc_conv_launch("vocoder_upsample", a, 16 * 512, dtype, stream);
}

extern "C" int ofa_vocoder_post(const void* x, const void* w, const void* bias, float* out, const int32_t* lens, int B, int L, int C, int k,
                                int len_scale, float slope, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "vocoder_post: bad dtype %d", dtype);
  OFA_REQUIRE(dtype != OFA_F32, OFA_ERR_UNSUPPORTED, "vocoder_post: fp16 or bf16 only");
  OFA_REQUIRE(B >= 0 && B <= 65535 && L > 0 && len_scale >= 1, OFA_ERR_INVALID, "vocoder_post: bad B=%d L=%d len_scale=%d", B, L, len_scale);
  OFA_REQUIRE(C % 8 == 0 && C >= 8 && C <= VOC_POST_MAX_C && k % 2 == 1 && k >= 1 && k <= VOC_POST_MAX_K, OFA_ERR_UNSUPPORTED,
              "vocoder_post: C=%d must be a multiple of 8 up to %d and k=%d odd up to %d", C, VOC_POST_MAX_C, k, VOC_POST_MAX_K);
  OFA_REQUIRE(B == 0 || (x && w && bias && out), OFA_ERR_INVALID, "vocoder_post: null operand");
  OFA_REQUIRE(B == 0 || aligned16(x), OFA_ERR_UNSUPPORTED, "vocoder_post: x must be 16-byte aligned");
  if (B == 0) return OFA_OK;
  const dim3 grid(cdiv(L, VOC_POST_TILE), B), block(VOC_POST_TILE);
  dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((voc_post_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, (const T*)w, (const T*)bias, out, lens, L, C, k,
                       len_scale, slope);
  });
  return check_launch("vocoder_post");
}

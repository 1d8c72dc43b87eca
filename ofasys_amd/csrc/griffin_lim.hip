// The Griffin-Lim vocoder's kernels (module/vocoder.py:29-103 of the reference), all in fp32.
//   gl_kernel<LOGN, FROM_PHASE>   one Griffin-Lim iteration in one launch (FROM_PHASE: the synthesis half alone, from supplied phases).
//       The reference computes the STFT and its inverse as dense products against a (n_fft + 2) x n_fft Fourier basis; here a frame is a
//       real FFT of N = n_fft points done by ONE wave, and a workgroup (4 waves) owns `R` frames' worth (`span` = R hop) of consecutive
//       output samples of one utterance.  It recomputes every frame that overlaps its span -- the run's own R and ceil(N / hop) - 1 halo
//       frames -- so the overlap-add ends inside the workgroup: no second pass, no atomics.
//       Per frame, in the wave's own LDS buffer of N floats (= M = N / 2 complex points):
//         1. stage      f[n] = window[n] * w[reflect(t hop + n - M)], the index reflected about both ends of the utterance's own length
//         2. forward    complex FFT of M points on z[m] = (f[2m], f[2m + 1]): radix-2 decimation in frequency, two stages per LDS pass
//                       (a thread holds the four points of a radix-2^2 butterfly in registers); the result lies in bit-reversed order
//         3. phase      lane k takes the pair (k, M - k): the split step gives the real transform's bins X_k, X_{M-k}; each is replaced
//                       by S[b, t, k] X / |X| (normalised by max(|re|, |im|) first; (1, 0) where X = 0) and the pair is folded back into
//                       the packed spectrum of the inverse, in place
//         4. inverse    radix-2 decimation in time from bit-reversed order, the mirror image of 2 with conjugated twiddles: the Hermitian
//                       inverse (DC and Nyquist real, weight 1 / N; the other bins 2 / N)
//         5. window     f[n] *= window[n] / N
//       Twiddles e^{-2 pi i j / N}, j < M, come from the host (float64, rounded once) and are staged into LDS once per workgroup.
//       Four frames -- one per wave -- make a round.  After a round's barrier the 256 threads add the four frames into the run buffer,
//       each thread its own output positions and the frames in ascending order: the sum of a sample has one fixed order.
//       The run is finished as GriffinLim.inverse does: divided by the window-sum-square where that exceeds 1.1754944e-38 (the table row of
//       THIS utterance's frame count), trimmed by M at both ends (the run buffer never holds the trimmed parts) and stored as float4 where
//       the address allows.  The reference's n_fft / hop scaling and its inverse in the synthesis basis cancel and are not applied.
//       LDS: N floats of twiddles + 4 N of frame buffers + span of run buffer; `gl_run` keeps it within 64 KiB.
//   gl_specgram_kernel<T>         S[r, k] = max(0, sum_j pinv_t[j, k] exp(x[r, j])): 8 rows per workgroup, exp(x) in LDS, one fp32 fma chain
//                                 in j order per output; pinv_t is the pseudo-inverse TRANSPOSED ([n_mels, K]) so that lanes read along k.
#include "common.h"
#include "fft_wave.h"   // gl_add .. gl_mulc, gl_wave_sync, gl_fft_forward: shared with audio_features.hip

namespace ofa {

constexpr int GL_THREADS = 256, GL_WAVES = 4;
constexpr int GL_LDS_BUDGET = 64 * 1024;
constexpr float GL_TINY = 1.1754944e-38f;
constexpr int GL_SPEC_ROWS = 8, GL_SPEC_MAX_MELS = 128;

struct GlArgs {
  const float* w_in;       // [B, hop (T-1)]      (project)
  const float* phase;      // [B, T, M + 1]       (inverse)
  const float* S;          // [B, T, M + 1]
  const float* window;     // [N]
  const float2* tw;        // [M]
  const float* wss;        // [B or 1][N + hop (T-1)]
  int64_t wss_stride;
  const int32_t* lens;
  float* w_out;            // [B, hop (T-1)]
  int B, T, hop, R;
};

// X / |X|; (1, 0) at X = 0
__device__ __forceinline__ float2 gl_unit(float2 x) {
  const float m = fmaxf(fabsf(x.x), fabsf(x.y));
  if (!(m > 0.f)) return make_float2(1.f, 0.f);
  const float re = x.x / m, im = x.y / m;
  const float r = 1.0f / sqrtf(re * re + im * im);
  return make_float2(re * r, im * r);
}

// Its mirror image: bit-reversed order in, natural order out, x[n] = sum_k X[k] e^{+2 pi i k n / M} (not normalised).
// Stage h: (a, b) at distance h -> (a + b conj(W_{2h}^j), a - b conj(W_{2h}^j)).
template <int LOGM> __device__ __forceinline__ void gl_fft_inverse(float2* z, const float2* tw, int lane) {
  constexpr int M = 1 << LOGM;
  int lh = 0;
  if (LOGM & 1) {
    for (int q = lane; q < M / 2; q += WAVE) {
      const float4 v = *reinterpret_cast<const float4*>(z + 2 * q);
      *reinterpret_cast<float4*>(z + 2 * q) = make_float4(v.x + v.z, v.y + v.w, v.x - v.z, v.y - v.w);
    }
    gl_wave_sync();
    lh = 1;
  }
#pragma unroll
  for (; lh + 1 < LOGM; lh += 2) {                              // stages h and 2 h
    const int h = 1 << lh;
    for (int q = lane; q < M / 4; q += WAVE) {
      const int j = q & (h - 1), i0 = ((q >> lh) << (lh + 2)) + j;
      const float2 a0 = z[i0], a1 = z[i0 + h], a2 = z[i0 + 2 * h], a3 = z[i0 + 3 * h];
      const float2 t1 = gl_mulc(a1, tw[j << (LOGM - lh)]), t3 = gl_mulc(a3, tw[j << (LOGM - lh)]);
      const float2 b0 = gl_add(a0, t1), b1 = gl_sub(a0, t1), b2 = gl_add(a2, t3), b3 = gl_sub(a2, t3);
      const float2 u2 = gl_mulc(b2, tw[j << (LOGM - lh - 1)]), u3 = gl_mulc(b3, tw[(j + h) << (LOGM - lh - 1)]);
      z[i0] = gl_add(b0, u2);
      z[i0 + 2 * h] = gl_sub(b0, u2);
      z[i0 + h] = gl_add(b1, u3);
      z[i0 + 3 * h] = gl_sub(b1, u3);
    }
    gl_wave_sync();
  }
}

// Steps 1-5 for frame t of utterance b (Lb samples) by one wave in its buffer f [N].
template <int LOGN, bool FROM_PHASE>
__device__ __forceinline__ void gl_frame(const GlArgs& a, float* f, const float2* tw, int b, int t, int Lb, int lane) {
  constexpr int N = 1 << LOGN, M = N / 2, LOGM = LOGN - 1;
  float2* z = reinterpret_cast<float2*>(f);
  const int64_t row = ((int64_t)b * a.T + t) * (M + 1);
  const float* S = a.S + row;
  if (!FROM_PHASE) {
    const float* w = a.w_in + (int64_t)b * a.hop * (a.T - 1);
    const int first = t * a.hop - M;
    for (int n = lane * 4; n < N; n += WAVE * 4) {
      const float4 wn = *reinterpret_cast<const float4*>(a.window + n);
      const float wv[4] = {wn.x, wn.y, wn.z, wn.w};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int i = first + n + e;
        i = i < 0 ? -i : (i >= Lb ? 2 * (Lb - 1) - i : i);
        i = min(max(i, 0), Lb - 1);                             // (an utterance too short to reflect is refused by the caller: stay inside it)
        v[e] = wv[e] * w[i];
      }
      *reinterpret_cast<float4*>(f + n) = make_float4(v[0], v[1], v[2], v[3]);
    }
    gl_wave_sync();
    gl_fft_forward<LOGM>(z, tw, lane);
  }
  for (int k = lane; k <= M / 2; k += WAVE) {
    if (k == 0) {                                               // DC and Nyquist: real bins, packed into z[0]
      float u0, um;
      if (FROM_PHASE) {
        u0 = cosf(a.phase[row]);
        um = cosf(a.phase[row + M]);
      } else {
        const float2 z0 = z[0];
        u0 = gl_unit(make_float2(z0.x + z0.y, 0.f)).x;
        um = gl_unit(make_float2(z0.x - z0.y, 0.f)).x;
      }
      const float y0 = S[0] * u0, ym = S[M] * um;
      z[0] = make_float2(y0 + ym, y0 - ym);
      continue;
    }
    const int pk = (int)(__brev((unsigned)k) >> (32 - LOGM)), pm = (int)(__brev((unsigned)(M - k)) >> (32 - LOGM));
    const float2 wk = tw[k];
    float2 uk, um;
    if (FROM_PHASE) {
      const float pa = a.phase[row + k], pb = a.phase[row + M - k];
      uk = make_float2(cosf(pa), sinf(pa));
      um = make_float2(cosf(pb), sinf(pb));
    } else {
      const float2 zk = z[pk], zm = z[pm];
      const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
      const float2 O = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
      const float2 tO = gl_mul(wk, O);
      uk = gl_unit(gl_add(E, tO));                              // X_k
      const float2 d = gl_sub(E, tO);
      um = gl_unit(make_float2(d.x, -d.y));                     // X_{M-k} = conj(E - w^k O)
    }
    const float sk = S[k], sm = S[M - k];
    const float2 yk = make_float2(sk * uk.x, sk * uk.y), ym = make_float2(sm * um.x, sm * um.y);
    const float2 A = make_float2(yk.x + ym.x, yk.y - ym.y);                     // Y_k + conj(Y_{M-k})
    const float2 Bv = gl_mulc(make_float2(yk.x - ym.x, yk.y + ym.y), wk);       // (Y_k - conj(Y_{M-k})) conj(w^k)
    z[pk] = make_float2(A.x - Bv.y, A.y + Bv.x);
    if (pm != pk) z[pm] = make_float2(A.x + Bv.y, Bv.x - A.y);
  }
  gl_wave_sync();
  gl_fft_inverse<LOGM>(z, tw, lane);
  constexpr float inv_n = 1.0f / N;
  for (int n = lane * 4; n < N; n += WAVE * 4) {
    const float4 wn = *reinterpret_cast<const float4*>(a.window + n);
    float4 v = *reinterpret_cast<const float4*>(f + n);
    v.x *= wn.x * inv_n; v.y *= wn.y * inv_n; v.z *= wn.z * inv_n; v.w *= wn.w * inv_n;
    *reinterpret_cast<float4*>(f + n) = v;
  }
}

template <int LOGN, bool FROM_PHASE>
__global__ __launch_bounds__(GL_THREADS) void gl_kernel(GlArgs a) {
  constexpr int N = 1 << LOGN, M = N / 2;
  extern __shared__ __attribute__((aligned(16))) float gl_smem[];
  float2* tw = reinterpret_cast<float2*>(gl_smem);              // [M]
  float* fbuf = gl_smem + N;                                    // [4][N]
  float* run = gl_smem + 5 * N;                                 // [span]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, hop = a.hop, span = a.R * hop;
  const int Lmax = hop * (a.T - 1);
  const int Tb = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int Lb = Tb > 0 ? hop * (Tb - 1) : 0;
  const int j0 = blockIdx.x * span;                             // the first owned sample, counted after the trim
  const int cnt = min(span, Lmax - j0);                         // owned samples of the buffer
  const int live = min(cnt, Lb - j0);                           // ... of the utterance
  float* out = a.w_out + (int64_t)b * Lmax + j0;

  if (live > 0) {
    for (int i = tid; i < M; i += GL_THREADS) tw[i] = a.tw[i];
    for (int i = tid; i < span; i += GL_THREADS) run[i] = 0.f;
    __syncthreads();
    // before the trim the owned samples are positions [P0, P1); frame t covers [t hop, t hop + N)
    const int P0 = j0 + M, P1 = P0 + live;
    const int t_lo = j0 < M ? 0 : (j0 - M) / hop + 1, t_hi = min(Tb - 1, (P1 - 1) / hop);
    for (int tb = t_lo; tb <= t_hi; tb += GL_WAVES) {
      if (tb + wave <= t_hi) gl_frame<LOGN, FROM_PHASE>(a, fbuf + wave * N, tw, b, tb + wave, Lb, lane);
      __syncthreads();
      const int lo = max(P0, tb * hop), hi = min(P1, (tb + GL_WAVES - 1) * hop + N);
      for (int p = lo + tid; p < hi; p += GL_THREADS) {
        float v = run[p - P0];
#pragma unroll
        for (int s = 0; s < GL_WAVES; ++s) {
          const int n = p - (tb + s) * hop;
          if (tb + s <= t_hi && n >= 0 && n < N) v += fbuf[s * N + n];
        }
        run[p - P0] = v;
      }
      __syncthreads();
    }
  }

  // the finish: window-sum-square, zeros past the utterance, float4 where the address is aligned
  const float* wss = a.wss + (int64_t)b * a.wss_stride + j0 + M;
  auto value = [&](int i) -> float {
    if (i >= live) return 0.f;
    const float s = wss[i];
    const float v = run[i];
    return s > GL_TINY ? v / s : v;
  };
  const int lead = min(cnt, (int)((4 - (((int64_t)b * Lmax + j0) & 3)) & 3));
  const int quads = (cnt - lead) / 4;
  for (int i = tid; i < lead; i += GL_THREADS) out[i] = value(i);
  for (int q = tid; q < quads; q += GL_THREADS) {
    const int i = lead + 4 * q;
    *reinterpret_cast<float4*>(out + i) = make_float4(value(i), value(i + 1), value(i + 2), value(i + 3));
  }
  for (int i = lead + 4 * quads + tid; i < cnt; i += GL_THREADS) out[i] = value(i);
}

template <typename T>
__global__ __launch_bounds__(GL_THREADS) void gl_specgram_kernel(const T* __restrict__ x, const float* __restrict__ pinv_t, float* __restrict__ S,
                                                                 int64_t rows, int n_mels, int K) {
  __shared__ float e[GL_SPEC_ROWS * GL_SPEC_MAX_MELS];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * GL_SPEC_ROWS;
  const int nr = (int)(rows - r0 < GL_SPEC_ROWS ? rows - r0 : GL_SPEC_ROWS);
  for (int i = tid; i < GL_SPEC_ROWS * n_mels; i += GL_THREADS) e[i] = i < nr * n_mels ? expf(ld1<T>(x + r0 * n_mels + i)) : 0.f;
  __syncthreads();
  for (int k = tid; k < K; k += GL_THREADS) {
    float acc[GL_SPEC_ROWS];
#pragma unroll
    for (int r = 0; r < GL_SPEC_ROWS; ++r) acc[r] = 0.f;
    for (int j = 0; j < n_mels; ++j) {
      const float p = pinv_t[(int64_t)j * K + k];
#pragma unroll
      for (int r = 0; r < GL_SPEC_ROWS; ++r) acc[r] = fmaf(p, e[r * n_mels + j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < GL_SPEC_ROWS; ++r)
      if (r < nr) S[(r0 + r) * K + k] = fmaxf(acc[r], 0.f);
  }
}

// ---------------------------------------------------------------- host side
static int gl_log2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return (1 << l) == n ? l : -1;
}

// Frames' worth of samples a workgroup owns; 0: the shape is not served.  Four times the halo keeps the recomputation at 1.25x; the run
// buffer takes what the twiddles and the four frame buffers leave of the LDS budget.
static int gl_run(int n_fft, int win, int hop) {
  const int l = gl_log2(n_fft);
  if (l < 8 || l > 11 || win < 1 || win > n_fft || hop < 1 || hop > n_fft) return 0;
  const int halo = (n_fft + hop - 1) / hop - 1;
  const int want = halo > 0 ? 4 * halo : 4, room = (GL_LDS_BUDGET / 4 - 5 * n_fft) / hop;
  return want < room ? want : room;
}

template <bool FROM_PHASE> static int gl_launch(const char* who, GlArgs a, int n_fft, int win, void* stream) {
  a.R = gl_run(n_fft, win, a.hop);
  OFA_REQUIRE(a.R > 0, OFA_ERR_UNSUPPORTED, "%s: n_fft=%d must be a power of two in 256..2048 with win=%d <= n_fft and 1 <= hop=%d <= n_fft", who,
              n_fft, win, a.hop);
  OFA_REQUIRE(a.B >= 0 && a.B <= 65535 && a.T >= 1, OFA_ERR_INVALID, "%s: bad B=%d T=%d", who, a.B, a.T);
  OFA_REQUIRE((int64_t)a.hop * (a.T - 1) + n_fft <= 0x7fffffff, OFA_ERR_UNSUPPORTED, "%s: T=%d frames at hop=%d are too many", who, a.T, a.hop);
  OFA_REQUIRE(a.wss_stride == 0 || a.wss_stride >= (int64_t)a.hop * (a.T - 1) + n_fft, OFA_ERR_INVALID,
              "%s: wss_stride=%lld is shorter than a table of n_fft + hop (T - 1)", who, (long long)a.wss_stride);
  OFA_REQUIRE(a.lens == nullptr || a.wss_stride > 0, OFA_ERR_INVALID, "%s: lens needs one window-sum-square row per utterance (wss_stride > 0)", who);
  const int Lmax = a.hop * (a.T - 1);
  if (a.B == 0 || Lmax == 0) return OFA_OK;
  OFA_REQUIRE((FROM_PHASE ? (const void*)a.phase : (const void*)a.w_in) && a.S && a.window && a.tw && a.wss && a.w_out, OFA_ERR_INVALID,
              "%s: null operand", who);
  OFA_REQUIRE(aligned16(a.window) && aligned16(a.w_out) && aligned16(a.tw), OFA_ERR_UNSUPPORTED, "%s: window, twiddle and w_out must be 16-byte aligned",
              who);
  OFA_REQUIRE((const void*)a.w_in != (const void*)a.w_out, OFA_ERR_INVALID, "%s: w_out must not alias w_in (other workgroups read their frames)", who);
  const int span = a.R * a.hop, lds = 4 * (5 * n_fft + span);
  const dim3 grid(cdiv(Lmax, span), a.B), block(GL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (gl_log2(n_fft)) {
    case 8: hipLaunchKernelGGL((gl_kernel<8, FROM_PHASE>), grid, block, lds, st, a); break;
    case 9: hipLaunchKernelGGL((gl_kernel<9, FROM_PHASE>), grid, block, lds, st, a); break;
    case 10: hipLaunchKernelGGL((gl_kernel<10, FROM_PHASE>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((gl_kernel<11, FROM_PHASE>), grid, block, lds, st, a); break;
  }
  return check_launch(who);
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_griffin_lim_run(int n_fft, int win, int hop) { return gl_run(n_fft, win, hop); }

extern "C" int ofa_griffin_lim_project(const float* w_in, const float* S, const float* window, const float* twiddle, const float* wss,
                                       int64_t wss_stride, const int32_t* lens, float* w_out, int B, int T, int n_fft, int win, int hop,
                                       void* stream) {
  const GlArgs a = {w_in, nullptr, S, window, reinterpret_cast<const float2*>(twiddle), wss, wss_stride, lens, w_out, B, T, hop, 0};
  return gl_launch<false>("griffin_lim_project", a, n_fft, win, stream);
}

extern "C" int ofa_griffin_lim_inverse(const float* phase, const float* S, const float* window, const float* twiddle, const float* wss,
                                       int64_t wss_stride, const int32_t* lens, float* w_out, int B, int T, int n_fft, int win, int hop,
                                       void* stream) {
  const GlArgs a = {nullptr, phase, S, window, reinterpret_cast<const float2*>(twiddle), wss, wss_stride, lens, w_out, B, T, hop, 0};
  return gl_launch<true>("griffin_lim_inverse", a, n_fft, win, stream);
}

extern "C" int ofa_griffin_lim_specgram(const void* x, const float* pinv_t, float* S, int64_t rows, int n_mels, int n_freq, int dtype,
                                        void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "griffin_lim_specgram: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && rows <= (int64_t)0x7fffffff * GL_SPEC_ROWS && n_freq >= 1, OFA_ERR_INVALID, "griffin_lim_specgram: bad rows=%lld n_freq=%d",
              (long long)rows, n_freq);
  OFA_REQUIRE(n_mels >= 1 && n_mels <= GL_SPEC_MAX_MELS, OFA_ERR_UNSUPPORTED, "griffin_lim_specgram: n_mels=%d must be in 1..%d", n_mels,
              GL_SPEC_MAX_MELS);
  if (rows == 0) return OFA_OK;
  OFA_REQUIRE(x && pinv_t && S, OFA_ERR_INVALID, "griffin_lim_specgram: null operand");
  const dim3 grid(cdiv(rows, GL_SPEC_ROWS)), block(GL_THREADS);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((gl_specgram_kernel<T>), grid, block, 0, (hipStream_t)stream, (const T*)x, pinv_t, S, rows, n_mels, n_freq);
  });
  return check_launch("griffin_lim_specgram");
}

// Log-mel feature extraction (preprocessor/default/audio.py:297-328, 485-565 and utils/audio_utils.py:202-261 of the reference) and
// utterance CMVN, all in fp32: the mirror image of griffin_lim.hip -- frame, window, real FFT in LDS, mel.
//   lm_kernel<LOGN>   waveforms [B, Lmax] -> log-mel rows [B, Tmax, n_mels] in one launch.  Two front ends differ only by argument:
//       kaldi (torchaudio.compliance.kaldi.fbank at its defaults, dither 0): snip-edge frames of `win` samples every `shift`, per frame the
//             mean removed, pre-emphasis 0.97 with x[-1] := x[0], the povey window, zero padding to N, |X|^2, the HTK-mel triangles
//       tts   (extract_logmel_spectrogram): frames of N samples centred every `hop`, reflected about both ends of the utterance's own
//             length, the window padded to N, input scale 2^-15, |X|, Slaney's filters
//       A workgroup (4 waves) owns R consecutive frames of one utterance.
//         1. stage    the span of (R - 1) shift + N samples the R frames cover goes to LDS once: the reflected (tts) or zero (kaldi) ends
//                     element by element, the part that lies inside the utterance as float4 where the address allows; the scale is
//                     applied here.  Every sample is read from HBM once per workgroup; the overlapping frames are built from LDS.
//         2. frame    one wave builds one frame per round in its own buffer f [N]: (kaldi) the mean -- a lane sums its samples in
//                     ascending order, then the wave's DPP reduction, one fixed order -- and the pre-emphasis; times the window
//         3. forward  the real N-point transform as a complex FFT of M = N / 2 points (fft_wave.h), bit-reversed order out
//         4. split    lane k takes the pair (k, M - k): X_k and X_{M-k} as in griffin_lim.hip; their power (kaldi) or magnitude (tts) is
//                     held in registers until every lane has read its pair, then written over f in natural order, bins 0 .. M
//         5. mel      the filter bank has about two non-zeros per bin, so it comes compressed: per filter its first bin and an offset
//                     into one packed weight array.  A lane owns filters m and m + 64 (the narrowest with the widest) and sums its bins
//                     in ascending order in one fp32 fma chain; then log(max(E, floor)), the optional (y - mean[m]) / std[m], and the
//                     row is stored coalesced.
//       Rows at or beyond the utterance's own frame count are written as zeros.  No atomics: equal inputs give equal bits, and an
//       utterance gives the same bits alone and inside a ragged batch (the run partition, the span and every sum depend on it alone).
//       LDS: N floats of twiddles + 4 N of frame buffers + the span; `lm_run` keeps it within 64 KiB.
//   cmvn_kernel       UtteranceCMVN in place on [B, Tmax, F], one workgroup per utterance: column sums of x and x^2 in double (a thread
//                     sums its rows in ascending order, the row groups are folded through LDS in ascending order), then the second sweep.
#include "common.h"
#include "fft_wave.h"

namespace ofa {

constexpr int LM_THREADS = 256, LM_WAVES = 4;
constexpr int LM_LDS_BUDGET = 64 * 1024;
constexpr int LM_MAX_MELS = 128, LM_WANT_RUN = 16;
constexpr int LM_KALDI = 0, LM_TTS = 1;
constexpr float LM_PREEMPH = 0.97f;
constexpr int CMVN_MAX_FEAT = 256;

struct LmArgs {
  const float* wav;        // [B, Lmax]
  const int32_t* lens;     // [B] samples, or null
  const float* window;     // [N]  (kaldi: the first `win` entries)
  const float2* tw;        // [M]
  const int32_t* fstart;   // [n_mels]      first bin of filter m
  const int32_t* foff;     // [n_mels + 1]  its weights are fw[foff[m] .. foff[m + 1])
  const float* fw;         // [n_weights]
  const float* mean;       // [n_mels] or null
  const float* stdv;       // [n_mels] or null
  float* out;              // [B, Tmax, n_mels]
  int B, Lmax, Tmax, n_mels, n_weights, kind, win, shift, R;
  float scale, floor_;
};

__host__ __device__ inline int lm_frames(int kind, int L, int n_fft, int win, int shift) {
  if (kind == LM_KALDI) return L < win ? 0 : 1 + (L - win) / shift;
  return L > 0 ? 1 + L / shift : 0;
}

template <int LOGN> __global__ __launch_bounds__(LM_THREADS) void lm_kernel(LmArgs a) {
  constexpr int N = 1 << LOGN, M = N / 2, LOGM = LOGN - 1;
  constexpr int PAIRS = M / 2 > WAVE ? M / 2 / WAVE : 1;        // pairs (k, M - k), 1 <= k < M / 2, per lane
  extern __shared__ __attribute__((aligned(16))) float lm_smem[];
  float2* tw = reinterpret_cast<float2*>(lm_smem);              // [M]
  float* fbuf = lm_smem + N;                                    // [4][N]
  float* span = lm_smem + 5 * N;                                // [(R - 1) shift + N]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * a.R, shift = a.shift, win = a.win, n_mels = a.n_mels;
  const bool kaldi = a.kind == LM_KALDI;
  const int Lb = a.lens ? min(max(a.lens[b], 0), a.Lmax) : a.Lmax;
  const int Tb = min(lm_frames(a.kind, Lb, N, win, shift), a.Tmax);
  float* out = a.out + ((int64_t)b * a.Tmax + t0) * n_mels;
  const int rows = min(a.R, a.Tmax - t0), live = min(rows, Tb - t0);

  if (live > 0) {
    // 1. stage: span[i] = scale * w[s0 + i]; outside [0, Lb) zero (kaldi: no live frame reads it) or reflected (tts)
    const int n_span = (live - 1) * shift + N, s0 = t0 * shift - (kaldi ? 0 : M);
    const float* w = a.wav + (int64_t)b * a.Lmax;
    const float scale = a.scale;
    for (int i = tid; i < M; i += LM_THREADS) tw[i] = a.tw[i];
    const int lo = min(max(-s0, 0), n_span), hi = max(min(n_span, Lb - s0), lo);     // span[lo, hi) lies inside the utterance
    for (int i = tid; i < n_span - (hi - lo); i += LM_THREADS) {
      const int p = i < lo ? i : i + (hi - lo);
      float v = 0.f;
      if (!kaldi) {
        int s = s0 + p;
        s = s < 0 ? -s : 2 * (Lb - 1) - s;
        v = scale * w[min(max(s, 0), Lb - 1)];                  // (an utterance too short to reflect is refused by the caller: stay inside it)
      }
      span[p] = v;
    }
    const float* src = w + s0 + lo;                             // &w[s0 + lo], inside the row
    const int cnt = hi - lo;
    const int lead = min(cnt, (int)((4 - (((int64_t)b * a.Lmax + s0 + lo) & 3)) & 3));
    const int quads = (cnt - lead) / 4;
    for (int i = tid; i < lead; i += LM_THREADS) span[lo + i] = scale * src[i];
    for (int q = tid; q < quads; q += LM_THREADS) {
      const int i = lead + 4 * q;
      const float4 v = *reinterpret_cast<const float4*>(src + i);
      span[lo + i] = scale * v.x; span[lo + i + 1] = scale * v.y; span[lo + i + 2] = scale * v.z; span[lo + i + 3] = scale * v.w;
    }
    for (int i = lead + 4 * quads + tid; i < cnt; i += LM_THREADS) span[lo + i] = scale * src[i];
    __syncthreads();

    for (int r = wave; r < live; r += LM_WAVES) {
      float* f = fbuf + wave * N;
      float2* z = reinterpret_cast<float2*>(f);
      const float* x = span + r * shift;
      // 2. the frame
      if (kaldi) {
        float s = 0.f;
        for (int n = lane; n < win; n += WAVE) s += x[n];
        const float mu = wave_sum(s) / (float)win;
        for (int n = lane; n < N; n += WAVE) {
          float v = 0.f;
          if (n < win) v = ((x[n] - mu) - LM_PREEMPH * (x[n > 0 ? n - 1 : 0] - mu)) * a.window[n];
          f[n] = v;
        }
      } else {
        for (int n = lane; n < N; n += WAVE) f[n] = a.window[n] * x[n];
      }
      gl_wave_sync();
      // 3. forward
      gl_fft_forward<LOGM>(z, tw, lane);
      // 4. split: bins k and M - k from the pair (k, M - k) of the packed transform
      auto mag = [&](float2 v) -> float {
        const float p = v.x * v.x + v.y * v.y;
        return kaldi ? p : sqrtf(p);
      };
      float pa[PAIRS], pb[PAIRS];
#pragma unroll
      for (int it = 0; it < PAIRS; ++it) {
        const int k = lane + it * WAVE;                         // k = 0 (DC and Nyquist, both real) is done below
        const int kk = k > 0 && k < M / 2 ? k : 1;
        const int pk = (int)(__brev((unsigned)kk) >> (32 - LOGM)), pm = (int)(__brev((unsigned)(M - kk)) >> (32 - LOGM));
        const float2 zk = z[pk], zm = z[pm];
        const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
        const float2 O = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
        const float2 tO = gl_mul(tw[kk], O);
        pa[it] = mag(gl_add(E, tO));                            // X_k
        pb[it] = mag(gl_sub(E, tO));                            // |X_{M-k}| = |conj(E - w^k O)|
      }
      const float2 z0 = z[0], zh = z[1];                        // z[1] is point M / 2 in bit-reversed order: X_{M/2} = conj(z_{M/2})
      const float p0 = mag(make_float2(z0.x + z0.y, 0.f)), pM = mag(make_float2(z0.x - z0.y, 0.f)), ph = mag(zh);
      gl_wave_sync();
#pragma unroll
      for (int it = 0; it < PAIRS; ++it) {
        const int k = lane + it * WAVE;
        if (k > 0 && k < M / 2) {
          f[k] = pa[it];
          f[M - k] = pb[it];
        }
      }
      if (lane == 0) {
        f[0] = p0;
        f[M] = pM;
        f[M / 2] = ph;
      }
      gl_wave_sync();
      // 5. mel, log, the column normalisation
      for (int m = lane; m < n_mels; m += WAVE) {
        const int start = min(max(a.fstart[m], 0), M + 1), o0 = min(max(a.foff[m], 0), a.n_weights);
        const int cnt_m = min(min(a.foff[m + 1], a.n_weights) - o0, M + 1 - start);
        const float* fw = a.fw + o0;
        float acc = 0.f;
        for (int j = 0; j < cnt_m; ++j) acc = fmaf(fw[j], f[start + j], acc);
        float y = logf(fmaxf(acc, a.floor_));
        if (a.mean) y = (y - a.mean[m]) / a.stdv[m];
        out[(int64_t)r * n_mels + m] = y;
      }
      gl_wave_sync();                                           // (the next round writes f)
    }
  }
  // rows past the utterance's frames
  const int first = max(live, 0);
  for (int i = first * n_mels + tid; i < rows * n_mels; i += LM_THREADS) out[i] = 0.f;
}

// UtteranceCMVN: CW columns (a power of two >= F) by 256 / CW row groups
__global__ __launch_bounds__(LM_THREADS) void cmvn_kernel(float* __restrict__ x, const int32_t* __restrict__ frames, int Tmax, int F, int CW,
                                                          int norm_means, int norm_vars) {
  __shared__ double part[2][LM_THREADS];
  __shared__ double stat[2][CMVN_MAX_FEAT];
  const int tid = threadIdx.x, c = tid & (CW - 1), g = tid / CW, groups = LM_THREADS / CW;
  const int T = frames ? min(max(frames[blockIdx.x], 0), Tmax) : Tmax;
  if (T == 0) return;
  float* rows = x + (int64_t)blockIdx.x * Tmax * F;
  double s = 0.0, q = 0.0;
  if (c < F)
    for (int t = g; t < T; t += groups) {
      const double v = (double)rows[(int64_t)t * F + c];
      s += v;
      q += v * v;
    }
  part[0][tid] = s;
  part[1][tid] = q;
  __syncthreads();
  if (tid < F) {
    double ts = 0.0, tq = 0.0;
    for (int i = 0; i < groups; ++i) {
      ts += part[0][i * CW + tid];
      tq += part[1][i * CW + tid];
    }
    const double mean = ts / T, var = tq / T - mean * mean;
    stat[0][tid] = norm_means ? mean : 0.0;
    stat[1][tid] = norm_vars ? sqrt(var > 1e-10 ? var : 1e-10) : 1.0;
  }
  __syncthreads();
  const int64_t n = (int64_t)T * F;
  for (int64_t i = tid; i < n; i += LM_THREADS) {
    const int col = (int)(i % F);
    rows[i] = (float)(((double)rows[i] - stat[0][col]) / stat[1][col]);
  }
}

// ---------------------------------------------------------------- host side
static int lm_log2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return (1 << l) == n ? l : -1;
}

// Frames a workgroup owns; 0: the configuration is not served.  Sixteen frames (four rounds of the four waves) bring the staging to
// within 1.2x of reading every sample once at the usual overlaps; fewer, a multiple of four where that leaves any, when the span no longer fits.
static int lm_run(int kind, int n_fft, int win, int shift) {
  const int l = lm_log2(n_fft);
  if ((kind != LM_KALDI && kind != LM_TTS) || l < 8 || l > 11 || win < 1 || win > n_fft || shift < 1 || shift > n_fft) return 0;
  const int room = (LM_LDS_BUDGET / 4 - 6 * n_fft) / shift + 1;
  const int r = LM_WANT_RUN < room ? LM_WANT_RUN : room;
  return r >= LM_WAVES ? r - r % LM_WAVES : r;
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_logmel_run(int kind, int n_fft, int win, int shift) { return lm_run(kind, n_fft, win, shift); }

extern "C" int ofa_logmel_fwd(const float* wav, const int32_t* lens, const float* window, const float* twiddle, const int32_t* filt_start,
                              const int32_t* filt_off, const float* filt_w, const float* cmvn_mean, const float* cmvn_std, float* out, int B,
                              int Lmax, int Tmax, int n_mels, int n_weights, int kind, int n_fft, int win, int shift, void* stream) {
  LmArgs a = {wav, lens, window, reinterpret_cast<const float2*>(twiddle), filt_start, filt_off, filt_w, cmvn_mean, cmvn_std, out,
              B, Lmax, Tmax, n_mels, n_weights, kind, win, shift, 0, kind == LM_TTS ? 1.0f / 32768.0f : 1.0f, kind == LM_TTS ? 1e-5f : 1.1920929e-07f};
  a.R = lm_run(kind, n_fft, win, shift);
  OFA_REQUIRE(a.R > 0, OFA_ERR_UNSUPPORTED,
              "logmel_fwd: kind=%d must be 0 (kaldi) or 1 (tts), n_fft=%d a power of two in 256..2048 with win=%d <= n_fft and 1 <= shift=%d <= n_fft",
              kind, n_fft, win, shift);
  OFA_REQUIRE(n_mels >= 1 && n_mels <= LM_MAX_MELS, OFA_ERR_UNSUPPORTED, "logmel_fwd: n_mels=%d must be in 1..%d", n_mels, LM_MAX_MELS);
  OFA_REQUIRE(B >= 0 && B <= 65535 && Lmax >= 0 && Tmax >= 0 && n_weights >= 0, OFA_ERR_INVALID, "logmel_fwd: bad B=%d Lmax=%d Tmax=%d n_weights=%d", B,
              Lmax, Tmax, n_weights);
  OFA_REQUIRE(Tmax <= lm_frames(kind, Lmax, n_fft, win, shift), OFA_ERR_INVALID, "logmel_fwd: Lmax=%d samples give fewer than Tmax=%d frames", Lmax, Tmax);
  OFA_REQUIRE((int64_t)Tmax * shift + n_fft <= 0x7fffffff, OFA_ERR_UNSUPPORTED, "logmel_fwd: Tmax=%d frames at shift=%d are too many", Tmax, shift);
  OFA_REQUIRE((cmvn_mean == nullptr) == (cmvn_std == nullptr), OFA_ERR_INVALID, "logmel_fwd: cmvn_mean and cmvn_std come together");
  if (B == 0 || Tmax == 0) return OFA_OK;
  OFA_REQUIRE(wav && window && twiddle && filt_start && filt_off && filt_w && out, OFA_ERR_INVALID, "logmel_fwd: null operand");
  OFA_REQUIRE(aligned16(wav), OFA_ERR_UNSUPPORTED, "logmel_fwd: wav must be 16-byte aligned");
  const int lds = 4 * (6 * n_fft + (a.R - 1) * shift);
  const dim3 grid(cdiv(Tmax, a.R), B), block(LM_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (lm_log2(n_fft)) {
    case 8: hipLaunchKernelGGL((lm_kernel<8>), grid, block, lds, st, a); break;
    case 9: hipLaunchKernelGGL((lm_kernel<9>), grid, block, lds, st, a); break;
    case 10: hipLaunchKernelGGL((lm_kernel<10>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((lm_kernel<11>), grid, block, lds, st, a); break;
  }
  return check_launch("logmel_fwd");
}

extern "C" int ofa_utterance_cmvn(float* x, const int32_t* frames, int B, int Tmax, int n_feat, int norm_means, int norm_vars, void* stream) {
  OFA_REQUIRE(B >= 0 && Tmax >= 0, OFA_ERR_INVALID, "utterance_cmvn: bad B=%d Tmax=%d", B, Tmax);
  OFA_REQUIRE(n_feat >= 1 && n_feat <= CMVN_MAX_FEAT, OFA_ERR_UNSUPPORTED, "utterance_cmvn: n_feat=%d must be in 1..%d", n_feat, CMVN_MAX_FEAT);
  if (B == 0 || Tmax == 0 || (!norm_means && !norm_vars)) return OFA_OK;
  OFA_REQUIRE(x, OFA_ERR_INVALID, "utterance_cmvn: null operand");
  int cw = 32;
  while (cw < n_feat) cw *= 2;
  hipLaunchKernelGGL(cmvn_kernel, dim3(B), dim3(LM_THREADS), 0, (hipStream_t)stream, x, frames, Tmax, n_feat, cw, norm_means, norm_vars);
  return check_launch("utterance_cmvn");
}

// Mel-cepstral-distortion evaluation (task/text_to_speech.py:128-295 of the reference), fp32 throughout, no atomics, nothing read on the host.
//   dtw_kernel<FEAT, C, DT>   dynamic time warping of a ragged batch of pairs in ONE launch; pair b is shapes[b] = (M_b, N_b), read here.
//       cum[0][j] and cum[i][0] are running sums in index order, elsewhere cum[i][j] = d[i][j] + min(left, up-left, up); the back pointer
//       is 0 = left, 1 = up-left, 2 = up, the LOWEST code on a tie (bp[0][j > 0] = 0, bp[i][0] = 2).  The length of the chosen path is
//       carried with cum (len[0][0] = 1, len = len[pred] + 1), so total = cum[M-1][N-1] and pathlen = len[M-1][N-1] need no backtrace.
//       FEAT = false: d is read from [B, maxM, maxN].  FEAT = true: d is computed from x1 [B, maxM, ld] and x2 [B, maxN, ld] (D <= 16 features
//       a row): sum_k (a_k - b_k)^2 in index order, rms: sqrtf(that / D); the [B, M, N] tensor is never formed.
//       One workgroup (4 waves) per pair.  Lane l owns the strip of C consecutive columns [l C, l C + C); its x2 rows sit in registers.  The
//       work is cut into register tiles of R = 4 rows x C columns, computed cell by cell inside the lane, and the wavefront runs over TILES:
//       at step s lane l computes tile t = s - l, so a pair costs ceil(M / 4) + ceil(N / C) - 1 steps instead of M + N - 1.
//         what travels   a tile's right edge (4 values of cum and len) goes to the next lane by DPP wave_shr:1 -- a VALU operand, no LDS
//                        round trip -- and from lane 63 of a wave to lane 0 of the next through a double-buffered LDS ring; one barrier a
//                        step.  The corner a tile needs is the last edge value of the step before, which the lane already holds.
//         x1             staged once in LDS feature-major, x1T[k][i]: a tile's 4 rows of feature k are ONE 16-byte read, and neighbouring
//                        lanes (tiles t, t - 1, ...) read neighbouring 16 bytes -- no bank conflict.  D * maxM * 4 bytes: 128 KiB at D = 16 and
//                        2048 rows, which is why this form serves M, N <= 2048.
//         d (FEAT false) the next tile's R x C distances are loaded one step ahead, as float4 where the row pitch allows.
//         cum / backptr  optional outputs (NULL: not written): a tile row is stored as float4 / one packed word where the pitch allows; stores
//                        are not waited for.  Cells outside [:M_b, :N_b] are left UNWRITTEN (lanes beyond the pair compute on zeros and
//                        store nothing; nothing in range depends on them).
//   dtw_backtrace_kernel      backptr + shapes -> path [B, maxM + maxN - 1, 2] from (0, 0) to (M_b - 1, N_b - 1), front-aligned, and its count.
//       One wave per pair.  A round fetches the 8 x 8 window of back pointers whose bottom-right cell is the current one (one byte a lane),
//       then walks inside it by v_readlane -- at least 8 path cells per memory round trip instead of one.  The cells go to LDS in walking
//       order and are written out reversed, coalesced.  Pointers are clamped (row 0 goes left, column 0 goes up): garbage cannot leave the matrix.
//   mfcc_rows_kernel          power spectrum rows [rows, n_bins] -> [rows, 16]: 13 MFCCs and 3 zeros.  A wave owns a row: staged in LDS, the
//       mel sums through the compressed filter bank of audio_features.hip (lane m and m + 64, bins ascending, one fma chain), log(mel + 1e-6)
//       kept in LDS -- no [rows, n_mels] intermediate in HBM -- and the orthonormal DCT-II rows, a lane each: four interleaved fma chains (n mod 4)
//       in n order, added as (0 + 1) + (2 + 3).
#include "common.h"
#include "fft_wave.h"

namespace ofa {

constexpr int DTW_THREADS = 256, DTW_WAVES = 4, DTW_R = 4;
constexpr int DTW_MAX_D = 16, DTW_FEAT_MAX = 2048, DTW_DIST_MAX = 4096;
constexpr int BT_WIN = 8, BT_MAX_PATH = 2 * DTW_DIST_MAX - 1;
constexpr int MFCC_THREADS = 256, MFCC_WAVES = 4, MFCC_ROWS = 16, MFCC_OUT = 16, MFCC_MAX_MELS = 128, MFCC_MAX_BINS = 2049;

struct DtwArgs {
  const float* d;          // [B, maxM, maxN]        (FEAT false)
  const float* x1;         // [B, maxM, ld]          (FEAT true)
  const float* x2;         // [B, maxN, ld]
  const int32_t* shapes;   // [B, 2]
  float* total;            // [B]
  int32_t* pathlen;        // [B]
  float* cum;              // [B, maxM, maxN] or null
  uint8_t* bp;             // [B, maxM, maxN] or null
  int B, maxM, maxN, D, ld, rms, vec;
};

// lane i receives lane i - 1's value (lane 0 keeps its own)
template <typename T> __device__ __forceinline__ T dtw_from_left(T v) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

template <bool FEAT, int C, int DT> __global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(DtwArgs a) {
  constexpr int R = DTW_R;
  extern __shared__ __attribute__((aligned(16))) float dtw_x1t[];           // [DT][P]
  __shared__ float ring_c[2][DTW_WAVES][R];
  __shared__ int ring_l[2][DTW_WAVES][R];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), b = blockIdx.x;
  const int M = min(max(a.shapes[2 * b], 0), a.maxM), N = min(max(a.shapes[2 * b + 1], 0), a.maxN);
  if (M == 0 || N == 0) {
    if (tid == 0) {
      a.total[b] = 0.f;
      a.pathlen[b] = 0;
    }
    return;
  }
  const int T = (M + R - 1) / R, nl = (N + C - 1) / C, j0 = tid * C, P = (a.maxM + 3) & ~3;
  const float INF = __builtin_inff();
  const int64_t cell0 = (int64_t)b * a.maxM * a.maxN;
  const bool vec = a.vec != 0;

  float xb[FEAT ? C : 1][FEAT ? DT : 1];
  if (FEAT) {
    const float* x1 = a.x1 + (int64_t)b * a.maxM * a.ld;
    for (int idx = tid; idx < P * DT; idx += DTW_THREADS) {
      const int i = idx / DT, k = idx - i * DT;
      dtw_x1t[k * P + i] = (i < M && k < a.D) ? x1[(int64_t)i * a.ld + k] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < DT; ++k) xb[c][k] = (j0 + c < N && k < a.D) ? a.x2[((int64_t)b * a.maxN + j0 + c) * a.ld + k] : 0.f;
    __syncthreads();
  }

  // FEAT false: the R x C distances of tile tt of this lane (zeros outside the pair)
  float dn[FEAT ? 1 : R][FEAT ? 1 : C];
  auto load_tile = [&](int tt) {
    if (FEAT) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = tt * R + r;
      const bool row = tt >= 0 && i < M && tid < nl;
      const float* src = a.d + cell0 + (int64_t)(row ? i : 0) * a.maxN;
#pragma unroll
      for (int c = 0; c < C; c += 4) {
        if (vec && row && j0 + c + 3 < a.maxN) {
          const float4 v = *reinterpret_cast<const float4*>(src + j0 + c);
          dn[r][c] = v.x; dn[r][c + 1] = v.y; dn[r][c + 2] = v.z; dn[r][c + 3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) dn[r][c + e] = (row && j0 + c + e < N) ? src[j0 + c + e] : 0.f;
        }
      }
    }
  };
  load_tile(-tid);

  float prev[C], E[R], corner = INF;
  int plen[C], El[R], cornerl = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) prev[c] = INF, plen[c] = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) E[r] = INF, El[r] = 0;
  const float fD = (float)a.D;

  const int steps = T + nl - 1;
  for (int s = 0; s < steps; ++s) {
    // the wave holds tiles s - 64 wave - 63 .. s - 64 wave: idle before its first lane starts and after its last one ends
    const bool wave_on = s - wave * 64 >= 0 && s - wave * 64 - 63 < T && wave * 64 < nl;
    float dc[FEAT ? 1 : R][FEAT ? 1 : C];
    if (!FEAT) {                                                  // (every step, idle waves too: a wave's first tile is loaded the step before)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) dc[r][c] = dn[r][c];
      load_tile(s + 1 - tid);
    }
    if (wave_on) {
      const int t = s - tid;
      const bool act = t >= 0 && t < T && tid < nl;
      float L[R];
      int Ll[R];
#pragma unroll
      for (int r = 0; r < R; ++r) L[r] = dtw_from_left(E[r]), Ll[r] = dtw_from_left(El[r]);
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          L[r] = wave == 0 ? INF : ring_c[(s - 1) & 1][wave - 1][r];
          Ll[r] = wave == 0 ? 0 : ring_l[(s - 1) & 1][wave - 1][r];
        }
      }
      if (t <= 0) {                                               // a lane's first tile starts from nothing above it
        corner = INF, cornerl = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) prev[c] = INF, plen[c] = 0;
      }
      const int i0 = act ? t * R : 0;
      float xa[FEAT ? DT : 1][FEAT ? R : 1];
      if (FEAT) {
#pragma unroll
        for (int k = 0; k < DT; ++k) {
          const float4 v = *reinterpret_cast<const float4*>(dtw_x1t + k * P + i0);
          xa[k][0] = v.x; xa[k][1] = v.y; xa[k][2] = v.z; xa[k][3] = v.w;
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = i0 + r;
        float left = L[r], diag = r == 0 ? corner : L[r - 1];
        int leftl = Ll[r], diagl = r == 0 ? cornerl : Ll[r - 1];
        float rowv[C];
        uint32_t rowc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float d;
          if (FEAT) {
            d = 0.f;
#pragma unroll
            for (int k = 0; k < DT; ++k) {
              const float df = xa[k][r] - xb[c][k];
              d = fmaf(df, df, d);
            }
            if (a.rms) d = sqrtf(d / fD);
          } else {
            d = dc[r][c];
          }
          const float up = prev[c];
          const int upl = plen[c];
          float best = left;
          int bl = leftl, code = 0;
          if (diag < best) best = diag, bl = diagl, code = 1;
          if (up < best) best = up, bl = upl, code = 2;
          if (c == 0 && (i | tid) == 0) best = 0.f, bl = 0, code = 2;         // cell (0, 0)
          const float nv = d + best;
          diag = up, diagl = upl;
          prev[c] = left = nv;
          plen[c] = leftl = bl + 1;
          rowv[c] = nv;
          rowc[c] = (uint32_t)code;
        }
        E[r] = left, El[r] = leftl;
        if (act && i < M) {
          if (i == M - 1 && N - 1 >= j0 && N - 1 < j0 + C) {
#pragma unroll
            for (int c = 0; c < C; ++c)
              if (j0 + c == N - 1) a.total[b] = rowv[c], a.pathlen[b] = plen[c];
          }
          const int64_t at = cell0 + (int64_t)i * a.maxN + j0;
          const bool whole = vec && j0 + C <= N;
          if (a.cum) {
            if (whole) {
#pragma unroll
              for (int c = 0; c < C; c += 4) *reinterpret_cast<float4*>(a.cum + at + c) = make_float4(rowv[c], rowv[c + 1], rowv[c + 2], rowv[c + 3]);
            } else {
#pragma unroll
              for (int c = 0; c < C; ++c)
                if (j0 + c < N) a.cum[at + c] = rowv[c];
            }
          }
          if (a.bp) {
            if (whole) {
#pragma unroll
              for (int c = 0; c < C; c += 4)
                *reinterpret_cast<uint32_t*>(a.bp + at + c) = rowc[c] | (rowc[c + 1] << 8) | (rowc[c + 2] << 16) | (rowc[c + 3] << 24);
            } else {
#pragma unroll
              for (int c = 0; c < C; ++c)
                if (j0 + c < N) a.bp[at + c] = (uint8_t)rowc[c];
            }
          }
        }
      }
      corner = L[R - 1], cornerl = Ll[R - 1];
      if (lane == 63) {
#pragma unroll
        for (int r = 0; r < R; ++r) ring_c[s & 1][wave][r] = E[r], ring_l[s & 1][wave][r] = El[r];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- backtrace
__global__ __launch_bounds__(64) void dtw_backtrace_kernel(const uint8_t* __restrict__ bp, const int32_t* __restrict__ shapes, int32_t* __restrict__ path,
                                                           int32_t* __restrict__ count, int maxM, int maxN) {
  __shared__ uint32_t cells[BT_MAX_PATH];                        // (i << 16) | j in walking order, (M-1, N-1) first
  const int lane = threadIdx.x, b = blockIdx.x;
  const int M = min(max(shapes[2 * b], 0), maxM), N = min(max(shapes[2 * b + 1], 0), maxN);
  if (M == 0 || N == 0) {
    if (lane == 0) count[b] = 0;
    return;
  }
  const uint8_t* src = bp + (int64_t)b * maxM * maxN;
  const int wi = lane / BT_WIN, wj = lane % BT_WIN;
  int i = M - 1, j = N - 1, k = 0;
  bool done = false;
  while (!done) {
    const int ci = i - wi, cj = j - wj;
    int code = (ci >= 0 && cj >= 0) ? (int)src[(int64_t)ci * maxN + cj] : 0;
    code = ci <= 0 ? 0 : (cj <= 0 ? 2 : min(code, 2));            // row 0 goes left, column 0 goes up
    int di = 0, dj = 0;
    while (di < BT_WIN && dj < BT_WIN) {
      if (lane == 0) cells[k] = ((uint32_t)(i - di) << 16) | (uint32_t)(j - dj);
      ++k;
      if (i - di == 0 && j - dj == 0) {
        done = true;
        break;
      }
      const int step = __builtin_amdgcn_readlane(code, __builtin_amdgcn_readfirstlane(di * BT_WIN + dj));
      di += step >= 1;
      dj += step <= 1;
    }
    i -= di, j -= dj;
  }
  __syncthreads();
  int32_t* out = path + (int64_t)b * (maxM + maxN - 1) * 2;
  for (int e = lane; e < k; e += 64) {
    const uint32_t v = cells[k - 1 - e];
    reinterpret_cast<int2*>(out)[e] = make_int2((int)(v >> 16), (int)(v & 0xffffu));
  }
  if (lane == 0) count[b] = k;
}

// ---------------------------------------------------------------- MFCC rows
struct MfccArgs {
  const float* power;      // [rows, n_bins]
  const int32_t* fstart;   // [n_mels]
  const int32_t* foff;     // [n_mels + 1]
  const float* fw;         // [n_weights]
  const float* dct;        // [n_mfcc, n_mels]
  float* out;              // [rows, 16]
  int64_t rows;
  int n_bins, n_mels, n_weights, n_mfcc;
};

__global__ __launch_bounds__(MFCC_THREADS) void mfcc_rows_kernel(MfccArgs a) {
  extern __shared__ __attribute__((aligned(16))) float mfcc_smem[];
  float* dct = mfcc_smem;                                        // [n_mfcc][n_mels]
  float* logmel = dct + MFCC_OUT * MFCC_MAX_MELS;                // [4][MFCC_MAX_MELS]
  float* spec = logmel + MFCC_WAVES * MFCC_MAX_MELS;             // [4][n_bins]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < a.n_mfcc * a.n_mels; i += MFCC_THREADS) dct[i] = a.dct[i];
  __syncthreads();
  float* f = spec + wave * a.n_bins;
  float* lm = logmel + wave * MFCC_MAX_MELS;
  const int64_t row0 = (int64_t)blockIdx.x * MFCC_ROWS;
  for (int r = wave; r < MFCC_ROWS && row0 + r < a.rows; r += MFCC_WAVES) {
    const float* p = a.power + (row0 + r) * a.n_bins;
    for (int n = lane; n < a.n_bins; n += WAVE) f[n] = p[n];
    gl_wave_sync();
    for (int m = lane; m < a.n_mels; m += WAVE) {
      const int start = min(max(a.fstart[m], 0), a.n_bins), o0 = min(max(a.foff[m], 0), a.n_weights);
      const int cnt = min(min(a.foff[m + 1], a.n_weights) - o0, a.n_bins - start);
      const float* fw = a.fw + o0;
      float acc = 0.f;
      for (int j = 0; j < cnt; ++j) acc = fmaf(fw[j], f[start + j], acc);
      lm[m] = logf(acc + 1e-6f);
    }
    gl_wave_sync();
    if (lane < MFCC_OUT) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;               // four interleaved chains: a fraction of one chain's rounding error
      if (lane < a.n_mfcc) {
        const float* w = dct + lane * a.n_mels;
        int n = 0;
        for (; n + 3 < a.n_mels; n += 4) {
          a0 = fmaf(w[n], lm[n], a0);
          a1 = fmaf(w[n + 1], lm[n + 1], a1);
          a2 = fmaf(w[n + 2], lm[n + 2], a2);
          a3 = fmaf(w[n + 3], lm[n + 3], a3);
        }
        if (n < a.n_mels) a0 = fmaf(w[n], lm[n], a0);
        if (n + 1 < a.n_mels) a1 = fmaf(w[n + 1], lm[n + 1], a1);
        if (n + 2 < a.n_mels) a2 = fmaf(w[n + 2], lm[n + 2], a2);
      }
      a.out[(row0 + r) * MFCC_OUT + lane] = (a0 + a1) + (a2 + a3);
    }
    gl_wave_sync();                                              // (the next round writes f and lm)
  }
}

// ---------------------------------------------------------------- host side
static int dtw_strip(int feat, int maxN, int strip) {
  const int widest = feat ? 8 : 16;
  if (strip == 0) strip = maxN <= 4 * DTW_THREADS ? 4 : (maxN <= 8 * DTW_THREADS ? 8 : 16);
  if ((strip != 4 && strip != 8 && strip != 16) || strip > widest || (int64_t)strip * DTW_THREADS < maxN) return 0;
  return strip;
}

template <bool FEAT, int C, int DT> static void dtw_launch(const DtwArgs& a, int lds, hipStream_t st) {
  auto kern = dtw_kernel<FEAT, C, DT>;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(DTW_THREADS), lds, st, a);
}

}  // namespace ofa
using namespace ofa;

extern "C" int ofa_dtw_strip(int features, int maxN, int strip) { return dtw_strip(features, maxN, strip); }

extern "C" int ofa_dtw(const float* distance, const float* x1, const float* x2, const int32_t* shapes, float* total, int32_t* pathlen, float* cumdist,
                       uint8_t* backptr, int B, int maxM, int maxN, int D, int ld, int metric, int strip, int dtype, void* stream) {
  const bool feat = distance == nullptr;
  OFA_REQUIRE(dtype == OFA_F32, OFA_ERR_UNSUPPORTED, "dtw: dtype=%d is not served, fp32 (0) only", dtype);
  OFA_REQUIRE(B >= 0 && maxM >= 0 && maxN >= 0, OFA_ERR_INVALID, "dtw: bad B=%d maxM=%d maxN=%d", B, maxM, maxN);
  OFA_REQUIRE(feat ? (x1 != nullptr) == (x2 != nullptr) : (x1 == nullptr && x2 == nullptr), OFA_ERR_INVALID,
              "dtw: give either distance or both x1 and x2");
  if (feat) {
    OFA_REQUIRE(D >= 1 && D <= DTW_MAX_D && ld >= D, OFA_ERR_UNSUPPORTED, "dtw: D=%d features (row pitch ld=%d) must be in 1..%d with ld >= D", D, ld,
                DTW_MAX_D);
    OFA_REQUIRE(metric == 0 || metric == 1, OFA_ERR_INVALID, "dtw: metric=%d must be 0 (l2) or 1 (rms)", metric);
    OFA_REQUIRE(maxM <= DTW_FEAT_MAX && maxN <= DTW_FEAT_MAX, OFA_ERR_UNSUPPORTED,
                "dtw: the features form serves M, N <= %d (x1 stays in LDS), got maxM=%d maxN=%d", DTW_FEAT_MAX, maxM, maxN);
  } else {
    OFA_REQUIRE(maxM <= DTW_DIST_MAX && maxN <= DTW_DIST_MAX, OFA_ERR_UNSUPPORTED, "dtw: the distance form serves M, N <= %d, got maxM=%d maxN=%d",
                DTW_DIST_MAX, maxM, maxN);
  }
  const int C = dtw_strip(feat, maxN, strip);
  OFA_REQUIRE(C > 0, OFA_ERR_UNSUPPORTED, "dtw: strip=%d must be 0 (chosen here), 4, 8 or 16 (distance form) with 256 strips covering maxN=%d", strip, maxN);
  if (B == 0 || maxM == 0 || maxN == 0) return OFA_OK;
  OFA_REQUIRE(shapes && total && pathlen && (feat ? x1 != nullptr : true), OFA_ERR_INVALID, "dtw: null operand");
  DtwArgs a = {distance, x1, x2, shapes, total, pathlen, cumdist, backptr, B, maxM, maxN, D, ld, metric, 0};
  a.vec = maxN % 4 == 0 && aligned16(distance) && aligned16(cumdist) && ((uintptr_t)backptr & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (feat) {
    const int DT = D == 13 ? 13 : DTW_MAX_D, lds = DT * ((maxM + 3) & ~3) * 4;
    if (C == 4 && DT == 13) dtw_launch<true, 4, 13>(a, lds, st);
    else if (C == 4) dtw_launch<true, 4, 16>(a, lds, st);
    else if (DT == 13) dtw_launch<true, 8, 13>(a, lds, st);
    else dtw_launch<true, 8, 16>(a, lds, st);
  } else {
    if (C == 4) dtw_launch<false, 4, 1>(a, 0, st);
    else if (C == 8) dtw_launch<false, 8, 1>(a, 0, st);
    else dtw_launch<false, 16, 1>(a, 0, st);
  }
  return check_launch("dtw");
}

extern "C" int ofa_dtw_backtrace(const uint8_t* backptr, const int32_t* shapes, int32_t* path, int32_t* count, int B, int maxM, int maxN, void* stream) {
  OFA_REQUIRE(B >= 0 && maxM >= 0 && maxN >= 0, OFA_ERR_INVALID, "dtw_backtrace: bad B=%d maxM=%d maxN=%d", B, maxM, maxN);
  OFA_REQUIRE(maxM <= DTW_DIST_MAX && maxN <= DTW_DIST_MAX, OFA_ERR_UNSUPPORTED, "dtw_backtrace: serves M, N <= %d, got maxM=%d maxN=%d", DTW_DIST_MAX,
              maxM, maxN);
  if (B == 0 || maxM == 0 || maxN == 0) return OFA_OK;
  OFA_REQUIRE(backptr && shapes && path && count, OFA_ERR_INVALID, "dtw_backtrace: null operand");
  hipLaunchKernelGGL(dtw_backtrace_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, backptr, shapes, path, count, maxM, maxN);
  return check_launch("dtw_backtrace");
}

extern "C" int ofa_mfcc_rows(const float* power, const int32_t* filt_start, const int32_t* filt_off, const float* filt_w, const float* dct, float* out,
                             int64_t rows, int n_bins, int n_mels, int n_weights, int n_mfcc, int dtype, void* stream) {
  OFA_REQUIRE(dtype == OFA_F32, OFA_ERR_UNSUPPORTED, "mfcc_rows: dtype=%d is not served, fp32 (0) only", dtype);
  OFA_REQUIRE(n_mfcc >= 1 && n_mfcc <= MFCC_OUT && n_mels >= n_mfcc && n_mels <= MFCC_MAX_MELS, OFA_ERR_UNSUPPORTED,
              "mfcc_rows: n_mfcc=%d must be in 1..%d and n_mels=%d in n_mfcc..%d", n_mfcc, MFCC_OUT, n_mels, MFCC_MAX_MELS);
  OFA_REQUIRE(n_bins >= 1 && n_bins <= MFCC_MAX_BINS, OFA_ERR_UNSUPPORTED, "mfcc_rows: n_bins=%d must be in 1..%d", n_bins, MFCC_MAX_BINS);
  OFA_REQUIRE(rows >= 0 && rows <= (int64_t)0x7fffffff * MFCC_ROWS && n_weights >= 0, OFA_ERR_INVALID, "mfcc_rows: bad rows=%lld n_weights=%d",
              (long long)rows, n_weights);
  if (rows == 0) return OFA_OK;
  OFA_REQUIRE(power && filt_start && filt_off && filt_w && dct && out, OFA_ERR_INVALID, "mfcc_rows: null operand");
  MfccArgs a = {power, filt_start, filt_off, filt_w, dct, out, rows, n_bins, n_mels, n_weights, n_mfcc};
  const int lds = 4 * (MFCC_OUT * MFCC_MAX_MELS + MFCC_WAVES * MFCC_MAX_MELS + MFCC_WAVES * n_bins);
  hipLaunchKernelGGL(mfcc_rows_kernel, dim3(cdiv(rows, MFCC_ROWS)), dim3(MFCC_THREADS), lds, (hipStream_t)stream, a);
  return check_launch("mfcc_rows");
}

// CTC loss on the encoder output (engine/criterion/speech_to_text_loss.py:217-225, 326-362: F.ctc_loss(log_softmax(x), blank = 0,
// reduction = "sum", zero_infinity) on x = enc . W[ds:de]^T), forward and gradient, without float atomics and without a host sync.
// A sentence b is the rows  seg[b].off + t * row_stride,  t < seg[b].len  of the logits [rows, C] -- the padded T x B x C encoder output
// (off = b, stride = B) and the packed [rows, C] form (off = q_off, stride = 1) alike.  Its labels are encoder_target[b, :] - ds at the
// positions that are neither pad nor eos, compacted in order by the kernel; S = 2 L + 1 extended states l' = (0, l_1, 0, l_2, ..., 0).
//   ctc_row_kernel    one wave per row: lse[r] = log sum_c exp x[r, c] and the arg-max class (lowest index among equals)
//   ctc_ab_kernel     grid 2 B: workgroup 2 b runs alpha of sentence b, workgroup 2 b + 1 runs beta, in fp32 log space on lp = x - lse,
//                     a thread owning NS states, the previous time step's row in LDS, one barrier per step; both store their [T, S] slab
//   ctc_grad_kernel   one workgroup per live row: d[r, c] = seed * (exp(lp_c) - sum_{s: l'_s = c} exp(alpha_s + beta_s - lp_c + nll))
// The sum over the states of a class runs in a fixed order: the blanks per thread, then a DPP wave sum, then the four waves in wave order;
// the occurrences of a label by ONE thread in target order, along the chain `next` that the alpha workgroup built.  Equal inputs give
// equal bits.  Precision: exp / log run in fp32 on differences of size O(1); what is ADDED up along the T steps -- lse, lp, alpha, beta, nll,
// quantities of the size of the loss -- is kept in fp64 (LDS rows and slabs included), so a step costs a few fp64 adds and the result does
// not carry one fp32 rounding of a number of size |loss| per time step.
// Edge cases: a segment description that leaves [0, rows) or exceeds Tmax is read as an EMPTY sentence (nll 0 without labels, +inf with:
// no wild address, but no other signal either); a row whose logits are all -inf has lse = -inf and its lp, and what follows, is NaN.
// A label outside [1, C) makes its sentence infeasible, as a target longer than the input does: nll = +inf (0 with
// zero_infinity), gradient rows NaN (exactly 0 with zero_infinity) -- torch's values.
#include "common.h"

namespace ofa {

constexpr int CTC_THREADS = 256;
constexpr int CTC_PF = 4;                 // time steps whose emissions are in flight ahead of the barrier chain
constexpr int CTC_MAX_NS = 9;             // states per thread of the widest recursion kernel: S <= 2304
constexpr int CTC_MAX_C = 8192;           // classes: the gradient kernel keeps one float per class in LDS

struct CtcSeg {
  const int32_t* seg;                     // [B, seg_ld]: (row offset, length) in columns 0 and 1
  int seg_ld;
  int64_t row_stride, rows;
  int Tmax;
};

// (offset, length) of sentence b; a description that would leave [0, rows) or exceed Tmax reads as an empty sentence
__device__ __forceinline__ void ctc_segment(const CtcSeg& g, int b, int64_t& off, int& len) {
  off = g.seg[(int64_t)b * g.seg_ld];
  len = g.seg[(int64_t)b * g.seg_ld + 1];
  if (off < 0 || len < 0 || len > g.Tmax || (len > 0 && off + (int64_t)(len - 1) * g.row_stride >= g.rows)) len = 0;
}

// log(exp a + exp b + exp c); all -inf gives -inf, not NaN.  The maximum is taken off in fp64, the three differences (<= 0) go through
// fp32 exp / log, and the result (<= log 3) is added back in fp64.
__device__ __forceinline__ double lae3(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + (double)logf(expf((float)(a - m)) + expf((float)(b - m)) + expf((float)(c - m)));
}

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_row_kernel(const T* __restrict__ x, int64_t ld, int64_t rows, int C,
                                                              double* __restrict__ row_lse, int32_t* __restrict__ row_argmax) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (CTC_THREADS / WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;                                  // (wave-uniform)
  const T* xr = x + row * ld;
  float m = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += WAVE) {
    const float v = ld1<T>(xr + c);
    if (v > m) { m = v; bi = c; }                           // (ascending c: the first of equals stays)
  }
  const float M = wave_max(m);
  int iw = m == M ? bi : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) iw = min(iw, __shfl_xor(iw, o, 64));
  float s = 0.f;
  if (M > -INFINITY)
    for (int c = lane; c < C; c += WAVE) s += expf(ld1<T>(xr + c) - M);
  s = wave_sum(s);
  if (lane == 0) {
    row_lse[row] = M > -INFINITY ? (double)M + (double)logf(s) : -INFINITY;
    if (row_argmax) row_argmax[row] = iw == 0x7fffffff ? 0 : iw;
  }
}

// The labels of sentence b into lab[0 .. L): wave 0 walks the target row in 64-position trips and compacts with a ballot.  Returns (to
// every thread, after a barrier) L, or -1 if a label lies outside [1, C).
__device__ __forceinline__ int ctc_labels(const int64_t* __restrict__ tgt, int Lmax, int64_t ds, int64_t pad, int64_t eos, int C, int* lab,
                                          int* sh) {
  if (threadIdx.x < WAVE) {
    const int lane = threadIdx.x;
    int base = 0, bad = 0;
    for (int p0 = 0; p0 < Lmax; p0 += WAVE) {
      const int p = p0 + lane;
      const int64_t v = p < Lmax ? tgt[p] : pad;
      const bool keep = p < Lmax && v != pad && v != eos;
      const uint64_t mask = __ballot(keep);
      if (keep) {
        const int64_t l = v - ds;
        bad |= l < 1 || l >= C;
        lab[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int)l;
      }
      base += __popcll(mask);
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) { sh[0] = base; sh[1] = bad; }
  }
  __syncthreads();
  return sh[1] ? -1 : sh[0];
}

// ws_meta: int32 [B, 3, Lmax] = (labels, next occurrence of the same label or -1, "first occurrence"), ws_L: int32 [B] (-1: a bad label).
template <typename T, int NS>
__global__ __launch_bounds__(CTC_THREADS) void ctc_ab_kernel(const T* __restrict__ x, int64_t ld, const double* __restrict__ row_lse, CtcSeg g,
                                                             const int64_t* __restrict__ target, int Lmax, int64_t ds, int64_t pad,
                                                             int64_t eos, int C, int Smax, double* __restrict__ alpha,
                                                             double* __restrict__ beta, int32_t* __restrict__ ws_meta,
                                                             int32_t* __restrict__ ws_L, double* __restrict__ nll_raw,
                                                             float* __restrict__ nll, double* __restrict__ nll64, int zero_inf) {
  constexpr int SCAP = CTC_THREADS * NS;
  __shared__ double buf[2][SCAP + 4];                        // state s at [s + 2]: two -inf cells on either side
  __shared__ int lab[SCAP / 2 + 1];
  __shared__ int sh[2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x >> 1;
  const bool fwd = (blockIdx.x & 1) == 0;
  int64_t off;
  int len;
  ctc_segment(g, b, off, len);
  const int L = ctc_labels(target + (int64_t)b * Lmax, Lmax, ds, pad, eos, C, lab, sh);
  if (fwd) {                                                // the gradient kernel's view of the labels
    int32_t* meta = ws_meta + (int64_t)b * 3 * Lmax;
    if (tid == 0) ws_L[b] = L;
    for (int i = tid; i < L; i += CTC_THREADS) {
      int nx = -1, first = 1;
      for (int j = i + 1; j < L; ++j)
        if (lab[j] == lab[i]) { nx = j; break; }
      for (int j = 0; j < i; ++j)
        if (lab[j] == lab[i]) { first = 0; break; }
      meta[i] = lab[i];
      meta[Lmax + i] = nx;
      meta[2 * Lmax + i] = first;
    }
  }
  const int S = 2 * L + 1;
  if (L < 0 || len == 0) {                                  // (uniform) nothing to recurse over: the slabs are not read either
    if (fwd && tid == 0) {
      const double v = (L == 0 && len == 0) ? 0. : INFINITY;
      nll_raw[b] = v;
      nll64[b] = (zero_inf && v == INFINITY) ? 0. : v;
      nll[b] = (float)nll64[b];
    }
    return;
  }
  for (int i = tid; i < 2 * (SCAP + 4); i += CTC_THREADS) (&buf[0][0])[i] = -INFINITY;
  // this thread's states
  int cls[NS];
  bool live[NS], skip[NS], init[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int s = tid + k * CTC_THREADS;
    live[k] = s < S;
    const int i = s >> 1;
    const bool odd = (s & 1) && live[k];
    cls[k] = odd ? lab[i] : 0;
    if (fwd) {
      skip[k] = odd && s >= 3 && lab[i] != lab[i - 1];
      init[k] = s < 2;
    } else {
      skip[k] = odd && s + 2 < S && lab[i] != lab[i + 1];
      init[k] = s >= S - 2;
    }
  }
  double* slab = (fwd ? alpha : beta) + (int64_t)b * g.Tmax * Smax;
  // lp[t', l'_s] of this thread's states at step t (t' = t, or len - 1 - t) is x[row, l'_s] - lse[row].  The loads of CTC_PF steps are
  // issued a chunk ahead and kept RAW (storage type, lse apart): nothing consumes them before their own step, so no wait for them
  // sits in front of the steps in between.  (A state past S reads class 0 of the row: a valid address, the value unused.)
  auto fetch = [&](int t, T* xr, double& l) {               // (steps past the end fetch the last step's row again: no branch around a load)
    const int tc = min(t, len - 1);
    const int64_t row = off + (int64_t)(fwd ? tc : len - 1 - tc) * g.row_stride;
    l = row_lse[row];
#pragma unroll
    for (int k = 0; k < NS; ++k) xr[k] = x[row * ld + cls[k]];
  };
  T xc[CTC_PF][NS], xn[CTC_PF][NS];
  double lc[CTC_PF], ln[CTC_PF];
#pragma unroll
  for (int j = 0; j < CTC_PF; ++j) fetch(j, xc[j], lc[j]);
  __syncthreads();                                          // (the -inf fill)
  for (int t0 = 0; t0 < len; t0 += CTC_PF) {
#pragma unroll
    for (int j = 0; j < CTC_PF; ++j) fetch(t0 + CTC_PF + j, xn[j], ln[j]);
#pragma unroll
    for (int j = 0; j < CTC_PF; ++j) {
      const int t = t0 + j;
      if (t < len) {                                        // (uniform)
        const double* prev = buf[(t + 1) & 1] + 2;
        double* cur = buf[t & 1] + 2;
        double* out = slab + (int64_t)(fwd ? t : len - 1 - t) * Smax;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          if (!live[k]) continue;
          const int s = tid + k * CTC_THREADS;
          const double e = (double)ld1<T>(&xc[j][k]) - lc[j];
          double v;
          if (t == 0) {
            v = init[k] ? e : -INFINITY;
          } else {
            const double a1 = prev[fwd ? s - 1 : s + 1];
            const double a2 = skip[k] ? prev[fwd ? s - 2 : s + 2] : -INFINITY;
            v = e + lae3(prev[s], a1, a2);                  // (-inf + finite = -inf)
          }
          cur[s] = v;
          out[s] = v;
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int j = 0; j < CTC_PF; ++j) {
      lc[j] = ln[j];
#pragma unroll
      for (int k = 0; k < NS; ++k) xc[j][k] = xn[j][k];
    }
  }
  if (fwd && tid == 0) {
    const double* last = buf[(len - 1) & 1] + 2;
    const double v = -lae3(last[S - 1], S > 1 ? last[S - 2] : -INFINITY, -INFINITY);
    nll_raw[b] = v;
    nll64[b] = (zero_inf && v == INFINITY) ? 0. : v;
    nll[b] = (float)nll64[b];
  }
}

template <typename T>
__global__ __launch_bounds__(CTC_THREADS) void ctc_grad_kernel(const T* __restrict__ x, int64_t ld, const double* __restrict__ row_lse,
                                                               CtcSeg g, int Lmax, int C, int Smax, const double* __restrict__ alpha,
                                                               const double* __restrict__ beta, const int32_t* __restrict__ ws_meta,
                                                               const int32_t* __restrict__ ws_L, const double* __restrict__ nll_raw,
                                                               const float* __restrict__ seed, T* __restrict__ d, int64_t ld_d,
                                                               int zero_inf) {
  extern __shared__ __attribute__((aligned(16))) float occ[];    // [C] posterior occupancy of a class at this row, then [4] wave partials
  const int tid = threadIdx.x;
  const int t = blockIdx.x, b = blockIdx.y;
  int64_t off;
  int len;
  ctc_segment(g, b, off, len);
  if (t >= len) return;                                     // (the row holds the zero fill)
  const int64_t row = off + (int64_t)t * g.row_stride;
  const T* xr = x + row * ld;
  T* dr = d + row * ld_d;
  const double nl = nll_raw[b];
  if (nl == INFINITY) {                                     // infeasible: zero_infinity leaves the zero fill (a NaN goes through the sums)
    if (!zero_inf)
      for (int c = tid; c < C; c += CTC_THREADS) st1<T>(dr + c, NAN);
    return;
  }
  const int L = ws_L[b];
  const int32_t* meta = ws_meta + (int64_t)b * 3 * Lmax;
  const double* ar = alpha + ((int64_t)b * g.Tmax + t) * Smax;
  const double* br = beta + ((int64_t)b * g.Tmax + t) * Smax;
  const double l = row_lse[row];
  const float sc = seed ? seed[0] : 1.0f;
  float* part = occ + C;
  for (int c = tid; c < C; c += CTC_THREADS) occ[c] = 0.f;
  const double k0 = nl - ((double)ld1<T>(xr) - l);          // blank: nll - lp_0 (the exponent's terms cancel in fp64, exp runs in fp32)
  float bs = 0.f;
  for (int j = tid; j <= L; j += CTC_THREADS) bs += expf((float)(ar[2 * j] + br[2 * j] + k0));
  bs = wave_sum(bs);
  if ((tid & 63) == 0) part[tid >> 6] = bs;
  __syncthreads();
  for (int i = tid; i < L; i += CTC_THREADS) {
    if (!meta[2 * Lmax + i]) continue;
    const int c = meta[i];
    const double kc = nl - ((double)ld1<T>(xr + c) - l);
    float acc = 0.f;
    for (int j = i; j >= 0; j = meta[Lmax + j]) acc += expf((float)(ar[2 * j + 1] + br[2 * j + 1] + kc));
    occ[c] = acc;                                           // (first occurrences have distinct classes, all >= 1)
  }
  __syncthreads();
  for (int c = tid; c < C; c += CTC_THREADS) {
    const float o = c == 0 ? ((part[0] + part[1]) + (part[2] + part[3])) : occ[c];
    st1<T>(dr + c, (expf((float)((double)ld1<T>(xr + c) - l)) - o) * sc);
  }
}

// Greedy CTC decode of sentence b from the row arg-max: consecutive duplicates collapsed, then blanks dropped; out[b, :n] the classes,
// -1 behind them, out_len[b] = n.  One wave per sentence, 64 time steps per trip, compacted with a ballot.
__global__ __launch_bounds__(WAVE) void ctc_greedy_kernel(const int32_t* __restrict__ row_argmax, CtcSeg g, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ out_len) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int64_t off;
  int len;
  ctc_segment(g, b, off, len);
  int32_t* o = out + (int64_t)b * g.Tmax;
  int base = 0;
  for (int t0 = 0; t0 < len; t0 += WAVE) {
    const int t = t0 + lane;
    int a = 0, p = 0;
    if (t < len) {
      a = row_argmax[off + (int64_t)t * g.row_stride];
      p = t > 0 ? row_argmax[off + (int64_t)(t - 1) * g.row_stride] : 0;
    }
    const bool keep = t < len && a != 0 && (t == 0 || a != p);
    const uint64_t mask = __ballot(keep);
    if (keep) o[base + __popcll(mask & ((1ull << lane) - 1ull))] = a;
    base += __popcll(mask);
  }
  for (int i = base + lane; i < g.Tmax; i += WAVE) o[i] = -1;
  if (lane == 0) out_len[b] = base;
}

static int ctc_ns(int64_t Lmax) {                           // states per thread of the recursion kernel that holds S = 2 Lmax + 1 states
  const int64_t S = 2 * Lmax + 1;
  return S <= CTC_THREADS ? 1 : S <= 3 * CTC_THREADS ? 3 : 9;
}

static int ctc_check(const char* who, const void* logits, int64_t ld, int64_t rows, int64_t C, const int32_t* seg, int64_t seg_ld,
                     int64_t row_stride, int64_t B, int64_t Tmax, int dtype) {
  const int64_t lim = (int64_t)1 << 31;
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(logits && seg && rows >= 0 && rows < lim && ld >= C && seg_ld >= 2 && seg_ld < lim && row_stride >= 1 && row_stride < lim,
              OFA_ERR_INVALID, "%s: bad argument", who);
  OFA_REQUIRE(C >= 2 && C <= CTC_MAX_C, OFA_ERR_UNSUPPORTED, "%s: C=%lld classes, this build takes 2 .. %d", who, (long long)C, CTC_MAX_C);
  OFA_REQUIRE(B >= 0 && B < 32768 && Tmax >= 0 && Tmax < 65536, OFA_ERR_UNSUPPORTED, "%s: B=%lld sentences of up to Tmax=%lld rows", who,
              (long long)B, (long long)Tmax);
  return 0;
}
}  // namespace ofa
using namespace ofa;

extern "C" int64_t ofa_ctc_max_classes(void) { return CTC_MAX_C; }
extern "C" int64_t ofa_ctc_max_target(void) { return (CTC_MAX_NS * CTC_THREADS - 1) / 2; }

extern "C" int ofa_ctc_rows(const void* logits, int64_t ld, int64_t rows, int64_t C, double* row_lse, int32_t* row_argmax, int dtype,
                            void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ctc_rows: bad dtype %d", dtype);
  OFA_REQUIRE(logits && row_lse && rows >= 0 && rows < ((int64_t)1 << 31) && ld >= C, OFA_ERR_INVALID, "ctc_rows: bad argument");
  OFA_REQUIRE(C >= 2 && C <= CTC_MAX_C, OFA_ERR_UNSUPPORTED, "ctc_rows: C=%lld classes, this build takes 2 .. %d", (long long)C, CTC_MAX_C);
  if (rows == 0) return 0;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ctc_row_kernel<T>), dim3((unsigned)cdiv(rows, CTC_THREADS / WAVE)), dim3(CTC_THREADS), 0, (hipStream_t)stream,
                       (const T*)logits, ld, rows, (int)C, row_lse, row_argmax);
  });
  return check_launch("ctc_rows");
}

extern "C" int ofa_ctc_alpha_beta(const void* logits, int64_t ld, int64_t rows, int64_t C, const double* row_lse, const int32_t* seg,
                                  int64_t seg_ld, int64_t row_stride, int64_t B, int64_t Tmax, const int64_t* target, int64_t Lmax,
                                  int64_t ds, int64_t pad, int64_t eos, double* alpha, double* beta, int32_t* ws_meta, int32_t* ws_L,
                                  double* nll_raw, float* nll, double* nll64, int zero_infinity, int dtype, void* stream) {
  if (int rc = ctc_check("ctc_alpha_beta", logits, ld, rows, C, seg, seg_ld, row_stride, B, Tmax, dtype)) return rc;
  OFA_REQUIRE(row_lse && target && alpha && beta && ws_meta && ws_L && nll_raw && nll && nll64 && Lmax >= 1, OFA_ERR_INVALID,
              "ctc_alpha_beta: bad argument");
  OFA_REQUIRE(2 * Lmax + 1 <= CTC_MAX_NS * CTC_THREADS, OFA_ERR_UNSUPPORTED, "ctc_alpha_beta: a target of %lld positions has %lld states, this build takes %d",
              (long long)Lmax, (long long)(2 * Lmax + 1), CTC_MAX_NS * CTC_THREADS);
  if (B == 0) return 0;
  const CtcSeg g{seg, (int)seg_ld, row_stride, rows, (int)Tmax};
  const int ns = ctc_ns(Lmax);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3((unsigned)(2 * B)), dim3(CTC_THREADS), 0, (hipStream_t)stream, (const T*)logits, ld, row_lse, g, target,
                         (int)Lmax, ds, pad, eos, (int)C, (int)(2 * Lmax + 1), alpha, beta, ws_meta, ws_L, nll_raw, nll, nll64, zero_infinity);
    };
    if (ns == 1) launch(ctc_ab_kernel<T, 1>);
    else if (ns == 3) launch(ctc_ab_kernel<T, 3>);
    else launch(ctc_ab_kernel<T, CTC_MAX_NS>);
  });
  return check_launch("ctc_alpha_beta");
}

extern "C" int ofa_ctc_grad(const void* logits, int64_t ld, int64_t rows, int64_t C, const double* row_lse, const int32_t* seg,
                            int64_t seg_ld, int64_t row_stride, int64_t B, int64_t Tmax, int64_t Lmax, const double* alpha,
                            const double* beta, const int32_t* ws_meta, const int32_t* ws_L, const double* nll_raw, const float* seed,
                            void* dlogits, int64_t ld_d, int zero_infinity, int dtype, void* stream) {
  if (int rc = ctc_check("ctc_grad", logits, ld, rows, C, seg, seg_ld, row_stride, B, Tmax, dtype)) return rc;
  OFA_REQUIRE(row_lse && alpha && beta && ws_meta && ws_L && nll_raw && dlogits && ld_d >= C && Lmax >= 1, OFA_ERR_INVALID,
              "ctc_grad: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // every row outside a sentence's length keeps this exact zero; the kernel stores the live rows
  if (hipMemsetAsync(dlogits, 0, (size_t)rows * (size_t)ld_d * dt_size(dtype), st) != hipSuccess) return check_launch("ctc_grad (zero fill)");
  if (B == 0 || Tmax == 0) return check_launch("ctc_grad");
  const CtcSeg g{seg, (int)seg_ld, row_stride, rows, (int)Tmax};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ctc_grad_kernel<T>), dim3((unsigned)Tmax, (unsigned)B), dim3(CTC_THREADS), (size_t)(C + 4) * sizeof(float), st,
                       (const T*)logits, ld, row_lse, g, (int)Lmax, (int)C, (int)(2 * Lmax + 1), alpha, beta, ws_meta, ws_L, nll_raw, seed,
                       (T*)dlogits, ld_d, zero_infinity);
  });
  return check_launch("ctc_grad");
}

extern "C" int ofa_ctc_greedy_decode(const int32_t* row_argmax, int64_t rows, const int32_t* seg, int64_t seg_ld, int64_t row_stride,
                                     int64_t B, int64_t Tmax, int32_t* out, int32_t* out_len, void* stream) {
  OFA_REQUIRE(row_argmax && seg && out && out_len && rows >= 0 && rows < ((int64_t)1 << 31) && seg_ld >= 2 && row_stride >= 1 && B >= 0 &&
                  B < ((int64_t)1 << 31) && Tmax >= 0 && Tmax < 65536,
              OFA_ERR_INVALID, "ctc_greedy_decode: bad argument");
  if (B == 0) return 0;
  const CtcSeg g{seg, (int)seg_ld, row_stride, rows, (int)Tmax};
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(WAVE), 0, (hipStream_t)stream, row_argmax, g, out, out_len);
  return check_launch("ctc_greedy_decode");
}

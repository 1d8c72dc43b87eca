// Sampling step for gfx950: the reference's Sampling.step (utils/search.py:596-715) under the bookkeeping of its SequenceGenerator
// (generator/sequence_generator.py:283-492), in two launches per decoding step that take only fixed device addresses and the
// step number, so they are recorded inside the per-step hipGraph like the beam kernels (ofasys_amd/generator.py).  A sentence's K
// "beams" are K independent samples.  No random numbers are made here: every draw is a deterministic function of the row's
// logits and ONE uniform number the caller supplies, so a test can pin it exactly.
//
// 1. ofa_sample_draw -- the row pass, one 1024-thread workgroup per row (16 waves to hide the latency of its reads).  The row's lprobs are ofa_beam_topk's: the fp32
//    log-softmax of x / T with constraint_range applied first (the normaliser is built from the same 4096-column parts by the same
//    helpers, so it is the same float), then the post-normaliser masks of beam_mask_key.  Weights w_c = expf(lprob_c), not
//    renormalised after the masks.  The kept set S: every token (plain), the k largest lprobs (top-k), or the tokens whose
//    strictly-ahead weight is < p (top-p, which wins over top-k) -- ranked by (lprob descending, token ascending).  The draw for
//    the uniform u: the kept token with the smallest id c* such that sum_{c in S, c <= c*} w_c > u * W, W = sum_{c in S} w_c: an
//    inverse CDF in VOCABULARY order, so no sort of the row is needed, only the threshold of S.
//    Order-free arithmetic: a weight is the integer floor(expf(lprob) * 2^40), sums are 64-bit integers (a row sums to about 2^40),
//    so no result depends on the order of the LDS atomics.  The threshold is a radix select (4 rounds of 8 bits) over the
//    order-preserving integer image of the lprob, with "weight ahead" histogrammed per digit (unit weights for top-k); what is
//    left of k / p at the last digit says how many of the tied tokens are kept, in token order.  Then every 1024-column chunk's
//    weight above the threshold and its ties are summed by one wave (fixed order), wave 0 scans the chunks (one lane each) and
//    locates the draw inside one of them, walking its 64-column segments.
//    When no kept token has a non-zero integer weight (the row's lprobs are all below -27.7, or -inf: a NaN row) the draw is the
//    top-ranked token.  At step 0 all K rows of a sentence read its row b * K (lprobs[:, ::beam_size]), each with its own uniform.
//    The row is read 2 (plain) or 6 times, from L2 after the first: 59 457 fp32 values are 232 KiB.
// 2. ofa_sample_select -- the sentence pass, one workgroup per sentence, over the K-wide candidate list (slot j draws once, with
//    itself as parent; parent 0 at step 0): score = scores[row, step - 1] + lprob, EOS draws of slots not ignored are finalised,
//    ignored slots stay ignored, the active slots are compacted to the front in column order, histories gathered in place, reorder
//    written: beam_common.h's beam_sentence_step, the bookkeeping ofa_beam_select runs, over a list of exactly K.
#include "beam_common.h"

namespace ofa {

constexpr int SAMPLE_THREADS = 1024, SAMPLE_WAVES = 16;     // one workgroup per row: 16 waves hide the latency of the row's reads
constexpr int SAMPLE_MAX_V = 1 << 16;                       // the ban bitmap and the chunk sums live in LDS
constexpr int SAMPLE_CHUNK = 64 * BEAM_PER_LANE;            // columns a wave sums at once: a quarter of a normaliser part
constexpr int SAMPLE_MAX_CHUNKS = SAMPLE_MAX_V / SAMPLE_CHUNK;   // <= 64: one lane of wave 0 each
constexpr int SAMPLE_HALF = 8;                              // reads in flight per lane while a chunk is summed
constexpr int SAMPLE_BATCH = 4;                             // loads in flight per thread in the radix rounds
constexpr int SAMPLE_COPIES = 8;                            // histogram copies by lane & 7: lprobs share few exponents
constexpr float SAMPLE_FIX_ONE = 1099511627776.f;           // 2^40
typedef unsigned long long u64;

struct SampleWs {
  float* lprob;                           // [rows] the drawn token's lprob (full softmax, after the masks)
  int* tok;                               // [rows] the drawn token
};
static inline SampleWs sample_ws_carve(const void* ws, int64_t rows) { return SampleWs{(float*)ws, (int*)ws + rows}; }

struct SampleDrawArgs {
  const void* logits; int64_t ld;
  int rows, V, K, S;
  ofa_gen_policy p;
  int mode;                               // 0 plain, 1 top-k, 2 top-p
  u64 limit;                              // k, or p in units of 2^-40
  const float* uniforms;
  SampleWs ws;
};

// order-preserving integer image of a float (no NaN): a < b <=> key(a) < key(b)
__device__ __forceinline__ uint32_t sample_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ u64 sample_fix(float lp) { return (u64)(expf(lp) * SAMPLE_FIX_ONE); }

// wave_sum (common.h) for 64-bit integers: the DPP moves carry the two halves, the add is exact; every lane receives the total
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
  v += dpp_u64<0xB1, 0xf>(v);
  v += dpp_u64<0x4E, 0xf>(v);
  v += dpp_u64<0x141, 0xf>(v);
  v += dpp_u64<0x140, 0xf>(v);
  v += dpp_u64<0x142, 0xa>(v);
  v += dpp_u64<0x143, 0xc>(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {       // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_draw_kernel(SampleDrawArgs a) {
  const int row = blockIdx.x, sent = row / a.K;
  const ofa_gen_policy& p = a.p;
  if (p.done && p.done[sent]) return;
  const int src_row = p.step == 0 ? sent * a.K : row;       // step 0: the sentence's first row only (search.py:661-664)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  __shared__ float red_m[SAMPLE_MAX_CHUNKS], red_s[SAMPLE_MAX_CHUNKS];
  __shared__ int red_nan[SAMPLE_MAX_CHUNKS];
  __shared__ float stats[2 * (SAMPLE_MAX_V / BEAM_CHUNK)];
  __shared__ uint32_t ban[SAMPLE_MAX_V / 32];
  __shared__ u64 hist[256 * SAMPLE_COPIES];
  __shared__ u64 chunk_gt[SAMPLE_MAX_CHUNKS];
  __shared__ uint32_t chunk_tie[SAMPLE_MAX_CHUNKS];
  __shared__ u64 wtot[4], sel_rem;
  __shared__ int sel_bin;
  __shared__ float top_lp[SAMPLE_WAVES];
  __shared__ int top_tok[SAMPLE_WAVES];

  const T* src = (const T*)a.logits + (int64_t)src_row * a.ld;
  for (int i = tid; i < (V + 31) / 32; i += SAMPLE_THREADS) ban[i] = 0u;
  __syncthreads();
  if (tid < BEAM_THREADS)
    beam_ngram_scan(p, src_row, tid, [&](int64_t tok) {
      if (tok >= 0 && tok < V) atomicOr(&ban[tok >> 5], 1u << (tok & 31));
    });
  // x / T under constraint_range: what the normaliser sees
  auto scaled = [&](float v, int c) -> float {
    if (p.temperature != 1.f) v = v / p.temperature;
    if (p.cstart >= 0 && ((c >= 4 && c < p.cstart) || c >= p.cend)) v = -INFINITY;
    return v;
  };
  // ---- the fp32 normaliser, built as ofa_beam_topk builds it: a wave's (max, sum) of its quarter of every 4096-column part
  // (beam_normaliser_part's wave stage, one wave per quarter, no barrier in between), the part's (max, sum) from its four
  // quarters, beam_row_lse over the parts -- the same float
  for (int q = wave; q < 4 * a.S; q += SAMPLE_WAVES) {
    float x[BEAM_PER_LANE];
    float m = -INFINITY;
    int has_nan = 0;
#pragma unroll
    for (int j = 0; j < BEAM_PER_LANE; ++j) {
      const int c = q * SAMPLE_CHUNK + j * 64 + lane;
      const float v = scaled(c < V ? ld1<T>(src + c) : 0.f, c);
      x[j] = v;
      if (c < V) {
        if (v != v) has_nan = 1;
        else m = fmaxf(m, v);
      }
    }
    m = wave_max(m);
    float sum = 0.f;
    if (m != -INFINITY) {
#pragma unroll
      for (int j = 0; j < BEAM_PER_LANE; ++j) {
        const int c = q * SAMPLE_CHUNK + j * 64 + lane;
        if (c < V && x[j] == x[j]) sum += expf(x[j] - m);
      }
    }
    sum = wave_sum(sum);
    has_nan = __any(has_nan) ? 1 : 0;
    if (lane == 0) { red_m[q] = m; red_s[q] = sum; red_nan[q] = has_nan; }
  }
  __syncthreads();                                           // (also orders the ban bitmap)
  if (tid < a.S) {
    const float* pm = red_m + 4 * tid;
    const float* ps = red_s + 4 * tid;
    const float M = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
    float S = 0.f;
    for (int w = 0; w < 4; ++w)
      if (pm[w] != -INFINITY) S += ps[w] * expf(pm[w] - M);
    const bool nan_ = red_nan[4 * tid] | red_nan[4 * tid + 1] | red_nan[4 * tid + 2] | red_nan[4 * tid + 3];
    stats[2 * tid] = nan_ ? NAN : M;
    stats[2 * tid + 1] = S;
  }
  __syncthreads();
  bool bad;
  const float lse = beam_row_lse(stats, a.S, bad);
  // the lprob of column c after every mask, from its stored logit (never NaN; one image for zero)
  auto lprob = [&](float raw, int c) -> float {
    float lp = bad ? -INFINITY : scaled(raw, c) - lse;
    const bool banned = (ban[c >> 5] >> (c & 31)) & 1u;
    float unk_val;
    lp = beam_mask_key(p, lp, c, banned, unk_val);
    return lp == 0.f ? 0.f : lp;
  };

  // ---- the threshold of the kept set: tokens with key > thr, and the first n_tie (token order) of those with key == thr
  uint32_t thr = 0u, n_tie = 0u;                             // plain: every key is above 0
  if (a.mode != 0) {
    uint32_t pref = 0u;
    u64 rem = a.limit;
    bool all = false;
    for (int r = 0; r < 4 && !all; ++r) {
      const int shift = 24 - 8 * r;
      for (int i = tid; i < 256 * SAMPLE_COPIES; i += SAMPLE_THREADS) hist[i] = 0ull;
      if (tid == 0) sel_bin = -1;
      __syncthreads();
      for (int c0 = tid; c0 < V; c0 += SAMPLE_BATCH * SAMPLE_THREADS) {
        float raw[SAMPLE_BATCH];
#pragma unroll
        for (int k = 0; k < SAMPLE_BATCH; ++k) {
          const int c = c0 + k * SAMPLE_THREADS;
          raw[k] = c < V ? ld1<T>(src + c) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < SAMPLE_BATCH; ++k) {
          const int c = c0 + k * SAMPLE_THREADS;
          if (c >= V) continue;
          const float lp = lprob(raw[k], c);
          const uint32_t key = sample_key(lp);
          if (r == 0 || (key >> (shift + 8)) == (pref >> (shift + 8))) {
            const u64 w = a.mode == 2 ? sample_fix(lp) : 1ull;
            if (w) atomicAdd(&hist[((key >> shift) & 255u) * SAMPLE_COPIES + (lane & (SAMPLE_COPIES - 1))], w);
          }
        }
      }
      __syncthreads();
      // thread t < 256 owns digit 255 - t: the weight ranked ahead of its digit is an exclusive scan
      const int bin = 255 - tid;
      u64 mine = 0ull, incl = 0ull;
      if (tid < 256) {
#pragma unroll
        for (int q = 0; q < SAMPLE_COPIES; ++q) mine += hist[bin * SAMPLE_COPIES + q];
        incl = wave_scan_u64(mine, lane);
        if (lane == 63) wtot[wave] = incl;
      }
      __syncthreads();
      if (tid < 256) {
        u64 ahead = incl - mine;
        for (int w = 0; w < wave; ++w) ahead += wtot[w];
        if (ahead < rem && rem <= ahead + mine) { sel_bin = bin; sel_rem = rem - ahead; }   // at most one digit
      }
      __syncthreads();
      const int sb = sel_bin;
      const u64 sr = sel_rem;
      __syncthreads();
      if (sb < 0) all = true;                                // the row's total is below the limit: everything is kept
      else { pref |= (uint32_t)sb << shift; rem = sr; }
    }
    if (!all) {
      thr = pref;
      const u64 unit = a.mode == 2 ? sample_fix(sample_unkey(thr)) : 1ull;
      const u64 n = unit ? (rem + unit - 1ull) / unit : 0xffffffffull;
      n_tie = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
    }
  }
  const u64 tie_w = sample_fix(sample_unkey(thr));           // the weight of one tied token

  // ---- weight above the threshold and ties of every 1024-column chunk (one wave each, fixed order: no atomics), and the
  // row's top-ranked token
  const int nchunk = (V + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;
  float best = NAN;
  int best_c = 0x7fffffff;
  for (int q = wave; q < nchunk; q += SAMPLE_WAVES) {
    u64 mass = 0ull;
    float ties = 0.f;                                        // (<= 1024 a chunk: exact)
#pragma unroll 1
    for (int h = 0; h < BEAM_PER_LANE; h += SAMPLE_HALF) {   // eight reads in flight
      float raw[SAMPLE_HALF];
#pragma unroll
      for (int j = 0; j < SAMPLE_HALF; ++j) {
        const int c = q * SAMPLE_CHUNK + (h + j) * 64 + lane;
        raw[j] = c < V ? ld1<T>(src + c) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < SAMPLE_HALF; ++j) {
        const int c = q * SAMPLE_CHUNK + (h + j) * 64 + lane;
        if (c >= V) continue;
        const float lp = lprob(raw[j], c);
        const uint32_t key = sample_key(lp);
        if (key > thr) mass += sample_fix(lp);
        if (key == thr) ties += 1.f;
        if (best_c == 0x7fffffff || lp > best) { best = lp; best_c = c; }
      }
    }
    mass = wave_sum_u64(mass);
    ties = wave_sum(ties);
    if (lane == 0) { chunk_gt[q] = mass; chunk_tie[q] = (uint32_t)ties; }
  }
  {
    float mx; int mi;
    const bool any = wave_argmax(best, best_c, mx, mi);
    if (lane == 0) { top_lp[wave] = any ? mx : NAN; top_tok[wave] = any ? mi : 0x7fffffff; }
  }
  __syncthreads();
  if (wave != 0) return;
  float tlp = NAN;
  int ttok = 0x7fffffff;
  for (int w = 0; w < SAMPLE_WAVES; ++w)
    if (top_lp[w] == top_lp[w] && (!(tlp == tlp) || top_lp[w] > tlp || (top_lp[w] == tlp && top_tok[w] < ttok))) {
      tlp = top_lp[w];
      ttok = top_tok[w];
    }
  // ---- wave 0: lane l owns chunk l; ties are kept in token order
  const uint32_t my_ties = lane < nchunk ? chunk_tie[lane] : 0u;
  const u64 ties_before = wave_scan_u64((u64)my_ties, lane) - my_ties;
  const u64 left = ties_before < n_tie ? (u64)n_tie - ties_before : 0ull;
  const u64 my_mass = lane < nchunk ? chunk_gt[lane] + (left < my_ties ? left : (u64)my_ties) * tie_w : 0ull;
  const u64 incl = wave_scan_u64(my_mass, lane);
  const u64 W = __shfl(incl, 63, 64);
  float u = a.uniforms[row];
  if (!(u >= 0.f)) u = 0.f;
  if (u >= 1.f) u = 0.99999994f;
  const u64 target = (u64)((double)u * (double)W);           // < W for W > 0: the draw is the first token whose prefix is > target
  int out_tok = ttok;
  float out_lp = tlp;
  const u64 hit = __ballot(incl > target);
  if (W > 0ull && hit) {
    const int L = __ffsll((long long)hit) - 1;
    u64 run = __shfl(incl - my_mass, L, 64);
    u64 tb = __shfl(ties_before, L, 64);
#pragma unroll 1
    for (int j = 0; j < BEAM_PER_LANE; ++j) {                // the chunk's 64-column segments, in order
      const int c = L * SAMPLE_CHUNK + j * 64 + lane;
      const bool valid = c < V;
      const float lp = valid ? lprob(ld1<T>(src + c), c) : -INFINITY;
      const uint32_t key = sample_key(lp);
      const bool tie = valid && key == thr;
      const u64 tmask = __ballot(tie);
      const u64 rank = tb + __popcll(tmask & ((1ull << lane) - 1ull));
      const bool kept = valid && (key > thr || (tie && rank < n_tie));
      const u64 wf = kept ? sample_fix(lp) : 0ull;
      const u64 pre = run + wave_scan_u64(wf, lane);
      const u64 found = __ballot(wf > 0ull && pre > target);
      if (found) {
        const int F = __ffsll((long long)found) - 1;
        out_tok = L * SAMPLE_CHUNK + j * 64 + F;
        out_lp = __shfl(lp, F, 64);
        break;
      }
      run = __shfl(pre, 63, 64);
      tb += __popcll(tmask);
    }
  }
  if (lane == 0) {
    a.ws.tok[row] = out_tok;
    a.ws.lprob[row] = out_lp;
  }
}

struct SampleSelectArgs {
  SampleWs ws;
  int bsz, K, step, max_len, eos;
  int normalize; float len_pen;
  ofa_gen_state st;
};

__global__ __launch_bounds__(BEAM_THREADS) void sample_select_kernel(SampleSelectArgs a) {
  const int sent = blockIdx.x;
  if (a.st.done[sent]) return;                               // finished: a no-op from then on
  const int tid = threadIdx.x;
  const int K = a.K, step = a.step, r0 = sent * K;
  extern __shared__ float smem[];
  __shared__ BeamSentScratch sh;

  // ---- the K candidates: slot j's draw, cumulative (search.py:708-713), with itself as parent (slot 0 at step 0)
  if (tid < K) {
    const float lp = a.ws.lprob[r0 + tid];
    sh.sel_sc[tid] = step > 0 ? lp + a.st.scores[(int64_t)(r0 + tid) * a.st.score_ld + step - 1] : lp;
    sh.sel_beam[tid] = step == 0 ? 0 : tid;
    sh.sel_tok[tid] = a.ws.tok[r0 + tid];
  }
  __syncthreads();
  beam_sentence_step(a.st, sh, sent, K, step, a.max_len, a.eos, a.normalize, a.len_pen, K, smem);
}

}  // namespace ofa

using namespace ofa;

extern "C" int64_t ofa_sample_ws_bytes(int rows, int V, int K) {
  if (rows <= 0 || V <= 0 || K <= 0) return 0;
  return (int64_t)rows * 8;
}

extern "C" int ofa_sample_draw(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol, int topk, float topp,
                               const float* uniforms, void* ws, int dtype, void* stream) {
  OFA_REQUIRE(logits && ws && uniforms && pol, OFA_ERR_INVALID, "ofa_sample_draw: null pointer");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ofa_sample_draw: bad dtype %d", dtype);
  OFA_REQUIRE(rows > 0 && V > 1 && ld >= V && pol->step >= 0, OFA_ERR_INVALID, "ofa_sample_draw: rows=%d V=%d ld=%lld step=%d", rows, V,
              (long long)ld, pol->step);
  OFA_REQUIRE(V <= SAMPLE_MAX_V, OFA_ERR_UNSUPPORTED, "ofa_sample_draw: vocabulary %d > %d", V, SAMPLE_MAX_V);
  OFA_REQUIRE(!(topp > 1.f) && topp == topp, OFA_ERR_INVALID, "ofa_sample_draw: top-p %g above 1", (double)topp);
  if (const int rc = beam_check_row_pass("ofa_sample_draw", rows, V, K, *pol)) return rc;
  int mode = 0;
  u64 limit = 0;
  if (topp > 0.f) { mode = 2; limit = (u64)((double)topp * (double)SAMPLE_FIX_ONE); }   // top-p wins (search.py:666-672)
  else if (topk > 0 && topk < V) { mode = 1; limit = (u64)topk; }
  SampleDrawArgs a{logits, ld, rows, V, K, beam_splits(V), *pol, mode, limit, uniforms, sample_ws_carve(ws, rows)};
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(sample_draw_kernel<typename decltype(tag)::type>, dim3(rows), dim3(SAMPLE_THREADS), 0, st, a);
  });
  return check_launch("ofa_sample_draw");
}

extern "C" int ofa_sample_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int step, int max_len, int eos, int normalize,
                                 float len_penalty, void* stream) {
  OFA_REQUIRE(ws, OFA_ERR_INVALID, "ofa_sample_select: null pointer");
  OFA_REQUIRE(bsz > 0 && step >= 0 && step <= max_len, OFA_ERR_INVALID, "ofa_sample_select: bsz=%d step=%d max_len=%d", bsz, step,
              max_len);
  if (const int rc = beam_check_state("ofa_sample_select", st, K, step, true)) return rc;
  const size_t smem = beam_history_lds(K, step);
  OFA_REQUIRE(smem <= 65536, OFA_ERR_UNSUPPORTED, "ofa_sample_select: beam %d x step %d needs %zu bytes of LDS", K, step, smem);
  SampleSelectArgs a{sample_ws_carve(ws, (int64_t)bsz * K), bsz, K, step, max_len, eos, normalize, len_penalty, *st};
  hipLaunchKernelGGL(sample_select_kernel, dim3(bsz), dim3(BEAM_THREADS), smem, (hipStream_t)stream, a);
  return check_launch("ofa_sample_select");
}

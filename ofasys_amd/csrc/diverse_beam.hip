// Diverse decoding for gfx950: the reference's DiverseBeamSearch.step (utils/search.py:549-593, Hamming diversity over groups of
// beams) and DiverseSiblingsSearch.step (:738-787, a penalty on the rank among a beam's own continuations) as SENTENCE PASSES over
// what ofa_beam_topk (beam_search.hip) already leaves in the workspace: every row's normaliser parts and, per 4096-column part,
// its best 2K candidates before the unk penalty.  No new row pass, and the bookkeeping after the candidate list is beam_common.h's
// beam_sentence_step, so a diverse step is the plain step with another second launch (recorded into the step graph alike).
//
// Both passes first reduce every row to ITS OWN top 2K by lprob (value - normaliser, unk - penalty, NaN -> -inf; a row whose
// normaliser is NaN or not finite lists tokens 0 .. min(V, 2K) - 1 at -inf), sorted by (lprob descending, token ascending): one wave
// per row, the row's <= 512 listed entries in registers, 2K rounds of wave arg-max.  That list is all either strategy needs:
//  - siblings: the reference takes each beam's top k = 2K (V > 2K), subtracts (rank + 1) * rate from (lprob + cumulative), and
//    takes the top 2K of the K * 2K rewritten scores; step 0 is the plain beam step (row 0, top min(2K, V - 1)).
//  - groups (G groups of m = K / G beams, group g owning beams g, g + G, ...; strength >= 0): group g picks its top
//    min(2m, rows * V - 1) of (lprob - strength * count[token]) + cumulative, count = the picks of groups 0 .. g-1 (every pick
//    counts: duplicates and -inf ones), at most P = (G - 1) * 2m of them.  A token in a row's penalised top 2m has fewer than 2m
//    unpenalised tokens above it that stay above it, and at most P - 1 penalised ones: its unpenalised rank is below
//    2m + P <= 2K.  A penalty reorders entries INSIDE the sorted list, so the selection is a rank by counting over the group's
//    <= m * 2K entries, not a merge by list heads.  At step 0 group g reads row g alone (the inner BeamSearch.step takes the
//    group's first row) and reports beam g.  The list handed on is the reference's interleave: rank j of group g at j * G + g.
// Ties everywhere: value descending, then beam * V + token ascending; NaN = empty.  The rewritten scores are what is carried on.
#include "beam_common.h"

namespace ofa {

constexpr int DIVERSE_PER_LANE = 8;                          // a row's listed entries (S parts x 2K) held by one wave: <= 512

struct DiverseArgs {
  BeamWs ws;
  int bsz, K, V, S, step, max_len, eos, unk; float unk_pen;
  int normalize; float len_pen;
  int groups;                                                // >= 1: DiverseBeamSearch; 0: DiverseSiblingsSearch
  float amount;                                              // diversity strength, or the sibling rate
  ofa_gen_state st;
};

// Threads rank the n staged entries (sc, fl) by counting the entries ahead of theirs -- (score desc, flat index asc), NaN = empty --
// and the best kk call take(entry, rank).  n <= 512: two entries per thread, every read of the inner loop an LDS broadcast.
template <typename Take>
__device__ __forceinline__ void diverse_rank(const float* sc, const int* fl, int n, int kk, int tid, Take take) {
  for (int e = tid; e < n; e += BEAM_THREADS) {
    const float v = sc[e];
    if (!(v == v)) continue;
    const int f = fl[e];
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (sc[q] > v || (sc[q] == v && fl[q] < f)) ? 1 : 0;
    if (rank < kk) take(e, rank);
  }
}

template <bool GROUPS>
__global__ __launch_bounds__(BEAM_THREADS) void diverse_select_kernel(DiverseArgs a) {
#pragma clang fp contract(off)                               // the reference adds, then adds: no fused multiply-add
  const int sent = blockIdx.x;
  if (a.st.done[sent]) return;                               // finished: a no-op from then on
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the loop over a wave's rows branches without masks)
  const int K = a.K, K2 = 2 * K, V = a.V, step = a.step, r0 = sent * K, G = GROUPS ? a.groups : 0;
  const int nr = (G == 0 && step == 0) ? 1 : K;              // siblings at step 0: the plain step over beam 0
  extern __shared__ float smem[];
  float* rsc = smem;                                         // [K * 2K] every row's own top 2K: lprob (NaN: none)
  int* rtok = (int*)(rsc + K * K2);                          // [K * 2K] their tokens (-1: none)
  float* gsc = (float*)(rtok + K * K2);                      // [<= K * 2K] the scores under selection
  int* gfl = (int*)(gsc + K * K2);                           // [<= K * 2K] their flat indices beam * V + token
  __shared__ float lse[BEAM_MAX_K], cum[BEAM_MAX_K];
  __shared__ int bad[BEAM_MAX_K];
  __shared__ int picked[2 * BEAM_MAX_K];                     // the tokens the earlier groups took
  __shared__ BeamSentScratch sh;
  // The state descriptor waits in LDS for the bookkeeping: held as kernel arguments, its 30 scalar registers stay live across the
  // whole pass and, with the 32 flags that beam_sentence_step's one thread keeps in scalar registers, exceed the register file.
  __shared__ ofa_gen_state parked;

  // ---- each beam row's normaliser from its parts; the list handed on starts out as harmless entries
  if (tid == 0) parked = a.st;
  if (tid < nr) {
    bool b;
    lse[tid] = beam_row_lse(a.ws.stats + (int64_t)(r0 + tid) * a.S * 2, a.S, b);
    bad[tid] = b;                                            // NaN or infinite: the whole row is -inf (log_softmax -> NaN -> -inf)
    cum[tid] = step > 0 ? a.st.scores[(int64_t)(r0 + tid) * a.st.score_ld + step - 1] : 0.f;
  }
  if (tid < K2) { sh.sel_sc[tid] = -INFINITY; sh.sel_beam[tid] = 0; sh.sel_tok[tid] = 0; }
  __syncthreads();
  // ---- every row's own top 2K by lprob: one wave per row, the listed entries in registers
  for (int r = wave; r < nr; r += BEAM_THREADS / 64) {
    float* osc = rsc + r * K2;
    int* otk = rtok + r * K2;
    if (__builtin_amdgcn_readfirstlane(bad[r])) {                                     // all -inf: the lowest tokens win the ties
      if (lane < K2) { osc[lane] = lane < V ? -INFINITY : NAN; otk[lane] = lane < V ? lane : -1; }
      continue;
    }
    const int64_t base = (int64_t)(r0 + r) * a.S * K2;
    const int ne = a.S * K2;
    float v[DIVERSE_PER_LANE];
    int t[DIVERSE_PER_LANE];
#pragma unroll
    for (int q = 0; q < DIVERSE_PER_LANE; ++q) {
      // (slots past the row's entries read its last entry and turn into token -1 arithmetically: no mask registers held per slot)
      const int e = q * 64 + lane, at = e < ne ? e : ne - 1;
      const int tok = a.ws.ctok[base + at] | ((ne - 1 - e) >> 31);
      float lp = a.ws.cval[base + at] - lse[r];
      if (tok == a.unk) lp = lp - a.unk_pen;
      if (lp != lp) lp = -INFINITY;
      const bool listed = (unsigned)tok < (unsigned)V;
      v[q] = listed ? lp : NAN;
      t[q] = listed ? tok : 0x7fffffff;
    }
    int it = 0;
    for (; it < K2; ++it) {
      float lb = NAN;
      int lt = 0x7fffffff;
#pragma unroll
      for (int q = 0; q < DIVERSE_PER_LANE; ++q)
        if (v[q] == v[q] && (!(lb == lb) || v[q] > lb || (v[q] == lb && t[q] < lt))) { lb = v[q]; lt = t[q]; }
      float mx; int mt;
      if (!wave_argmax(lb, lt, mx, mt)) break;
      if (lb == lb && lt == mt) {
        osc[it] = mx;
        otk[it] = mt;
#pragma unroll
        for (int q = 0; q < DIVERSE_PER_LANE; ++q)
          if (t[q] == mt) v[q] = NAN;                        // (a row lists a token once: tokens are unique per part, parts disjoint)
      }
    }
    if (lane >= it && lane < K2) { osc[lane] = NAN; otk[lane] = -1; }
  }
  __syncthreads();

  int n;                                                     // the length of the list handed on
  if constexpr (!GROUPS) {
    // ---- siblings: (lprob + cumulative) - (rank + 1) * rate over every row's list, then the top k of all of them
    const int64_t avail = (int64_t)nr * V - 1;
    const int kk = (int)(avail < K2 ? avail : K2);
    for (int e = tid; e < nr * K2; e += BEAM_THREADS) {
      const int r = e / K2, j = e % K2, tok = rtok[e];
      float sc = NAN;
      if (tok >= 0) {
        sc = rsc[e];
        if (step > 0) { sc = sc + cum[r]; sc = sc - (float)(j + 1) * a.amount; }
      }
      gsc[e] = sc;
      gfl[e] = tok < 0 ? 0x7fffffff : r * V + tok;
    }
    __syncthreads();
    diverse_rank(gsc, gfl, nr * K2, kk, tid, [&](int e, int rank) {
      sh.sel_sc[rank] = gsc[e];
      sh.sel_beam[rank] = e / K2;
      sh.sel_tok[rank] = rtok[e];
    });
    n = kk;
  } else {
    // ---- groups, in order: penalise by the earlier groups' picks, rank, take, count
    const int m = K / G, rows_g = step == 0 ? 1 : m;         // step 0: the group's first row only
    const int64_t avail = (int64_t)rows_g * V - 1;
    const int kg = (int)(avail < 2 * m ? avail : 2 * m);
    for (int g = 0; g < G; ++g) {
      const int ne = rows_g * K2, np = g * kg;
      for (int e = tid; e < ne; e += BEAM_THREADS) {
        const int r = g + (e / K2) * G, src = r * K2 + e % K2, tok = rtok[src];
        float sc = NAN;
        if (tok >= 0) {
          int cnt = 0;
          for (int q = 0; q < np; ++q) cnt += picked[q] == tok ? 1 : 0;
          sc = rsc[src] + (-a.amount * (float)cnt);
          if (step > 0) sc = sc + cum[r];
        }
        gsc[e] = sc;
        gfl[e] = tok < 0 ? 0x7fffffff : r * V + tok;
      }
      __syncthreads();
      diverse_rank(gsc, gfl, ne, kg, tid, [&](int e, int rank) {
        const int r = g + (e / K2) * G, tok = rtok[r * K2 + e % K2], at = rank * G + g;
        sh.sel_sc[at] = gsc[e];
        sh.sel_beam[at] = r;
        sh.sel_tok[at] = tok;
        picked[np + rank] = tok;
      });
      __syncthreads();
    }
    n = G * kg;
  }
  __syncthreads();
  const ofa_gen_state st = parked;
  beam_sentence_step(st, sh, sent, K, step, a.max_len, a.eos, a.normalize, a.len_pen, n, smem);
}

// the pass's dynamic LDS: the rows' lists and the entries under selection, then (over them) the history gather
static size_t diverse_smem(int K, int step) {
  const size_t cand = (size_t)K * 2 * K * 16;
  const size_t hist = beam_history_lds(K, step);
  return cand > hist ? cand : hist;
}

}  // namespace ofa

using namespace ofa;

static int diverse_launch(const char* who, const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len,
                          int eos, int unk, float unk_penalty, int normalize, float len_penalty, int groups, float amount,
                          void* stream) {
  OFA_REQUIRE(ws, OFA_ERR_INVALID, "%s: null pointer", who);
  OFA_REQUIRE(bsz > 0 && V > 1 && step >= 0 && step <= max_len, OFA_ERR_INVALID, "%s: bsz=%d V=%d step=%d max_len=%d", who, bsz, V,
              step, max_len);
  if (const int rc = beam_check_state(who, st, K, step, true)) return rc;
  OFA_REQUIRE((int64_t)K * V < (1 << 24), OFA_ERR_UNSUPPORTED, "%s: beam * vocabulary must stay below 2^24", who);
  if (groups > 0) {
    OFA_REQUIRE(groups <= K && K % groups == 0, OFA_ERR_INVALID, "%s: beam %d is not divisible into %d groups", who, K, groups);
    OFA_REQUIRE(amount >= 0.f && amount <= 3.4e38f, OFA_ERR_INVALID,
                "%s: diversity strength %g must be finite and >= 0 (a reward leaves a row's top 2K)", who, (double)amount);
  } else {
    OFA_REQUIRE(V > 2 * K, OFA_ERR_INVALID, "%s: vocabulary %d must exceed 2 * beam = %d (every beam lists its own top 2K)", who, V,
                2 * K);
    OFA_REQUIRE(fabsf(amount) <= 3.4e38f, OFA_ERR_INVALID, "%s: diversity rate %g must be finite", who, (double)amount);
  }
  const int S = beam_splits(V);
  OFA_REQUIRE(S * 2 * K <= 64 * DIVERSE_PER_LANE, OFA_ERR_UNSUPPORTED,
              "%s: beam %d x %d vocabulary parts list %d candidates a row, above %d", who, K, S, S * 2 * K, 64 * DIVERSE_PER_LANE);
  const size_t smem = diverse_smem(K, step);
  OFA_REQUIRE(smem <= 65536, OFA_ERR_UNSUPPORTED, "%s: beam %d x step %d needs %zu bytes of LDS", who, K, step, smem);
  DiverseArgs a{beam_ws_carve(ws, (int64_t)bsz * K, S, K), bsz, K, V, S, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                groups, amount, *st};
  if (groups > 0) hipLaunchKernelGGL(diverse_select_kernel<true>, dim3(bsz), dim3(BEAM_THREADS), smem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(diverse_select_kernel<false>, dim3(bsz), dim3(BEAM_THREADS), smem, (hipStream_t)stream, a);
  return check_launch(who);
}

extern "C" int ofa_diverse_group_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos,
                                        int unk, float unk_penalty, int normalize, float len_penalty, int groups, float strength,
                                        void* stream) {
  OFA_REQUIRE(groups >= 1, OFA_ERR_INVALID, "ofa_diverse_group_select: %d groups", groups);
  return diverse_launch("ofa_diverse_group_select", ws, st, bsz, K, V, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                        groups, strength, stream);
}

extern "C" int ofa_diverse_sibling_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len,
                                          int eos, int unk, float unk_penalty, int normalize, float len_penalty, float rate,
                                          void* stream) {
  return diverse_launch("ofa_diverse_sibling_select", ws, st, bsz, K, V, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                        0, rate, stream);
}

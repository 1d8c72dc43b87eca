// What the beam-search row passes (beam_search.hip: ofa_beam_topk over [rows, V] logits; trie_beam.hip: ofa_trie_beam_topk over
// the child edges of a trie node; sample.hip: ofa_sample_draw) and the sentence passes (ofa_beam_select, ofa_sample_select,
// diverse_beam.hip: ofa_diverse_group_select / ofa_diverse_sibling_select) have in common, defined once: the limits, the workspace layout the row passes write and the sentence pass reads, the checks of the
// two descriptors of the C ABI (ofa_gen_policy, ofa_gen_state), the reference's post-normaliser masks in its order, the tie rules
// (value descending, token ascending, NaN = empty), the candidate-list machinery around the per-wave selection loops, which stay
// with their kernels (one selects over 16 register-held values per lane, the other over an LDS array strided by thread), and the
// bookkeeping of a step over a sentence's candidate list.  Device helpers and host helpers only: no kernels, no entry points.
#pragma once
#include "common.h"

namespace ofa {

constexpr int BEAM_MAX_K = 16;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_PER_LANE = 16;
constexpr int BEAM_CHUNK = BEAM_THREADS * BEAM_PER_LANE;   // vocabulary columns per part of the workspace layout

static inline int beam_splits(int V) { return (V + BEAM_CHUNK - 1) / BEAM_CHUNK; }

// ---------------------------------------------------------------- the workspace: S = beam_splits(V) parts per row
struct BeamWs {
  float* stats;                           // [rows, S, 2]  (max, sum exp(x - max)) of the part; NaN max: the part holds a NaN
  float* cval;                            // [rows, S, 2K] the part's best candidates, (value desc, token asc); value before the unk penalty
  int* ctok;                              // [rows, S, 2K] their tokens, -1: none
};
static inline int64_t beam_ws_cval_off(int64_t rows, int64_t S) { return rows * S * 2; }                      // in 4-byte words
static inline int64_t beam_ws_ctok_off(int64_t rows, int64_t S, int64_t K) { return beam_ws_cval_off(rows, S) + rows * S * 2 * K; }
static inline int64_t beam_ws_words(int64_t rows, int64_t S, int64_t K) { return beam_ws_ctok_off(rows, S, K) + rows * S * 2 * K; }
static inline BeamWs beam_ws_carve(const void* ws, int64_t rows, int64_t S, int64_t K) {
  float* p = (float*)ws;
  return BeamWs{p, p + beam_ws_cval_off(rows, S), (int*)(p + beam_ws_ctok_off(rows, S, K))};
}

// ---------------------------------------------------------------- the descriptors' checks, before any launch; `who`: the entry point
// The policy of a row pass (ofa_gen_policy: it crosses the C ABI and, by value, the kernel arguments as it is).
static inline int beam_check_row_pass(const char* who, int rows, int V, int K, const ofa_gen_policy& p) {
  OFA_REQUIRE(K >= 1 && K <= BEAM_MAX_K, OFA_ERR_UNSUPPORTED, "%s: beam size %d outside [1, %d]", who, K, BEAM_MAX_K);
  OFA_REQUIRE(rows % K == 0, OFA_ERR_INVALID, "%s: rows %d not a multiple of the beam size %d", who, rows, K);
  OFA_REQUIRE((int64_t)K * V < (1 << 24), OFA_ERR_UNSUPPORTED, "%s: beam * vocabulary must stay below 2^24", who);
  OFA_REQUIRE(p.temperature > 0.f, OFA_ERR_INVALID, "%s: temperature must be > 0", who);
  OFA_REQUIRE(p.ngram <= 0 || (p.tokens && p.tok_ld > p.step), OFA_ERR_INVALID, "%s: n-gram bans need the token history", who);
  return OFA_OK;
}

// The sentence state at `step` (>= 0).  fin: the caller finalises hypotheses, so the fin_* buffers are needed as well.
static inline int beam_check_state(const char* who, const ofa_gen_state* st, int K, int step, bool fin) {
  OFA_REQUIRE(st && st->tokens && st->scores && st->ignore && st->done && st->nfin && st->reorder &&
                  (!fin || (st->fin_tok && st->fin_pos && st->fin_score && st->fin_len && st->fin_cnt)),
              OFA_ERR_INVALID, "%s: null pointer", who);
  OFA_REQUIRE(K >= 1 && K <= BEAM_MAX_K, OFA_ERR_UNSUPPORTED, "%s: beam size %d outside [1, %d]", who, K, BEAM_MAX_K);
  OFA_REQUIRE(st->tok_cap >= step + 1 && st->tok_ld >= st->tok_cap && st->score_ld > step && (!fin || st->fin_ld > step), OFA_ERR_INVALID,
              "%s: history buffers too short for step %d (tok_cap=%d tok_ld=%lld score_ld=%lld fin_ld=%lld)", who, step, st->tok_cap,
              (long long)st->tok_ld, (long long)st->score_ld, (long long)st->fin_ld);
  return OFA_OK;
}

// dynamic LDS of the sentence pass's in-place history gather: K rows of step + 1 tokens and step scores
static inline size_t beam_history_lds(int K, int step) { return (size_t)K * (step + 1) * 8 + (size_t)K * step * 4; }

// ---------------------------------------------------------------- device side
// wave arg-max of (key desc, idx asc) over the lanes; NaN keys are empty.  Returns false when every lane is empty.
__device__ __forceinline__ bool wave_argmax(float key, int idx, float& mx, int& mi) {
  mx = wave_max(key);
  if (mx != mx) return false;
  const float neg = (key == mx) ? -(float)idx : -INFINITY;     // indices < 2^24: exact as float
  mi = (int)(-wave_max(neg));
  return true;
}

// LDS scratch of the list machinery of one 256-thread workgroup: every wave's sorted list and its part of the normaliser
struct BeamListScratch {
  float lkey[4][2 * BEAM_MAX_K], lval[4][2 * BEAM_MAX_K];
  int ltok[4][2 * BEAM_MAX_K];
  float red_m[4], red_s[4];
  int red_nan[4];
};
static_assert(sizeof(BeamListScratch) % 16 == 0, "embedded in front of 16-byte aligned LDS data");

// n-gram bans of a row (utils/ngram_repeat_block.py over the history tokens[row, 0..step]): every earlier occurrence of the row's
// last n-1 tokens bans the token that followed it; ban(token) is called by the thread that found the occurrence.
// plen >= 0: the sample carries prefix_tokens and the row's prefix has plen tokens -- the reference then skips the rows with
// plen >= step + n - 1 (sequence_generator.py:327-334).
template <typename Sink>
__device__ __forceinline__ void beam_ngram_scan(const ofa_gen_policy& p, int row, int tid, Sink ban, int plen = -1) {
  const int n = p.ngram;
  if (n > 0 && p.step + 2 - n >= 0 && plen < p.step + n - 1) {
    const int64_t* h = p.tokens + (int64_t)row * p.tok_ld;
    const int last = p.step - n + 2;                        // the row's last n-1 tokens start here
    for (int i = tid; i + n - 1 <= p.step; i += BEAM_THREADS) {
      bool match = true;
      for (int q = 0; q < n - 1; ++q) match = match && (h[i + q] == h[last + q]);
      if (match) ban(h[i + n - 1]);
    }
  }
}

// A row's fp32 normaliser from its S parts (max, sum); bad: a part held a NaN or the result is not finite -- the whole row is -inf.
__device__ __forceinline__ float beam_row_lse(const float* st, int S, bool& bad) {
  float M = -INFINITY;
  bool isnan_ = false;
  for (int s = 0; s < S; ++s) {
    const float ms = st[2 * s];
    if (ms != ms) isnan_ = true; else M = fmaxf(M, ms);
  }
  float sum = 0.f;
  for (int s = 0; s < S; ++s)
    if (st[2 * s] != -INFINITY) sum += st[2 * s + 1] * expf(st[2 * s] - M);
  const float l = M + logf(sum);
  bad = isnan_ || !(fabsf(l) <= 3.4e38f);
  return l;
}

// The workgroup's part of the fp32 normaliser: m = the lane's max over its non-NaN values, has_nan = it saw a NaN,
// lane_sum(M) = the lane's sum of exp(value - M) given its wave's max.  Thread 0 stores (max, sum) -- NaN max for a part
// that holds a NaN -- to st.  Contains a workgroup barrier: LDS written before the call is visible to every thread after it.
template <typename LaneSum>
__device__ __forceinline__ void beam_normaliser_part(BeamListScratch& sh, int tid, float m, int has_nan, LaneSum lane_sum, float* st) {
  const int lane = tid & 63, wave = tid >> 6;
  m = wave_max(m);
  float s = 0.f;
  if (m != -INFINITY) s = lane_sum(m);
  s = wave_sum(s);
  has_nan = __any(has_nan) ? 1 : 0;
  if (lane == 0) { sh.red_m[wave] = m; sh.red_s[wave] = s; sh.red_nan[wave] = has_nan; }
  __syncthreads();
  if (tid == 0) {
    const float M = fmaxf(fmaxf(sh.red_m[0], sh.red_m[1]), fmaxf(sh.red_m[2], sh.red_m[3]));
    float S = 0.f;
    for (int w = 0; w < 4; ++w)
      if (sh.red_m[w] != -INFINITY) S += sh.red_s[w] * expf(sh.red_m[w] - M);
    const bool bad = sh.red_nan[0] | sh.red_nan[1] | sh.red_nan[2] | sh.red_nan[3];
    st[0] = bad ? NAN : M;
    st[1] = S;
  }
}

// The masks after the normaliser for value v of token c, in the reference's order (sequence_generator.py:296-311, 319-343):
// EOS at step < min_len, NaN -> -inf, PAD, step >= max_len: all but EOS, n-gram bans, unk -= unk_penalty.  Returns the
// ordering key; the penalty orders only -- unk_val keeps the value of unk, and the sentence pass subtracts the penalty after
// the normaliser.
__device__ __forceinline__ float beam_mask_key(const ofa_gen_policy& p, float v, int c, bool banned, float& unk_val) {
  if (c == p.eos && p.step < p.min_len) v = -INFINITY;
  if (v != v) v = -INFINITY;
  if (c == p.pad) v = -INFINITY;
  if (p.step >= p.max_len && c != p.eos) v = -INFINITY;
  if (banned) v = -INFINITY;
  if (c == p.unk) { unk_val = v; v = v - p.unk_penalty; }
  return v;
}

// a wave whose candidates ran out after `it` entries closes its sorted list
__device__ __forceinline__ void beam_close_list(BeamListScratch& sh, int wave, int lane, int it, int K2) {
  if (lane == 0) for (int r = it; r < K2; ++r) { sh.lkey[wave][r] = NAN; sh.ltok[wave][r] = -1; }
}

// Wave 0 merges the four waves' sorted lists (<= 128 entries: two per lane) into ov / ot, (key desc, token asc); returns the
// number of entries written (< K2: the lists ran out; the caller fills the tail).  listed: if given, an LDS copy of ot.
__device__ __forceinline__ int beam_merge_lists(const BeamListScratch& sh, int lane, int K2, float* ov, int* ot, int* listed = nullptr) {
  float k0 = NAN, k1 = NAN;
  int t0 = 0x7fffffff, t1 = 0x7fffffff;
  const int e0 = lane, e1 = lane + 64;
  if (e0 < 4 * K2 && sh.ltok[e0 / K2][e0 % K2] >= 0) { k0 = sh.lkey[e0 / K2][e0 % K2]; t0 = sh.ltok[e0 / K2][e0 % K2]; }
  if (e1 < 4 * K2 && sh.ltok[e1 / K2][e1 % K2] >= 0) { k1 = sh.lkey[e1 / K2][e1 % K2]; t1 = sh.ltok[e1 / K2][e1 % K2]; }
  int it = 0;
  for (; it < K2; ++it) {
    const bool use0 = k0 == k0 && (!(k1 == k1) || k0 > k1 || (k0 == k1 && t0 < t1));
    const float lb = use0 ? k0 : k1;
    const int lt = use0 ? t0 : t1;
    float mx; int mt;
    if (!wave_argmax(lb, lt, mx, mt)) break;
    if (lb == lb && lt == mt) {
      const int e = use0 ? e0 : e1;
      ov[it] = sh.lval[e / K2][e % K2];
      ot[it] = mt;
      if (listed) listed[it] = mt;
      if (use0) k0 = NAN; else k1 = NAN;
    }
  }
  return it;
}

// ---------------------------------------------------------------- the sentence pass after its candidate list
// LDS of one sentence: the caller stages the list -- n entries of (cumulative score, source beam, token), best first -- in sel_*
struct BeamSentScratch {
  float sel_sc[2 * BEAM_MAX_K];
  int sel_beam[2 * BEAM_MAX_K], sel_tok[2 * BEAM_MAX_K];
  int act_beam[BEAM_MAX_K], act_tok[BEAM_MAX_K], new_ign[BEAM_MAX_K];
  float act_sc[BEAM_MAX_K];
  int fin_beam[BEAM_MAX_K], fin_slot[BEAM_MAX_K];
  float fin_sc[BEAM_MAX_K];
  int nfin_jobs, finished;
};

// The bookkeeping of one step (sequence_generator.py:345-492, finalize_hypos :530-627) for sentence `sent` over the n <= 2K
// candidates staged in sh (n = K for sampling: slot j's one draw): the EOS candidates among the first K are finalised, the K
// active candidates picked (the active_mask topk), cands_to_ignore carried, the token / score histories gathered in place through
// `lds` (beam_history_lds bytes, free to overwrite), reorder written.  A sentence with K hypotheses or at step == max_len sets its
// done flag, bumps the all-finished counter and keeps the identity reorder.  Call it after the barrier that publishes the list.
__device__ __forceinline__ void beam_sentence_step(const ofa_gen_state& a, BeamSentScratch& sh, int sent, int K, int step, int max_len,
                                                   int eos, int normalize, float len_pen, int n, void* lds) {
  const int tid = threadIdx.x, r0 = sent * K;
  if (tid == 0) {                                            // one thread, <= 2K candidates
    bool eosm[2 * BEAM_MAX_K];
    for (int j = 0; j < n; ++j) {
      eosm[j] = sh.sel_tok[j] == eos && sh.sel_sc[j] != -INFINITY;
      if (j < K && a.ignore[r0 + j]) eosm[j] = false;
    }
    int cnt = a.fin_cnt[sent], jobs = 0;
    for (int j = 0; j < n && j < K; ++j) {
      if (!eosm[j]) continue;
      if (cnt < K) {
        sh.fin_beam[jobs] = sh.sel_beam[j];
        sh.fin_slot[jobs] = cnt;
        sh.fin_sc[jobs] = sh.sel_sc[j];
        ++jobs;
        ++cnt;
      }
    }
    a.fin_cnt[sent] = cnt;
    sh.nfin_jobs = jobs;
    const int fin = (cnt == K || step >= max_len) ? 1 : 0;
    sh.finished = fin;
    if (fin) {
      a.done[sent] = 1;
      atomicAdd(a.nfin, 1);
    } else {
      // active_mask = eos_mask * cand_size + offset; its K smallest: the first K unmasked candidates, then the masked ones
      int nb = 0;
      for (int pass = 0; pass < 2 && nb < K; ++pass)
        for (int j = 0; j < n && nb < K; ++j) {
          const bool masked = eosm[j] || (j < K && a.ignore[r0 + j]);
          if (masked != (pass == 1)) continue;
          sh.act_beam[nb] = sh.sel_beam[j];
          sh.act_tok[nb] = sh.sel_tok[j];
          sh.act_sc[nb] = sh.sel_sc[j];
          sh.new_ign[nb] = masked ? 1 : 0;
          ++nb;
        }
    }
  }
  __syncthreads();
  // ---- finalised hypotheses: tokens 1..step then EOS, positional scores as differences of the cumulative scores
  const int jobs = sh.nfin_jobs;
  const int len = step + 1;
  for (int e = tid; e < jobs * len; e += BEAM_THREADS) {
    const int q = e / len, i = e % len;
    const int64_t row = r0 + sh.fin_beam[q];
    const int slot = sh.fin_slot[q];
    const int64_t o = ((int64_t)sent * K + slot) * a.fin_ld + i;
    a.fin_tok[o] = i < step ? a.tokens[row * a.tok_ld + i + 1] : (int64_t)eos;
    const float cur = i < step ? a.scores[row * a.score_ld + i] : sh.fin_sc[q];
    const float prev = i > 0 ? a.scores[row * a.score_ld + i - 1] : 0.f;
    a.fin_pos[o] = i > 0 ? cur - prev : cur;
  }
  if (tid < jobs) {
    const int slot = sh.fin_slot[tid];
    float sc = sh.fin_sc[tid];
    if (normalize) sc = sc / (float)pow((double)len, (double)len_pen);
    a.fin_score[sent * K + slot] = sc;
    a.fin_len[sent * K + slot] = len;
  }
  if (sh.finished) {
    if (tid < K) a.reorder[r0 + tid] = r0 + tid;
    return;
  }
  __syncthreads();                                           // finalisation read the old histories
  // ---- gather the K rows' histories in place: LDS copy of the sentence's rows, then the selected rows back
  int64_t* htok = (int64_t*)lds;                             // [K][step + 1]
  float* hsc = (float*)(htok + K * len);                     // [K][step]
  for (int e = tid; e < K * len; e += BEAM_THREADS) {
    const int b = e / len, i = e % len;
    htok[e] = a.tokens[(int64_t)(r0 + b) * a.tok_ld + i];
  }
  for (int e = tid; e < K * step; e += BEAM_THREADS) {
    const int b = e / step, i = e % step;
    hsc[e] = a.scores[(int64_t)(r0 + b) * a.score_ld + i];
  }
  __syncthreads();
  for (int e = tid; e < K * len; e += BEAM_THREADS) {
    const int b = e / len, i = e % len;
    a.tokens[(int64_t)(r0 + b) * a.tok_ld + i] = htok[sh.act_beam[b] * len + i];
  }
  for (int e = tid; e < K * step; e += BEAM_THREADS) {
    const int b = e / step, i = e % step;
    a.scores[(int64_t)(r0 + b) * a.score_ld + i] = hsc[sh.act_beam[b] * step + i];
  }
  if (tid < K) {
    const int64_t row = r0 + tid;
    if (step + 1 < a.tok_cap) a.tokens[row * a.tok_ld + step + 1] = sh.act_tok[tid];
    a.scores[row * a.score_ld + step] = sh.act_sc[tid];
    a.reorder[row] = r0 + sh.act_beam[tid];
    a.ignore[row] = sh.new_ign[tid];
  }
}

}  // namespace ofa

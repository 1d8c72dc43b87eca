// Beam-search step for gfx950: the policy of the reference's SequenceGenerator (generator/sequence_generator.py:283-492,
// 530-627) and BeamSearch.step (utils/search.py:107-142), in two launches per decoding step that take only fixed device
// addresses and the step number, so they are recorded inside the per-step hipGraph (ofasys_amd/generator.py).
//
// 1. ofa_beam_topk -- the row pass.  Grid (splits, rows): a 256-thread workgroup reads ONE 4096-column chunk of one logits row
//    exactly once (16 columns per lane, held in registers) and writes
//      - the chunk's part of the fp32 log-softmax normaliser of x/T: (max, sum exp(x/T - max)), NaN max when the chunk holds a NaN;
//      - the chunk's best 2K candidates (raw value x/T after the masks below, token), sorted by (value desc, token asc).
//    Masks that change the normaliser (applied first): temperature (:724), constraint_range (:742-745: [4, start) and [end, V)
//    are -inf).  Masks after the normaliser (:296-311, 319-343, in the reference's order): EOS at step < min_len, NaN -> -inf,
//    PAD, unk -= unk_penalty (ordering only; the value keeps x/T, the select pass subtracts the penalty after the normaliser),
//    step >= max_len: all but EOS, n-gram bans (utils/ngram_repeat_block.py: every earlier occurrence of the row's last n-1
//    tokens bans the token that followed it; BOS included).  Selection per wave is an iterative arg-max over the lanes'
//    registers (2K rounds of two DPP reductions); the four waves' lists are merged the same way by wave 0.
// 2. ofa_beam_select -- the sentence pass, one workgroup per sentence.  Combines each beam row's normaliser parts, turns the
//    row candidates into scores (lprob + cumulative score), merges the K x splits sorted lists into the sentence's top
//    k = min(2K, K*V - 1) (beam 0 only at step 0; ties to the lower flat index beam*V + token, as torch.topk on the
//    reference's CPU path), finalises the EOS candidates among the first K (finalize_hypos), picks the K active candidates
//    (the active_mask topk), carries cands_to_ignore, and gathers the token / score histories in place.  A finished sentence
//    (K hypotheses or step == max_len) sets its done flag, bumps the all-finished counter and is a no-op afterwards; its rows
//    keep the identity reorder.
#include "beam_common.h"

namespace ofa {

struct BeamTopkArgs {
  const void* logits; int64_t ld;
  int rows, V, K, S;
  int cstart, cend;
  BeamPolicy p;
  BeamWs ws;
};

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_topk_kernel(BeamTopkArgs a) {
  const int split = blockIdx.x, row = blockIdx.y;
  const BeamPolicy& p = a.p;
  if (p.done && p.done[row / a.K]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = split * BEAM_CHUNK, K2 = 2 * a.K;
  const int64_t part = (int64_t)row * a.S + split;
  __shared__ uint32_t ban[BEAM_CHUNK / 32];
  __shared__ BeamListScratch sh;

  // ---- the row's logits chunk: one read, 16 columns per lane in flight together
  const T* src = (const T*)a.logits + (int64_t)row * a.ld;
  float x[BEAM_PER_LANE];
#pragma unroll
  for (int j = 0; j < BEAM_PER_LANE; ++j) {
    const int c = base + wave * (64 * BEAM_PER_LANE) + j * 64 + lane;
    x[j] = c < a.V ? ld1<T>(src + c) : 0.f;
  }
  for (int i = tid; i < BEAM_CHUNK / 32; i += BEAM_THREADS) ban[i] = 0u;
  __syncthreads();
  // ---- n-gram bans of this row, as a bitmap over the chunk
  beam_ngram_scan(p, row, tid, [&](int64_t tok) {
    const int64_t col = tok - base;
    if (col >= 0 && col < BEAM_CHUNK) atomicOr(&ban[col >> 5], 1u << (col & 31));
  });
  // ---- pre-normaliser masks + the chunk's normaliser part
  float m = -INFINITY;
  int has_nan = 0;
#pragma unroll
  for (int j = 0; j < BEAM_PER_LANE; ++j) {
    const int c = base + wave * (64 * BEAM_PER_LANE) + j * 64 + lane;
    float v = x[j];
    if (p.temperature != 1.f) v = v / p.temperature;
    if (a.cstart >= 0 && ((c >= 4 && c < a.cstart) || c >= a.cend)) v = -INFINITY;
    x[j] = v;
    if (c < a.V) {
      if (v != v) has_nan = 1;
      else m = fmaxf(m, v);
    }
  }
  beam_normaliser_part(sh, tid, m, has_nan, [&](float wm) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < BEAM_PER_LANE; ++j) {
      const int c = base + wave * (64 * BEAM_PER_LANE) + j * 64 + lane;
      if (c < a.V && x[j] == x[j]) s += expf(x[j] - wm);
    }
    return s;
  }, a.ws.stats + part * 2);                                // (its barrier also orders the ban bitmap)
  // ---- post-normaliser masks -> ordering keys (NaN key = no candidate; -inf stays a candidate)
  float unk_val = 0.f;
#pragma unroll
  for (int j = 0; j < BEAM_PER_LANE; ++j) {
    const int c = base + wave * (64 * BEAM_PER_LANE) + j * 64 + lane;
    const bool banned = c < a.V && (ban[(c - base) >> 5] >> ((c - base) & 31)) & 1u;
    const float v = beam_mask_key(p, x[j], c, banned, unk_val);
    x[j] = c < a.V ? v : NAN;
  }
  // ---- per-wave top 2K, sorted
  for (int it = 0; it < K2; ++it) {
    float lb = NAN;
    int lj = -1;
#pragma unroll
    for (int j = 0; j < BEAM_PER_LANE; ++j)
      if (x[j] == x[j] && (lj < 0 || x[j] > lb)) { lb = x[j]; lj = j; }
    const int lc = lj < 0 ? 0x7fffffff : base + wave * (64 * BEAM_PER_LANE) + lj * 64 + lane;
    float mx; int mc;
    if (!wave_argmax(lb, lc, mx, mc)) {
      beam_close_list(sh, wave, lane, it, K2);
      break;
    }
    if (lj >= 0 && lc == mc) {
      sh.lkey[wave][it] = lb;
      sh.lval[wave][it] = mc == p.unk ? unk_val : lb;
      sh.ltok[wave][it] = mc;
#pragma unroll
      for (int j = 0; j < BEAM_PER_LANE; ++j)
        if (j == lj) x[j] = NAN;
    }
  }
  __syncthreads();
  if (wave == 0) {
    float* ov = a.ws.cval + part * K2;
    int* ot = a.ws.ctok + part * K2;
    const int got = beam_merge_lists(sh, lane, K2, ov, ot);
    if (lane == 0) for (int r = got; r < K2; ++r) { ov[r] = -INFINITY; ot[r] = -1; }
  }
}

struct BeamSelectArgs {
  BeamWs ws;
  int bsz, K, V, S, step, max_len, eos, unk; float unk_pen;
  int normalize; float len_pen;
  int64_t* tokens; int64_t tok_ld; int tok_cap;
  float* scores; int64_t score_ld;
  int* ignore; int* done; int* nfin; int64_t* reorder;
  int64_t* fin_tok; float* fin_pos; int64_t fin_ld; float* fin_score; int* fin_len; int* fin_cnt;
};

__global__ __launch_bounds__(BEAM_THREADS) void beam_select_kernel(BeamSelectArgs a) {
  const int sent = blockIdx.x;
  if (a.done[sent]) return;                                  // finished: a no-op from then on
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, K2 = 2 * K, step = a.step, r0 = sent * K;
  const int nr = step == 0 ? 1 : K;                          // step 0: beam 0 only (search.py:126-129)
  const int L = nr * a.S;                                    // sorted candidate lists
  extern __shared__ float smem[];
  float* csc = smem;                                         // [L * 2K] scores (NaN: empty)
  int* cfl = (int*)(csc + L * K2);                           // [L * 2K] flat index beam * V + token
  int* pos = cfl + L * K2;                                   // [L] list heads
  __shared__ float lse[BEAM_MAX_K], cum[BEAM_MAX_K];
  __shared__ int bad[BEAM_MAX_K];
  __shared__ float sel_sc[2 * BEAM_MAX_K];
  __shared__ int sel_fl[2 * BEAM_MAX_K];
  __shared__ int act_beam[BEAM_MAX_K], act_tok[BEAM_MAX_K], new_ign[BEAM_MAX_K];
  __shared__ float act_sc[BEAM_MAX_K];
  __shared__ int fin_beam[BEAM_MAX_K], fin_slot[BEAM_MAX_K];
  __shared__ float fin_sc[BEAM_MAX_K];
  __shared__ int nfin_jobs, finished, nsel;

  // ---- each beam row's normaliser from its splits' parts
  if (tid < nr) {
    const float* st = a.ws.stats + (int64_t)(r0 + tid) * a.S * 2;
    float M = -INFINITY;
    bool isnan_ = false;
    for (int s = 0; s < a.S; ++s) {
      const float ms = st[2 * s];
      if (ms != ms) isnan_ = true; else M = fmaxf(M, ms);
    }
    float S = 0.f;
    for (int s = 0; s < a.S; ++s)
      if (st[2 * s] != -INFINITY) S += st[2 * s + 1] * expf(st[2 * s] - M);
    const float l = M + logf(S);
    lse[tid] = l;
    bad[tid] = isnan_ || !(fabsf(l) <= 3.4e38f);             // NaN or infinite: the whole row is -inf (log_softmax -> NaN -> -inf)
    cum[tid] = step > 0 ? a.scores[(int64_t)(r0 + tid) * a.score_ld + step - 1] : 0.f;
  }
  __syncthreads();
  // ---- candidates -> scores (lprob + cumulative score, search.py:131), staged in LDS
  for (int e = tid; e < L * K2; e += BEAM_THREADS) {
    const int li = e / K2, j = e % K2, r = li / a.S, s = li % a.S;
    float sc = NAN;
    int tok = -1;
    if (bad[r]) {                                            // all -inf: the lowest tokens win the ties
      if (s == 0 && j < a.V) { tok = j; sc = -INFINITY; }
    } else {
      const int64_t off = ((int64_t)(r0 + r) * a.S + s) * K2 + j;
      tok = a.ws.ctok[off];
      if (tok >= 0) {
        float lp = a.ws.cval[off] - lse[r];
        if (tok == a.unk) lp = lp - a.unk_pen;
        if (lp != lp) lp = -INFINITY;
        sc = step > 0 ? lp + cum[r] : lp;
      }
    }
    csc[e] = sc;
    cfl[e] = tok < 0 ? 0x7fffffff : r * a.V + tok;
  }
  for (int li = tid; li < L; li += BEAM_THREADS) pos[li] = 0;
  __syncthreads();
  // ---- merge the sorted lists into the sentence's top k (wave 0)
  const int64_t avail = (int64_t)nr * a.V - 1;
  const int kk = (int)(avail < K2 ? avail : K2);
  if (wave == 0) {
    int got = 0;
    for (int it = 0; it < kk; ++it) {
      float lb = NAN;
      int lf = 0x7fffffff, lli = -1;
      for (int li = lane; li < L; li += 64) {
        const int p = pos[li];
        if (p >= K2) continue;
        const float sc = csc[li * K2 + p];
        const int fl = cfl[li * K2 + p];
        if (!(sc == sc)) continue;
        if (lli < 0 || sc > lb || (sc == lb && fl < lf)) { lb = sc; lf = fl; lli = li; }
      }
      float mx; int mf;
      if (!wave_argmax(lb, lf, mx, mf)) break;
      if (lli >= 0 && lf == mf) {
        pos[lli] += 1;
        sel_sc[it] = mx;
        sel_fl[it] = mf;
      }
      ++got;
    }
    if (lane == 0) nsel = got;
  }
  __syncthreads();
  // ---- bookkeeping of one step (sequence_generator.py:345-492, finalize_hypos :530-627): one thread, <= 2K candidates
  if (tid == 0) {
    const int k = nsel;
    bool eosm[2 * BEAM_MAX_K];
    for (int j = 0; j < k; ++j) {
      const int tok = sel_fl[j] % a.V;
      eosm[j] = tok == a.eos && sel_sc[j] != -INFINITY;
      if (j < K && a.ignore[r0 + j]) eosm[j] = false;
    }
    int cnt = a.fin_cnt[sent], jobs = 0;
    for (int j = 0; j < k && j < K; ++j) {
      if (!eosm[j]) continue;
      if (cnt < K) {
        fin_beam[jobs] = sel_fl[j] / a.V;
        fin_slot[jobs] = cnt;
        fin_sc[jobs] = sel_sc[j];
        ++jobs;
        ++cnt;
      }
    }
    a.fin_cnt[sent] = cnt;
    nfin_jobs = jobs;
    const int fin = (cnt == K || step >= a.max_len) ? 1 : 0;
    finished = fin;
    if (fin) {
      a.done[sent] = 1;
      atomicAdd(a.nfin, 1);
    } else {
      // active_mask = eos_mask * cand_size + offset; its K smallest: the first K unmasked candidates, then the masked ones
      int nb = 0;
      for (int pass = 0; pass < 2 && nb < K; ++pass)
        for (int j = 0; j < k && nb < K; ++j) {
          const bool masked = eosm[j] || (j < K && a.ignore[r0 + j]);
          if (masked != (pass == 1)) continue;
          act_beam[nb] = sel_fl[j] / a.V;
          act_tok[nb] = sel_fl[j] % a.V;
          act_sc[nb] = sel_sc[j];
          new_ign[nb] = masked ? 1 : 0;
          ++nb;
        }
    }
  }
  __syncthreads();
  // ---- finalised hypotheses: tokens 1..step then EOS, positional scores as differences of the cumulative scores
  const int jobs = nfin_jobs;
  const int len = step + 1;
  for (int e = tid; e < jobs * len; e += BEAM_THREADS) {
    const int q = e / len, i = e % len;
    const int64_t row = r0 + fin_beam[q];
    const int slot = fin_slot[q];
    const int64_t o = ((int64_t)sent * K + slot) * a.fin_ld + i;
    a.fin_tok[o] = i < step ? a.tokens[row * a.tok_ld + i + 1] : (int64_t)a.eos;
    const float cur = i < step ? a.scores[row * a.score_ld + i] : fin_sc[q];
    const float prev = i > 0 ? a.scores[row * a.score_ld + i - 1] : 0.f;
    a.fin_pos[o] = i > 0 ? cur - prev : cur;
  }
  if (tid < jobs) {
    const int slot = fin_slot[tid];
    float sc = fin_sc[tid];
    if (a.normalize) sc = sc / (float)pow((double)len, (double)a.len_pen);
    a.fin_score[sent * K + slot] = sc;
    a.fin_len[sent * K + slot] = len;
  }
  if (finished) {
    if (tid < K) a.reorder[r0 + tid] = r0 + tid;
    return;
  }
  __syncthreads();                                           // finalisation read the old histories
  // ---- gather the K rows' histories in place: LDS copy of the sentence's rows, then the selected rows back
  int64_t* htok = (int64_t*)smem;                            // [K][step + 1]
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
    a.tokens[(int64_t)(r0 + b) * a.tok_ld + i] = htok[act_beam[b] * len + i];
  }
  for (int e = tid; e < K * step; e += BEAM_THREADS) {
    const int b = e / step, i = e % step;
    a.scores[(int64_t)(r0 + b) * a.score_ld + i] = hsc[act_beam[b] * step + i];
  }
  if (tid < K) {
    const int64_t row = r0 + tid;
    if (step + 1 < a.tok_cap) a.tokens[row * a.tok_ld + step + 1] = act_tok[tid];
    a.scores[row * a.score_ld + step] = act_sc[tid];
    a.reorder[row] = r0 + act_beam[tid];
    a.ignore[row] = new_ign[tid];
  }
}

static size_t select_smem(int K, int S, int step) {
  const int nr = step == 0 ? 1 : K, L = nr * S;
  const size_t cand = (size_t)L * 2 * K * 8 + (size_t)L * 4;
  const size_t hist = (size_t)K * (step + 1) * 8 + (size_t)K * step * 4;
  return cand > hist ? cand : hist;
}

}  // namespace ofa

using namespace ofa;

extern "C" int64_t ofa_beam_ws_bytes(int rows, int V, int K) {
  if (rows <= 0 || V <= 0 || K <= 0) return 0;
  return beam_ws_words(rows, beam_splits(V), K) * 4;
}

extern "C" int ofa_beam_topk(const void* logits, int64_t ld, int rows, int V, int K, float temperature, int cstart, int cend,
                             int step, int min_len, int max_len, int pad, int unk, int eos, float unk_penalty, int ngram,
                             const int64_t* tokens, int64_t tok_ld, const int* done, void* ws, int dtype, void* stream) {
  OFA_REQUIRE(logits && ws, OFA_ERR_INVALID, "ofa_beam_topk: null pointer");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ofa_beam_topk: bad dtype %d", dtype);
  OFA_REQUIRE(rows > 0 && V > 1 && ld >= V && step >= 0, OFA_ERR_INVALID, "ofa_beam_topk: rows=%d V=%d ld=%lld step=%d", rows, V,
              (long long)ld, step);
  if (const int rc = beam_check_row_pass("ofa_beam_topk", rows, V, K, temperature, step, ngram, tokens, tok_ld)) return rc;
  const int S = beam_splits(V);
  BeamTopkArgs a{logits, ld, rows, V, K, S, cstart, cend,
                 BeamPolicy{temperature, step, min_len, max_len, pad, unk, eos, unk_penalty, ngram, tokens, tok_ld, done},
                 beam_ws_carve(ws, rows, S, K)};
  dim3 grid(S, rows);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == OFA_F32) hipLaunchKernelGGL(beam_topk_kernel<float>, grid, dim3(BEAM_THREADS), 0, st, a);
  else if (dtype == OFA_BF16) hipLaunchKernelGGL(beam_topk_kernel<bf16_t>, grid, dim3(BEAM_THREADS), 0, st, a);
  else hipLaunchKernelGGL(beam_topk_kernel<f16_t>, grid, dim3(BEAM_THREADS), 0, st, a);
  return check_launch("ofa_beam_topk");
}

extern "C" int ofa_beam_select(const void* ws, int bsz, int K, int V, int step, int max_len, int eos, int unk, float unk_penalty,
                               int normalize, float len_penalty, int64_t* tokens, int64_t tok_ld, int tok_cap, float* scores,
                               int64_t score_ld, int* ignore, int* done, int* nfin, int64_t* reorder, int64_t* fin_tok,
                               float* fin_pos, int64_t fin_ld, float* fin_score, int* fin_len, int* fin_cnt, void* stream) {
  OFA_REQUIRE(ws && tokens && scores && ignore && done && nfin && reorder && fin_tok && fin_pos && fin_score && fin_len && fin_cnt,
              OFA_ERR_INVALID, "ofa_beam_select: null pointer");
  OFA_REQUIRE(bsz > 0 && V > 1 && step >= 0 && step <= max_len, OFA_ERR_INVALID, "ofa_beam_select: bsz=%d V=%d step=%d max_len=%d",
              bsz, V, step, max_len);
  OFA_REQUIRE(K >= 1 && K <= BEAM_MAX_K, OFA_ERR_UNSUPPORTED, "ofa_beam_select: beam size %d outside [1, %d]", K, BEAM_MAX_K);
  OFA_REQUIRE((int64_t)K * V < (1 << 24), OFA_ERR_UNSUPPORTED, "ofa_beam_select: beam * vocabulary must stay below 2^24");
  OFA_REQUIRE(tok_cap >= step + 1 && tok_ld >= tok_cap && score_ld > step && fin_ld > step, OFA_ERR_INVALID,
              "ofa_beam_select: history buffers too short for step %d (tok_cap=%d tok_ld=%lld score_ld=%lld fin_ld=%lld)", step,
              tok_cap, (long long)tok_ld, (long long)score_ld, (long long)fin_ld);
  const int S = beam_splits(V);
  const size_t smem = select_smem(K, S, step);
  OFA_REQUIRE(smem <= 65536, OFA_ERR_UNSUPPORTED, "ofa_beam_select: beam %d x %d vocabulary splits x step %d needs %zu bytes of LDS",
              K, S, step, smem);
  BeamSelectArgs a{beam_ws_carve(ws, (int64_t)bsz * K, S, K), bsz, K, V, S, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                   tokens, tok_ld, tok_cap, scores, score_ld, ignore, done, nfin, reorder, fin_tok, fin_pos, fin_ld, fin_score,
                   fin_len, fin_cnt};
  hipLaunchKernelGGL(beam_select_kernel, dim3(bsz), dim3(BEAM_THREADS), smem, (hipStream_t)stream, a);
  return check_launch("ofa_beam_select");
}

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
//    keep the identity reorder.  Everything after the merge is beam_common.h's beam_sentence_step, which ofa_sample_select
//    (sample.hip) runs over its K-wide list as well.
// 3. Steps under a forced target prefix (sample["prefix_tokens"], sequence_generator.py:297-343, 497-523), three launches:
//    ofa_beam_prefix_topk -- the row pass above without the min_len mask; it also stores every row's scaled logit at its prefix
//    token, and a forced row (prefix token != pad) stops after its normaliser part: no selection loop.  ofa_beam_prefix_fill --
//    one workgroup per forced row: the batch-wide fill f = min(prefix lprobs) - 1 and the row's candidates under the tie rule, as
//    lprobs.  ofa_beam_prefix_select -- the sentence pass, taking a forced row's values as normalised.  On the free steps of such
//    a sample ofa_beam_prefix_topk (prefix = null) is the row pass of 1. with the n-gram bans following the prefix lengths.
#include "beam_common.h"

namespace ofa {

struct BeamTopkArgs {
  const void* logits; int64_t ld;
  int rows, V, K, S;
  ofa_gen_policy p;
  BeamWs ws;
  // ofa_beam_prefix_topk only (PREFIX): the forced tokens of this step (null: a free step), the prefix lengths, g's logit
  const int64_t* prefix; int64_t prefix_ld;
  const int* plen;
  float* glogit;
};

// The row pass of both entry points.  PREFIX (ofa_beam_prefix_topk): every row stores the scaled logit of its prefix token; a
// forced row (prefix token != pad) stops after its normaliser part -- its candidates come from beam_prefix_fill_kernel -- and the
// n-gram bans follow the prefix length.
template <typename T, bool PREFIX>
__device__ __forceinline__ void beam_row_pass(const BeamTopkArgs& a) {
  const int split = blockIdx.x, row = blockIdx.y;
  const ofa_gen_policy& p = a.p;
  if (p.done && p.done[row / a.K]) return;
  int64_t ftok = -1;                                         // the row's prefix token at this step (PREFIX, prefix step)
  bool forced = false;
  int plen = -1;
  if constexpr (PREFIX) {
    if (a.prefix) {
      ftok = a.prefix[(int64_t)(row / a.K) * a.prefix_ld + p.step];
      forced = ftok != p.pad;
    }
    plen = a.plen[row / a.K];
  }
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
  if (!forced)
    beam_ngram_scan(p, row, tid, [&](int64_t tok) {
      const int64_t col = tok - base;
      if (col >= 0 && col < BEAM_CHUNK) atomicOr(&ban[col >> 5], 1u << (col & 31));
    }, plen);
  // ---- pre-normaliser masks + the chunk's normaliser part
  float m = -INFINITY;
  int has_nan = 0;
#pragma unroll
  for (int j = 0; j < BEAM_PER_LANE; ++j) {
    const int c = base + wave * (64 * BEAM_PER_LANE) + j * 64 + lane;
    float v = x[j];
    if (p.temperature != 1.f) v = v / p.temperature;
    if (p.cstart >= 0 && ((c >= 4 && c < p.cstart) || c >= p.cend)) v = -INFINITY;
    x[j] = v;
    if (c < a.V) {
      if (v != v) has_nan = 1;
      else m = fmaxf(m, v);
      if constexpr (PREFIX) if (c == ftok) a.glogit[row] = v;
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
  if (forced) return;                                        // (the whole workgroup: one row)
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

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_topk_kernel(BeamTopkArgs a) { beam_row_pass<T, false>(a); }

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_prefix_row_kernel(BeamTopkArgs a) { beam_row_pass<T, true>(a); }

// ---- the candidates of the forced rows of a prefix step (ofa_beam_prefix_fill), one workgroup per forced row.
// f = min over the rows of every unfinished sentence of g[r] - 1 (g[r] = lprob of the row's prefix token, <pad> for a free row;
// torch.min: a NaN wins) is recomputed by every workgroup from the rows' normaliser parts and ofa_beam_prefix_topk's logits:
// rows x S x 2 floats from L2 and one thread per row, against a launch of its own in between.  The row's distribution is then
// f everywhere but at its prefix token; after the reference's later masks (NaN -> -inf, PAD, unk penalty, n-gram bans) and the
// tie rule its best 2K are the prefix token, the 2K lowest unmasked tokens at f and unk at f - unk_penalty, ranked.  They are
// written as split 0's list, ALREADY NORMALISED (the sentence pass takes a forced row's normaliser as 0), so every filled
// token of a row carries the identical float.  The host guarantees 2K unmasked tokens below BEAM_FILL_POOL.
constexpr int BEAM_FILL_POOL = 1024;

struct BeamFillArgs {
  BeamWs ws;
  int rows, V, K, S;
  const int64_t* prefix; int64_t prefix_ld;
  const int* plen;
  const float* glogit;
  ofa_gen_policy p;
};

__global__ __launch_bounds__(BEAM_THREADS) void beam_prefix_fill_kernel(BeamFillArgs a) {
  const int row = blockIdx.x, sent = row / a.K;
  const ofa_gen_policy& p = a.p;
  if (p.done && p.done[sent]) return;
  const int64_t ftok = a.prefix[(int64_t)sent * a.prefix_ld + p.step];
  if (ftok == p.pad) return;                                 // a free row: ofa_beam_prefix_topk listed its candidates
  if (p.step == 0 && row % a.K) return;                      // step 0 reads the first beam only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K2 = 2 * a.K;
  __shared__ float red_m[4];
  __shared__ int red_nan[4], wcnt[4];
  __shared__ float g_own;
  __shared__ uint32_t ban[BEAM_FILL_POOL / 32];
  __shared__ int ftok_banned;
  __shared__ int plain[2 * BEAM_MAX_K];
  __shared__ float ekey[2 * BEAM_MAX_K + 2], eval_[2 * BEAM_MAX_K + 2];
  __shared__ int etok[2 * BEAM_MAX_K + 2];

  // ---- f: the batch-wide minimum
  float mn = INFINITY;
  int has_nan = 0;
  for (int r = tid; r < a.rows; r += BEAM_THREADS) {
    if (p.done && p.done[r / a.K]) continue;
    bool bad;
    const float l = beam_row_lse(a.ws.stats + (int64_t)r * a.S * 2, a.S, bad);
    const float g = bad ? NAN : a.glogit[r] - l;
    if (g != g) has_nan = 1; else mn = fminf(mn, g);
    if (r == row) g_own = g;
  }
  for (int i = tid; i < BEAM_FILL_POOL / 32; i += BEAM_THREADS) ban[i] = 0u;
  if (tid == 0) ftok_banned = 0;
  mn = -wave_max(-mn);
  has_nan = __any(has_nan) ? 1 : 0;
  if (lane == 0) { red_m[wave] = mn; red_nan[wave] = has_nan; }
  __syncthreads();
  const bool f_nan = red_nan[0] | red_nan[1] | red_nan[2] | red_nan[3];
  const float fval = f_nan ? -INFINITY : fminf(fminf(red_m[0], red_m[1]), fminf(red_m[2], red_m[3])) - 1.f;   // NaN -> -inf
  const bool fin = fval != -INFINITY;
  // ---- n-gram bans of this row: a bitmap over the pool, and whether the prefix token is banned
  beam_ngram_scan(p, row, tid, [&](int64_t tok) {
    if (tok == ftok) ftok_banned = 1;
    if (tok >= 0 && tok < BEAM_FILL_POOL) atomicOr(&ban[tok >> 5], 1u << (tok & 31));
  }, a.plen[sent]);
  __syncthreads();
  // ---- the 2K lowest tokens that stay at f: not the prefix token and, unless f is -inf anyway, not masked and not unk
  const bool unk_apart = fin && p.unk_penalty != 0.f && p.unk != ftok && p.unk >= 0 && p.unk < a.V;
  int have = 0;
  for (int base = 0; base < BEAM_FILL_POOL && base < a.V && have < K2; base += BEAM_THREADS) {
    const int c = base + tid;
    const bool banned = (ban[c >> 5] >> (c & 31)) & 1u;
    const bool is_plain = c < a.V && c != ftok && (!fin || (c != p.pad && !(unk_apart && c == p.unk) && !banned));
    const unsigned long long mask = __ballot(is_plain);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int at = have + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += wcnt[w];
    if (is_plain && at < K2) plain[at] = c;
    have += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  if (have > K2) have = K2;
  // ---- rank the <= 2K + 2 entries by (key desc, token asc): the plain run, the prefix token, unk
  const int n = have + 1 + (unk_apart ? 1 : 0);
  if (tid < n) {
    float v = fval;
    int tok = 0;
    if (tid < have) tok = plain[tid];
    else if (tid == have) {
      tok = (int)ftok;
      v = g_own;
      if (v != v || ftok_banned) v = -INFINITY;
    } else {
      tok = p.unk;
      if ((ban[tok >> 5] >> (tok & 31)) & 1u) v = -INFINITY;
    }
    eval_[tid] = v;                                          // (before the unk penalty, as the layout has it)
    ekey[tid] = tok == p.unk ? v - p.unk_penalty : v;
    etok[tid] = tok;
  }
  __syncthreads();
  float* ov = a.ws.cval + (int64_t)row * a.S * K2;
  int* ot = a.ws.ctok + (int64_t)row * a.S * K2;
  if (tid < n) {
    int rank = 0;
    for (int e = 0; e < n; ++e) rank += (ekey[e] > ekey[tid] || (ekey[e] == ekey[tid] && etok[e] < etok[tid])) ? 1 : 0;
    if (rank < K2) { ov[rank] = eval_[tid]; ot[rank] = etok[tid]; }
  }
  const int listed = n < K2 ? n : K2;
  for (int e = listed + tid; e < a.S * K2; e += BEAM_THREADS) ot[e] = -1;     // the other splits hold nothing
}

struct BeamSelectArgs {
  BeamWs ws;
  int bsz, K, V, S, step, max_len, eos, unk; float unk_pen;
  int normalize; float len_pen;
  ofa_gen_state st;
  const int64_t* prefix; int64_t prefix_ld; int pad;        // ofa_beam_prefix_select: the forced tokens of this step (else null)
};

__global__ __launch_bounds__(BEAM_THREADS) void beam_select_kernel(BeamSelectArgs a) {
  const int sent = blockIdx.x;
  if (a.st.done[sent]) return;                               // finished: a no-op from then on
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
  __shared__ BeamSentScratch sh;
  __shared__ int nsel;

  // ---- each beam row's normaliser from its splits' parts
  if (tid < nr) {
    bool b;
    float l = beam_row_lse(a.ws.stats + (int64_t)(r0 + tid) * a.S * 2, a.S, b);
    if (a.prefix && a.prefix[(int64_t)sent * a.prefix_ld + step] != a.pad) { l = 0.f; b = false; }   // a forced row's list is normalised
    lse[tid] = l;
    bad[tid] = b;                                            // NaN or infinite: the whole row is -inf (log_softmax -> NaN -> -inf)
    cum[tid] = step > 0 ? a.st.scores[(int64_t)(r0 + tid) * a.st.score_ld + step - 1] : 0.f;
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
        sh.sel_sc[it] = mx;
        sh.sel_beam[it] = mf / a.V;
        sh.sel_tok[it] = mf % a.V;
      }
      ++got;
    }
    if (lane == 0) nsel = got;
  }
  __syncthreads();
  beam_sentence_step(a.st, sh, sent, K, step, a.max_len, a.eos, a.normalize, a.len_pen, nsel, smem);
}

// the sentence pass's dynamic LDS: the candidate lists, then (over them) the history gather
static size_t select_smem(int K, int S, int step) {
  const int nr = step == 0 ? 1 : K, L = nr * S;
  const size_t cand = (size_t)L * 2 * K * 8 + (size_t)L * 4;
  const size_t hist = beam_history_lds(K, step);
  return cand > hist ? cand : hist;
}

}  // namespace ofa

using namespace ofa;

// the two descriptors of the generation steps as kernels._GenPolicy / _GenState mirror them (natural alignment on both sides)
static_assert(sizeof(ofa_gen_policy) == 72, "ofa_gen_policy: 2 floats and 9 int32 (44 bytes, padded to 48), then 2 pointers and 1 int64");
static_assert(sizeof(ofa_gen_state) == 120, "ofa_gen_state: 11 pointers and 3 int64; tok_cap (int32) sits in an 8-byte slot");

extern "C" int64_t ofa_beam_ws_bytes(int rows, int V, int K) {
  if (rows <= 0 || V <= 0 || K <= 0) return 0;
  return beam_ws_words(rows, beam_splits(V), K) * 4;
}

// the row pass of ofa_beam_topk and ofa_beam_prefix_topk (plen: the latter's prefix lengths; prefix: a prefix step's forced tokens)
static int beam_topk_launch(const char* who, const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol,
                            const int64_t* prefix, int64_t prefix_ld, const int* plen, float* glogit, void* ws, int dtype,
                            void* stream) {
  OFA_REQUIRE(logits && ws && pol, OFA_ERR_INVALID, "%s: null pointer", who);
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(rows > 0 && V > 1 && ld >= V && pol->step >= 0, OFA_ERR_INVALID, "%s: rows=%d V=%d ld=%lld step=%d", who, rows, V,
              (long long)ld, pol->step);
  if (const int rc = beam_check_row_pass(who, rows, V, K, *pol)) return rc;
  const int S = beam_splits(V);
  BeamTopkArgs a{logits, ld, rows, V, K, S, *pol, beam_ws_carve(ws, rows, S, K), prefix, prefix_ld, plen, glogit};
  if (prefix) a.p.min_len = 0;       // a prefix step applies the min_len mask to no row (the `elif` of sequence_generator.py:297-301)
  dim3 grid(S, rows);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (plen) hipLaunchKernelGGL(beam_prefix_row_kernel<T>, grid, dim3(BEAM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(beam_topk_kernel<T>, grid, dim3(BEAM_THREADS), 0, st, a);
  });
  return check_launch(who);
}

extern "C" int ofa_beam_topk(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol, void* ws, int dtype,
                             void* stream) {
  return beam_topk_launch("ofa_beam_topk", logits, ld, rows, V, K, pol, nullptr, 0, nullptr, nullptr, ws, dtype, stream);
}

// the sentence pass of ofa_beam_select and ofa_beam_prefix_select (prefix: the forced tokens of a prefix step, else null)
static int beam_select_launch(const char* who, const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len,
                              int eos, int unk, float unk_penalty, int normalize, float len_penalty, const int64_t* prefix,
                              int64_t prefix_ld, int pad, void* stream) {
  OFA_REQUIRE(ws, OFA_ERR_INVALID, "%s: null pointer", who);
  OFA_REQUIRE(bsz > 0 && V > 1 && step >= 0 && step <= max_len, OFA_ERR_INVALID, "%s: bsz=%d V=%d step=%d max_len=%d", who,
              bsz, V, step, max_len);
  if (const int rc = beam_check_state(who, st, K, step, true)) return rc;
  OFA_REQUIRE((int64_t)K * V < (1 << 24), OFA_ERR_UNSUPPORTED, "%s: beam * vocabulary must stay below 2^24", who);
  const int S = beam_splits(V);
  const size_t smem = select_smem(K, S, step);
  OFA_REQUIRE(smem <= 65536, OFA_ERR_UNSUPPORTED, "%s: beam %d x %d vocabulary splits x step %d needs %zu bytes of LDS", who,
              K, S, step, smem);
  BeamSelectArgs a{beam_ws_carve(ws, (int64_t)bsz * K, S, K), bsz, K, V, S, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                   *st, prefix, prefix_ld, pad};
  hipLaunchKernelGGL(beam_select_kernel, dim3(bsz), dim3(BEAM_THREADS), smem, (hipStream_t)stream, a);
  return check_launch(who);
}

extern "C" int ofa_beam_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos, int unk,
                               float unk_penalty, int normalize, float len_penalty, void* stream) {
  return beam_select_launch("ofa_beam_select", ws, st, bsz, K, V, step, max_len, eos, unk, unk_penalty, normalize, len_penalty, nullptr,
                            0, 0, stream);
}

// ---------------------------------------------------------------- steps under a forced target prefix
extern "C" int ofa_beam_prefix_topk(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol,
                                    const int64_t* prefix, int64_t prefix_ld, const int* plen, float* glogit, void* ws, int dtype,
                                    void* stream) {
  OFA_REQUIRE(pol && plen, OFA_ERR_INVALID, "ofa_beam_prefix_topk: null pointer");
  OFA_REQUIRE(!prefix || (glogit && prefix_ld > pol->step && pol->step < pol->max_len), OFA_ERR_INVALID,
              "ofa_beam_prefix_topk: a prefix step needs glogit, prefix_ld=%lld > step=%d and step < max_len=%d", (long long)prefix_ld,
              pol->step, pol->max_len);
  return beam_topk_launch("ofa_beam_prefix_topk", logits, ld, rows, V, K, pol, prefix, prefix_ld, plen, glogit, ws, dtype, stream);
}

extern "C" int ofa_beam_prefix_fill(void* ws, int rows, int V, int K, const ofa_gen_policy* pol, const int64_t* prefix,
                                    int64_t prefix_ld, const int* plen, const float* glogit, void* stream) {
  OFA_REQUIRE(ws && pol && prefix && plen && glogit, OFA_ERR_INVALID, "ofa_beam_prefix_fill: null pointer");
  ofa_gen_policy p = *pol;                                   // its subset; what it does not read is out of the checks' way
  p.temperature = 1.f;
  p.cstart = p.cend = p.eos = -1;
  p.min_len = p.max_len = 0;
  const int step = p.step;
  OFA_REQUIRE(rows > 0 && V > 1 && step >= 0 && prefix_ld > step, OFA_ERR_INVALID, "ofa_beam_prefix_fill: rows=%d V=%d step=%d prefix_ld=%lld",
              rows, V, step, (long long)prefix_ld);
  if (const int rc = beam_check_row_pass("ofa_beam_prefix_fill", rows, V, K, p)) return rc;
  // at most step + 4 of the lowest tokens are not at f (the prefix token, pad, unk, step + 1 banned ones): 2K more are there
  const int pool = V < BEAM_FILL_POOL ? V : BEAM_FILL_POOL;
  OFA_REQUIRE(2 * K + step + 4 <= pool && p.unk < pool, OFA_ERR_UNSUPPORTED,
              "ofa_beam_prefix_fill: beam %d at step %d needs %d tokens among the first %d of the vocabulary", K, step,
              2 * K + step + 4, pool);
  const int S = beam_splits(V);
  BeamFillArgs a{beam_ws_carve(ws, rows, S, K), rows, V, K, S, prefix, prefix_ld, plen, glogit, p};
  hipLaunchKernelGGL(beam_prefix_fill_kernel, dim3(rows), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("ofa_beam_prefix_fill");
}

extern "C" int ofa_beam_prefix_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos,
                                      int unk, float unk_penalty, int normalize, float len_penalty, const int64_t* prefix,
                                      int64_t prefix_ld, int pad, void* stream) {
  OFA_REQUIRE(prefix && prefix_ld > step, OFA_ERR_INVALID, "ofa_beam_prefix_select: prefix=%p prefix_ld=%lld step=%d", (const void*)prefix,
              (long long)prefix_ld, step);
  return beam_select_launch("ofa_beam_prefix_select", ws, st, bsz, K, V, step, max_len, eos, unk, unk_penalty, normalize, len_penalty,
                            prefix, prefix_ld, pad, stream);
}

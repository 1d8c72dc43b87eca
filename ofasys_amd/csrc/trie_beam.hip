// Trie-constrained beam-search step for gfx950: the reference's generator with a `constraint_trie`
// (generator/sequence_generator.py:729-741: every row's logits are masked to the children of the trie node its prefix has
// reached, then log-softmax) without the [rows, V] output projection.  After the mask a row's distribution is a log-softmax over
// the CHILDREN OF ONE TRIE NODE, so the only logits that have to exist are one dot product per child edge (the algebra of
// closed_set_score.hip, per decoding step instead of under teacher forcing).  The trie arrives as the flat arrays of
// ofasys_amd/traverse.py TraversePlan; next to the beam state lives one trie node per row (int32 [rows], -1 = dead: off the
// trie, past an EOS edge, or at a score of -inf).
//
// 1. ofa_trie_beam_topk -- the row pass, replacing ofa_beam_topk.  Grid (Su, rows): workgroup `split` of a row takes edges
//    [split * epw, (split + 1) * epw) of the row's node, epw = 256 * p edges per workgroup and Su = ceil(max_degree / epw) fixed per
//    plan (p the smallest count for which Su fits the sentence pass's layout, below), so a captured grid never changes.  The
//    hidden row is staged once in LDS as raw 16-byte vectors; 16 lanes share an edge: they gather W[edge_token[e]] with 16-byte
//    loads, accumulate in fp32 and reduce with DPP inside their row of 16 lanes (four edges per wave in flight); + bias,
//    / temperature.  The workgroup then writes IN ofa_beam_topk'S WORKSPACE LAYOUT AND ORDER (value descending, token ascending)
//      - its (max, sum exp) part of the fp32 normaliser -- NaN for a dead row or a NaN logit, which ofa_beam_select turns into an
//        all -inf row;
//      - its best 2K candidates after the reference's post-normaliser masks in order (:296-343: EOS below min_len, NaN, PAD, unk
//        penalty, step >= max_len, n-gram bans).
//    so that ofa_beam_select (beam_search.hip) consumes them unchanged; the layout's parts Su .. splits(V) - 1 are written empty.
//    Only FINITE candidates are listed.  Everything else of the row is -inf in the reference (non-children by the mask, children
//    by the masks above), and torch.topk breaks those ties towards the lower index: split 0 completes its list to 2K entries with
//    -inf candidates at the lowest token ids it has not listed (fewer than 2K finite candidates in split 0 means a node of fewer
//    than epw edges, i.e. the other splits are empty; with a larger node a refill can repeat a token another split lists as
//    finite -- only the token of a -inf beam can differ from the reference then, which nothing observes).
// 2. ofa_beam_select runs as it is.
// 3. ofa_trie_beam_advance -- one workgroup per sentence, after the sentence pass: every new active row takes the child of its
//    parent's node (read through `reorder`; all K old nodes are read into LDS before any is written) through the chosen token;
//    dead if the parent was dead, the score is -inf or the edge is EOS.  A sentence whose K active slots are all ignored or at
//    -inf is marked done and the all-finished counter bumped: nothing can be finalised from such slots (:361 finalises finite
//    scores only), so the results are the reference's without the max_len + 1 - depth empty steps it runs.
// No host synchronisation, fixed addresses, workspace passed in.  Every index read from the plan or the state is range-checked
// before it addresses memory (an invalid node is a dead row, an invalid token a NaN logit).
#include "beam_common.h"

namespace ofa {

constexpr int TB_BAN_MAX = 256;           // n-gram bans of one row: at most step + 1
constexpr int TB_LDS_MAX = 65536;

// edges per workgroup: the smallest multiple of 256 for which ceil(max_degree / epw) parts fit the layout (max_degree <= V: <= 4096)
static inline int tb_edges_per_wg(int max_degree, int V) {
  const int S = beam_splits(V);
  int p = 1;
  while (cdiv(max_degree, BEAM_THREADS * p) > S) ++p;
  return BEAM_THREADS * p;
}

struct TrieTopkArgs {
  const void* h; int64_t ld_h;
  const void* W; int64_t ld_w; const void* bias;
  int D, V, rows, K, S, Su, epw;
  const int* node; const int* node_edge_off; const int* edge_token; int N, E;
  ofa_gen_policy p;
  BeamWs ws;
};

struct TrieTopkScratch {                  // the row pass's fixed LDS scratch, at the start of its dynamic region
  BeamListScratch lists;
  int banl[TB_BAN_MAX];
  int mtok[2 * BEAM_MAX_K];
  int nban, ngot;
  float unk_val;
  int pad_;
};
static_assert(sizeof(TrieTopkScratch) % 16 == 0, "the staged row behind the scratch is read with 16-byte LDS loads");

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void trie_beam_topk_kernel(TrieTopkArgs a) {
  constexpr int NV = Vec<T>::N;
  const int split = blockIdx.x, row = blockIdx.y;
  const ofa_gen_policy& p = a.p;
  if (p.done && p.done[row / a.K]) return;
  if (p.step == 0 && row % a.K != 0) return;                  // the sentence pass reads beam 0 only at step 0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K2 = 2 * a.K, nv = a.D / NV;
  // all LDS scratch lives in the dynamic region, so its base -- and with it the 16-byte reads of the staged row -- stays 16-byte
  // aligned whatever the fixed scratch adds up to (static __shared__ in front of an extern region shifts its base unpadded)
  extern __shared__ __attribute__((aligned(16))) uint4 tb_smem[];
  TrieTopkScratch& sh = *(TrieTopkScratch*)tb_smem;
  uint4* hrow = tb_smem + sizeof(TrieTopkScratch) / 16;       // [D / NV] the hidden row, raw
  float* key = (float*)(hrow + nv);                           // [epw] logits, then ordering keys (NaN: no candidate)
  int* tokl = (int*)(key + a.epw);                            // [epw] their tokens

  const int64_t part = (int64_t)row * a.S + split;
  float* st = a.ws.stats + part * 2;
  float* ov = a.ws.cval + part * K2;
  int* ot = a.ws.ctok + part * K2;
  // ---- the layout's parts this plan never uses: empty
  if (split == 0) {
    for (int e = tid; e < (a.S - a.Su) * K2; e += BEAM_THREADS) {
      const int64_t o = ((int64_t)row * a.S + a.Su) * K2 + e;
      a.ws.cval[o] = -INFINITY;
      a.ws.ctok[o] = -1;
    }
    for (int s = a.Su + tid; s < a.S; s += BEAM_THREADS) {
      a.ws.stats[((int64_t)row * a.S + s) * 2] = -INFINITY;
      a.ws.stats[((int64_t)row * a.S + s) * 2 + 1] = 0.f;
    }
  }
  // ---- the row's node and this workgroup's slice of its edges (all uniform)
  const int nd = a.node[row];
  int e0 = 0, e1 = 0;
  bool live = (unsigned)nd < (unsigned)a.N;
  if (live) {
    e0 = a.node_edge_off[nd];
    e1 = a.node_edge_off[nd + 1];
    live = e0 >= 0 && e1 > e0 && e1 <= a.E;
  }
  const int b0 = e0 + split * a.epw;
  const int cnt = live ? max(0, min(a.epw, e1 - b0)) : 0;
  if (cnt == 0) {                                             // a dead row (NaN normaliser: the whole row is -inf) or an empty slice
    if (tid == 0) {
      st[0] = (!live && split == 0) ? NAN : -INFINITY;
      st[1] = 0.f;
    }
    for (int r = tid; r < K2; r += BEAM_THREADS) { ov[r] = -INFINITY; ot[r] = -1; }
    return;
  }
  const uint4* hsrc = (const uint4*)((const T*)a.h + (int64_t)row * a.ld_h);
  for (int v = tid; v < nv; v += BEAM_THREADS) hrow[v] = hsrc[v];
  if (tid == 0) { sh.nban = 0; sh.unk_val = 0.f; }
  __syncthreads();
  // ---- n-gram bans of this row, as a list
  beam_ngram_scan(p, row, tid, [&](int64_t tok) {
    const int q = atomicAdd(&sh.nban, 1);
    if (q < TB_BAN_MAX) sh.banl[q] = (int)tok;
  });
  // ---- one dot product per edge: 16 lanes per edge, four edges per wave at a time
  const int grp = lane >> 4, gl = lane & 15;
  for (int base = wave * 4; base < cnt; base += 16) {         // (wave-uniform bound: all 64 lanes reach the DPP reduction)
    const int i = base + grp;
    const int tok = i < cnt ? a.edge_token[b0 + i] : -1;
    const bool ok = (unsigned)tok < (unsigned)a.V;
    float acc = 0.f;
    if (ok) {
      const uint4* w = (const uint4*)((const T*)a.W + (int64_t)tok * a.ld_w);
      for (int v = gl; v < nv; v += 16) {
        float wf[NV], hf[NV];
        unpack16<T>(w[v], wf);
        unpack16<T>(hrow[v], hf);
#pragma unroll
        for (int q = 0; q < NV; ++q) acc = fmaf(wf[q], hf[q], acc);
      }
    }
    acc = row16_sum(acc);
    if (gl == 0 && i < cnt) {
      float z = NAN;
      if (ok) {
        z = acc;
        if (a.bias) z += ld1<T>((const T*)a.bias + tok);
        if (p.temperature != 1.f) z = z / p.temperature;
      }
      key[i] = z;
      tokl[i] = tok;
    }
  }
  __syncthreads();
  // ---- this slice's part of the normaliser
  float m = -INFINITY;
  int has_nan = 0;
  for (int i = tid; i < cnt; i += BEAM_THREADS) {
    const float v = key[i];
    if (v != v) has_nan = 1;
    else m = fmaxf(m, v);
  }
  beam_normaliser_part(sh.lists, tid, m, has_nan, [&](float wm) {
    float s = 0.f;
    for (int i = tid; i < cnt; i += BEAM_THREADS) {
      const float v = key[i];
      if (v == v) s += expf(v - wm);
    }
    return s;
  }, st);                                                     // (its barrier also orders the ban list)
  // ---- post-normaliser masks -> ordering keys; -inf is no candidate (entry i is read and written by thread i % 256 only)
  const int nb = min(sh.nban, TB_BAN_MAX);
  for (int i = tid; i < cnt; i += BEAM_THREADS) {
    const int c = tokl[i];
    bool banned = false;
    for (int q = 0; q < nb; ++q) banned = banned || sh.banl[q] == c;
    const float v = beam_mask_key(p, key[i], c, banned, sh.unk_val);
    key[i] = v == -INFINITY ? NAN : v;
  }
  // ---- per-wave top 2K, sorted by (key desc, token asc)
  for (int it = 0; it < K2; ++it) {
    float lb = NAN;
    int lc = 0x7fffffff, li = -1;
    for (int i = tid; i < cnt; i += BEAM_THREADS) {
      const float v = key[i];
      if (v == v) {
        const int c = tokl[i];
        if (li < 0 || v > lb || (v == lb && c < lc)) { lb = v; lc = c; li = i; }
      }
    }
    float mx; int mc;
    if (!wave_argmax(lb, lc, mx, mc)) {
      beam_close_list(sh.lists, wave, lane, it, K2);
      break;
    }
    if (li >= 0 && lc == mc) {
      sh.lists.lkey[wave][it] = lb;
      sh.lists.lval[wave][it] = mc == p.unk ? sh.unk_val : lb;
      sh.lists.ltok[wave][it] = mc;
      key[li] = NAN;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const int got = beam_merge_lists(sh.lists, lane, K2, ov, ot, sh.mtok);
    if (lane == 0) sh.ngot = got;
  }
  __syncthreads();
  // ---- fewer than 2K finite candidates: split 0 refills with -inf at the lowest token ids it has not listed, the others stay empty
  if (tid == 0) {
    const int got = sh.ngot;
    int t = 0;
    for (int r = got; r < K2; ++r) {
      int tok = -1;
      if (split == 0) {
        for (; t < a.V; ++t) {
          bool used = false;
          for (int q = 0; q < got; ++q) used = used || sh.mtok[q] == t;
          if (!used) break;
        }
        if (t < a.V) tok = t++;
      }
      ov[r] = -INFINITY;
      ot[r] = tok;
    }
  }
}

struct TrieAdvanceArgs {
  int* node; const int* node_edge_off; const int* edge_token; const int* edge_child; int N, E;
  int bsz, K, step;
  ofa_gen_state st;                       // read: the histories, ignore, reorder; written: done, nfin
};

__global__ __launch_bounds__(BEAM_THREADS) void trie_beam_advance_kernel(TrieAdvanceArgs a) {
  const int sent = blockIdx.x;
  const ofa_gen_state& st = a.st;
  if (st.done[sent]) return;                                  // finished (possibly by this step's sentence pass): its nodes are not read again
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, r0 = sent * K;
  __shared__ int old[BEAM_MAX_K];
  __shared__ int alive;
  if (tid < K) old[tid] = a.node[r0 + tid];
  if (tid == 0) alive = 0;
  __syncthreads();                                            // every old node is read before any is written
  for (int b = wave; b < K; b += 4) {
    const int64_t row = r0 + b;
    const int64_t parent = st.reorder[row] - r0;
    const float sc = st.scores[row * st.score_ld + a.step];
    const bool finite = sc == sc && sc != -INFINITY;
    int child = -1;
    if (finite && parent >= 0 && parent < K && a.step + 1 < st.tok_cap) {
      const int pn = old[parent];
      if ((unsigned)pn < (unsigned)a.N) {
        const int64_t tok = st.tokens[row * st.tok_ld + a.step + 1];
        const int e0 = max(a.node_edge_off[pn], 0), e1 = min(a.node_edge_off[pn + 1], a.E);
        float found = -1.f;                                   // node ids < 2^24: exact as float
        for (int e = e0 + lane; e < e1; e += WAVE)
          if ((int64_t)a.edge_token[e] == tok) found = fmaxf(found, (float)a.edge_child[e]);
        child = (int)wave_max(found);
        if (child >= a.N) child = -1;
      }
    }
    if (lane == 0) {
      a.node[row] = child;
      if (finite && !st.ignore[row]) atomicOr(&alive, 1);
    }
  }
  __syncthreads();
  if (tid == 0 && !alive) {                                   // every slot ignored or at -inf: nothing more can be finalised
    st.done[sent] = 1;
    atomicAdd(st.nfin, 1);
  }
}

}  // namespace ofa

using namespace ofa;

extern "C" int ofa_trie_beam_splits(int max_degree, int V) {
  if (max_degree <= 0 || V <= 1 || max_degree > V) return 0;
  return cdiv(max_degree, tb_edges_per_wg(max_degree, V));
}

extern "C" int ofa_trie_beam_topk(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias, int D, int V,
                                  int rows, int K, const int* node, const int* node_edge_off, const int* edge_token, int N, int E,
                                  int max_degree, const ofa_gen_policy* pol, void* ws, void* stream) {
  OFA_REQUIRE(h && W && node && node_edge_off && edge_token && ws && pol, OFA_ERR_INVALID, "ofa_trie_beam_topk: null pointer");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ofa_trie_beam_topk: bad dtype %d", dtype);
  const int step = pol->step;
  OFA_REQUIRE(rows > 0 && V > 1 && D > 0 && step >= 0 && N > 0 && E > 0, OFA_ERR_INVALID,
              "ofa_trie_beam_topk: rows=%d V=%d D=%d step=%d N=%d E=%d", rows, V, D, step, N, E);
  if (const int rc = beam_check_row_pass("ofa_trie_beam_topk", rows, V, K, *pol)) return rc;
  OFA_REQUIRE(pol->cstart < 0, OFA_ERR_INVALID, "ofa_trie_beam_topk: a constraint range [%d, %d) cannot be combined with the trie",
              pol->cstart, pol->cend);
  OFA_REQUIRE(max_degree >= 1 && max_degree <= V && max_degree <= E, OFA_ERR_INVALID,
              "ofa_trie_beam_topk: max_degree %d outside [1, min(V, E)]", max_degree);
  OFA_REQUIRE(pol->ngram <= 0 || step < TB_BAN_MAX, OFA_ERR_UNSUPPORTED, "ofa_trie_beam_topk: n-gram bans beyond step %d", TB_BAN_MAX);
  if (const int rc = check_proj_operands("ofa_trie_beam_topk", dtype, D, h, ld_h, W, ld_w)) return rc;
  const int S = beam_splits(V), epw = tb_edges_per_wg(max_degree, V);
  TrieTopkArgs a{h, ld_h, W, ld_w, bias, D, V, rows, K, S, cdiv(max_degree, epw), epw, node, node_edge_off, edge_token, N, E,
                 *pol, beam_ws_carve(ws, rows, S, K)};
  const size_t smem = sizeof(TrieTopkScratch) + (size_t)D * dt_size(dtype) + (size_t)a.epw * 8;
  OFA_REQUIRE(smem <= TB_LDS_MAX, OFA_ERR_UNSUPPORTED, "ofa_trie_beam_topk: D=%d with %d edges per workgroup needs %zu bytes of LDS",
              D, a.epw, smem);
  OFA_REQUIRE(rows <= 65535, OFA_ERR_UNSUPPORTED, "ofa_trie_beam_topk: %d rows", rows);
  dim3 grid(a.Su, rows);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(trie_beam_topk_kernel<typename decltype(tag)::type>, grid, dim3(BEAM_THREADS), smem, st, a);
  });
  return check_launch("ofa_trie_beam_topk");
}

extern "C" int ofa_trie_beam_advance(int* node, const int* node_edge_off, const int* edge_token, const int* edge_child, int N, int E,
                                     const ofa_gen_state* st, int bsz, int K, int step, void* stream) {
  OFA_REQUIRE(node && node_edge_off && edge_token && edge_child, OFA_ERR_INVALID, "ofa_trie_beam_advance: null pointer");
  OFA_REQUIRE(bsz > 0 && step >= 0 && N > 0 && E > 0 && N < (1 << 24), OFA_ERR_INVALID, "ofa_trie_beam_advance: bsz=%d step=%d N=%d E=%d",
              bsz, step, N, E);
  if (const int rc = beam_check_state("ofa_trie_beam_advance", st, K, step, false)) return rc;
  TrieAdvanceArgs a{node, node_edge_off, edge_token, edge_child, N, E, bsz, K, step, *st};
  hipLaunchKernelGGL(trie_beam_advance_kernel, dim3(bsz), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("ofa_trie_beam_advance");
}

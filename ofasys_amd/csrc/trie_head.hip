// Trie-edge head for closed-set training: the output projection, the label-smoothed loss and both gradients of a closed-set micro-batch
// computed over the CHILDREN of each row's trie node, never over the vocabulary.  The dense route projects [rows, D] features onto V
// logits, hands the node criterion (trie_loss.hip) a [rows, V] row of which it reads C columns, and runs the dX and dW products over a
// [rows, V] gradient that is zero except those C columns.  Here, with row r on node n = node[r], edges [e0, e1) = node_edge_off[n .. n+1]
// and slot j = edge e0 + j (at most Cmax = the plan's max_degree slots):
//   1. trie_head_fwd_kernel   z[r, j] = feats[r] . W[edge_token[e0 + j]] (+ bias), then trie_lsce_kernel's row core over z[r, :]
//                             (max-then-rescale sums, C, eps_i, "the target is an allowed child") -> lse, row_loss, row_nll, row_cnt and
//                             the UNSCALED compact gradient g[r, j] = w_nll (p_j - [tok_j == t]) + eps_i (C p_j - 1); with row_hit also
//                             trie_eval_kernel's arg-max (value, then lowest token).  A disallowed slot gets exactly 0, an ignored, filler
//                             or dead row all zeros.  Slots past the row's degree are not written and never read.
//   2. trie_head_dx_kernel    dfeats[r, :] = gs row_w[r] sum_j g[r, j] W[tok_j, :]; every row written in full, no collisions.
//   3. trie_head_dw_kernel    dW[u, :] += gs sum_{(r, j): tok = u} row_w[r] g[r, j] feats[r, :] (and dbias[u]) WITHOUT float atomics: one wave
//                             owns one distinct token u, walks u's edges in ascending edge index (the plan's inverse CSR by token), per
//                             edge the rows sitting on the edge's node in ascending row index (the step's row buckets), accumulates in
//                             fp32 registers and does ONE read-modify-write of dW[u] in the gradient's dtype.  The order is fixed, so a
//                             step replays bit for bit; a token none of whose rows contributes touches nothing.
// Loss scaling (gs, a device scalar) and drop-worst (row_w) enter in 2 and 3 only: one forward serves every backward.
// Every index read from device memory is clamped or skipped before it addresses anything: a node outside [0, N), an edge range outside
// [0, E], a degree above Cmax, a token outside [0, V) (never dereferenced), an edge, node or row index of the inverse lists out of range.
#include "common.h"

namespace ofa {

struct TrieHeadCfg {
  const int32_t* node;            // [rows]
  const int32_t* node_edge_off;   // [N + 1]
  const int32_t* edge_token;      // [E]
  int N, E, Cmax, V;
  float eps;
  int cs, ce;                     // cs < 0: no constraint range
};

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_WAVES = HEAD_THREADS / WAVE;
constexpr int HEAD_UNROLL = 4;    // the row core's edges per thread and trip: trie_lsce_kernel's TRIE_UNROLL, the same reduction order
constexpr int HEAD_EU = 8;        // slots one wave projects (forward) / sums (dX) per trip: that many W rows in flight per lane
constexpr int HEAD_RU = 8;        // rows one wave of the dW kernel has in flight
constexpr int HEAD_VPL = 2;       // 16-byte vectors of D per lane and pass of the dX and dW kernels
constexpr int HEAD_LDS_MAX = 65536 - 1024;

__device__ __forceinline__ bool head_allowed(const TrieHeadCfg& c, int tok) {
  return tok >= 0 && tok < c.V && (c.cs < 0 || tok < 4 || (tok >= c.cs && tok < c.ce));
}

// the row's clamped edge range: [lo, hi) inside [0, E], at most Cmax edges; lo = hi = 0 for a node outside [0, N)
__device__ __forceinline__ void head_range(const TrieHeadCfg& c, int64_t row, int& lo, int& hi) {
  const int n = c.node[row];
  lo = hi = 0;
  if (n >= 0 && n < c.N) {
    lo = max(c.node_edge_off[n], 0);
    hi = min(c.node_edge_off[n + 1], c.E);
    hi = max(min(hi, lo + c.Cmax), lo);
  }
}

// One 256-thread block per row.  HIT: validation (row_hit is written, g may be null).
template <typename T, bool HIT>
__global__ __launch_bounds__(HEAD_THREADS) void trie_head_fwd_kernel(const T* __restrict__ feats, int64_t ld_x, const T* __restrict__ W,
                                                                     int64_t ld_w, const T* __restrict__ bias, int D,
                                                                     const int64_t* __restrict__ target, int64_t ignore_index,
                                                                     TrieHeadCfg cfg, float* z, float* __restrict__ lse,
                                                                     float* __restrict__ row_loss, float* __restrict__ row_nll,
                                                                     float* __restrict__ row_cnt, float* __restrict__ g,
                                                                     int32_t* __restrict__ row_hit) {
  constexpr int N = Vec<T>::N;
  constexpr int NO_TOK = 0x7fffffff;
  extern __shared__ uint4 head_x[];                        // the row's features, raw 16-byte vectors [D / N]
  __shared__ float sm[4], ss[4], sx[4], sc[4], szt;
  __shared__ int sf[4], si[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nv = D / N;
  const int64_t t = target[row];
  const bool ignored = t == ignore_index;
  int lo, hi;
  head_range(cfg, row, lo, hi);
  const int deg = hi - lo;
  float* zr = z + row * cfg.Cmax;
  if (tid == 0) szt = 0.f;
  if (deg > 0) {
    const uint4* xr = reinterpret_cast<const uint4*>(feats + row * ld_x);
    for (int v = tid; v < nv; v += HEAD_THREADS) head_x[v] = xr[v];
  }
  __syncthreads();
  // ---- 1. the children's logits: wave w projects slots [w * EU, (w + 1) * EU) of every trip of 4 * EU slots
  for (int j0 = wave * HEAD_EU; j0 < deg; j0 += HEAD_WAVES * HEAD_EU) {
    int tok[HEAD_EU];
    float acc[HEAD_EU];
#pragma unroll
    for (int i = 0; i < HEAD_EU; ++i) {
      tok[i] = j0 + i < deg ? cfg.edge_token[lo + j0 + i] : -1;      // (wave-uniform)
      if (!head_allowed(cfg, tok[i])) tok[i] = -1;                   // (a token outside [0, V) is skipped, never dereferenced)
      acc[i] = 0.f;
    }
    for (int v = lane; v < nv; v += WAVE) {
      uint4 wv[HEAD_EU];
#pragma unroll
      for (int i = 0; i < HEAD_EU; ++i)
        wv[i] = tok[i] >= 0 ? reinterpret_cast<const uint4*>(W + (int64_t)tok[i] * ld_w)[v] : make_uint4(0, 0, 0, 0);
      float xf[N];
      unpack16<T>(head_x[v], xf);
#pragma unroll
      for (int i = 0; i < HEAD_EU; ++i) {
        float wf[N];
        unpack16<T>(wv[i], wf);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[i] = fmaf(wf[k], xf[k], acc[i]);
      }
    }
    float out = 0.f;
    int mytok = -1;
#pragma unroll
    for (int i = 0; i < HEAD_EU; ++i) {
      const float s = wave_sum(acc[i]);
      if (lane == i) { out = s; mytok = tok[i]; }
    }
    if (lane < HEAD_EU && j0 + lane < deg) {
      if (mytok >= 0 && bias) out += ld1<T>(bias + mytok);
      zr[j0 + lane] = mytok >= 0 ? out : 0.f;              // (a disallowed slot: a defined value nobody reads)
    }
  }
  __syncthreads();                                         // the block's own stores of z[row, :] are visible to all of its waves
  // ---- 2. trie_lsce_kernel's row core over z[row, 0 .. deg)
  float m = -INFINITY, s = 0.f, sumx = 0.f, cnt = 0.f, bm = -INFINITY;
  int found = 0, bi = NO_TOK;
  for (int e0 = lo + tid; e0 < hi; e0 += HEAD_THREADS * HEAD_UNROLL) {
    int tok[HEAD_UNROLL];
    float a[HEAD_UNROLL];
    float lm = -INFINITY;
#pragma unroll
    for (int j = 0; j < HEAD_UNROLL; ++j) {
      const int e = e0 + j * HEAD_THREADS;
      tok[j] = e < hi ? cfg.edge_token[e] : -1;
      if (!head_allowed(cfg, tok[j])) tok[j] = -1;
      a[j] = tok[j] >= 0 ? zr[e - lo] : -INFINITY;
      if (tok[j] >= 0 && tok[j] == t) { found = 1; szt = a[j]; }      // (a node's tokens are distinct: one writer)
      lm = fmaxf(lm, a[j]);
    }
    if (lm > -INFINITY) {                                  // max first, then ONE rescale of the running sum
      const float mm = fmaxf(m, lm);
      float acc = s * expf(m - mm);
#pragma unroll
      for (int j = 0; j < HEAD_UNROLL; ++j) {
        acc += expf(a[j] - mm);                            // (a skipped edge: exp(-inf) = 0)
        sumx += tok[j] >= 0 ? a[j] : 0.f;
        cnt += tok[j] >= 0 ? 1.f : 0.f;
        if (HIT && tok[j] >= 0 && (a[j] > bm || (a[j] == bm && tok[j] < bi))) { bm = a[j]; bi = tok[j]; }
      }
      m = mm;
      s = acc;
    }
  }
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * expf(m - mw));
  sumx = wave_sum(sumx);
  cnt = wave_sum(cnt);
  int iw = NO_TOK;
  if constexpr (HIT) {
    iw = (bm == mw && bi != NO_TOK) ? bi : NO_TOK;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) iw = min(iw, __shfl_xor(iw, o, 64));
  }
  found = __any(found) ? 1 : 0;
  if (lane == 0) { sm[wave] = mw; ss[wave] = sw; sx[wave] = sumx; sc[wave] = cnt; sf[wave] = found; si[wave] = iw; }
  __syncthreads();
  found = sf[0] | sf[1] | sf[2] | sf[3];
  const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float S = 0.f;
  int amax = NO_TOK;
  if (M > -INFINITY) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      S += ss[w] * expf(sm[w] - M);                        // (every thread: the same four values in the same order)
      if (HIT && sm[w] == M) amax = min(amax, si[w]);
    }
  }
  const float l = M > -INFINITY ? M + logf(S) : -INFINITY; // (no child allowed: lse = -inf)
  const float C = sc[0] + sc[1] + sc[2] + sc[3];
  const bool dead = !ignored && !found;                    // a live target that is no allowed child of the node: loss +inf, no gradient
  const float eps_i = cfg.eps / (C - 1.f + 1e-6f);
  const float w_nll = 1.f - cfg.eps - eps_i;
  if (tid == 0) {
    lse[row] = l;
    row_cnt[row] = C;
    float rl = 0.f, rn = 0.f;
    if (dead) {
      rl = rn = INFINITY;
    } else if (!ignored) {
      const float X = sx[0] + sx[1] + sx[2] + sx[3];
      rn = l - szt;
      rl = w_nll * rn + eps_i * (C * l - X);
    }
    row_loss[row] = rl;
    row_nll[row] = rn;
    if constexpr (HIT) row_hit[row] = (!ignored && !dead && amax == (int)t) ? 1 : 0;
  }
  if (!g) return;
  float* gr = g + row * cfg.Cmax;
  const bool zero = ignored || dead;
  for (int e = lo + tid; e < hi; e += HEAD_THREADS) {
    const int tok = cfg.edge_token[e];
    float d = 0.f;
    if (!zero && head_allowed(cfg, tok)) {
      const float p = expf(zr[e - lo] - l);
      d = w_nll * (p - (tok == t ? 1.f : 0.f)) + eps_i * (C * p - 1.f);
    }
    gr[e - lo] = d;
  }
}

// One 256-thread block per row: wave w sums slots [w * EU, (w + 1) * EU) of every trip into fp32 registers, HEAD_VPL 16-byte vectors of
// D per lane and pass; the four waves' partial sums meet in LDS and are added in wave order.
template <typename T>
__global__ __launch_bounds__(HEAD_THREADS) void trie_head_dx_kernel(const float* __restrict__ g, const T* __restrict__ W, int64_t ld_w,
                                                                    int D, const int64_t* __restrict__ target, int64_t ignore_index,
                                                                    const float* __restrict__ row_w, const float* __restrict__ gscale,
                                                                    TrieHeadCfg cfg, T* __restrict__ dx, int64_t ld_dx) {
  constexpr int N = Vec<T>::N;
  __shared__ float part[HEAD_WAVES - 1][HEAD_VPL][WAVE][N + 1];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nv = D / N;
  int lo, hi;
  head_range(cfg, row, lo, hi);
  float scale = gscale ? gscale[0] : 1.0f;
  if (row_w) scale *= row_w[row];
  const int deg = (target[row] == ignore_index || scale == 0.f) ? 0 : hi - lo;       // (uniform over the block)
  const float* gr = g + row * cfg.Cmax;
  for (int vb = 0; vb < nv; vb += WAVE * HEAD_VPL) {       // (one pass up to D = 1024 in 16 bits)
    float acc[HEAD_VPL][N];
#pragma unroll
    for (int q = 0; q < HEAD_VPL; ++q) {
#pragma unroll
      for (int k = 0; k < N; ++k) acc[q][k] = 0.f;
    }
    for (int j0 = wave * HEAD_EU; j0 < deg; j0 += HEAD_WAVES * HEAD_EU) {
      float gj[HEAD_EU];
      uint4 wv[HEAD_EU][HEAD_VPL];
#pragma unroll
      for (int i = 0; i < HEAD_EU; ++i) {
        const int tok = j0 + i < deg ? cfg.edge_token[lo + j0 + i] : -1;             // (wave-uniform)
        gj[i] = head_allowed(cfg, tok) ? gr[j0 + i] : 0.f;                           // (a disallowed slot holds exactly 0)
#pragma unroll
        for (int q = 0; q < HEAD_VPL; ++q) {
          const int v = vb + q * WAVE + lane;
          wv[i][q] = (gj[i] != 0.f && v < nv) ? reinterpret_cast<const uint4*>(W + (int64_t)tok * ld_w)[v] : make_uint4(0, 0, 0, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < HEAD_EU; ++i) {
#pragma unroll
        for (int q = 0; q < HEAD_VPL; ++q) {
          float wf[N];
          unpack16<T>(wv[i][q], wf);
#pragma unroll
          for (int k = 0; k < N; ++k) acc[q][k] = fmaf(gj[i], wf[k], acc[q][k]);
        }
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int q = 0; q < HEAD_VPL; ++q) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[wave - 1][q][lane][k] = acc[q][k];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < HEAD_VPL; ++q) {
        const int v = vb + q * WAVE + lane;
        if (v < nv) {
#pragma unroll
          for (int w = 0; w < HEAD_WAVES - 1; ++w) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[q][k] += part[w][q][lane][k];
          }
#pragma unroll
          for (int k = 0; k < N; ++k) acc[q][k] *= scale;
          store_vec<T>(dx + row * ld_dx + (int64_t)v * N, acc[q]);
        }
      }
    }
    __syncthreads();
  }
}

struct TrieHeadDwArgs {
  const float* g;                 // [rows, Cmax]
  const float* row_w;             // [rows] or null
  const float* gscale;            // device scalar or null
  const int32_t* node_edge_off;   // [N + 1]
  const int32_t* edge_node;       // [E]
  const int32_t* head_tokens;     // [U] distinct edge tokens, ascending
  const int32_t* tok_edge_off;    // [U + 1]
  const int32_t* tok_edge;        // [E] edge indices, ascending within a token
  const int32_t* bucket_rows;     // [rows] row indices ordered by node, ascending within a node
  const int32_t* bucket_off;      // [N + 1]
  int N, E, Cmax, V, U, rows, cs, ce;
};

// One wave per distinct token.  The lists are walked once per pass of HEAD_VPL * 64 vectors of D (one pass up to D = 1024 in 16 bits).
// (Four waves per token, each summing every fourth group of 8 rows and meeting in LDS, measured SLOWER -- 648 against 574 us at 1536
// rows, 345 of them on the root: the walk is bound by the rows it streams, not by one wave's latency chain.)
template <typename T>
__global__ __launch_bounds__(WAVE) void trie_head_dw_kernel(TrieHeadDwArgs a, const T* __restrict__ feats, int64_t ld_x, int D,
                                                            T* __restrict__ dW, int64_t ld_dw, T* __restrict__ dbias) {
  constexpr int N = Vec<T>::N;
  const int u = blockIdx.x, lane = threadIdx.x, nv = D / N;
  const int tok = a.head_tokens[u];
  if (!(tok >= 0 && tok < a.V && (a.cs < 0 || tok < 4 || (tok >= a.cs && tok < a.ce)))) return;   // (a junk token owns no row of dW)
  const int p0 = max(a.tok_edge_off[u], 0), p1 = min(a.tok_edge_off[u + 1], a.E);
  const float gs = a.gscale ? a.gscale[0] : 1.0f;
  for (int vb = 0; vb < nv; vb += WAVE * HEAD_VPL) {
    float acc[HEAD_VPL][N];
#pragma unroll
    for (int q = 0; q < HEAD_VPL; ++q) {
#pragma unroll
      for (int k = 0; k < N; ++k) acc[q][k] = 0.f;
    }
    float bsum = 0.f;
    bool any = false;
    // the token's edges, 64 at a time: lane l looks up edge p0 + l (its node, slot and the node's row bucket); the edges whose node
    // has rows in this batch are then taken one by one in ascending edge index.  EOS hangs under every answer's last node: thousands
    // of edges, a few of which have rows.
    for (int pb = p0; pb < p1; pb += WAVE) {
      int j = -1, r0 = 0, r1 = 0;
      if (pb + lane < p1) {
        const int e = a.tok_edge[pb + lane];
        if ((unsigned)e < (unsigned)a.E) {
          const int n = a.edge_node[e];
          if ((unsigned)n < (unsigned)a.N) {
            j = e - a.node_edge_off[n];
            if (j >= 0 && j < a.Cmax) {                    // (the forward clamps a degree to Cmax: a slot past it was never written)
              r0 = max(a.bucket_off[n], 0);
              r1 = min(a.bucket_off[n + 1], a.rows);
            }
          }
        }
      }
      unsigned long long todo = __ballot(r1 > r0);
      while (todo) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        todo &= todo - 1;
        const int jj = __builtin_amdgcn_readlane(j, l), q0b = __builtin_amdgcn_readlane(r0, l), q1b = __builtin_amdgcn_readlane(r1, l);
        for (int q0 = q0b; q0 < q1b; q0 += HEAD_RU) {
          float c[HEAD_RU];
          uint4 xv[HEAD_RU][HEAD_VPL];
#pragma unroll
          for (int i = 0; i < HEAD_RU; ++i) {
            const int r = q0 + i < q1b ? a.bucket_rows[q0 + i] : -1;                  // (wave-uniform)
            c[i] = 0.f;
            if ((unsigned)r < (unsigned)a.rows) {
              c[i] = a.g[(int64_t)r * a.Cmax + jj];
              if (a.row_w) c[i] *= a.row_w[r];
            }
#pragma unroll
            for (int q = 0; q < HEAD_VPL; ++q) {
              const int v = vb + q * WAVE + lane;
              xv[i][q] = (c[i] != 0.f && v < nv) ? reinterpret_cast<const uint4*>(feats + (int64_t)r * ld_x)[v] : make_uint4(0, 0, 0, 0);
            }
          }
#pragma unroll
          for (int i = 0; i < HEAD_RU; ++i) {
            if (c[i] == 0.f) continue;                     // (uniform; an ignored, dead or dropped row adds nothing)
            any = true;
            bsum += c[i];
#pragma unroll
            for (int q = 0; q < HEAD_VPL; ++q) {
              float xf[N];
              unpack16<T>(xv[i][q], xf);
#pragma unroll
              for (int k = 0; k < N; ++k) acc[q][k] = fmaf(c[i], xf[k], acc[q][k]);
            }
          }
        }
      }
    }
    if (!any) return;                                      // (uniform, and the same in every pass) no row of the batch touches the token
#pragma unroll
    for (int q = 0; q < HEAD_VPL; ++q) {
      const int v = vb + q * WAVE + lane;
      if (v < nv) {
        T* dst = dW + (int64_t)tok * ld_dw + (int64_t)v * N;
        float old[N];
        load_vec<T>(dst, old);
#pragma unroll
        for (int k = 0; k < N; ++k) old[k] = fmaf(gs, acc[q][k], old[k]);
        store_vec<T>(dst, old);
      }
    }
    if (dbias && vb == 0 && lane == 0) st1<T>(dbias + tok, fmaf(gs, bsum, ld1<T>(dbias + tok)));
  }
}

static int trie_head_check(const char* who, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                           const int32_t* edge_token, int64_t N, int64_t E, int64_t Cmax, int64_t rows, int64_t D, int64_t V, float eps,
                           int64_t cstart, int64_t cend, int dtype) {
  const int64_t lim = (int64_t)1 << 31;
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(rows >= 0 && rows < lim && V > 1 && V < lim && D > 0 && D < lim && target && node && node_edge_off, OFA_ERR_INVALID,
              "%s: bad argument", who);
  OFA_REQUIRE(N >= 1 && N < lim && E >= 0 && E < lim - 2 * HEAD_THREADS * HEAD_UNROLL && (edge_token || E == 0), OFA_ERR_INVALID,
              "%s: bad trie (N=%lld E=%lld)", who, (long long)N, (long long)E);
  OFA_REQUIRE(Cmax >= 1 && Cmax < lim && rows * Cmax < ((int64_t)1 << 40), OFA_ERR_INVALID, "%s: bad Cmax=%lld", who, (long long)Cmax);
  OFA_REQUIRE(eps >= 0.f && eps < 1.f && (cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V)), OFA_ERR_INVALID,
              "%s: bad eps / constraint range [%lld, %lld)", who, (long long)cstart, (long long)cend);
  return 0;
}
}  // namespace ofa
using namespace ofa;

extern "C" int ofa_trie_head_fwd(const void* feats, int64_t ld_x, const void* W, int64_t ld_w, const void* bias, int64_t D, int64_t V,
                                 const int64_t* target, const int32_t* node, const int32_t* node_edge_off, const int32_t* edge_token,
                                 int64_t N, int64_t E, int64_t Cmax, float* z, float* lse, float* row_loss, float* row_nll,
                                 float* row_cnt, float* g, int32_t* row_hit, int64_t rows, int64_t ignore_index, float eps,
                                 int64_t cstart, int64_t cend, int dtype, void* stream) {
  if (int rc = trie_head_check("trie_head_fwd", target, node, node_edge_off, edge_token, N, E, Cmax, rows, D, V, eps, cstart, cend, dtype))
    return rc;
  OFA_REQUIRE(feats && W && z && lse && row_loss && row_nll && row_cnt && (g || row_hit), OFA_ERR_INVALID, "trie_head_fwd: null pointer");
  if (int rc = check_proj_operands("trie_head_fwd", dtype, (int)D, feats, ld_x, W, ld_w)) return rc;
  const size_t smem = (size_t)D * dt_size(dtype);
  OFA_REQUIRE(smem <= HEAD_LDS_MAX, OFA_ERR_UNSUPPORTED, "trie_head_fwd: D=%lld needs %zu bytes of LDS", (long long)D, smem);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const TrieHeadCfg cfg{node, node_edge_off, edge_token, (int)N, (int)E, (int)Cmax, (int)V, eps, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (row_hit)
      hipLaunchKernelGGL((trie_head_fwd_kernel<T, true>), dim3((unsigned)rows), dim3(HEAD_THREADS), smem, st, (const T*)feats, ld_x,
                         (const T*)W, ld_w, (const T*)bias, (int)D, target, ignore_index, cfg, z, lse, row_loss, row_nll, row_cnt, g, row_hit);
    else
      hipLaunchKernelGGL((trie_head_fwd_kernel<T, false>), dim3((unsigned)rows), dim3(HEAD_THREADS), smem, st, (const T*)feats, ld_x,
                         (const T*)W, ld_w, (const T*)bias, (int)D, target, ignore_index, cfg, z, lse, row_loss, row_nll, row_cnt, g, row_hit);
  });
  return check_launch("trie_head_fwd");
}

extern "C" int ofa_trie_head_bwd_dx(const float* g, const void* W, int64_t ld_w, int64_t D, int64_t V, const int64_t* target,
                                    const int32_t* node, const int32_t* node_edge_off, const int32_t* edge_token, int64_t N, int64_t E,
                                    int64_t Cmax, const float* row_w, const float* grad_scale, void* dfeats, int64_t ld_dx,
                                    int64_t rows, int64_t ignore_index, int64_t cstart, int64_t cend, int dtype, void* stream) {
  if (int rc = trie_head_check("trie_head_bwd_dx", target, node, node_edge_off, edge_token, N, E, Cmax, rows, D, V, 0.f, cstart, cend, dtype))
    return rc;
  OFA_REQUIRE(g && W && dfeats, OFA_ERR_INVALID, "trie_head_bwd_dx: null pointer");
  if (int rc = check_proj_operands("trie_head_bwd_dx", dtype, (int)D, dfeats, ld_dx, W, ld_w)) return rc;
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const TrieHeadCfg cfg{node, node_edge_off, edge_token, (int)N, (int)E, (int)Cmax, (int)V, 0.f, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((trie_head_dx_kernel<T>), dim3((unsigned)rows), dim3(HEAD_THREADS), 0, st, g, (const T*)W, ld_w, (int)D, target,
                       ignore_index, row_w, grad_scale, cfg, (T*)dfeats, ld_dx);
  });
  return check_launch("trie_head_bwd_dx");
}

extern "C" int ofa_trie_head_bwd_dw(const float* g, const void* feats, int64_t ld_x, int64_t D, int64_t V, const int32_t* node_edge_off,
                                    const int32_t* edge_node, int64_t N, int64_t E, int64_t Cmax, const int32_t* head_tokens,
                                    const int32_t* tok_edge_off, const int32_t* tok_edge, int64_t U, const int32_t* bucket_rows,
                                    const int32_t* bucket_off, const float* row_w, const float* grad_scale, void* dW, int64_t ld_dw,
                                    void* dbias, int64_t rows, int64_t cstart, int64_t cend, int dtype, void* stream) {
  const int64_t lim = (int64_t)1 << 31;
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "trie_head_bwd_dw: bad dtype %d", dtype);
  OFA_REQUIRE(g && feats && dW && node_edge_off && head_tokens && tok_edge_off && bucket_off && (rows == 0 || bucket_rows) &&
                  (E == 0 || (edge_node && tok_edge)),
              OFA_ERR_INVALID, "trie_head_bwd_dw: null pointer");
  OFA_REQUIRE(rows >= 0 && rows < lim && V > 1 && V < lim && D > 0 && D < lim && N >= 1 && N < lim && E >= 0 && E < lim && U >= 0 && U <= E,
              OFA_ERR_INVALID, "trie_head_bwd_dw: bad argument (rows=%lld V=%lld D=%lld N=%lld E=%lld U=%lld)", (long long)rows,
              (long long)V, (long long)D, (long long)N, (long long)E, (long long)U);
  OFA_REQUIRE(Cmax >= 1 && Cmax < lim && rows * Cmax < ((int64_t)1 << 40), OFA_ERR_INVALID, "trie_head_bwd_dw: bad Cmax=%lld",
              (long long)Cmax);
  OFA_REQUIRE(cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V), OFA_ERR_INVALID,
              "trie_head_bwd_dw: bad constraint range [%lld, %lld)", (long long)cstart, (long long)cend);
  if (int rc = check_proj_operands("trie_head_bwd_dw", dtype, (int)D, feats, ld_x, dW, ld_dw)) return rc;
  if (rows == 0 || U == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const TrieHeadDwArgs a{g, row_w, grad_scale, node_edge_off, edge_node, head_tokens, tok_edge_off, tok_edge, bucket_rows, bucket_off,
                         (int)N, (int)E, (int)Cmax, (int)V, (int)U, (int)rows, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((trie_head_dw_kernel<T>), dim3((unsigned)U), dim3(WAVE), 0, st, a, (const T*)feats, ld_x, (int)D, (T*)dW, ld_dw,
                       (T*)dbias);
  });
  return check_launch("trie_head_bwd_dw");
}

// Label-smoothed cross entropy for closed-set targets, the allowed set named by a trie NODE instead of a [rows, V] byte mask
// (engine/criterion/label_smoothed_cross_entropy.py:62-191 with sample["constraint_masks"]; the trie is traverse.TraversePlan's CSR).
// A row's allowed set A is the children of node[row] -- edge_token[node_edge_off[n] .. node_edge_off[n + 1]) -- inside [0, V) and,
// with a constraint range, inside [0, 4) U [cstart, cend).  The formulas are lsce_fwd_kernel's / lsce_bwd_kernel's (loss_optim.hip):
//     C = |A|;  lse = log sum_A exp x;  p_v = exp(x_v - lse);  eps_i = eps / (C - 1 + 1e-6)
//     nll = lse - x_t;  loss = (1 - eps - eps_i) nll + eps_i (C lse - sum_A x)
//     d_v = ((1 - eps - eps_i)(p_v - [v == t]) + eps_i (C p_v - 1)) grad_scale row_w   on A, exactly 0 elsewhere
// but a row reads C logits (1 for a finished answer, a few thousand at the root of an answer list) instead of V bytes and V logits.
#include "common.h"

namespace ofa {

struct TrieCfg {
  const int32_t* node;            // [rows]
  const int32_t* node_edge_off;   // [N + 1]
  const int32_t* edge_token;      // [E]
  int N, E;
  float eps;
  int cs, ce;                     // cs < 0: no constraint range
};

constexpr int TRIE_THREADS = 256;
constexpr int TRIE_UNROLL = 4;    // edges per thread and trip of the gather loop: a trip is 1024 edges

// One 256-thread block per row.  FWD: gather the node's children (tokens, then their logits), reduce (max, sum exp, sum x, count, "the
// target is a child"), write lse / row_loss / row_nll / row_cnt and, with dx, the gradient row.  !FWD: lse and row_cnt are inputs, only
// "the target is a child" is worked out again, and the gradient row is written at grad_scale * row_w.
// The gradient row is zero except C columns: every thread stores zero vectors over [0, ld), waits for those stores to be acknowledged
// (s_waitcnt vmcnt(0): nothing of this wave is in flight any more), the block meets at a barrier, and only then are the C values stored.
// A child's store can therefore not be overtaken by the zero vector that covers it; a node's tokens are distinct, so the scatter has
// no collisions of its own.
template <typename T, bool FWD>
__global__ __launch_bounds__(TRIE_THREADS) void trie_lsce_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 const float* __restrict__ gscale, const float* __restrict__ row_w,
                                                                 float* __restrict__ lse, float* __restrict__ row_loss,
                                                                 float* __restrict__ row_nll, float* __restrict__ row_cnt,
                                                                 T* __restrict__ dlogits, int64_t V, int64_t ld, int64_t ignore_index,
                                                                 TrieCfg cfg) {
  constexpr int N = Vec<T>::N;
  __shared__ float sm[4], ss[4], sx[4], sc[4];
  __shared__ int sf[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const T* x = logits + row * ld;
  T* dx = dlogits ? dlogits + row * ld : nullptr;
  const int64_t t = target[row];
  const bool ignored = t == ignore_index;
  if (dx) {                                                // (the stores are in flight while the children are gathered)
    const int64_t nvec = ld / N;                           // ld is a multiple of the vector width (launch precondition)
    for (int64_t v = tid; v < nvec; v += TRIE_THREADS) *reinterpret_cast<uint4*>(dx + v * N) = make_uint4(0, 0, 0, 0);
  }
  const int n = cfg.node[row];
  int lo = 0, hi = 0;
  if (n >= 0 && n < cfg.N) {
    lo = max(cfg.node_edge_off[n], 0);
    hi = min(cfg.node_edge_off[n + 1], cfg.E);
  }
  auto allowed = [&](int tok) {
    return tok >= 0 && tok < V && (cfg.cs < 0 || tok < 4 || (tok >= cfg.cs && tok < cfg.ce));
  };
  float m = -INFINITY, s = 0.f, sumx = 0.f, cnt = 0.f;
  int found = 0;
  for (int e0 = lo + tid; e0 < hi; e0 += TRIE_THREADS * TRIE_UNROLL) {
    int tok[TRIE_UNROLL];
#pragma unroll
    for (int j = 0; j < TRIE_UNROLL; ++j) {
      const int e = e0 + j * TRIE_THREADS;
      tok[j] = e < hi ? cfg.edge_token[e] : -1;
      if (!allowed(tok[j])) tok[j] = -1;                   // (an edge_token outside [0, V) is skipped, never dereferenced)
      found |= tok[j] >= 0 && tok[j] == t;
    }
    if constexpr (FWD) {
      float a[TRIE_UNROLL];
      float lm = -INFINITY;
#pragma unroll
      for (int j = 0; j < TRIE_UNROLL; ++j) {
        a[j] = tok[j] >= 0 ? ld1<T>(x + tok[j]) : -INFINITY;
        lm = fmaxf(lm, a[j]);
      }
      if (lm > -INFINITY) {                                // max first, then ONE rescale of the running sum (finite logits: the new max is finite)
        const float mm = fmaxf(m, lm);
        float acc = s * expf(m - mm);
#pragma unroll
        for (int j = 0; j < TRIE_UNROLL; ++j) {
          acc += expf(a[j] - mm);                          // (a skipped edge: exp(-inf) = 0)
          sumx += tok[j] >= 0 ? a[j] : 0.f;
          cnt += tok[j] >= 0 ? 1.f : 0.f;
        }
        m = mm;
        s = acc;
      }
    }
  }
  if constexpr (FWD) {
    const float mw = wave_max(m);
    const float sw = wave_sum(mw == -INFINITY ? 0.f : s * expf(m - mw));
    sumx = wave_sum(sumx);
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) { sm[tid >> 6] = mw; ss[tid >> 6] = sw; sx[tid >> 6] = sumx; sc[tid >> 6] = cnt; }
  }
  found = __any(found) ? 1 : 0;
  if ((tid & 63) == 0) sf[tid >> 6] = found;
  if (dx) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's zero vectors are acknowledged before the barrier lets a child be stored
  __syncthreads();
  found = sf[0] | sf[1] | sf[2] | sf[3];
  float l, C;
  if constexpr (FWD) {
    const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float S = 0.f;
    if (M > -INFINITY) {
#pragma unroll
      for (int w = 0; w < 4; ++w) S += ss[w] * expf(sm[w] - M);      // (every thread: the same four values in the same order)
    }
    l = M > -INFINITY ? M + logf(S) : -INFINITY;          // (no child allowed: lse = -inf)
    C = sc[0] + sc[1] + sc[2] + sc[3];
  } else {
    l = lse[row];
    C = row_cnt[row];
  }
  // a live target that is no allowed child of the node (the node outside [0, N), no child allowed at all): the reference's loss is +inf
  // (the target's log-probability is masked to -inf); the gradient row stays zero, as the SCST entry treats an invalid target
  const bool dead = !ignored && !found;
  const float eps_i = cfg.eps / (C - 1.f + 1e-6f);
  const float w_nll = 1.f - cfg.eps - eps_i;
  if constexpr (FWD) {
    if (tid == 0) {
      lse[row] = l;
      row_cnt[row] = C;
      float rl = 0.f, rn = 0.f;
      if (dead) {
        rl = rn = INFINITY;
      } else if (!ignored) {
        const float X = sx[0] + sx[1] + sx[2] + sx[3];
        rn = l - ld1<T>(x + t);                            // (found: t is an allowed column of [0, V))
        rl = w_nll * rn + eps_i * (C * l - X);
      }
      row_loss[row] = rl;
      row_nll[row] = rn;
    }
  }
  if (!dx || ignored || dead) return;                      // (uniform over the block)
  float g = gscale ? gscale[0] : 1.0f;
  if (row_w) g *= row_w[row];
  if (g == 0.f) return;
  for (int e = lo + tid; e < hi; e += TRIE_THREADS) {
    const int tok = cfg.edge_token[e];
    if (!allowed(tok)) continue;
    const float p = expf(ld1<T>(x + tok) - l);
    st1<T>(dx + tok, (w_nll * (p - (tok == t ? 1.f : 0.f)) + eps_i * (C * p - 1.f)) * g);
  }
}

// Validation's node form (ofa_criterion_eval with nodes): the forward half of the row core above -- the same gather, the same
// max-then-rescale sums -- plus the arg-max over the children as (stored value, lowest token): a node's children come in edge order,
// not token order, so an equal value takes the smaller token at every step.  Writes row_loss, row_nll and row_hit; nothing else.
template <typename T>
__global__ __launch_bounds__(TRIE_THREADS) void trie_eval_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 float* __restrict__ row_loss, float* __restrict__ row_nll,
                                                                 int32_t* __restrict__ row_hit, int64_t V, int64_t ld, int64_t ignore_index,
                                                                 TrieCfg cfg) {
  constexpr int NO_TOK = 0x7fffffff;
  __shared__ float sm[4], ss[4], sx[4], sc[4];
  __shared__ int sf[4], si[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const T* x = logits + row * ld;
  const int64_t t = target[row];
  const bool ignored = t == ignore_index;
  const int n = cfg.node[row];
  int lo = 0, hi = 0;
  if (n >= 0 && n < cfg.N) {
    lo = max(cfg.node_edge_off[n], 0);
    hi = min(cfg.node_edge_off[n + 1], cfg.E);
  }
  auto allowed = [&](int tok) {
    return tok >= 0 && tok < V && (cfg.cs < 0 || tok < 4 || (tok >= cfg.cs && tok < cfg.ce));
  };
  float m = -INFINITY, s = 0.f, sumx = 0.f, cnt = 0.f;
  int found = 0, bi = NO_TOK;
  for (int e0 = lo + tid; e0 < hi; e0 += TRIE_THREADS * TRIE_UNROLL) {
    int tok[TRIE_UNROLL];
    float a[TRIE_UNROLL];
    float lm = -INFINITY;
#pragma unroll
    for (int j = 0; j < TRIE_UNROLL; ++j) {
      const int e = e0 + j * TRIE_THREADS;
      tok[j] = e < hi ? cfg.edge_token[e] : -1;
      if (!allowed(tok[j])) tok[j] = -1;                   // (an edge_token outside [0, V) is skipped, never dereferenced)
      found |= tok[j] >= 0 && tok[j] == t;
      a[j] = tok[j] >= 0 ? ld1<T>(x + tok[j]) : -INFINITY;
      lm = fmaxf(lm, a[j]);
    }
    if (lm > -INFINITY) {
      const float mm = fmaxf(m, lm);
      float acc = s * expf(m - mm);
#pragma unroll
      for (int j = 0; j < TRIE_UNROLL; ++j) {
        acc += expf(a[j] - mm);
        sumx += tok[j] >= 0 ? a[j] : 0.f;
        cnt += tok[j] >= 0 ? 1.f : 0.f;
        if (tok[j] >= 0 && (a[j] > m || (a[j] == m && tok[j] < bi))) { m = a[j]; bi = tok[j]; }    // (m ends as mm: the largest of them)
      }
      m = mm;
      s = acc;
    }
  }
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * expf(m - mw));
  sumx = wave_sum(sumx);
  cnt = wave_sum(cnt);
  int iw = m == mw ? bi : NO_TOK;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) iw = min(iw, __shfl_xor(iw, o, 64));
  found = __any(found) ? 1 : 0;
  if ((tid & 63) == 0) { sm[tid >> 6] = mw; ss[tid >> 6] = sw; sx[tid >> 6] = sumx; sc[tid >> 6] = cnt; sf[tid >> 6] = found; si[tid >> 6] = iw; }
  __syncthreads();
  if (tid != 0) return;
  found = sf[0] | sf[1] | sf[2] | sf[3];
  const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float S = 0.f;
  int amax = NO_TOK;
  if (M > -INFINITY) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      S += ss[w] * expf(sm[w] - M);
      if (sm[w] == M) amax = min(amax, si[w]);
    }
  }
  const float l = M > -INFINITY ? M + logf(S) : -INFINITY;
  const float C = sc[0] + sc[1] + sc[2] + sc[3];
  float rl = 0.f, rn = 0.f;
  int hit = 0;
  if (!ignored && !found) {
    rl = rn = INFINITY;                                    // (no allowed child of the node: as the row core above)
  } else if (!ignored) {
    const float eps_i = cfg.eps / (C - 1.f + 1e-6f);
    rn = l - ld1<T>(x + t);                                // (found: t is an allowed column of [0, V))
    rl = (1.f - cfg.eps - eps_i) * rn + eps_i * (C * l - (sx[0] + sx[1] + sx[2] + sx[3]));
    hit = amax == (int)t;
  }
  row_loss[row] = rl;
  row_nll[row] = rn;
  row_hit[row] = hit;
}

void trie_criterion_eval_launch(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                const int32_t* edge_token, int64_t N, int64_t E, float* row_loss, float* row_nll, int32_t* row_hit,
                                int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend,
                                int dtype, hipStream_t st) {
  const TrieCfg cfg{node, node_edge_off, edge_token, (int)N, (int)E, eps, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((trie_eval_kernel<T>), dim3((unsigned)rows), dim3(TRIE_THREADS), 0, st, (const T*)logits, target, row_loss, row_nll,
                       row_hit, V, ld, ignore_index, cfg);
  });
}

static int trie_check(const char* who, const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                      const int32_t* edge_token, int64_t N, int64_t E, int64_t rows, int64_t V, int64_t ld, float eps, int64_t cstart,
                      int64_t cend, const void* dlogits, int dtype) {
  const int64_t lim = (int64_t)1 << 31;
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(rows >= 0 && rows < lim && V > 1 && V < lim && ld >= V && logits && target && node && node_edge_off, OFA_ERR_INVALID,
              "%s: bad argument", who);
  // (E leaves room for the gather loop's 32-bit edge index to step past the last edge)
  OFA_REQUIRE(N >= 1 && N < lim && E >= 0 && E < lim - 2 * TRIE_THREADS * TRIE_UNROLL && (edge_token || E == 0), OFA_ERR_INVALID,
              "%s: bad trie (N=%lld E=%lld)", who, (long long)N, (long long)E);
  OFA_REQUIRE(ld % dt_vecn(dtype) == 0, OFA_ERR_INVALID, "%s: ld=%lld must be a multiple of the 16-byte vector width", who, (long long)ld);
  OFA_REQUIRE(!dlogits || aligned16(dlogits), OFA_ERR_INVALID, "%s: dlogits must be 16-byte aligned", who);
  OFA_REQUIRE(eps >= 0.f && eps < 1.f && (cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V)), OFA_ERR_INVALID,
              "%s: bad eps / constraint range [%lld, %lld)", who, (long long)cstart, (long long)cend);
  return 0;
}
}  // namespace ofa
using namespace ofa;

extern "C" int ofa_trie_ls_cross_entropy_fwd(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                             const int32_t* edge_token, int64_t N, int64_t E, const float* grad_scale, float* lse,
                                             float* row_loss, float* row_nll, float* row_cnt, void* dlogits, int64_t rows, int64_t V,
                                             int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend, int dtype,
                                             void* stream) {
  if (int rc = trie_check("trie_ls_cross_entropy_fwd", logits, target, node, node_edge_off, edge_token, N, E, rows, V, ld, eps, cstart,
                          cend, dlogits, dtype)) return rc;
  OFA_REQUIRE(lse && row_loss && row_nll && row_cnt, OFA_ERR_INVALID, "trie_ls_cross_entropy_fwd: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const TrieCfg cfg{node, node_edge_off, edge_token, (int)N, (int)E, eps, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((trie_lsce_kernel<T, true>), dim3((unsigned)rows), dim3(TRIE_THREADS), 0, st, (const T*)logits, target, grad_scale,
                       (const float*)nullptr, lse, row_loss, row_nll, row_cnt, (T*)dlogits, V, ld, ignore_index, cfg);
  });
  return check_launch("trie_ls_cross_entropy_fwd");
}

extern "C" int ofa_trie_ls_cross_entropy_bwd(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                             const int32_t* edge_token, int64_t N, int64_t E, const float* lse, const float* row_cnt,
                                             const float* row_w, const float* grad_scale, void* dlogits, int64_t rows, int64_t V,
                                             int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend, int dtype,
                                             void* stream) {
  if (int rc = trie_check("trie_ls_cross_entropy_bwd", logits, target, node, node_edge_off, edge_token, N, E, rows, V, ld, eps, cstart,
                          cend, dlogits, dtype)) return rc;
  OFA_REQUIRE(lse && row_cnt && dlogits, OFA_ERR_INVALID, "trie_ls_cross_entropy_bwd: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const TrieCfg cfg{node, node_edge_off, edge_token, (int)N, (int)E, eps, cstart < 0 ? -1 : (int)cstart, (int)cend};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((trie_lsce_kernel<T, false>), dim3((unsigned)rows), dim3(TRIE_THREADS), 0, st, (const T*)logits, target, grad_scale,
                       row_w, const_cast<float*>(lse), (float*)nullptr, (float*)nullptr, const_cast<float*>(row_cnt), (T*)dlogits, V, ld,
                       ignore_index, cfg);
  });
  return check_launch("trie_ls_cross_entropy_bwd");
}

// Closed-set scoring for gfx950: the arithmetic of the reference's TraverseTask.inference (task/traverse_task.py:63-110) without
// the full-vocabulary projection.  The reference projects every (answer, position) onto V logits, masks them to the children of
// the answer trie's node, takes a log-softmax over V and gathers one value.  After the mask, position t of answer c is a
// log-softmax over the CHILDREN OF ONE TRIE NODE, and answers that share a prefix share the node, so per sentence the result is
//   z[e]     = h[rep(node(e))] . W[edge_token[e]] (+ bias)        one dot product per trie edge
//   lse[n]   = log sum_{e out of n} exp z[e]                      one log-sum-exp per trie node
//   score[c] = sum_{e on path(c)} (z[e] - lse[node(e)])           one short sum per answer
// The trie arrives as flat arrays (ofasys_amd/traverse.py TraversePlan): edges grouped by node (CSR), per node the (answer,
// position) whose decoder row holds its hidden state, per answer the edges of its path, and `items` -- the edges cut into work
// items of a few (TraversePlan.ITEM_EDGES) edges of ONE node, which is how the root (up to C edges) spreads over many workgroups.
//
// 1. closed_set_edge_kernel, grid (items, ceil(bsz / CS_BT)), one wave per workgroup: the node's hidden rows of CS_BT sentences
//    are staged once in LDS as raw 16-byte vectors; per edge the wave gathers the W row with 16-byte loads (each lane every
//    64th vector), multiplies it against the CS_BT staged rows (fp32 accumulation) and reduces across the lanes (DPP).
//    Callable per chunk of answers: a chunk contributes the nodes whose representative answer lies in it (a contiguous range of
//    nodes, edges and items, because nodes are numbered in order of first appearance).
// 2. closed_set_lse_kernel: one wave per (sentence, node), max-subtracted fp32 log-sum-exp over the node's edges.
// 3. closed_set_path_kernel: one thread per (sentence, answer).
// No host synchronisation, fixed addresses, workspace passed in.  Every index read from the plan is range-checked before it
// addresses memory (an invalid token gives a NaN logit, an invalid representative skips the item).
#include "common.h"

namespace ofa {

constexpr int CS_BT = 8;              // sentences per edge workgroup (hidden rows staged in LDS)
constexpr int CS_LDS_MAX = 65536;

struct ClosedSetEdgeArgs {
  const void* h; int64_t ld_h;
  const void* W; int64_t ld_w; const void* bias;
  int D, V, bsz, chunk, T, c0, E, N;
  const int* items;                   // [n_items, 3]: node, first edge, one past the last edge
  const int* edge_token; const int* rep_ans; const int* rep_pos;
  float* z;                           // [bsz, E]
};

template <typename T>
__global__ __launch_bounds__(WAVE) void closed_set_edge_kernel(ClosedSetEdgeArgs a) {
  constexpr int N = Vec<T>::N;
  extern __shared__ uint4 cs_rows[];  // [CS_BT][D / N]
  const int lane = threadIdx.x, nv = a.D / N;
  const int node = a.items[3 * blockIdx.x], e0 = a.items[3 * blockIdx.x + 1], e1 = a.items[3 * blockIdx.x + 2];
  const int b0 = blockIdx.y * CS_BT, nb = min(CS_BT, a.bsz - b0);
  if ((unsigned)node >= (unsigned)a.N) return;
  const int ans = a.rep_ans[node] - a.c0, pos = a.rep_pos[node];
  if (ans < 0 || ans >= a.chunk || pos < 0 || pos >= a.T || e0 < 0 || e1 > a.E) return;     // (uniform) not this chunk's node
#pragma unroll
  for (int j = 0; j < CS_BT; ++j) {
    const int b = b0 + min(j, nb - 1);                                  // rows past the batch repeat the last one (never stored)
    const uint4* row = (const uint4*)((const T*)a.h + (((int64_t)b * a.chunk + ans) * a.T + pos) * a.ld_h);
    for (int v = lane; v < nv; v += WAVE) cs_rows[j * nv + v] = row[v];
  }
  __syncthreads();
  for (int e = e0; e < e1; ++e) {
    const int tok = a.edge_token[e];
    const bool ok = (unsigned)tok < (unsigned)a.V;
    float acc[CS_BT];
#pragma unroll
    for (int j = 0; j < CS_BT; ++j) acc[j] = 0.f;
    if (ok) {
      const uint4* w = (const uint4*)((const T*)a.W + (int64_t)tok * a.ld_w);
      for (int v = lane; v < nv; v += WAVE) {
        float wf[N];
        unpack16<T>(w[v], wf);
#pragma unroll
        for (int j = 0; j < CS_BT; ++j) {
          float hf[N];
          unpack16<T>(cs_rows[j * nv + v], hf);
#pragma unroll
          for (int i = 0; i < N; ++i) acc[j] = fmaf(wf[i], hf[i], acc[j]);
        }
      }
    }
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < CS_BT; ++j) {
      const float s = wave_sum(acc[j]);
      if (lane == j) out = s;
    }
    if (lane < nb) {
      if (!ok) out = NAN;
      else if (a.bias) out += ld1<T>((const T*)a.bias + tok);
      a.z[(int64_t)(b0 + lane) * a.E + e] = out;
    }
  }
}

__global__ __launch_bounds__(256) void closed_set_lse_kernel(const float* z, const int* node_edge_off, float* lse, int bsz, int N,
                                                             int E) {
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (int64_t)bsz * N) return;
  const int lane = threadIdx.x & 63, n = (int)(wid % N), b = (int)(wid / N);
  const int e0 = max(node_edge_off[n], 0), e1 = min(node_edge_off[n + 1], E);
  const float* zb = z + (int64_t)b * E;
  float m = -INFINITY;
  for (int e = e0 + lane; e < e1; e += WAVE) m = fmaxf(m, zb[e]);
  m = wave_max(m);
  float s = 0.f;
  for (int e = e0 + lane; e < e1; e += WAVE) s += expf(zb[e] - m);
  s = wave_sum(s);
  if (lane == 0) lse[(int64_t)b * N + n] = m + logf(s);
}

__global__ __launch_bounds__(256) void closed_set_path_kernel(const float* z, const float* lse, const int* edge_node,
                                                              const int* path_off, const int* path_edge, float* scores, int bsz,
                                                              int C, int N, int E, int P) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)bsz * C) return;
  const int c = (int)(idx % C), b = (int)(idx / C);
  const int p0 = max(path_off[c], 0), p1 = min(path_off[c + 1], P);
  float s = 0.f;
  for (int p = p0; p < p1; ++p) {
    const int e = path_edge[p];
    const int n = (unsigned)e < (unsigned)E ? edge_node[e] : -1;
    s += (unsigned)n < (unsigned)N ? z[(int64_t)b * E + e] - lse[(int64_t)b * N + n] : NAN;
  }
  scores[idx] = s;
}

}  // namespace ofa

using namespace ofa;

extern "C" int64_t ofa_closed_set_ws_bytes(int bsz, int E, int N) {
  if (bsz <= 0 || E <= 0 || N <= 0) return 0;
  return (int64_t)bsz * ((int64_t)E + N) * 4;
}

extern "C" int ofa_closed_set_edge_logits(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias,
                                          int D, int V, int bsz, int chunk, int T, int c0, const int* items, int n_items,
                                          const int* edge_token, const int* rep_ans, const int* rep_pos, int N, int E,
                                          void* ws, void* stream) {
  OFA_REQUIRE(h && W && items && edge_token && rep_ans && rep_pos && ws, OFA_ERR_INVALID, "ofa_closed_set_edge_logits: null pointer");
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ofa_closed_set_edge_logits: bad dtype %d", dtype);
  OFA_REQUIRE(D > 0 && V > 0 && bsz > 0 && chunk > 0 && T > 0 && c0 >= 0 && N > 0 && E > 0 && n_items >= 0, OFA_ERR_INVALID,
              "ofa_closed_set_edge_logits: D=%d V=%d bsz=%d chunk=%d T=%d c0=%d E=%d items=%d", D, V, bsz, chunk, T, c0, E, n_items);
  if (const int rc = check_proj_operands("ofa_closed_set_edge_logits", dtype, D, h, ld_h, W, ld_w)) return rc;
  const size_t smem = (size_t)CS_BT * D * dt_size(dtype);
  OFA_REQUIRE(smem <= CS_LDS_MAX, OFA_ERR_UNSUPPORTED, "ofa_closed_set_edge_logits: D=%d needs %zu bytes of LDS", D, smem);
  if (n_items == 0) return OFA_OK;
  ClosedSetEdgeArgs a{h, ld_h, W, ld_w, bias, D, V, bsz, chunk, T, c0, E, N, items, edge_token, rep_ans, rep_pos, (float*)ws};
  dim3 grid(n_items, cdiv(bsz, CS_BT));
  OFA_REQUIRE(grid.y <= 65535, OFA_ERR_UNSUPPORTED, "ofa_closed_set_edge_logits: bsz %d too large", bsz);
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(closed_set_edge_kernel<typename decltype(tag)::type>, grid, dim3(WAVE), smem, st, a);
  });
  return check_launch("ofa_closed_set_edge_logits");
}

extern "C" int ofa_closed_set_reduce(int bsz, int C, int N, int E, int P, const int* node_edge_off, const int* edge_node,
                                     const int* path_off, const int* path_edge, void* ws, float* scores, void* stream) {
  OFA_REQUIRE(node_edge_off && edge_node && path_off && path_edge && ws && scores, OFA_ERR_INVALID,
              "ofa_closed_set_reduce: null pointer");
  OFA_REQUIRE(bsz > 0 && C > 0 && N > 0 && E > 0 && P > 0, OFA_ERR_INVALID, "ofa_closed_set_reduce: bsz=%d C=%d N=%d E=%d P=%d", bsz,
              C, N, E, P);
  float* z = (float*)ws;
  float* lse = z + (int64_t)bsz * E;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(closed_set_lse_kernel, dim3(cdiv((int64_t)bsz * N, 4)), dim3(256), 0, st, z, node_edge_off, lse, bsz, N, E);
  hipLaunchKernelGGL(closed_set_path_kernel, dim3(cdiv((int64_t)bsz * C, 256)), dim3(256), 0, st, z, lse, edge_node, path_off,
                     path_edge, scores, bsz, C, N, E, P);
  return check_launch("ofa_closed_set_reduce");
}

extern "C" int ofa_closed_set_score(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias, int D,
                                    int V, int bsz, int C, int Tmax, int N, int E, int P, const int* items, int n_items,
                                    const int* node_edge_off, const int* edge_token, const int* edge_node, const int* rep_ans,
                                    const int* rep_pos, const int* path_off, const int* path_edge, void* ws, float* scores,
                                    void* stream) {
  const int rc = ofa_closed_set_edge_logits(h, ld_h, dtype, W, ld_w, bias, D, V, bsz, C, Tmax, 0, items, n_items, edge_token, rep_ans,
                                            rep_pos, N, E, ws, stream);
  if (rc != OFA_OK) return rc;
  return ofa_closed_set_reduce(bsz, C, N, E, P, node_edge_off, edge_node, path_off, path_edge, ws, scores, stream);
}

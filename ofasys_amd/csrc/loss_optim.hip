// Criterion + train-step glue for gfx950 (HBM-bound, fp32 math):
//   cross entropy   engine/criterion/cross_entropy.py:27-67 (log_softmax in fp32, NLL sum, ignore_index = pad)
//   sum of squares  module/utils.py:342-384 (total grad norm for clip_grad_norm_)
//   Adam            engine/optim/adam.py:144-218 on the fp32 master copy of engine/optim/fp16_optimizer.py:32-71,
//                   fused with the grad multiply (engine/trainer.py:857-860) and the model-dtype copy-back.
#include "common.h"

namespace ofa {

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }
  s = s * expf(m - mm) + s2 * expf(m2 - mm);
  m = mm;
}

// ---- the row core of every fused loss kernel below: a running (max, sum of exp(x - max)) per thread, fed a vector at a time.
// The exponential exp(v - c) about a centre c, in the two forms the kernels use:
struct ExpLib {                                          // the library expf (~12 instructions): the 256-thread streaming kernels
  float c;
  __device__ __forceinline__ explicit ExpLib(float centre) : c(centre) {}
  __device__ __forceinline__ float operator()(float v) const { return expf(v - c); }
};
// ONE v_exp_f32 behind an FMA (2^(v log2 e - c log2 e), 1 ulp): with two exponentials per logit (one for the sum, one for the
// probability) the library's arithmetic, not HBM, set the time of the one-pass kernel
constexpr float L2E = 1.4426950408889634f;
__device__ __forceinline__ float ex2(float v) { return __builtin_amdgcn_exp2f(v); }
struct Exp2Fma {
  float k;
  __device__ __forceinline__ explicit Exp2Fma(float centre) : k(-centre * L2E) {}
  __device__ __forceinline__ float operator()(float v) const { return ex2(fmaf(v, L2E, k)); }
};
// one vector into (m, s): the vector's max, ONE rescale of s, N exponentials about the new max (m == -inf before the first: exp(-inf) = 0)
template <typename Exp, int N>
__device__ __forceinline__ void vec_merge(float& m, float& s, const float (&a)[N]) {
  float lm = a[0];
#pragma unroll
  for (int j = 1; j < N; ++j) lm = fmaxf(lm, a[j]);
  const float mm = fmaxf(m, lm);
  const Exp e(mm);
  float acc = s * e(m);
#pragma unroll
  for (int j = 0; j < N; ++j) acc += e(a[j]);
  m = mm;
  s = acc;
}
// the (m, s) of a 256-thread block's threads -> the row's log-sum-exp, handed to `row_done(lse)` in thread 0 ONLY: lanes by xor 32..1,
// one (m, s) per wave through LDS, then thread 0 merges waves 0..3 in order.  (That order is part of these kernels' results, bit for bit.)
// Call it at most once per kernel, from all 256 threads: the LDS below is the helper's own, and its early `return` for threads 1..255
// leaves the helper, after its barrier, not the kernel.
template <typename F>
__device__ __forceinline__ void block256_lse(float m, float s, F&& row_done) {
  __shared__ float sm[4], ss[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = m; ss[threadIdx.x >> 6] = s; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float M = sm[0], S = ss[0];
  for (int w = 1; w < 4; ++w) online_merge(M, S, sm[w], ss[w]);
  row_done(M + logf(S));
}

// one 256-thread block per row
template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                     float* __restrict__ lse, float* __restrict__ row_loss, int64_t V,
                                                     int64_t ld, int64_t ignore_index) {
  constexpr int N = Vec<T>::N;
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  float m = -INFINITY, s = 0.f;
  const int64_t nvec = V / N;
  for (int64_t v = threadIdx.x; v < nvec; v += 256) {
    float a[N];
    load_vec<T>(x + v * N, a);
    vec_merge<ExpLib>(m, s, a);
  }
  for (int64_t e = nvec * N + threadIdx.x; e < V; e += 256) online_merge(m, s, ld1<T>(x + e), 1.f);
  block256_lse(m, s, [&](float l) {
    lse[row] = l;
    const int64_t t = target[row];
    row_loss[row] = (t == ignore_index) ? 0.f : l - ld1<T>(x + t);
  });
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse, const float* __restrict__ gscale,
                                                     T* __restrict__ dlogits, int64_t V, int64_t ld, int64_t ignore_index) {
  constexpr int N = Vec<T>::N;
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  T* dx = dlogits + row * ld;
  const int64_t t = target[row];
  const bool ignored = t == ignore_index;
  const float g = gscale ? gscale[0] : 1.0f;
  const float l = lse[row];
  const int64_t nvec = ld / N;   // ld is a multiple of the vector width (launch precondition)
  for (int64_t v = threadIdx.x; v < nvec; v += 256) {
    float a[N], o[N];
    load_vec<T>(x + v * N, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int64_t c = v * N + j;
      float d = 0.f;
      if (!ignored && c < V) d = (expf(a[j] - l) - (c == t ? 1.f : 0.f)) * g;
      o[j] = d;
    }
    store_vec<T>(dx + v * N, o);
  }
}

// Forward AND gradient in one pass over the logits (16-bit types, V <= 65536): the [rows, V] logits of the vocabulary projection
// (158 MB at cfg-2: 1536 decoder rows x 51265) were read by ce_fwd, read again and written as a gradient by ce_bwd -- 53 + 65 us.  The
// criterion is the LAST node of the forward graph and its upstream gradient is a scalar the caller knows before the forward runs (the
// backward seed 1, or the loss scale), so one kernel can do both: a 1024-thread block holds its whole row in registers (NV x 8 elements
// per thread), reduces max / sum-exp (waves by shuffles, the 16 waves through LDS), and writes lse, the row's loss and
// dlogits = (softmax - onehot) * grad_scale from the same registers: one read, one write.  Exponentials by v_exp_f32 (1 ulp), a 1024-wide
// reduction tree: lse and the probabilities agree with ce_fwd_kernel / ce_bwd_kernel to fp32 rounding, not bit for bit.
template <typename T, int NV>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void ce_fwd_grad_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target, const float* __restrict__ gscale, float* __restrict__ lse,
    float* __restrict__ row_loss, T* __restrict__ dlogits, int V, int ld, int64_t ignore_index, float* __restrict__ loss_out,
    double* __restrict__ stats, unsigned* __restrict__ ticket) {
  // (two blocks per CU -- 64 registers -- so that one block's loads and stores overlap the other's arithmetic: with one, 141 us at cfg-2
  // against 118 for the two kernels it replaces.  32-bit indices and scalar-base + 32-bit-offset addressing keep it there.)
  constexpr int N = Vec<T>::N;
  static_assert(N == 8, "16-bit element types");
  __shared__ float sm[17], ss[16];                       // (sm[16]: the fused statistics' "this block drew the last ticket")
  const int64_t row = blockIdx.x;
  const char* xb = reinterpret_cast<const char*>(logits + row * ld);       // (uniform: scalar registers)
  char* db = reinterpret_cast<char*>(dlogits + row * ld);
  const int nvec = ld / N;                               // ld is a multiple of the vector width (launch precondition)
  const int tid = threadIdx.x;
  uint4 raw[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * 1024;
    raw[i] = v < nvec ? *reinterpret_cast<const uint4*>(xb + (uint32_t)v * 16u) : make_uint4(0, 0, 0, 0);
  }
  float m = -INFINITY, s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c0 = (tid + i * 1024) * N;
    if (c0 >= V) continue;
    float a[N];
    unpack16<T>(raw[i], a);
    if (c0 + N <= V) {
      vec_merge<Exp2Fma>(m, s, a);
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (c0 + j < V) online_merge(m, s, a[j], 1.f);
    }
  }
  // max first, then ONE rescale per partial sum: the pairwise online merges of ce_fwd_kernel (two expf each, six shuffle levels and
  // fifteen serial merges of the wave results) were this block's critical path -- nothing else runs on the CU while it reduces
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * ex2((m - mw) * L2E));
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { sm[wave] = mw; ss[wave] = sw; }
  __syncthreads();
  float M = sm[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) M = fmaxf(M, sm[w]);
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) S += ss[w] * ex2((sm[w] - M) * L2E);   // (every thread: the same 16 values in the same order)
  const float l = M + logf(S);
  const int64_t t64 = target[row];
  const bool ignored = t64 == ignore_index;
  const int t = (t64 >= 0 && t64 < V) ? (int)t64 : -1;
  // a target outside [0, V) that is not ignore_index is a caller error the kernel survives as the SCST entry does: x[t] is not read,
  // row_loss = +inf (the -lprob of a column that does not exist), the gradient row is zero
  const bool dead = ignored || t < 0;
  if (tid == 0) {
    lse[row] = l;
    const float rl = ignored ? 0.f : t < 0 ? INFINITY : l - ld1<T>(reinterpret_cast<const T*>(xb) + t);
    // (fused statistics: a write-through store, which the last block's agent-scope loads see without a fence in every block)
    if (ticket) {
      // The ticket counts PUBLISHED ROW LOSSES, not finished blocks: it is drawn here, before the gradient row is written, so that its
      // round trip (and the store's acknowledgement before it) hides under this block's stores instead of lengthening every block by
      // it (ticket at the end: 67.4 -> 71.0 us at cfg-2).  The statistics need the row losses and the targets, nothing else.
      __hip_atomic_store(row_loss + row, rl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      sm[16] = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1.f : 0.f;
    } else {
      row_loss[row] = rl;
    }
  }
  const float g = dead ? 0.f : (gscale ? gscale[0] : 1.0f);
  const Exp2Fma prob(l);                                 // exp(x - lse)
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * 1024;
    if (v >= nvec) continue;
    float a[N], o[N];
    unpack16<T>(raw[i], a);
    const int c0 = v * N;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float d = 0.f;
      if (!dead && c0 + j < V) d = (prob(a[j]) - (c0 + j == t ? 1.f : 0.f)) * g;
      o[j] = d;
    }
    uint4 w;
    w.x = pack2<T>(o[0], o[1]); w.y = pack2<T>(o[2], o[3]); w.z = pack2<T>(o[4], o[5]); w.w = pack2<T>(o[6], o[7]);
    *reinterpret_cast<uint4*>(db + (uint32_t)v * 16u) = w;
  }
  if (!ticket) return;
  // Fused statistics (ticket != NULL): the block that drew the LAST ticket (above) sums the row losses in reduce_sum_f32_kernel's order
  // (256 lanes striding the rows, wave sums, the four wave results in order), writes the loss and adds [count of target != ignore_index,
  // loss, the same count] to stats as step_stats_add_kernel does -- two single-block launches less -- and resets the ticket.  Thread 0
  // stored its row loss write-through and had the store acknowledged before it drew; the rows are read with agent-scope loads.  No
  // __threadfence(): a release fence in each of the 1792 cfg-2 blocks writes back an L2 full of gradient rows -- measured 67 -> 155 us.
  // What this rests on: on gfx950 an agent-scope relaxed atomic store is a write-through (sc1) store and an agent-scope relaxed atomic
  // load an sc1 load, which is served from the memory side of the XCDs' L2s, never from a line another XCD's store left stale; EVERY
  // load of row_loss below is such a load, so no acquire (cache invalidate) is needed for them.  That is this part's measured behaviour
  // and what hipcc emits for these builtins today, not a guarantee of the memory model: relaxed atomics order nothing by themselves,
  // the s_waitcnt between the store's acknowledgement and the ticket does.
  __syncthreads();                                       // (sm[16] is written; every thread is long done with sm[0..15] / ss)
  if (sm[16] == 0.f) return;                             // (uniform over the block)
  const int64_t rows = gridDim.x;
  float ls_ = 0.f;
  int cnt = 0;
  if (tid < 256)
    for (int64_t i = tid; i < rows; i += 256) {
      ls_ += __hip_atomic_load(row_loss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cnt += target[i] != ignore_index;
    }
  ls_ = wave_sum(ls_);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (tid < 256 && (tid & 63) == 0) { ss[tid >> 6] = ls_; sm[tid >> 6] = __int_as_float(cnt); }
  __syncthreads();
  if (tid == 0) {
    const float loss = ss[0] + ss[1] + ss[2] + ss[3];
    const double c = (double)(__float_as_int(sm[0]) + __float_as_int(sm[1]) + __float_as_int(sm[2]) + __float_as_int(sm[3]));
    loss_out[0] = loss;
    stats[0] += c;
    stats[1] += (double)loss;
    stats[2] += c;
    *ticket = 0u;
  }
}

// ---- label-smoothed cross entropy (engine/criterion/label_smoothed_cross_entropy.py:62-191), fused with the
// log-softmax: per non-ignored row
//     nll = lse - x[t];   smooth = sum_{v allowed} (lse - x[v]);   eps_i = eps / (Vc - 1 [+1e-6 with constraints])
//     loss = (1 - eps - eps_i) * nll + eps_i * smooth
// where the allowed set is the whole vocabulary, or [0,4) U [cstart, cend) (constraint_range; logits outside are -inf in
// the reference, :140-151) intersected with an optional per-row byte mask (sample["constraint_masks"]).
struct LsCfg { float eps; int64_t cstart, cend; const uint8_t* cmask; };
__device__ __forceinline__ bool ls_allowed(const LsCfg& c, int64_t row, int64_t v, int64_t V) {
  bool ok = c.cstart < 0 || v < 4 || (v >= c.cstart && v < c.cend);
  if (ok && c.cmask) ok = c.cmask[row * V + v] != 0;
  return ok;
}

template <typename T>
__global__ __launch_bounds__(256) void lsce_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                       float* __restrict__ lse, float* __restrict__ row_loss,
                                                       float* __restrict__ row_nll, float* __restrict__ row_cnt, int64_t V,
                                                       int64_t ld, int64_t ignore_index, LsCfg cfg) {
  __shared__ float sx[4], sc[4];
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  float m = -INFINITY, s = 0.f, sumx = 0.f, cnt = 0.f;
  for (int64_t v = threadIdx.x; v < V; v += 256) {
    if (!ls_allowed(cfg, row, v, V)) continue;
    const float a = ld1<T>(x + v);
    online_merge(m, s, a, 1.f);
    sumx += a;
    cnt += 1.f;
  }
  sumx = wave_sum(sumx);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) { sx[threadIdx.x >> 6] = sumx; sc[threadIdx.x >> 6] = cnt; }
  block256_lse(m, s, [&](float l) {                      // (its barrier orders sx / sc too)
    const float X = sx[0] + sx[1] + sx[2] + sx[3], C = sc[0] + sc[1] + sc[2] + sc[3];
    lse[row] = l;
    row_cnt[row] = C;
    const int64_t t = target[row];
    if (t == ignore_index) {
      row_loss[row] = 0.f;
      row_nll[row] = 0.f;
    } else {
      const float nll = l - ld1<T>(x + t);
      const float smooth = C * l - X;
      const float eps_i = cfg.eps / (cfg.cstart < 0 && !cfg.cmask ? (C - 1.f) : (C - 1.f + 1e-6f));
      row_nll[row] = nll;
      row_loss[row] = (1.f - cfg.eps - eps_i) * nll + eps_i * smooth;
    }
  });
}

// d loss_row / d x[v] = (1 - eps - eps_i)(p_v - [v == t]) + eps_i (C p_v - 1)   for allowed v, 0 elsewhere; times
// row_w[row] (drop_worst / ignored rows: 0) and the scalar grad_scale.
template <typename T>
__global__ __launch_bounds__(256) void lsce_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                       const float* __restrict__ lse, const float* __restrict__ row_cnt,
                                                       const float* __restrict__ row_w, const float* __restrict__ gscale,
                                                       T* __restrict__ dlogits, int64_t V, int64_t ld, int64_t ignore_index,
                                                       LsCfg cfg) {
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  T* dx = dlogits + row * ld;
  const int64_t t = target[row];
  float g = gscale ? gscale[0] : 1.0f;
  if (row_w) g *= row_w[row];
  if (t == ignore_index) g = 0.f;
  const float l = lse[row], C = row_cnt[row];
  const float eps_i = cfg.eps / (cfg.cstart < 0 && !cfg.cmask ? (C - 1.f) : (C - 1.f + 1e-6f));
  const float w_nll = 1.f - cfg.eps - eps_i;
  for (int64_t v = threadIdx.x; v < ld; v += 256) {
    float d = 0.f;
    if (g != 0.f && v < V && ls_allowed(cfg, row, v, V)) {
      const float p = expf(ld1<T>(x + v) - l);
      d = (w_nll * (p - (v == t ? 1.f : 0.f)) + eps_i * (C * p - 1.f)) * g;
    }
    st1<T>(dx + v, d);
  }
}

// ---- self-critical sequence training (engine/criterion/scst_loss.py:24-36, 214-233): per row the NLL of the GENERATED token times the
// reward of the row's sentence, over the allowed vocabulary (all of it, or [0,4) U [cstart,cend): the reference sets the other logits
// to -inf, :215-217).  The logits are [B*K rows, V] -- K times the cross-entropy step's -- so forward and gradient share one pass:
//     w = reward[s],  s = row_seq ? row_seq[r] : r / rows_per_seq      (a sentence index outside [0, nseq) reads nothing: w = 0)
//     lse = log sum_{v in A} exp(x_v);   row_loss = w (lse - x_t);   dlogits_v = w g (exp(x_v - lse) - [v == t]) on A, exactly 0 elsewhere
// An ignored row, a row of weight 0 and a row whose target is not an allowed column of [0, V) (a caller error: row_loss = +inf, as the
// reference's -lprob) get a zero gradient row.
__device__ __forceinline__ bool scst_ok(int64_t c, int64_t V, int64_t cs, int64_t ce) {
  return c < V && (cs < 0 || c < 4 || (c >= cs && c < ce));
}
// a vector of N columns from c0: 2 = every column allowed, 0 = none, 1 = cut (by V, by cstart / cend, or the [0,4) vector)
__device__ __forceinline__ int scst_vec_class(int64_t c0, int N, int64_t V, int64_t cs, int64_t ce) {
  if (c0 >= V) return 0;
  if (cs < 0) return c0 + N <= V ? 2 : 1;
  if (c0 >= cs && c0 + N <= ce) return c0 + N <= V ? 2 : 1;
  if (c0 >= 4 && (c0 + N <= cs || c0 >= ce)) return 0;
  return 1;
}
struct ScstRow { float w; int64_t t; bool ignored, valid; };
__device__ __forceinline__ ScstRow scst_row(int64_t row, const int64_t* target, const float* reward, const int32_t* row_seq,
                                            int64_t rows_per_seq, int64_t nseq, int64_t V, int64_t cs, int64_t ce, int64_t ignore_index) {
  ScstRow r;
  const int64_t s = row_seq ? (int64_t)row_seq[row] : row / rows_per_seq;
  r.w = (s >= 0 && s < nseq) ? reward[s] : 0.f;
  r.t = target[row];
  r.ignored = r.t == ignore_index;
  r.valid = r.t >= 0 && scst_ok(r.t, V, cs, ce);
  return r;
}

// Registers form (16-bit logits, ld <= 65536): ce_fwd_grad_kernel's block -- 1024 threads hold the row in NV x 8 registers each, one
// read and one write -- with the allowed-set test made per VECTOR: a vector wholly inside the range takes the plain path, one wholly
// outside is skipped (and written as zeros), and only the cut ones (the [0,4) vector, the two that cstart / cend cut, the one V cuts)
// go element by element.
template <typename T, int NV>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void scst_fwd_grad_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target, const float* __restrict__ reward,
    const int32_t* __restrict__ row_seq, int rows_per_seq, const float* __restrict__ gscale, float* __restrict__ lse,
    float* __restrict__ row_loss, T* __restrict__ dlogits, int nseq, int V, int ld, int64_t ignore_index, int cs, int ce) {
  constexpr int N = Vec<T>::N;
  static_assert(N == 8, "16-bit element types");
  __shared__ float sm[16], ss[16];
  const int64_t row = blockIdx.x;
  const char* xb = reinterpret_cast<const char*>(logits + row * ld);
  char* db = reinterpret_cast<char*>(dlogits + row * ld);
  const int nvec = ld / N;
  const int tid = threadIdx.x;
  uint4 raw[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i)      // (past the row's end the last vector is loaded again, in bounds, and never used: no branch per slab)
    raw[i] = *reinterpret_cast<const uint4*>(xb + (uint32_t)min(tid + i * 1024, nvec - 1) * 16u);
  // the allowed set by VECTOR index (uniform bounds; the host hands cs = 0, ce = V for "no range"): every column allowed in [f_lo, f_hi),
  // some column allowed in [a_lo, a_hi) and in vector 0 -- so a wave meets the per-element test only where cstart, cend or V cut
  const int f_lo = (cs + 7) >> 3, f_hi = ce >> 3, a_lo = cs >> 3, a_hi = (ce + 7) >> 3;
  // (one bit per slab in two registers, worked out once)
  uint32_t some_bits = 0, full_bits = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * 1024;
    some_bits |= (uint32_t)(((v >= a_lo) & (v < a_hi)) | (v == 0)) << i;
    full_bits |= (uint32_t)((v >= f_lo) & (v < f_hi)) << i;
  }
  auto some = [&](uint32_t bits, int i) { return (bits >> i) & 1u; };
  auto okc = [&](int th8, int k) {                       // column th8 + k, k = slab * 8192 + element: again against moved uniform bounds
    return (th8 < V - k) & ((th8 < 4 - k) | ((th8 >= cs - k) & (th8 < ce - k)));
  };
  const int tid8 = tid * N;
  float m = -INFINITY, s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!some(some_bits, i)) continue;
    float a[N];
    unpack16<T>(raw[i], a);
    if (!some(full_bits, i)) {                           // a cut vector: its disallowed columns enter the sums as -inf
#pragma unroll
      for (int j = 0; j < N; ++j) a[j] = okc(tid8, i * 8192 + j) ? a[j] : -INFINITY;
    }
    vec_merge<Exp2Fma>(m, s, a);                         // (every vector that gets here holds an allowed column: the new max is finite)
  }
  // max first, then ONE rescale per partial sum: the pairwise online merges of block256_lse (two expf each, six shuffle levels and the
  // serial merges of the wave results) would be this block's critical path -- nothing else runs on the CU while it reduces
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * ex2((m - mw) * L2E));
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { sm[wave] = mw; ss[wave] = sw; }
  __syncthreads();
  // the 16 wave results, one per lane, reduced by every wave in the same order (ce_fwd_grad_kernel reads all 32 values into registers of
  // every thread, which with the row's 28 is where it spills); the results come back through a lane read: uniform from here on
  const int lane = tid & 63;
  const float mv = lane < 16 ? sm[lane] : -INFINITY, sv = lane < 16 ? ss[lane] : 0.f;
  const float M = wave_max(mv);
  const float S = wave_sum(sv * ex2((mv - M) * L2E));      // (a wave of disallowed columns only, and lanes 16..63: 0 * 2^-inf = 0)
  const float l = M + logf(S);
  const ScstRow r = scst_row(row, target, reward, row_seq, rows_per_seq, nseq, V, cs, ce, ignore_index);
  if (tid == 0) {
    lse[row] = l;
    row_loss[row] = r.ignored ? 0.f : !r.valid ? INFINITY : r.w * (l - ld1<T>(reinterpret_cast<const T*>(xb) + r.t));
  }
  const float g = (r.ignored || !r.valid) ? 0.f : r.w * (gscale ? gscale[0] : 1.0f);
  const int trel = (r.valid ? (int)r.t : -1) - tid8;     // the target's column relative to this thread's first: slab i, element j is i * 8192 + j
  const Exp2Fma prob(l);                                 // exp(x - lse)
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (tid >= nvec - i * 1024) continue;
    uint4 w = make_uint4(0, 0, 0, 0);
    if ((g != 0.f) & (some(some_bits, i) != 0)) {
      float a[N], o[N];
      unpack16<T>(raw[i], a);
#pragma unroll
      for (int j = 0; j < N; ++j) o[j] = (prob(a[j]) - (trel == i * 8192 + j ? 1.f : 0.f)) * g;
      if (!some(full_bits, i)) {
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = okc(tid8, i * 8192 + j) ? o[j] : 0.f;
      }
      w.x = pack2<T>(o[0], o[1]); w.y = pack2<T>(o[2], o[3]); w.z = pack2<T>(o[4], o[5]); w.w = pack2<T>(o[6], o[7]);
    }
    *reinterpret_cast<uint4*>(db + (uint32_t)(tid + i * 1024) * 16u) = w;
  }
}

// Streaming form (fp32 logits, or rows longer than the registers form holds): one 256-thread block per row reads the row twice.
template <typename T>
__global__ __launch_bounds__(256) void scst_stream_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target, const float* __restrict__ reward,
    const int32_t* __restrict__ row_seq, int64_t rows_per_seq, const float* __restrict__ gscale, float* __restrict__ lse,
    float* __restrict__ row_loss, T* __restrict__ dlogits, int64_t nseq, int64_t V, int64_t ld, int64_t ignore_index, int64_t cs,
    int64_t ce) {
  constexpr int N = Vec<T>::N;
  __shared__ float sl;
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  T* dx = dlogits + row * ld;
  const int64_t nvec = ld / N;                             // ld is a multiple of the vector width (launch precondition)
  float m = -INFINITY, s = 0.f;
  for (int64_t v = threadIdx.x; v < nvec; v += 256) {
    const int64_t c0 = v * N;
    const int cls = scst_vec_class(c0, N, V, cs, ce);
    if (cls == 0) continue;
    float a[N];
    load_vec<T>(x + c0, a);
    if (cls == 2) {
      vec_merge<ExpLib>(m, s, a);
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (scst_ok(c0 + j, V, cs, ce)) online_merge(m, s, a[j], 1.f);
    }
  }
  const ScstRow r = scst_row(row, target, reward, row_seq, rows_per_seq, nseq, V, cs, ce, ignore_index);
  block256_lse(m, s, [&](float l) {
    sl = l;
    lse[row] = l;
    row_loss[row] = r.ignored ? 0.f : !r.valid ? INFINITY : r.w * (l - ld1<T>(x + r.t));
  });
  __syncthreads();
  const float l = sl;
  const float g = (r.ignored || !r.valid) ? 0.f : r.w * (gscale ? gscale[0] : 1.0f);
  for (int64_t v = threadIdx.x; v < nvec; v += 256) {
    const int64_t c0 = v * N;
    const int cls = g == 0.f ? 0 : scst_vec_class(c0, N, V, cs, ce);
    float o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = 0.f;
    if (cls != 0) {
      float a[N];
      load_vec<T>(x + c0, a);
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (cls == 2 || scst_ok(c0 + j, V, cs, ce)) o[j] = (expf(a[j] - l) - (c0 + j == r.t ? 1.f : 0.f)) * g;
    }
    store_vec<T>(dx + c0, o);
  }
}

// ---- validation (engine/criterion/label_smoothed_cross_entropy.py:114-198 in eval mode: compute_loss + compute_accuracy): per row the
// label-smoothed loss, the NLL and "the target is the arg-max of the allowed logits" from ONE read of the row -- no gradient, no lse, no
// log-probabilities.  The formulas are lsce_fwd_kernel's; the arg-max is carried as (value, lowest column) next to (max, sum): a
// thread meets its columns in rising order and takes a column only on a strictly larger stored value, the reductions take the largest
// value and, among equal values, the smallest column as an int -- lprobs.argmax(1) of the reference on the CPU, exactly.
constexpr int NO_COL = 0x7fffffff;
__device__ __forceinline__ int wave_min_i(int v) {
#ifndef OFA_WAVE_REDUCE_SHFL
#define OFA_DPP_I(CTRL, MASK) __builtin_amdgcn_update_dpp(v, v, CTRL, MASK, 0xf, false)
  v = min(v, OFA_DPP_I(0xB1, 0xf));                      // (wave_max's steps: lanes outside the row mask keep `old` = v)
  v = min(v, OFA_DPP_I(0x4E, 0xf));
  v = min(v, OFA_DPP_I(0x141, 0xf));
  v = min(v, OFA_DPP_I(0x140, 0xf));
  v = min(v, OFA_DPP_I(0x142, 0xa));
  v = min(v, OFA_DPP_I(0x143, 0xc));
#undef OFA_DPP_I
  return __builtin_amdgcn_readlane(v, 63);
#else
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
#endif
}
struct EvalCfg { float eps; int cs, ce, ranged; };          // ranged == 0: cs = 0, ce = V
// the row's outputs from its reduced (lse, sum of allowed x, count, arg-max column); `valid`: the target is an allowed column of [0, V)
template <typename T>
__device__ __forceinline__ void eval_row_done(const T* x, int64_t row, int64_t t, bool ignored, bool valid, float l, float X, float C,
                                              int amax, float eps, bool constrained, float* row_loss, float* row_nll, int32_t* row_hit) {
  float rl = 0.f, rn = 0.f;
  int hit = 0;
  if (!ignored && !valid) {
    rl = rn = INFINITY;                                  // (the -lprob of a column that is masked or does not exist; x[t] is not read)
  } else if (!ignored) {
    rn = l - ld1<T>(x + t);
    const float eps_i = eps / (constrained ? (C - 1.f + 1e-6f) : (C - 1.f));
    rl = (1.f - eps - eps_i) * rn + eps_i * (C * l - X);
    hit = amax == (int)t;
  }
  row_loss[row] = rl;
  row_nll[row] = rn;
  row_hit[row] = hit;
}

// Registers form (16-bit logits, ld <= 65536, no byte mask): scst_fwd_grad_kernel's block and per-VECTOR range test, nothing written back.
template <typename T, int NV>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void criterion_eval_regs_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target, float* __restrict__ row_loss, float* __restrict__ row_nll,
    int32_t* __restrict__ row_hit, int V, int ld, int64_t ignore_index, EvalCfg cfg) {
  constexpr int N = Vec<T>::N;
  static_assert(N == 8, "16-bit element types");
  __shared__ float sm[16], ss[16], sx[16];
  __shared__ int si[16];
  const int64_t row = blockIdx.x;
  const char* xb = reinterpret_cast<const char*>(logits + row * ld);
  const int nvec = ld / N;
  const int tid = threadIdx.x;
  const int cs = cfg.cs, ce = cfg.ce;
  uint4 raw[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i)      // (past the row's end the last vector is loaded again, in bounds, and never used: no branch per slab)
    raw[i] = *reinterpret_cast<const uint4*>(xb + (uint32_t)min(tid + i * 1024, nvec - 1) * 16u);
  const int f_lo = (cs + 7) >> 3, f_hi = ce >> 3, a_lo = cs >> 3, a_hi = (ce + 7) >> 3;
  uint32_t some_bits = 0, full_bits = 0;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + i * 1024;
    some_bits |= (uint32_t)(((v >= a_lo) & (v < a_hi)) | (v == 0)) << i;
    full_bits |= (uint32_t)((v >= f_lo) & (v < f_hi)) << i;
  }
  auto okc = [&](int th8, int k) {                       // column th8 + k, k = slab * 8192 + element, against moved uniform bounds
    return (th8 < V - k) & ((th8 < 4 - k) | ((th8 >= cs - k) & (th8 < ce - k)));
  };
  const int tid8 = tid * N;
  float m = -INFINITY, s = 0.f, sumx = 0.f;
  int bi = NO_COL;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!((some_bits >> i) & 1u)) continue;
    float a[N];
    unpack16<T>(raw[i], a);
    if (!((full_bits >> i) & 1u)) {                      // a cut vector: its disallowed columns are -inf to the max, the sum and the arg-max
#pragma unroll
      for (int j = 0; j < N; ++j) a[j] = okc(tid8, i * 8192 + j) ? a[j] : -INFINITY;
    }
    float cur = m;                                       // (m IS the largest allowed value so far: the arg-max needs no copy of it)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool gt = a[j] > cur;
      cur = gt ? a[j] : cur;
      bi = gt ? tid8 + i * 8192 + j : bi;
      sumx += a[j] == -INFINITY ? 0.f : a[j];
    }
    vec_merge<Exp2Fma>(m, s, a);                         // (every vector that gets here holds an allowed column: the new max is finite)
  }
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * ex2((m - mw) * L2E));
  const float xw = wave_sum(sumx);
  const int iw = wave_min_i(m == mw ? bi : NO_COL);
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { sm[wave] = mw; ss[wave] = sw; sx[wave] = xw; si[wave] = iw; }
  __syncthreads();
  if (tid >= 64) return;                                 // (wave 0 finishes the row: one wave result per lane)
  const int lane = tid;
  const float mv = lane < 16 ? sm[lane] : -INFINITY, sv = lane < 16 ? ss[lane] : 0.f, xv = lane < 16 ? sx[lane] : 0.f;
  const int iv = lane < 16 ? si[lane] : NO_COL;
  const float M = wave_max(mv);
  const float S = wave_sum(sv * ex2((mv - M) * L2E));      // (a wave of disallowed columns only, and lanes 16..63: 0 * 2^-inf = 0)
  const float X = wave_sum(xv);
  const int amax = wave_min_i(mv == M ? iv : NO_COL);
  if (tid != 0) return;
  const int64_t t = target[row];
  const bool valid = t >= 0 && t < V && (t < 4 || (t >= cs && t < ce));
  const float C = cfg.ranged ? (float)(4 + ce - cs) : (float)V;     // (cs >= 4, ce <= V: |[0,4) U [cs,ce)| needs no count)
  eval_row_done<T>(reinterpret_cast<const T*>(xb), row, t, t == ignore_index, valid, M + logf(S), X, C, amax, cfg.eps, cfg.ranged != 0,
                   row_loss, row_nll, row_hit);
}

// NN allowed-or-minus-infinity values of rising columns from c0 into a thread's (m, s, sum x, count, arg-max column)
template <int NN>
__device__ __forceinline__ void eval_merge(const float (&a)[NN], int c0, float& m, float& s, float& sumx, float& cnt, int& bi) {
  float lm = a[0];
#pragma unroll
  for (int j = 1; j < NN; ++j) lm = fmaxf(lm, a[j]);
  if (lm == -INFINITY) return;
  float cur = m;
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const bool gt = a[j] > cur;
    cur = gt ? a[j] : cur;
    bi = gt ? c0 + j : bi;
  }
  float acc = s * expf(m - cur);                         // max first, then ONE rescale (cur = the new max, finite; m = -inf: s = 0)
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    const bool on = a[j] != -INFINITY;
    acc += expf(a[j] - cur);
    sumx += on ? a[j] : 0.f;
    cnt += on ? 1.f : 0.f;
  }
  m = cur;
  s = acc;
}

// Streaming form (fp32 logits, a byte mask, rows the registers form does not hold, an ld that is no multiple of the vector): one
// 256-thread block reads the row once, by 16-byte vectors where `vec_ok` (ld a multiple of the vector width, the base aligned).
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void criterion_eval_stream_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target, const uint8_t* __restrict__ cmask, float* __restrict__ row_loss,
    float* __restrict__ row_nll, int32_t* __restrict__ row_hit, int64_t V, int64_t ld, int64_t ignore_index, EvalCfg cfg, int vec_ok) {
  constexpr int N = Vec<T>::N;
  __shared__ float sm[4], ss[4], sx[4], sc[4];
  __shared__ int si[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const T* x = logits + row * ld;
  const uint8_t* mk = MASK ? cmask + row * V : nullptr;
  const int64_t cs = cfg.ranged ? cfg.cs : -1, ce = cfg.ce;
  float m = -INFINITY, s = 0.f, sumx = 0.f, cnt = 0.f;
  int bi = NO_COL;
  const int64_t nvec = vec_ok ? V / N : 0;                 // (whole vectors below V; the rest of the row goes column by column)
  for (int64_t v = tid; v < nvec; v += 256) {
    const int64_t c0 = v * N;
    const int cls = scst_vec_class(c0, N, V, cs, ce);
    if (cls == 0) continue;
    float a[N];
    load_vec<T>(x + c0, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {                          // a disallowed column: -inf to the max, the sums and the arg-max (selects, no branches)
      bool ok = (cls == 2) | scst_ok(c0 + j, V, cs, ce);
      if constexpr (MASK) ok &= mk[c0 + j] != 0;
      a[j] = ok ? a[j] : -INFINITY;
    }
    eval_merge<N>(a, (int)c0, m, s, sumx, cnt, bi);
  }
  for (int64_t c = nvec * N + tid; c < V; c += 256) {
    bool ok = scst_ok(c, V, cs, ce);
    if constexpr (MASK) ok &= mk[c] != 0;
    const float a[1] = {ok ? ld1<T>(x + c) : -INFINITY};     // (c < V: the load is in bounds whatever `ok` says)
    eval_merge<1>(a, (int)c, m, s, sumx, cnt, bi);
  }
  const float mw = wave_max(m);
  const float sw = wave_sum(mw == -INFINITY ? 0.f : s * expf(m - mw));
  const float xw = wave_sum(sumx), cw = wave_sum(cnt);
  const int iw = wave_min_i(m == mw ? bi : NO_COL);
  if ((tid & 63) == 0) { sm[tid >> 6] = mw; ss[tid >> 6] = sw; sx[tid >> 6] = xw; sc[tid >> 6] = cw; si[tid >> 6] = iw; }
  __syncthreads();
  if (tid != 0) return;
  const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float S = 0.f;
  int amax = NO_COL;
  if (M > -INFINITY) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      S += ss[w] * expf(sm[w] - M);
      if (sm[w] == M) amax = min(amax, si[w]);
    }
  }
  const int64_t t = target[row];
  bool valid = t >= 0 && scst_ok(t, V, cs, ce);
  if constexpr (MASK) valid = valid && mk[t] != 0;
  eval_row_done<T>(x, row, t, t == ignore_index, valid, M > -INFINITY ? M + logf(S) : -INFINITY, sx[0] + sx[1] + sx[2] + sx[3],
                   sc[0] + sc[1] + sc[2] + sc[3], amax, cfg.eps, cfg.ranged != 0 || MASK, row_loss, row_nll, row_hit);
}

// One validation batch into the running accumulator acc fp64[4] = [ntokens, loss_sum, nll_sum, n_correct]: a single block sums the
// rows in reduce_sum_f32_kernel's order (256 lanes striding the rows, wave sums, the four wave results in order) and counts the
// targets that are not ignore_index -- one block, one order, no atomics: the same inputs give the same bits.
__global__ __launch_bounds__(256) void eval_stats_add_kernel(double* __restrict__ acc, const float* __restrict__ row_loss,
                                                             const float* __restrict__ row_nll, const int32_t* __restrict__ row_hit,
                                                             const int64_t* __restrict__ target, int64_t rows, int64_t ignore_index) {
  __shared__ float sl[4], sn[4];
  __shared__ int sh[4], st[4];
  float l = 0.f, n = 0.f;
  int h = 0, c = 0;
  for (int64_t i = threadIdx.x; i < rows; i += 256) {
    l += row_loss[i];
    n += row_nll[i];
    h += row_hit[i] != 0;
    c += target[i] != ignore_index;
  }
  l = wave_sum(l);
  n = wave_sum(n);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { h += __shfl_xor(h, o, 64); c += __shfl_xor(c, o, 64); }
  if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = l; sn[threadIdx.x >> 6] = n; sh[threadIdx.x >> 6] = h; st[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc[0] += (double)(st[0] + st[1] + st[2] + st[3]);
    acc[1] += (double)(sl[0] + sl[1] + sl[2] + sl[3]);
    acc[2] += (double)(sn[0] + sn[1] + sn[2] + sn[3]);
    acc[3] += (double)(sh[0] + sh[1] + sh[2] + sh[3]);
  }
}

// get_normalized_probs (model/ofa.py:287-299): fp32 softmax / log-softmax of the logits, one block per row.
__device__ __forceinline__ float block_sum(float v, float* sw) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  return sw[0] + sw[1] + sw[2] + sw[3];
}
template <typename T>
__global__ __launch_bounds__(256) void probs_fwd_kernel(const T* __restrict__ x, float* __restrict__ y, int64_t V, int64_t ld,
                                                        int log_probs) {
  __shared__ float sw[4];
  const T* xr = x + (int64_t)blockIdx.x * ld;
  float* yr = y + (int64_t)blockIdx.x * V;
  float m = -INFINITY;
  for (int64_t c = threadIdx.x; c < V; c += 256) m = fmaxf(m, ld1<T>(xr + c));
  m = wave_max(m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sw[0], sw[1]), fmaxf(sw[2], sw[3]));
  float s = 0.f;
  for (int64_t c = threadIdx.x; c < V; c += 256) s += expf(ld1<T>(xr + c) - m);
  s = block_sum(s, sw);
  const float l = m + logf(s);
  for (int64_t c = threadIdx.x; c < V; c += 256) {
    const float t = ld1<T>(xr + c) - l;
    yr[c] = log_probs ? t : expf(t);
  }
}
// log: dx = dy - exp(y)*sum(dy);   prob: dx = y*(dy - sum(dy*y))
template <typename T>
__global__ __launch_bounds__(256) void probs_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                        T* __restrict__ dx, int64_t V, int64_t ld, int log_probs) {
  __shared__ float sw[4];
  const float* dyr = dy + (int64_t)blockIdx.x * V;
  const float* yr = y + (int64_t)blockIdx.x * V;
  T* dxr = dx + (int64_t)blockIdx.x * ld;
  float s = 0.f;
  for (int64_t c = threadIdx.x; c < V; c += 256) s += log_probs ? dyr[c] : dyr[c] * yr[c];
  s = block_sum(s, sw);
  for (int64_t c = threadIdx.x; c < ld; c += 256) {
    float g = 0.f;
    if (c < V) g = log_probs ? dyr[c] - expf(yr[c]) * s : yr[c] * (dyr[c] - s);
    st1<T>(dxr + c, g);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sumsq_kernel(const T* __restrict__ x, float* __restrict__ partial, int64_t n) {
  constexpr int N = Vec<T>::N;
  __shared__ float sw[4];
  float s = 0.f;
  const int64_t nvec = n / N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float a[N];
    load_vec<T>(x + v * N, a);
#pragma unroll
    for (int j = 0; j < N; ++j) s += a[j] * a[j];
  }
  if (blockIdx.x == 0)
    for (int64_t e = nvec * N + threadIdx.x; e < n; e += 256) { const float a = ld1<T>(x + e); s += a * a; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int nb) {
  __shared__ float sw[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] += sw[0] + sw[1] + sw[2] + sw[3];
}

template <typename T>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                   const T* __restrict__ grad, T* __restrict__ model,
                                                   const float* __restrict__ coef, int64_t n, float lr, float beta1,
                                                   float beta2, float eps, float wd, float step_size, int dev_sched) {
  const float gmul = coef ? coef[0] : 1.0f;
  if (dev_sched) {                       // schedule state lives on the device: coef = [grad multiplier, step size, lr, skip]
    if (coef[3] != 0.f) return;          // non-finite gradient norm / empty batch: parameters and both moments stay untouched
    step_size = coef[1];
    lr = coef[2];
  }
  auto upd = [&](float g, float& p, float& mi, float& vi) {
    g *= gmul;
    mi = mi * beta1 + (1.f - beta1) * g;
    vi = vi * beta2 + (1.f - beta2) * g * g;
    if (wd != 0.f) p -= wd * lr * p;
    p -= step_size * mi / (sqrtf(vi) + eps);
  };
  // Two quads (4 parameters each) per thread and trip, every load of the trip issued before the first update.  The fp32 state and
  // the gradient are streamed with NONTEMPORAL loads / stores (each byte is touched once per step and the arrays are many times
  // the size of L2 / MALL): tools/experiments/adam_stream_bench.hip, 141.6 M parameters = 3.96 GB per pass: plain accesses on a
  // 4096-block grid 778 us (5.1 TB/s), nontemporal + 65536 blocks 620 us (6.4 TB/s).  The model-dtype copy is read by the next
  // forward: plain store.
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const int64_t nq = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q0 = (int64_t)blockIdx.x * 256 + threadIdx.x; q0 < nq; q0 += 2 * stride) {
    f4v p4[2], m4[2], v4[2], g4[2];
    u2v g2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t q = q0 + k * stride;
      if (q < nq) {
        const int64_t i = q << 2;
        p4[k] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(master + i));
        m4[k] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(m + i));
        v4[k] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(v + i));
        if constexpr (sizeof(T) == 4) g4[k] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(grad + i));
        else g2[k] = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(grad + i));
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t q = q0 + k * stride;
      if (q < nq) {
        const int64_t i = q << 2;
        float g[4];
        if constexpr (sizeof(T) == 4) {
          g[0] = g4[k].x; g[1] = g4[k].y; g[2] = g4[k].z; g[3] = g4[k].w;
        } else {
          // (the two words as scalars first: hipcc 7.2 folds __builtin_bit_cast(f16x2_t, v.y) of an ext-vector ELEMENT to element 0 --
          // the fp16 kernel updated elements 2, 3 of every quad with the gradients of elements 0, 1; tests/test_fp16_gpu.py)
          const uint32_t gx = g2[k][0], gy = g2[k][1];
          if constexpr (!__is_same(T, bf16_t)) {                                  // fp16
            const f16x2_t a = __builtin_bit_cast(f16x2_t, gx), b = __builtin_bit_cast(f16x2_t, gy);
            g[0] = (float)a[0]; g[1] = (float)a[1]; g[2] = (float)b[0]; g[3] = (float)b[1];
          } else {
            g[0] = __uint_as_float(gx << 16); g[1] = __uint_as_float(gx & 0xffff0000u);
            g[2] = __uint_as_float(gy << 16); g[3] = __uint_as_float(gy & 0xffff0000u);
          }
        }
        float px = p4[k].x, py = p4[k].y, pz = p4[k].z, pw = p4[k].w;
        float mx = m4[k].x, my = m4[k].y, mz = m4[k].z, mw = m4[k].w;
        float vx = v4[k].x, vy = v4[k].y, vz = v4[k].z, vw = v4[k].w;
        upd(g[0], px, mx, vx);
        upd(g[1], py, my, vy);
        upd(g[2], pz, mz, vz);
        upd(g[3], pw, mw, vw);
        const f4v mo = {mx, my, mz, mw}, vo = {vx, vy, vz, vw}, po = {px, py, pz, pw};
        __builtin_nontemporal_store(mo, reinterpret_cast<f4v*>(m + i));
        __builtin_nontemporal_store(vo, reinterpret_cast<f4v*>(v + i));
        __builtin_nontemporal_store(po, reinterpret_cast<f4v*>(master + i));
        if constexpr (sizeof(T) == 4) {
          *reinterpret_cast<f4v*>(model + i) = po;
        } else {
          u2v o;
          o.x = pack2<T>(px, py);
          o.y = pack2<T>(pz, pw);
          *reinterpret_cast<u2v*>(model + i) = o;
        }
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // tail
    const int64_t i = (nq << 2) + threadIdx.x;
    float p = master[i], mi = m[i], vi = v[i];
    upd(ld1<T>(grad + i), p, mi, vi);
    m[i] = mi;
    v[i] = vi;
    master[i] = p;
    st1<T>(model + i, p);
  }
}

// ---------------------------------------------------------------- EMA shadow of the weights (engine/ema/ema.py:140-194)
// Does this update average, and with which decay?  Decided on the device from the schedule state the step just wrote -- step[0] = t,
// the number of completed updates, and sched[3], the skip flag -- so that a captured step replays the rule, not one outcome of it:
//   apply <=> the update was not skipped and t % update_freq == 0     (ema.py:188-192: the counter advances on stepped updates only)
//   d = t < start_update ? 0 : decay ; a = 1 - d                      (ema.py:187; `a` rounded from the host's double: ema_rule)
// Uniform over the launch: every thread reads the same two words.
struct EmaRule {
  float d_on, a_on;          // fp32(decay), 1 - decay as torch's add_(alpha =) takes it (ema_rule)
  double start_update;
  int64_t update_freq;
};
__device__ __forceinline__ bool ema_decide(const double* __restrict__ step, const float* __restrict__ sched, const EmaRule& r,
                                           float& d, float& a) {
  if (sched[3] != 0.f) return false;
  const double t = step[0];
  if (r.update_freq > 1 && (int64_t)t % r.update_freq != 0) return false;
  const bool on = !(t < r.start_update);
  d = on ? r.d_on : 0.f;
  a = on ? r.a_on : 1.f;
  return true;
}
// One element: the reference's mul_(d) then add_(p, alpha = a) on a state of type S -- each a rounding to S -- written without
// contraction: the stated formula rounds both products and the sum to fp32 on their own.  (HIP's __fmul_rn / __fadd_rn are plain
// `*` / `+` compiled under hipcc's default -ffp-contract=fast inside the header: with them the sum came out as v_pk_fma_f32 whatever
// the caller's pragma said.  Plain operators under `fp contract(off)` compile to v_pk_mul_f32 / v_pk_add_f32.)
template <typename S> __device__ __forceinline__ float ema_round(float x);
template <> __device__ __forceinline__ float ema_round<float>(float x) { return x; }
template <> __device__ __forceinline__ float ema_round<bf16_t>(float x) { return bf2f(f2bf(x)); }
// (the fp32 value is pinned in a register first: hipcc selects fptrunc(fmul(fpext(half), float)) as ONE v_fma_mixlo_f16, which rounds
// the exact product to fp16 once -- torch rounds it to fp32 and then to fp16, and with d = 0.9f the product of an 11-bit state lands
// within half an fp32 ulp below an fp16 tie in 4 % of the elements: 40 of 1045 were one fp16 ulp off the recorded reference)
template <> __device__ __forceinline__ float ema_round<f16_t>(float x) {
  asm volatile("" : "+v"(x));
  return (float)(f16_t)x;
}
template <typename S> __device__ __forceinline__ float ema_one(float e, float p, float d, float a) {
#pragma clang fp contract(off)
  const float r = ema_round<S>(e * d);
  const float ap = a * p;
  return ema_round<S>(r + ap);
}
// the two 32-bit words of a 16-bit quad as four floats (the words arrive as scalars: see adam_kernel on bit_cast of a vector ELEMENT)
template <typename T> __device__ __forceinline__ void unpack_quad16(uint32_t x, uint32_t y, float* o) {
  if constexpr (!__is_same(T, bf16_t)) {                                  // fp16
    const f16x2_t a = __builtin_bit_cast(f16x2_t, x), b = __builtin_bit_cast(f16x2_t, y);
    o[0] = (float)a[0]; o[1] = (float)a[1]; o[2] = (float)b[0]; o[3] = (float)b[1];
  } else {
    o[0] = __uint_as_float(x << 16); o[1] = __uint_as_float(x & 0xffff0000u);
    o[2] = __uint_as_float(y << 16); o[3] = __uint_as_float(y & 0xffff0000u);
  }
}

// state (S = float, or the model dtype T) <- EMA of the model-dtype arena p; `shadow` (optional, T): round_T(state) for the forward
// of the averaged model.  adam_kernel's streaming pattern: two 4-element quads per thread and trip, every load of the trip issued
// before the first use; the fp32 state is touched once per step (nontemporal both ways), p was just written by Adam and the 16-bit
// results are read by an inference forward (plain).  Not applying writes nothing.
template <typename T, typename S>
__global__ __launch_bounds__(256) void ema_kernel(S* __restrict__ state, const T* __restrict__ p, T* __restrict__ shadow, int64_t n,
                                                  const double* __restrict__ step, const float* __restrict__ sched, EmaRule rule) {
  float d, a;
  if (!ema_decide(step, sched, rule, d, a)) return;
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  constexpr bool S32 = sizeof(S) == 4, T32 = sizeof(T) == 4;
  const int64_t nq = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q0 = (int64_t)blockIdx.x * 256 + threadIdx.x; q0 < nq; q0 += 2 * stride) {
    f4v e4[2], p4[2];
    u2v e2[2], p2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t q = q0 + k * stride;
      if (q < nq) {
        const int64_t i = q << 2;
        if constexpr (S32) e4[k] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(state + i));
        else e2[k] = *reinterpret_cast<const u2v*>(state + i);
        if constexpr (T32) p4[k] = *reinterpret_cast<const f4v*>(p + i);
        else p2[k] = *reinterpret_cast<const u2v*>(p + i);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t q = q0 + k * stride;
      if (q < nq) {
        const int64_t i = q << 2;
        float e[4], x[4];
        if constexpr (S32) { e[0] = e4[k].x; e[1] = e4[k].y; e[2] = e4[k].z; e[3] = e4[k].w; }
        else { const uint32_t ex = e2[k][0], ey = e2[k][1]; unpack_quad16<S>(ex, ey, e); }
        if constexpr (T32) { x[0] = p4[k].x; x[1] = p4[k].y; x[2] = p4[k].z; x[3] = p4[k].w; }
        else { const uint32_t px = p2[k][0], py = p2[k][1]; unpack_quad16<T>(px, py, x); }
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = ema_one<S>(e[j], x[j], d, a);
        if constexpr (S32) {
          const f4v eo = {e[0], e[1], e[2], e[3]};
          __builtin_nontemporal_store(eo, reinterpret_cast<f4v*>(state + i));
        } else {
          u2v o;
          o.x = pack2<S>(e[0], e[1]);
          o.y = pack2<S>(e[2], e[3]);
          *reinterpret_cast<u2v*>(state + i) = o;
        }
        if (shadow) {
          if constexpr (T32) {
            const f4v so = {e[0], e[1], e[2], e[3]};
            *reinterpret_cast<f4v*>(shadow + i) = so;
          } else {
            u2v o;
            o.x = pack2<T>(e[0], e[1]);
            o.y = pack2<T>(e[2], e[3]);
            *reinterpret_cast<u2v*>(shadow + i) = o;
          }
        }
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // tail
    const int64_t i = (nq << 2) + threadIdx.x;
    const float e = ema_one<S>(ld1<S>(state + i), ld1<T>(p + i), d, a);
    st1<S>(state + i, e);
    if (shadow) st1<T>(shadow + i, e);
  }
}

// The floating-point buffers of the state dict (BatchNorm running statistics: ~400 tensors of a ResNet-101, none of them in the
// arena) in ONE launch over a device-resident table: segment s averages len elements at src into state[off, off + len).  The grid
// is (blocks per segment, segments); a segment's blocks stride over it element by element (the buffers are short and have no
// alignment to speak of).  A segment that would leave the state array is skipped.
struct EmaSegment {
  const void* src;
  int64_t off, len;
};
template <typename T, typename S>
__global__ __launch_bounds__(256) void ema_segments_kernel(S* __restrict__ state, const EmaSegment* __restrict__ segs,
                                                           T* __restrict__ shadow, int64_t state_numel,
                                                           const double* __restrict__ step, const float* __restrict__ sched,
                                                           EmaRule rule) {
  float d, a;
  if (!ema_decide(step, sched, rule, d, a)) return;
  const EmaSegment sg = segs[blockIdx.y];
  if (sg.off < 0 || sg.len < 0 || sg.off > state_numel - sg.len) return;
  const T* src = static_cast<const T*>(sg.src);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.len; i += (int64_t)gridDim.x * 256) {
    const float e = ema_one<S>(ld1<S>(state + sg.off + i), ld1<T>(src + i), d, a);
    st1<S>(state + sg.off + i, e);
    if (shadow) st1<T>(shadow + sg.off + i, e);
  }
}

// One thread: the scalar arithmetic between the gradient norm and the Adam update, kept on the device so that a captured
// train step replays it (trainer.py:857-884 clip + 1/sample_size, adam.py:205-207 bias corrections).  ~25 tiny torch
// kernels otherwise, ~4.5 us each inside a hipGraph.
// Guard (engine/trainer.py:866-876 raises FloatingPointError("gradients are Nan/Inf") and never reaches optimizer.step): when the
// gradient norm is not finite or the step saw no target token (sample_size <= 0), sched = [0, 0, lr, 1] -- ofa_adam_step(step = 0)
// then returns without touching master weights or moments -- the update counter does not advance, and sched[4] (a running count
// of skipped updates) is incremented for the host to poll.
__device__ __forceinline__ void step_schedule_one(float gsq0, const double* __restrict__ sample_size, double* __restrict__ step,
                                                  const double* __restrict__ lr, float* __restrict__ sched, float* __restrict__ gnorm,
                                                  float clip_norm, double beta1, double beta2) {
  const double n = sample_size[0];
  const float inv_n = n > 0.0 ? (float)(1.0 / n) : 0.f;
  const float gn = sqrtf(gsq0) * inv_n;
  gnorm[0] = n > 0.0 ? gn : __builtin_nanf("");
  if (!(n > 0.0) || !isfinite(gn)) {
    sched[0] = 0.f;
    sched[1] = 0.f;
    sched[2] = (float)lr[0];
    sched[3] = 1.f;
    sched[4] += 1.f;
    return;
  }
  sched[3] = 0.f;
  float coef = inv_n;
  if (clip_norm > 0.f) coef *= fminf(clip_norm / (gn + 1e-6f), 1.0f);
  const double t = step[0] + 1.0;
  step[0] = t;
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  sched[0] = coef;
  sched[1] = (float)(lr[0] * sqrt(bc2) / bc1);
  sched[2] = (float)lr[0];
  gnorm[0] = gn;
}
__global__ void step_schedule_kernel(const float* __restrict__ gsq, const double* __restrict__ sample_size,
                                     double* __restrict__ step, const double* __restrict__ lr, float* __restrict__ sched,
                                     float* __restrict__ gnorm, float clip_norm, double beta1, double beta2) {
  if (threadIdx.x || blockIdx.x) return;
  step_schedule_one(gsq[0], sample_size, step, lr, sched, gnorm, clip_norm, beta1, beta2);
}

// The scaled-loss variant of step_schedule_kernel: engine/optim/fp16_optimizer.py:170-204 + dynamic_loss_scaler.py:9-70 in one
// device thread.  `ls` (fp64[8]) = [loss_scale, iter, last_overflow_iter, last_rescale_iter, overflows_since_rescale, fatal,
// 0, 0]; the gradients in the arena are loss_scale * (sum of per-sample gradients).
//   multiply_factor = 1 / (loss_scale * sample_size)                        (zero_grad :228-229, trainer.py:857-860)
//   grad_norm       = multiply_factor * ||g||                               (:178)
//   if grad_norm > max_norm > 0: multiply_factor *= max_norm / grad_norm    (:181-182; no "+1e-6", no clamp: the fp16 form)
//   overflow (inf / nan norm): check_overflow (:44-70) -- last_overflow_iter = iter, ++overflows_since_rescale, and when
//       overflows / iters_since_rescale >= tolerance: loss_scale = max(loss_scale / factor, threshold), last_rescale_iter = iter;
//       loss_scale <= min_loss_scale restores the previous scale and sets `fatal` (the reference raises FloatingPointError);
//       ++iter; the update is SKIPPED (trainer.py catches OverflowError and zeroes the grads)
//   otherwise update() (:33-37): if (iter - last_overflow_iter) % scale_window == 0: loss_scale *= factor,
//       last_rescale_iter = iter; ++iter.
__device__ __forceinline__ void step_schedule_scaled_one(float gsq0, const double* __restrict__ sample_size, double* __restrict__ step,
                                                         const double* __restrict__ lr, float* __restrict__ sched,
                                                         float* __restrict__ gnorm, double* __restrict__ ls, float clip_norm,
                                                         double beta1, double beta2, double scale_factor, double scale_window,
                                                         double tolerance, double threshold, double min_loss_scale) {
  const double n = sample_size[0];
  const double scale = ls[0];
  double mf = n > 0.0 ? 1.0 / (scale * n) : 0.0;
  const float gn = (float)(mf * sqrt((double)gsq0));
  gnorm[0] = n > 0.0 ? gn : __builtin_nanf("");
  if (!(n > 0.0)) {                              // an EMPTY batch is not an overflow: skip the update, leave the scaler's state alone
    sched[0] = 0.f;                              // (the reference's scaler only reacts to an inf / nan norm, dynamic_loss_scaler.py:44-70)
    sched[1] = 0.f;
    sched[2] = (float)lr[0];
    sched[3] = 1.f;
    sched[4] += 1.f;
    return;
  }
  if (!isfinite(gn)) {                           // overflow: the loss scaler's check_overflow, the update is skipped
    const double it = ls[1];
    const double since = it - ls[3];
    ls[2] = it;
    ls[4] += 1.0;
    const double pct = ls[4] / since;             // (since == 0 -> inf / nan >= tolerance is true / false as in Python's float division
    if (since <= 0.0 || pct >= tolerance) {      //  ... which raises ZeroDivisionError there; treated as "decrease" here)
      double dec = scale / scale_factor;
      if (threshold > 0.0 && dec < threshold) dec = threshold;
      ls[0] = dec;
      ls[3] = it;
      ls[4] = 0.0;
    }
    if (ls[0] <= min_loss_scale) {                // FloatingPointError in the reference: raised BEFORE its `_iter += 1`
      ls[0] = scale;
      ls[5] = 1.0;
    } else {
      ls[1] = it + 1.0;
    }
    sched[0] = 0.f;
    sched[1] = 0.f;
    sched[2] = (float)lr[0];
    sched[3] = 1.f;
    sched[4] += 1.f;
    return;
  }
  sched[3] = 0.f;
  if (clip_norm > 0.f && gn > clip_norm) mf *= (double)clip_norm / (double)gn;
  const double t = step[0] + 1.0;
  step[0] = t;
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  sched[0] = (float)mf;
  sched[1] = (float)(lr[0] * sqrt(bc2) / bc1);
  sched[2] = (float)lr[0];
  const double it = ls[1];
  if (fmod(it - ls[2], scale_window) == 0.0) {
    ls[0] = scale * scale_factor;
    ls[3] = it;
  }
  ls[1] = it + 1.0;
}
__global__ void step_schedule_scaled_kernel(const float* __restrict__ gsq, const double* __restrict__ sample_size,
                                            double* __restrict__ step, const double* __restrict__ lr, float* __restrict__ sched,
                                            float* __restrict__ gnorm, double* __restrict__ ls, float clip_norm, double beta1,
                                            double beta2, double scale_factor, double scale_window, double tolerance,
                                            double threshold, double min_loss_scale) {
  if (threadIdx.x || blockIdx.x) return;
  step_schedule_scaled_one(gsq[0], sample_size, step, lr, sched, gnorm, ls, clip_norm, beta1, beta2, scale_factor, scale_window,
                           tolerance, threshold, min_loss_scale);
}

// The gradient norm's sum of squares, its final fold and the step's scalar schedule in ONE launch: sumsq_kernel's blocks, and the
// LAST block to finish (a ticket drawn once the block's write-through partial is acknowledged; it resets the ticket itself) folds the block partials in
// sumsq_final_kernel's order, then runs step_schedule_one / step_schedule_scaled_one and the Philox counter add that followed as
// launches of their own.  gsq[0] is written, not added to: it needs no clearing and holds what the separate launches leave there.
struct SchedArgs {
  const double* sample_size; double* step; const double* lr; float* sched; float* gnorm; double* ls;   // ls NULL: no loss scaler
  int64_t* counter; int64_t counter_add;                                                                // counter NULL: none
  float clip_norm; double beta1, beta2, scale_factor, scale_window, tolerance, threshold, min_loss_scale;
};
template <typename T>
__global__ __launch_bounds__(256) void sumsq_schedule_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                                             float* __restrict__ gsq, unsigned* __restrict__ ticket, int64_t n,
                                                             SchedArgs a) {
  constexpr int N = Vec<T>::N;
  __shared__ float sw[4];
  __shared__ float fin[4];
  float s = 0.f;
  const int64_t nvec = n / N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float e[N];
    load_vec<T>(x + v * N, e);
#pragma unroll
    for (int j = 0; j < N; ++j) s += e[j] * e[j];
  }
  if (blockIdx.x == 0)
    for (int64_t e = nvec * N + threadIdx.x; e < n; e += 256) { const float q = ld1<T>(x + e); s += q * q; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    // a write-through store of the partial, its acknowledgement, then the ticket (relaxed, agent scope): the last arriver reads the
    // partials with agent-scope loads.  (With __threadfence() on both sides the kernel took 105 us instead of 58: DESIGN.md 5p.
    // The same hand-off, resting on the same measured gfx950 behaviour, as ce_fwd_grad_kernel's statistics tail: see there.)
    __hip_atomic_store(partial + blockIdx.x, sw[0] + sw[1] + sw[2] + sw[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    fin[0] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (fin[0] == 0.f) return;                               // (uniform over the block)
  const int nb = (int)gridDim.x;
  float t = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) t += __hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = t;   // (sw was last read before the barrier above)
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = 0.f + (sw[0] + sw[1] + sw[2] + sw[3]);   // (sumsq_final_kernel adds onto a cleared gsq)
    gsq[0] = total;
    if (a.ls) step_schedule_scaled_one(total, a.sample_size, a.step, a.lr, a.sched, a.gnorm, a.ls, a.clip_norm, a.beta1, a.beta2,
                                       a.scale_factor, a.scale_window, a.tolerance, a.threshold, a.min_loss_scale);
    else step_schedule_one(total, a.sample_size, a.step, a.lr, a.sched, a.gnorm, a.clip_norm, a.beta1, a.beta2);
    if (a.counter) a.counter[0] += a.counter_add;
    *ticket = 0u;
  }
}
}  // namespace ofa
using namespace ofa;

extern "C" int ofa_cross_entropy_fwd(const void* logits, const int64_t* target, float* lse, float* row_loss, int64_t rows,
                                     int64_t V, int64_t ld, int64_t ignore_index, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "cross_entropy_fwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 0 && ld >= V && logits && target && lse && row_loss, OFA_ERR_INVALID, "cross_entropy_fwd: bad argument");
  OFA_REQUIRE(ld % dt_vecn(dtype) == 0, OFA_ERR_INVALID, "cross_entropy_fwd: ld=%lld must be a multiple of the 16-byte vector width", (long long)ld);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ce_fwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, lse, row_loss, V, ld, ignore_index);
  });
  return check_launch("cross_entropy_fwd");
}

// the whole row lives in the block's registers: NV vectors of 8 per thread, 1024 threads
template <typename T>
static bool ce_fwd_grad_launch(const T* logits, const int64_t* target, const float* gs, float* lse, float* row_loss, T* dlogits,
                               int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, hipStream_t st, float* loss_out = nullptr,
                               double* stats = nullptr, unsigned* ticket = nullptr) {
  const int64_t per_thread = (ld / 8 + 1023) / 1024;
#define CE_FG(NV) hipLaunchKernelGGL((ce_fwd_grad_kernel<T, NV>), dim3((unsigned)rows), dim3(1024), 0, st, logits, target, gs, lse, row_loss, dlogits, (int)V, (int)ld, ignore_index, loss_out, stats, ticket)
  if (per_thread <= 1) CE_FG(1);
  else if (per_thread <= 2) CE_FG(2);
  else if (per_thread <= 4) CE_FG(4);
  else if (per_thread <= 7) CE_FG(7);
  else if (per_thread <= 8) CE_FG(8);
  else return false;
#undef CE_FG
  return true;
}

extern "C" int ofa_cross_entropy_fwd_grad_ok(int64_t V, int64_t ld, int dtype) {
  return (dtype == OFA_BF16 || dtype == OFA_F16) && V > 0 && ld >= V && ld % 8 == 0 && ld <= 8 * 1024 * 8;
}

extern "C" int ofa_cross_entropy_fwd_grad(const void* logits, const int64_t* target, const float* grad_scale, float* lse,
                                          float* row_loss, void* dlogits, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index,
                                          int dtype, void* stream) {
  OFA_REQUIRE(ofa_cross_entropy_fwd_grad_ok(V, ld, dtype), OFA_ERR_UNSUPPORTED,
              "cross_entropy_fwd_grad: 16-bit logits of at most 65536 (padded) columns, ld a multiple of 8 (V=%lld ld=%lld dtype=%d)", (long long)V, (long long)ld, dtype);
  OFA_REQUIRE(rows >= 0 && logits && target && lse && row_loss && dlogits, OFA_ERR_INVALID, "cross_entropy_fwd_grad: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const bool ok = dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return ce_fwd_grad_launch<T>((const T*)logits, target, grad_scale, lse, row_loss, (T*)dlogits, rows, V, ld, ignore_index, st);
  });
  OFA_REQUIRE(ok, OFA_ERR_UNSUPPORTED, "cross_entropy_fwd_grad: row too long");
  return check_launch("cross_entropy_fwd_grad");
}

extern "C" int ofa_cross_entropy_fwd_grad_stats(const void* logits, const int64_t* target, const float* grad_scale, float* lse,
                                                float* row_loss, void* dlogits, int64_t rows, int64_t V, int64_t ld,
                                                int64_t ignore_index, int dtype, float* loss, double* stats, unsigned int* ticket,
                                                void* stream) {
  OFA_REQUIRE(ofa_cross_entropy_fwd_grad_ok(V, ld, dtype), OFA_ERR_UNSUPPORTED,
              "cross_entropy_fwd_grad_stats: 16-bit logits of at most 65536 (padded) columns, ld a multiple of 8 (V=%lld ld=%lld dtype=%d)", (long long)V, (long long)ld, dtype);
  OFA_REQUIRE(rows >= 1 && logits && target && lse && row_loss && dlogits && loss && stats && ticket, OFA_ERR_INVALID,
              "cross_entropy_fwd_grad_stats: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const bool ok = dispatch_dtype16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return ce_fwd_grad_launch<T>((const T*)logits, target, grad_scale, lse, row_loss, (T*)dlogits, rows, V, ld, ignore_index, st, loss,
                                 stats, ticket);
  });
  OFA_REQUIRE(ok, OFA_ERR_UNSUPPORTED, "cross_entropy_fwd_grad_stats: row too long");
  return check_launch("cross_entropy_fwd_grad_stats");
}

extern "C" int ofa_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* grad_scale,
                                     void* dlogits, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, int dtype,
                                     void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "cross_entropy_bwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 0 && ld >= V && logits && target && lse && dlogits, OFA_ERR_INVALID, "cross_entropy_bwd: bad argument");
  OFA_REQUIRE(ld % dt_vecn(dtype) == 0, OFA_ERR_INVALID, "cross_entropy_bwd: ld must be a multiple of the 16-byte vector width");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ce_bwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, lse, grad_scale, (T*)dlogits, V, ld, ignore_index);
  });
  return check_launch("cross_entropy_bwd");
}

extern "C" int ofa_ls_cross_entropy_fwd(const void* logits, const int64_t* target, float* lse, float* row_loss, float* row_nll,
                                        float* row_cnt, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps,
                                        int64_t cstart, int64_t cend, const uint8_t* cmask, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ls_cross_entropy_fwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 1 && ld >= V && logits && target && lse && row_loss && row_nll && row_cnt, OFA_ERR_INVALID,
              "ls_cross_entropy_fwd: bad argument");
  OFA_REQUIRE(eps >= 0.f && eps < 1.f && (cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V)), OFA_ERR_INVALID,
              "ls_cross_entropy_fwd: bad eps / constraint range [%lld, %lld)", (long long)cstart, (long long)cend);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const LsCfg cfg{eps, cstart, cend, cmask};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((lsce_fwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, lse, row_loss, row_nll, row_cnt, V, ld, ignore_index, cfg);
  });
  return check_launch("ls_cross_entropy_fwd");
}

extern "C" int ofa_ls_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* row_cnt,
                                        const float* row_w, const float* grad_scale, void* dlogits, int64_t rows, int64_t V,
                                        int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend,
                                        const uint8_t* cmask, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "ls_cross_entropy_bwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 1 && ld >= V && logits && target && lse && row_cnt && dlogits, OFA_ERR_INVALID,
              "ls_cross_entropy_bwd: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const LsCfg cfg{eps, cstart, cend, cmask};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((lsce_bwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, lse, row_cnt, row_w, grad_scale, (T*)dlogits, V, ld, ignore_index, cfg);
  });
  return check_launch("ls_cross_entropy_bwd");
}

// the registers form holds 16-bit rows of at most 8 slabs x 1024 threads x 8 columns; everything else streams
template <typename T>
static void scst_launch(const T* logits, const int64_t* target, const float* reward, const int32_t* row_seq, int64_t rows_per_seq,
                        const float* gs, float* lse, float* row_loss, T* dlogits, int64_t rows, int64_t nseq, int64_t V, int64_t ld,
                        int64_t ignore_index, int64_t cs, int64_t ce, hipStream_t st) {
  if constexpr (sizeof(T) == 2) {
    const int64_t per_thread = (ld / 8 + 1023) / 1024;
#define SCST_FG(NV) hipLaunchKernelGGL((scst_fwd_grad_kernel<T, NV>), dim3((unsigned)rows), dim3(1024), 0, st, logits, target, reward, row_seq, (int)rows_per_seq, gs, lse, row_loss, dlogits, (int)nseq, (int)V, (int)ld, ignore_index, (int)cs, (int)ce)
    if (per_thread <= 1) { SCST_FG(1); return; }
    if (per_thread <= 2) { SCST_FG(2); return; }
    if (per_thread <= 4) { SCST_FG(4); return; }
    if (per_thread <= 7) { SCST_FG(7); return; }
    if (per_thread <= 8) { SCST_FG(8); return; }
#undef SCST_FG
  }
  hipLaunchKernelGGL((scst_stream_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, logits, target, reward, row_seq, rows_per_seq, gs,
                     lse, row_loss, dlogits, nseq, V, ld, ignore_index, cs, ce);
}

extern "C" int ofa_scst_loss_fwd_grad(const void* logits, const int64_t* target, const float* reward, const int32_t* row_seq,
                                      int64_t rows_per_seq, const float* grad_scale, float* lse, float* row_loss, void* dlogits,
                                      int64_t rows, int64_t nseq, int64_t V, int64_t ld, int64_t ignore_index, int64_t cstart,
                                      int64_t cend, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "scst_loss_fwd_grad: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 31) && nseq > 0 && nseq < ((int64_t)1 << 31) && V > 1 && ld >= V && logits && target &&
                  reward && lse && row_loss && dlogits,
              OFA_ERR_INVALID, "scst_loss_fwd_grad: bad argument");
  OFA_REQUIRE(row_seq || (rows_per_seq >= 1 && rows_per_seq < ((int64_t)1 << 31)), OFA_ERR_INVALID,
              "scst_loss_fwd_grad: rows_per_seq=%lld without a row_seq map", (long long)rows_per_seq);
  OFA_REQUIRE(ld % dt_vecn(dtype) == 0, OFA_ERR_INVALID, "scst_loss_fwd_grad: ld=%lld must be a multiple of the 16-byte vector width", (long long)ld);
  OFA_REQUIRE(cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V), OFA_ERR_INVALID,
              "scst_loss_fwd_grad: bad constraint range [%lld, %lld)", (long long)cstart, (long long)cend);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    scst_launch<T>((const T*)logits, target, reward, row_seq, row_seq ? 1 : rows_per_seq, grad_scale, lse, row_loss, (T*)dlogits, rows, nseq,
                   V, ld, ignore_index, cstart < 0 ? 0 : cstart, cstart < 0 ? V : cend, st);      // (no range: [0, V))
  });
  return check_launch("scst_loss_fwd_grad");
}

namespace ofa {
// the node form: trie_loss.hip, next to the row core whose formulas it shares (arguments checked by the caller below)
void trie_criterion_eval_launch(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                const int32_t* edge_token, int64_t N, int64_t E, float* row_loss, float* row_nll, int32_t* row_hit,
                                int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend,
                                int dtype, hipStream_t st);
}
static bool criterion_eval_regs_ok(const void* logits, const uint8_t* cmask, int64_t V, int64_t ld, int dtype) {
  return (dtype == OFA_BF16 || dtype == OFA_F16) && !cmask && ld % 8 == 0 && ld <= 8 * 1024 * 8 && aligned16(logits);
}

extern "C" int ofa_criterion_eval(const void* logits, const int64_t* target, const uint8_t* cmask, const int32_t* node,
                                  const int32_t* node_edge_off, const int32_t* edge_token, int64_t N, int64_t E, float* row_loss,
                                  float* row_nll, int32_t* row_hit, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps,
                                  int64_t cstart, int64_t cend, int dtype, void* stream) {
  const int64_t lim = (int64_t)1 << 31;
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "criterion_eval: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && rows < lim && V > 1 && V < lim && ld >= V && logits && target && row_loss && row_nll && row_hit, OFA_ERR_INVALID,
              "criterion_eval: bad argument (rows=%lld V=%lld ld=%lld)", (long long)rows, (long long)V, (long long)ld);
  OFA_REQUIRE(eps >= 0.f && eps < 1.f && (cstart < 0 || (cstart >= 4 && cend > cstart && cend <= V)), OFA_ERR_INVALID,
              "criterion_eval: bad eps / constraint range [%lld, %lld)", (long long)cstart, (long long)cend);
  OFA_REQUIRE(!(node && cmask), OFA_ERR_INVALID, "criterion_eval: a closed set comes as a byte mask or as trie nodes, not both");
  // (E leaves room for the gather loop's 32-bit edge index to step past the last edge, as ofa_trie_ls_cross_entropy_fwd)
  OFA_REQUIRE(!node || (node_edge_off && N >= 1 && N < lim && E >= 0 && E < lim - 4096 && (edge_token || E == 0)), OFA_ERR_INVALID,
              "criterion_eval: nodes without a trie (N=%lld E=%lld)", (long long)N, (long long)E);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (node) {
    trie_criterion_eval_launch(logits, target, node, node_edge_off, edge_token, N, E, row_loss, row_nll, row_hit, rows, V, ld, ignore_index,
                               eps, cstart, cend, dtype, st);
    return check_launch("criterion_eval");
  }
  const EvalCfg cfg{eps, cstart < 0 ? 0 : (int)cstart, cstart < 0 ? (int)V : (int)cend, cstart < 0 ? 0 : 1};      // (no range: [0, V))
  const bool regs = criterion_eval_regs_ok(logits, cmask, V, ld, dtype);
  const int vec_ok = ld % dt_vecn(dtype) == 0 && aligned16(logits);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if constexpr (sizeof(T) == 2) {
      if (regs) {
        const int64_t per_thread = (ld / 8 + 1023) / 1024;
#define EVAL_RG(NV) hipLaunchKernelGGL((criterion_eval_regs_kernel<T, NV>), dim3((unsigned)rows), dim3(1024), 0, st, (const T*)logits, target, row_loss, row_nll, row_hit, (int)V, (int)ld, ignore_index, cfg)
        if (per_thread <= 1) EVAL_RG(1);
        else if (per_thread <= 2) EVAL_RG(2);
        else if (per_thread <= 4) EVAL_RG(4);
        else if (per_thread <= 7) EVAL_RG(7);
        else EVAL_RG(8);
#undef EVAL_RG
        return;
      }
    }
    if (cmask)
      hipLaunchKernelGGL((criterion_eval_stream_kernel<T, true>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, cmask,
                         row_loss, row_nll, row_hit, V, ld, ignore_index, cfg, vec_ok);
    else
      hipLaunchKernelGGL((criterion_eval_stream_kernel<T, false>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, target, cmask,
                         row_loss, row_nll, row_hit, V, ld, ignore_index, cfg, vec_ok);
  });
  return check_launch("criterion_eval");
}

extern "C" int ofa_eval_stats_add(double* acc, const float* row_loss, const float* row_nll, const int32_t* row_hit, const int64_t* target,
                                  int64_t rows, int64_t ignore_index, void* stream) {
  OFA_REQUIRE(acc && rows >= 0 && (rows == 0 || (row_loss && row_nll && row_hit && target)), OFA_ERR_INVALID, "eval_stats_add: bad argument");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(eval_stats_add_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, acc, row_loss, row_nll, row_hit, target, rows,
                     ignore_index);
  return check_launch("eval_stats_add");
}

extern "C" int ofa_probs_fwd(const void* logits, float* out, int64_t rows, int64_t V, int64_t ld, int log_probs, int dtype,
                             void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "probs_fwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 0 && ld >= V && logits && out, OFA_ERR_INVALID, "probs_fwd: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((probs_fwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, (const T*)logits, out, V, ld, log_probs);
  });
  return check_launch("probs_fwd");
}

extern "C" int ofa_probs_bwd(const float* dy, const float* y, void* dlogits, int64_t rows, int64_t V, int64_t ld,
                             int log_probs, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "probs_bwd: bad dtype %d", dtype);
  OFA_REQUIRE(rows >= 0 && V > 0 && ld >= V && dy && y && dlogits, OFA_ERR_INVALID, "probs_bwd: bad argument");
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((probs_bwd_kernel<T>), dim3((unsigned)rows), dim3(256), 0, st, dy, y, (T*)dlogits, V, ld, log_probs);
  });
  return check_launch("probs_bwd");
}

extern "C" int ofa_sumsq_ws_floats(void) { return 1024; }

extern "C" int ofa_sumsq(const void* x, float* out, float* ws, int64_t n, int dtype, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "sumsq: bad dtype %d", dtype);
  OFA_REQUIRE(n >= 0 && out && ws && (n == 0 || x), OFA_ERR_INVALID, "sumsq: bad argument");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int vecw = dt_vecn(dtype);
  int64_t nbl = (n / vecw + 255) / 256;
  const int nb = (int)(nbl < 1 ? 1 : (nbl > 1024 ? 1024 : nbl));
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((sumsq_kernel<T>), dim3(nb), dim3(256), 0, st, (const T*)x, ws, n);
  });
  int rc = check_launch("sumsq");
  if (rc) return rc;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, out, nb);
  return check_launch("sumsq_final");
}

extern "C" int ofa_sumsq_schedule(const void* x, float* gsq, float* ws, unsigned int* ticket, int64_t n, int dtype,
                                  const double* sample_size, double* step, const double* lr, float* sched, float* gnorm,
                                  double* loss_scaler, int64_t* counter, int64_t counter_add, float clip_norm, double beta1,
                                  double beta2, double scale_factor, double scale_window, double tolerance, double threshold,
                                  double min_loss_scale, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "sumsq_schedule: bad dtype %d", dtype);
  OFA_REQUIRE(n >= 1 && x && gsq && ws && ticket && sample_size && step && lr && sched && gnorm, OFA_ERR_INVALID,
              "sumsq_schedule: bad argument");
  OFA_REQUIRE(!loss_scaler || (scale_factor > 1.0 && scale_window >= 1.0 && min_loss_scale >= 0.0), OFA_ERR_INVALID,
              "sumsq_schedule: bad scaler configuration");
  hipStream_t st = (hipStream_t)stream;
  const int vecw = dt_vecn(dtype);
  int64_t nbl = (n / vecw + 255) / 256;
  const int nb = (int)(nbl < 1 ? 1 : (nbl > 1024 ? 1024 : nbl));                 // (ofa_sumsq's grid: the same partials)
  SchedArgs a{sample_size, step, lr, sched, gnorm, loss_scaler, counter, counter_add, clip_norm, beta1, beta2,
              scale_factor, scale_window, tolerance, threshold, min_loss_scale};
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((sumsq_schedule_kernel<T>), dim3(nb), dim3(256), 0, st, (const T*)x, ws, gsq, ticket, n, a);
  });
  return check_launch("sumsq_schedule");
}

// Host only: the blocks ofa_adam_step_grid launches for n parameters -- one thread per parameter (a thread owns quads, so three in four
// idle below the cap), at most max_blocks (0: the kernel's own cap of 65536); -1 for a bad argument.
extern "C" int ofa_adam_step_blocks(int64_t n, int max_blocks) {
  if (n < 0 || max_blocks < 0) return -1;
  const int64_t nbl = (n + 255) / 256;
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;      // (small blocks of work: the tail of a 4096-block grid cost 15 %)
  return (int)(nbl > cap ? cap : nbl);
}

extern "C" int ofa_adam_step_grid(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, void* model_param,
                                  const float* coef, int64_t n, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, int step, int dtype, int max_blocks, void* stream) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "adam_step: bad dtype %d", dtype);
  OFA_REQUIRE(n >= 0 && step >= 0 && max_blocks >= 0 && master && exp_avg && exp_avg_sq && grad && model_param, OFA_ERR_INVALID, "adam_step: bad argument");
  OFA_REQUIRE(step >= 1 || coef, OFA_ERR_INVALID, "adam_step: step == 0 takes the step size and lr from coef[1], coef[2]");
  if (n == 0) return 0;
  // adam.py:205-207
  const int dev_sched = step == 0;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float step_size = dev_sched ? 0.f : (float)(lr * sqrt(bc2) / bc1);
  hipStream_t st = (hipStream_t)stream;
  OFA_REQUIRE(!(((uintptr_t)master | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) && !(((uintptr_t)grad | (uintptr_t)model_param) & 7),
              OFA_ERR_INVALID, "adam_step: arenas must be 16-byte (fp32 state) / 8-byte (grad, model copy) aligned");
  const int nb = ofa_adam_step_blocks(n, max_blocks);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((adam_kernel<T>), dim3(nb), dim3(256), 0, st, master, exp_avg, exp_avg_sq, (const T*)grad, (T*)model_param, coef, n, lr, beta1, beta2, eps, weight_decay, step_size, dev_sched);
  });
  return check_launch("adam_step");
}

extern "C" int ofa_adam_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, void* model_param,
                             const float* coef, int64_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, int dtype, void* stream) {
  return ofa_adam_step_grid(master, exp_avg, exp_avg_sq, grad, model_param, coef, n, lr, beta1, beta2, eps, weight_decay, step, dtype, 0,
                            stream);
}

// the checks the two EMA entry points share; fills the rule the kernels take
static int ema_rule(const char* who, const void* state, const void* p, const double* step, const float* sched, double decay,
                    int64_t start_update, int64_t update_freq, int dtype, int state_dtype, int max_blocks, EmaRule* rule) {
  OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, "%s: bad dtype %d", who, dtype);
  OFA_REQUIRE(state_dtype == OFA_F32 || state_dtype == dtype, OFA_ERR_INVALID,
              "%s: the state is fp32 or of the model dtype (dtype %d, state dtype %d)", who, dtype, state_dtype);
  OFA_REQUIRE(state && p && step && sched && max_blocks >= 0, OFA_ERR_INVALID, "%s: bad argument", who);
  OFA_REQUIRE(decay >= 0.0 && decay <= 1.0 && start_update >= 0 && update_freq >= 1, OFA_ERR_INVALID,
              "%s: decay in [0, 1], start_update >= 0, update_freq >= 1 (got %g, %lld, %lld)", who, decay, (long long)start_update,
              (long long)update_freq);
  // torch hands `mul_` its scalar in fp32 for every dtype, but `add_(alpha =)` on a 16-bit tensor converts alpha to the tensor's
  // dtype first (the CPU kernel the recorded reference ran: bf16(0.1) = 0.10009765625): a 16-bit state takes that alpha.  torch's GPU
  // kernel keeps alpha in fp32: a 16-bit state can differ in its last bit from a reference run there (include/ofasys_amd.h)
  float a = (float)(1.0 - decay);
  if (state_dtype == OFA_F16) a = (float)(_Float16)a;
  if (state_dtype == OFA_BF16) {
    uint32_t u;
    memcpy(&u, &a, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;      // round to nearest even
    memcpy(&a, &u, 4);
  }
  *rule = EmaRule{(float)decay, a, (double)start_update, update_freq};
  return 0;
}

extern "C" int ofa_ema_step(void* state, const void* p, void* shadow, int64_t n, const double* step, const float* sched,
                            double decay, int64_t start_update, int64_t update_freq, int dtype, int state_dtype, int max_blocks,
                            void* stream) {
  EmaRule rule;
  if (int rc = ema_rule("ema_step", state, p, step, sched, decay, start_update, update_freq, dtype, state_dtype, max_blocks, &rule)) return rc;
  OFA_REQUIRE(n >= 0, OFA_ERR_INVALID, "ema_step: bad argument");
  if (n == 0) return 0;
  // one quad is 16 bytes of fp32, 8 bytes of a 16-bit type
  const uintptr_t sa = state_dtype == OFA_F32 ? 15 : 7, ta = dtype == OFA_F32 ? 15 : 7;
  OFA_REQUIRE(!((uintptr_t)state & sa) && !(((uintptr_t)p | (uintptr_t)shadow) & ta), OFA_ERR_INVALID,
              "ema_step: arenas must be 16-byte (fp32) / 8-byte (16-bit) aligned");
  const int64_t nbl = ((n >> 2) + 511) / 512;               // two quads per thread
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  const int nb = (int)(nbl < 1 ? 1 : (nbl > cap ? cap : nbl));
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (state_dtype == OFA_F32) hipLaunchKernelGGL((ema_kernel<T, float>), dim3(nb), dim3(256), 0, st, (float*)state, (const T*)p, (T*)shadow, n, step, sched, rule);
    else hipLaunchKernelGGL((ema_kernel<T, T>), dim3(nb), dim3(256), 0, st, (T*)state, (const T*)p, (T*)shadow, n, step, sched, rule);
  });
  return check_launch("ema_step");
}

extern "C" int ofa_ema_segments_step(void* state, const void* segments, void* shadow, int64_t n, int64_t state_numel, int64_t max_len,
                                     const double* step, const float* sched, double decay, int64_t start_update, int64_t update_freq,
                                     int dtype, int state_dtype, int max_blocks, void* stream) {
  EmaRule rule;
  if (int rc = ema_rule("ema_segments_step", state, segments, step, sched, decay, start_update, update_freq, dtype, state_dtype, max_blocks, &rule)) return rc;
  OFA_REQUIRE(n >= 0 && n <= 65535 && state_numel >= 0 && max_len >= 0 && !((uintptr_t)segments & 7), OFA_ERR_INVALID,
              "ema_segments_step: at most 65535 segments in an 8-byte aligned table (n=%lld)", (long long)n);
  if (n == 0 || max_len == 0) return 0;
  const int64_t nbl = (max_len + 255) / 256;
  const int64_t cap = max_blocks > 0 ? max_blocks : 64;
  const int nb = (int)(nbl > cap ? cap : nbl);
  hipStream_t st = (hipStream_t)stream;
  const EmaSegment* segs = (const EmaSegment*)segments;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (state_dtype == OFA_F32) hipLaunchKernelGGL((ema_segments_kernel<T, float>), dim3(nb, (unsigned)n), dim3(256), 0, st, (float*)state, segs, (T*)shadow, state_numel, step, sched, rule);
    else hipLaunchKernelGGL((ema_segments_kernel<T, T>), dim3(nb, (unsigned)n), dim3(256), 0, st, (T*)state, segs, (T*)shadow, state_numel, step, sched, rule);
  });
  return check_launch("ema_segments_step");
}

// One micro-batch's contribution to the step statistics [sample_size, loss_sum, ntokens] (engine/trainer.py:842-860: the criterion's
// logging outputs summed over the micro-batches of an update): the count of non-pad targets, the loss sum (a device scalar) and the
// count again, in ONE single-block launch -- was target.ne(pad).sum() plus three read-modify-writes of a fp64 element, nine launches.
__global__ __launch_bounds__(256) void step_stats_add_kernel(double* __restrict__ stats, const float* __restrict__ loss,
                                                             const int64_t* __restrict__ target, int64_t n, int64_t pad) {
  __shared__ int red[4];
  int cnt = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) cnt += target[i] != pad;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double c = (double)(red[0] + red[1] + red[2] + red[3]);
    stats[0] += c;
    stats[1] += (double)loss[0];
    stats[2] += c;
  }
}

extern "C" int ofa_step_stats_add(double* stats, const float* loss, const int64_t* target, int64_t n, int64_t pad, void* stream) {
  OFA_REQUIRE(stats && loss && (target || n == 0) && n >= 0, OFA_ERR_INVALID, "step_stats_add: bad argument");
  hipLaunchKernelGGL(step_stats_add_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, loss, target, n, pad);
  return check_launch("step_stats_add");
}

extern "C" int ofa_step_schedule_scaled(const float* gsq, const double* sample_size, double* step, const double* lr, float* sched,
                                        float* gnorm, double* loss_scaler, float clip_norm, double beta1, double beta2,
                                        double scale_factor, double scale_window, double tolerance, double threshold,
                                        double min_loss_scale, void* stream) {
  OFA_REQUIRE(gsq && sample_size && step && lr && sched && gnorm && loss_scaler, OFA_ERR_INVALID, "step_schedule_scaled: null pointer");
  OFA_REQUIRE(scale_factor > 1.0 && scale_window >= 1.0 && tolerance >= 0.0 && min_loss_scale >= 0.0, OFA_ERR_INVALID,
              "step_schedule_scaled: bad scaler configuration");
  hipLaunchKernelGGL(step_schedule_scaled_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gsq, sample_size, step, lr, sched, gnorm,
                     loss_scaler, clip_norm, beta1, beta2, scale_factor, scale_window, tolerance, threshold, min_loss_scale);
  return check_launch("step_schedule_scaled");
}

extern "C" int ofa_step_schedule(const float* gsq, const double* sample_size, double* step, const double* lr, float* sched,
                                 float* gnorm, float clip_norm, double beta1, double beta2, void* stream) {
  OFA_REQUIRE(gsq && sample_size && step && lr && sched && gnorm, OFA_ERR_INVALID, "step_schedule: null pointer");
  hipLaunchKernelGGL(step_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gsq, sample_size, step, lr, sched, gnorm,
                     clip_norm, beta1, beta2);
  return check_launch("step_schedule");
}

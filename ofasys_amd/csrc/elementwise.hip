// HBM-bound pieces of the layer for gfx950: 16-byte vector loads, grid-stride loops, wave64 ballots.
//   GELU fwd/bwd            module/gelu.py:18-19 (exact erf, fp32 math)
//   dropout(x) + residual   transformer_layer.py:181-182, 203-206 (Philox4x32-10 counter RNG, mask never stored)
//   embedding gather        adaptor/text.py:124-125, module/layer.py:8-15
//   embedding grad          dense scatter-add, deterministic: one wave per vocabulary row scans the ids with ballots
//   add + row-vector + row mask   adaptor/base.py:168-173, model/transformer.py:110-112
//   im2col of p x p patches  adaptor/image_patch_embed.py:59-73
#include "common.h"

namespace ofa {

// v rounded to the storage type T and read back (the value a store of v followed by a load hands on)
template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to<bf16_t>(float v) { return bf2f(f2bf(v)); }
template <> __device__ __forceinline__ float round_to<f16_t>(float v) { return (float)(f16_t)v; }

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ y,
                                                   int64_t nvec, int64_t n) {
  constexpr int N = Vec<T>::N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float a[N], g[N], o[N];
    load_vec<T>(x + v * N, a);
    if (BWD) load_vec<T>(dy + v * N, g);
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = BWD ? g[j] * gelu_grad_f(a[j]) : gelu_f(a[j]);
    store_vec<T>(y + v * N, o);
  }
  // tail (n not a multiple of the vector width)
  if (blockIdx.x == 0) {
    for (int64_t e = nvec * N + threadIdx.x; e < n; e += 256) {
      const float a = ld1<T>(x + e);
      st1<T>(y + e, BWD ? ld1<T>(dy + e) * gelu_grad_f(a) : gelu_f(a));
    }
  }
}

// element e uses Philox counter (offset + e/8), halfword e%8 (philox_keep in common.h).
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                      int64_t n, float p, uint64_t seed, uint64_t offset,
                                                      const int64_t* __restrict__ offset_base) {
  if (offset_base) offset += (uint64_t)offset_base[0];   // device-resident stream position (hipGraph replays advance it)
  const Philox rng(seed);
  const float keep_scale = 1.0f / (1.0f - p);
  const uint32_t thresh = philox_thresh(p);
  const int64_t nq = (n + 7) / 8;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    const uint4 r = rng(offset + (uint64_t)q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t e = q * 8 + j;
      if (e < n) {
        float v = philox_keep(r, j, thresh) ? ld1<T>(x + e) * keep_scale : 0.f;
        if (ADD) v += ld1<T>(res + e);
        st1<T>(y + e, v);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void add_rowvec_mask_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                              const T* __restrict__ vec, const uint8_t* __restrict__ rowmask,
                                                              T* __restrict__ y, int64_t rows, int cols, int64_t b_period) {
  constexpr int N = Vec<T>::N;
  const int vpr = cols / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    float x[N], t[N];
    load_vec<T>(a + r * cols + c, x);
    if (b) {
      load_vec<T>(b + (b_period ? r % b_period : r) * cols + c, t);     // b_period rows of b serve every sample (shared positions)
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] += t[j];
    }
    if (vec) {
      load_vec<T>(vec + c, t);
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] += t[j];
    }
    if (rowmask && rowmask[r]) {
#pragma unroll
      for (int j = 0; j < N; ++j) x[j] = 0.f;
    }
    store_vec<T>(y + r * cols + c, x);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void embedding_fwd_kernel(const T* __restrict__ w, const int64_t* __restrict__ ids,
                                                            T* __restrict__ out, int64_t n, int D, int64_t V,
                                                            uint8_t* __restrict__ is_pad, int64_t pad_id) {
  constexpr int N = Vec<T>::N;
  const int vpr = D / N;
  const int64_t total = n * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    int64_t id = ids[r];
    if (is_pad && c == 0) is_pad[r] = id == pad_id;         // the padding mask of the same ids (adaptor/text.py:108-111), one byte per row
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    *reinterpret_cast<typename Vec<T>::type*>(out + r * D + c) =
        *reinterpret_cast<const typename Vec<T>::type*>(w + id * D + c);
  }
}

// out[r] = index[r] >= 0 ? src[index[r]] : 0   -- the pack / unpack step of the ragged row layout (ofasys_amd/packing.py): the
// forward gathers the non-pad rows of the padded [B*T, D] adaptor output, the backward is the same kernel with the inverse index
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ src, const int64_t* __restrict__ index,
                                                          T* __restrict__ out, int64_t n, int D, int64_t src_rows) {
  constexpr int N = Vec<T>::N;
  const int vpr = D / N;
  const int64_t total = n * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    const int64_t id = index[r];
    typename Vec<T>::type val = {};
    if (id >= 0 && id < src_rows) val = *reinterpret_cast<const typename Vec<T>::type*>(src + id * D + c);
    *reinterpret_cast<typename Vec<T>::type*>(out + r * D + c) = val;
  }
}

// The same gather over the VIRTUAL concatenation of up to 8 slot outputs along the sequence (adaptor/general.py:245-282 `torch.cat(.., dim=1)`):
// index[r] names a position b * T + t of the concatenated [B, T, D]; slot k holds the positions start[k] <= t < start[k+1] of every sample as
// its own contiguous [B, n_k, D].  The packed rows are gathered straight from the slots' outputs: the concatenated tensor is never built.
struct GatherParts { const void* src[8]; int start[9]; int n; };
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_parts_kernel(GatherParts gp, const int64_t* __restrict__ index, T* __restrict__ out,
                                                                int64_t n, int D, int Ttot, int64_t batch) {
  constexpr int N = Vec<T>::N;
  const int vpr = D / N;
  const int64_t total = n * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    const int64_t id = index[r];
    typename Vec<T>::type val = {};
    if (id >= 0 && id < batch * Ttot) {
      const int64_t b = id / Ttot;
      const int t = (int)(id - b * Ttot);
      int k = 0;
#pragma unroll
      for (int q = 1; q < 8; ++q)
        if (q < gp.n && t >= gp.start[q]) k = q;
      const int nk = gp.start[k + 1] - gp.start[k];
      val = *reinterpret_cast<const typename Vec<T>::type*>((const T*)gp.src[k] + ((b * nk + (t - gp.start[k])) * D + c));
    }
    *reinterpret_cast<typename Vec<T>::type*>(out + r * D + c) = val;
  }
}

// ... and its backward for ONE slot: out[b * nk + j] = inverse[b * T + start + j] >= 0 ? src[inverse[..]] : 0  (src: the packed-row gradient)
template <typename T>
__global__ __launch_bounds__(256) void scatter_rows_part_kernel(const T* __restrict__ src, const int64_t* __restrict__ inverse,
                                                                T* __restrict__ out, int64_t batch, int nk, int Ttot, int start, int D,
                                                                int64_t src_rows) {
  constexpr int N = Vec<T>::N;
  const int vpr = D / N;
  const int64_t total = batch * nk * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    const int64_t b = r / nk;
    const int j = (int)(r - b * nk);
    const int64_t id = inverse[b * Ttot + start + j];
    typename Vec<T>::type val = {};
    if (id >= 0 && id < src_rows) val = *reinterpret_cast<const typename Vec<T>::type*>(src + id * D + c);
    *reinterpret_cast<typename Vec<T>::type*>(out + r * D + c) = val;
  }
}

// narrow tables (rel-pos bias tables are [n_rel, heads], heads = 4..16): element-wise gather
template <typename T>
__global__ __launch_bounds__(256) void embedding_fwd_scalar_kernel(const T* __restrict__ w, const int64_t* __restrict__ ids,
                                                                   T* __restrict__ out, int64_t n, int D, int64_t V) {
  const int64_t total = n * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / D;
    const int c = (int)(e % D);
    int64_t id = ids[r];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    out[e] = w[id * D + c];
  }
}

__global__ __launch_bounds__(256) void embedding_mark_kernel(const int64_t* __restrict__ ids, uint8_t* __restrict__ present,
                                                             int64_t n, int64_t V) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t id = ids[i];
    if (id >= 0 && id < V) present[id] = 1;     // benign race: every writer stores the same value
  }
}

// dweight[v] += sum_{i : ids[i]==v} dout[i], deterministic, no atomics.  Wave (v, s) sweeps slice s of the id list 64 ids
// at a time, ballots the matches and adds the matching rows (16-byte loads) in increasing position order.  Big tables
// (vocabulary: few hits per row) use one slice and add straight into dweight; small tables (positions, token types:
// thousands of hits per row, which one wave would walk serially) are cut into S slices whose fp32 partial rows are
// folded in slice order by embedding_fold_kernel.  Rows that do not occur are skipped through a presence byte.
template <typename T, int NV>
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                            T* __restrict__ dw, float* __restrict__ part, int64_t n, int D,
                                                            int64_t V, int64_t padding_idx,
                                                            const uint8_t* __restrict__ present, int S) {
  constexpr int N = Vec<T>::N;
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int sl = blockIdx.y;
  if (v >= V || v == padding_idx) return;
  if (present && !present[v]) return;      // most vocabulary rows do not occur in a batch: skip their scan
  float acc[NV][N];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) acc[i][j] = 0.f;
  const int64_t per = ((n + S - 1) / S + 63) / 64 * 64;
  const int64_t lo = sl * per, hi = lo + per < n ? lo + per : n;
  bool any = false;
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t idx = base + lane;
    const bool hit = idx < hi && ids[idx] == v;
    unsigned long long m = __ballot(hit);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      any = true;
      const T* row = dout + (base + src) * D;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * N;
        if (c < D) {
          float x[N];
          load_vec<T>(row + c, x);
#pragma unroll
          for (int j = 0; j < N; ++j) acc[i][j] += x[j];
        }
      }
    }
  }
  if (S == 1) {
    if (!any) return;
    T* wr = dw + v * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * N;
      if (c < D) {
        float o[N];
        load_vec<T>(wr + c, o);
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] += acc[i][j];
        store_vec<T>(wr + c, o);
      }
    }
  } else {                                 // (zeros too: the fold reads every slice of a present row)
    float* pr = part + ((int64_t)sl * V + v) * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * N;
      if (c < D)
#pragma unroll
        for (int j = 0; j < N; ++j) pr[c + j] = acc[i][j];
    }
  }
}

// narrow / unaligned tables (rel-pos bias tables are [n_rel, heads]): element-wise variant of the same sweep
template <typename T>
__global__ __launch_bounds__(256) void embedding_bwd_scalar_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                                   T* __restrict__ dw, float* __restrict__ part, int64_t n,
                                                                   int D, int64_t V, int64_t padding_idx,
                                                                   const uint8_t* __restrict__ present, int S) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int sl = blockIdx.y;
  if (v >= V || v == padding_idx) return;
  if (present && !present[v]) return;
  constexpr int MAXC = 32;                 // columns per lane held in registers: D <= 2048
  float acc[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) acc[j] = 0.f;
  const int64_t per = ((n + S - 1) / S + 63) / 64 * 64;
  const int64_t lo = sl * per, hi = lo + per < n ? lo + per : n;
  bool any = false;
  for (int64_t base = lo; base < hi; base += 64) {
    const int64_t idx = base + lane;
    const bool hit = idx < hi && ids[idx] == v;
    unsigned long long m = __ballot(hit);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      any = true;
      const T* row = dout + (base + src) * D;
#pragma unroll
      for (int j = 0; j < MAXC; ++j) {
        const int c = j * 64 + lane;
        if (c < D) acc[j] += ld1<T>(row + c);
      }
    }
  }
  if (S == 1 && !any) return;
#pragma unroll
  for (int j = 0; j < MAXC; ++j) {
    const int c = j * 64 + lane;
    if (c < D) {
      if (S == 1) st1<T>(dw + v * D + c, ld1<T>(dw + v * D + c) + acc[j]);
      else part[((int64_t)sl * V + v) * D + c] = acc[j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void embedding_fold_kernel(const float* __restrict__ part, T* __restrict__ dw, int D,
                                                             int64_t V, int64_t padding_idx,
                                                             const uint8_t* __restrict__ present, int S) {
  const int64_t v = blockIdx.x;
  if (v == padding_idx || (present && !present[v])) return;
  for (int c = threadIdx.x; c < D; c += 256) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += part[((int64_t)s * V + v) * D + c];
    st1<T>(dw + v * D + c, ld1<T>(dw + v * D + c) + a);
  }
}

// The same scatter-add ID-MAJOR, for id lists that fit the LDS (the token table: V = 51265 rows, a few thousand ids -- the V-sized grid
// above spends its time on waves that read a presence byte and leave, behind a memset, a mark pass and their launches).  Every block
// stages the ids once as int32 (-1: out of range or the padding id); one wave per POSITION: the first position that holds an id owns
// it, every other wave leaves after the look-back.  The owner walks the list from its own position on, 64 ids per ballot, and queues
// the matching positions (in order) in LDS; the queue is drained G rows at a time -- G row loads in flight, then the additions in
// increasing position order (an id every sample holds, like <bos>, is otherwise one exposed memory latency per sample) -- with SLICED in
// the slices embedding_bwd_kernel would cut (`per` ids each, partial sums folded in slice order).  Then the one read-modify-write of
// dw[v]: bit for bit what the table-row-major kernels give.
constexpr int EMB_IDS_WAVES = 8;
template <typename T, int NV, bool SLICED>
__global__ __launch_bounds__(EMB_IDS_WAVES * 64) void embedding_bwd_ids_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                                               T* __restrict__ dw, int n, int D, int64_t V,
                                                                               int64_t padding_idx, int per) {
  constexpr int N = Vec<T>::N;
  constexpr int G = NV <= 1 ? 8 : 4;                             // rows in flight per drain step (registers: two blocks per CU)
  typedef typename Vec<T>::type raw_t;
  extern __shared__ int sid[];                                   // (n rounded up to 64) ids, then 64 queue entries per wave
  const int npad = (n + 63) & ~63;
  for (int i = threadIdx.x; i < npad; i += EMB_IDS_WAVES * 64) {
    const int64_t id = i < n ? ids[i] : -1;
    sid[i] = (id >= 0 && id < V && id != padding_idx) ? (int)id : -1;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int* queue = sid + npad + (threadIdx.x >> 6) * 64;
  for (int pos = blockIdx.x * EMB_IDS_WAVES + (threadIdx.x >> 6); pos < n; pos += gridDim.x * EMB_IDS_WAVES) {      // (wave-uniform)
    const int v = sid[pos];
    if (v < 0) continue;
    const int base0 = pos & ~63;
    bool earlier = false;                                        // does an earlier position hold v?  (no exit inside: the reads pipeline)
    for (int base = 0; base <= base0; base += 64) earlier |= (base + lane < pos) && sid[base + lane] == v;
    if (__ballot(earlier)) continue;
    float acc[NV][N], tot[SLICED ? NV : 1][N];                   // the current slice's sum / the folded slices
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) acc[i][j] = 0.f;
#pragma unroll
    for (int i = 0; i < (SLICED ? NV : 1); ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) tot[i][j] = 0.f;
    int cnt = 0;                                                 // queued positions (wave-uniform)
    auto drain = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the queue entries other lanes of this wave wrote
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int k = 0; k < cnt; k += G) {
        raw_t raw[G][NV];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const T* row = dout + (int64_t)queue[k + g < cnt ? k + g : cnt - 1] * D;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int c = (i * 64 + lane) * N;
            if (c < D) raw[g][i] = *reinterpret_cast<const raw_t*>(row + c);
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (k + g < cnt) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
              if ((i * 64 + lane) * N < D) {
                float x[N];
                unpack16<T>(__builtin_bit_cast(uint4, raw[g][i]), x);
#pragma unroll
                for (int j = 0; j < N; ++j) acc[i][j] += x[j];
              }
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();                           // (the reads above before the next entries are written)
      cnt = 0;
    };
    auto push = [&](unsigned long long m, int base) {            // (positions before `pos` in the first chunk cannot match)
      if (!m) return;
      const int c = __popcll(m);
      if (cnt + c > 64) drain();
      if ((m >> lane) & 1) queue[cnt + __popcll(m & ((1ull << lane) - 1))] = base + lane;
      cnt += c;
    };
    int base = base0;
    if (!SLICED) {
      for (; base + 256 <= npad; base += 256) {                  // four LDS reads in flight per trip
        const int a0 = sid[base + lane], a1 = sid[base + 64 + lane], a2 = sid[base + 128 + lane], a3 = sid[base + 192 + lane];
        const unsigned long long m0 = __ballot(a0 == v), m1 = __ballot(a1 == v), m2 = __ballot(a2 == v), m3 = __ballot(a3 == v);
        if (m0 | m1 | m2 | m3) {
          push(m0, base);
          push(m1, base + 64);
          push(m2, base + 128);
          push(m3, base + 192);
        }
      }
    }
    for (; base < npad; base += 64) {
      if (SLICED && base > base0 && base % per == 0) {           // a slice ends: fold its partial sum, start the next from zero
        drain();
#pragma unroll
        for (int i = 0; i < NV; ++i)
#pragma unroll
          for (int j = 0; j < N; ++j) { tot[SLICED ? i : 0][j] += acc[i][j]; acc[i][j] = 0.f; }
      }
      push(__ballot(sid[base + lane] == v), base);
    }
    drain();
    T* wr = dw + (int64_t)v * D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * N;
      if (c < D) {
        float o[N];
        load_vec<T>(wr + c, o);
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] += SLICED ? tot[SLICED ? i : 0][j] + acc[i][j] : acc[i][j];
        store_vec<T>(wr + c, o);
      }
    }
  }
}

// Lookup by a contiguous id range r0 .. r0 + T - 1 (position tables read with arange(T)): the gradient needs no scatter.
// dw[r0 + t] += round_T(sum_b dout[b][t]) -- the batch sum accumulated in fp32 in batch order and rounded to the storage type (what
// batch_sum_kernel hands on), then the one fp32 add per table element the row-major kernels do (0 + x first, as their accumulators do).
template <typename T>
__global__ __launch_bounds__(256) void embedding_range_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dw, int batch, int64_t n) {
  constexpr int N = Vec<T>::N;
  const int64_t total = n / N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    float acc[N], t[N], o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
#pragma unroll 8
    for (int b = 0; b < batch; ++b) {
      load_vec<T>(dout + (int64_t)b * n + v * N, t);
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += t[j];
    }
    load_vec<T>(dw + v * N, o);
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] += 0.f + round_to<T>(acc[j]);
    store_vec<T>(dw + v * N, o);
  }
}

// col[(b*(lead + nph*npw) + lead + ph*npw + pw)][c*p*p + i*p + j] = img[b][c][ph*p+i][pw*p+j]; columns K..Kpad-1 are zero, and so are the
// `lead` rows in front of every sample's patches (the class-token position of adaptor/image_patch_embed.py:71-73: the projection GEMM then
// runs over the [B, 1 + N, D] rows the adaptor returns -- no concatenation -- and the weight-gradient GEMM over the same rows sees zeros there)
template <typename T>
__global__ __launch_bounds__(256) void im2col_patch_kernel(const T* __restrict__ img, T* __restrict__ col, int B, int C, int H,
                                                           int W, int p, int Kpad, int lead) {
  const int nph = H / p, npw = W / p, K = C * p * p;
  const int64_t per = (int64_t)lead + (int64_t)nph * npw;
  const int64_t total = (int64_t)B * per * Kpad;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int k = (int)(e % Kpad);
    const int64_t r = e / Kpad;
    const int64_t b = r / per, rs = r % per - lead;
    float v = 0.f;
    if (k < K && rs >= 0) {
      const int j = k % p, i = (k / p) % p, c = k / (p * p);
      const int pw = (int)(rs % npw), ph = (int)(rs / npw);
      v = ld1<T>(img + ((b * C + c) * H + ph * p + i) * W + pw * p + j);
    }
    st1<T>(col + e, v);
  }
}
// The same matrix for 16-bit types and even p, moved in runs: a patch row is p contiguous pixels of the image -- 2p bytes that start and
// end on a dword boundary in both the image (W is a multiple of p) and the column row (c*p*p + i*p is even) -- so a dword never straddles
// two runs.  One thread writes 16 bytes of a column row (Kpad % 8 == 0) from four dword loads, walking (c, i, j) by increments: five
// 32-bit divisions per 8 elements instead of nine 64-bit ones per element.
template <typename T>
__global__ __launch_bounds__(256) void im2col_patch_runs_kernel(const T* __restrict__ img, T* __restrict__ col, int B, int C, int H,
                                                                int W, int p, int Kpad, int lead) {
  static_assert(sizeof(T) == 2, "dword runs of 16-bit elements");
  const int nph = H / p, npw = W / p, K = C * p * p, vpr = Kpad / 8;
  const int per = lead + nph * npw;
  const unsigned total = (unsigned)B * per * vpr;              // (the host checks that it fits)
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(img);
  for (unsigned v = blockIdx.x * 256 + threadIdx.x; v < total; v += gridDim.x * 256) {
    const unsigned r = v / vpr;
    const int k0 = (int)(v - r * vpr) * 8;
    const int b = (int)(r / per), rs = (int)(r - (unsigned)b * per) - lead;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (rs >= 0 && k0 < K) {
      const int ph = rs / npw, pw = rs - ph * npw;
      int c = k0 / (p * p);
      int i = (k0 - c * p * p) / p;
      int j = k0 - c * p * p - i * p;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (k0 + 2 * q < K) w[q] = src[((((int64_t)b * C + c) * H + ph * p + i) * W + pw * p + j) >> 1];
        j += 2;
        if (j >= p) { j = 0; if (++i >= p) { i = 0; ++c; } }
      }
    }
    *reinterpret_cast<uint4*>(col + (int64_t)v * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// column sums of a [rows, cols] matrix (bias gradients): 32 column-vectors x 8 row-lanes per block, grid.y row groups,
// fp32 partials [grid.y][cols] folded by a second pass (deterministic).
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, float* __restrict__ partial,
                                                             int64_t rows, int cols, int64_t ld) {
  constexpr int N = Vec<T>::N;
  __shared__ float red[8][32][N];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cx) * N;
  float acc[N];
#pragma unroll
  for (int j = 0; j < N; ++j) acc[j] = 0.f;
  if (c < cols) {
    for (int64_t r = (int64_t)blockIdx.y * 8 + ry; r < rows; r += (int64_t)gridDim.y * 8) {
      float v[N];
      load_vec<T>(x + r * ld + c, v);
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) red[ry][cx][j] = acc[j];
  __syncthreads();
  if (ry == 0 && c < cols) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) t += red[r][cx][j];
      partial[(int64_t)blockIdx.y * cols + c + j] = t;
    }
  }
}
template <typename TO>
__global__ __launch_bounds__(1024) void colsum_final_kernel(const float* __restrict__ partial, TO* __restrict__ out,
                                                            int cols, int groups, float alpha, int accumulate) {
  __shared__ float sm[16][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  float s = 0.f;
  if (c < cols)
    for (int g = ry; g < groups; g += 16) s += partial[(int64_t)g * cols + c];
  sm[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += sm[r][cx];
    t *= alpha;
    if (accumulate) t += ld1<TO>(out + c);
    st1<TO>(out + c, t);
  }
}

static inline int grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace ofa
using namespace ofa;

#define OFA_DT_CHECK(name) OFA_REQUIRE(OFA_DT_OK(dtype), OFA_ERR_INVALID, name ": bad dtype %d", dtype)

extern "C" int ofa_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream) {
  OFA_DT_CHECK("gelu_fwd");
  OFA_REQUIRE(n >= 0 && (n == 0 || (x && y)), OFA_ERR_INVALID, "gelu_fwd: bad argument");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((gelu_kernel<T, false>), dim3(grid_for(n / Vec<T>::N)), dim3(256), 0, st, (const T*)nullptr, (const T*)x,
                       (T*)y, n / Vec<T>::N, n);
  });
  return check_launch("gelu_fwd");
}

extern "C" int ofa_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, void* stream) {
  OFA_DT_CHECK("gelu_bwd");
  OFA_REQUIRE(n >= 0 && (n == 0 || (dy && x && dx)), OFA_ERR_INVALID, "gelu_bwd: bad argument");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((gelu_kernel<T, true>), dim3(grid_for(n / Vec<T>::N)), dim3(256), 0, st, (const T*)dy, (const T*)x,
                       (T*)dx, n / Vec<T>::N, n);
  });
  return check_launch("gelu_bwd");
}

extern "C" int ofa_dropout_add_fwd(const void* x, const void* residual, void* y, int64_t n, float p, uint64_t seed,
                                   uint64_t offset, const int64_t* offset_base, int dtype, void* stream) {
  OFA_DT_CHECK("dropout_add_fwd");
  OFA_REQUIRE(n >= 0 && p >= 0.f && p < 1.f && (n == 0 || (x && y)), OFA_ERR_INVALID, "dropout_add_fwd: bad argument");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(grid_for((n + 7) / 8)), block(256);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (residual) hipLaunchKernelGGL((dropout_kernel<T, true>), grid, block, 0, st, (const T*)x, (const T*)residual, (T*)y, n, p, seed, offset, offset_base);
    else hipLaunchKernelGGL((dropout_kernel<T, false>), grid, block, 0, st, (const T*)x, (const T*)nullptr, (T*)y, n, p, seed, offset, offset_base);
  });
  return check_launch("dropout_add_fwd");
}

extern "C" int ofa_dropout_bwd(const void* dy, void* dx, int64_t n, float p, uint64_t seed, uint64_t offset,
                               const int64_t* offset_base, int dtype, void* stream) {
  return ofa_dropout_add_fwd(dy, nullptr, dx, n, p, seed, offset, offset_base, dtype, stream);
}

extern "C" int ofa_add_rowvec_mask(const void* a, const void* b, const void* vec, const uint8_t* rowmask, void* y,
                                   int64_t rows, int cols, int64_t b_period, int dtype, void* stream) {
  OFA_DT_CHECK("add_rowvec_mask");
  OFA_REQUIRE(rows >= 0 && cols > 0 && a && y && b_period >= 0, OFA_ERR_INVALID, "add_rowvec_mask: bad argument");
  OFA_REQUIRE(cols % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "add_rowvec_mask: cols=%d not vectorizable", cols);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((add_rowvec_mask_kernel<T>), dim3(grid_for(rows * cols / Vec<T>::N)), dim3(256), 0, st, (const T*)a,
                       (const T*)b, (const T*)vec, rowmask, (T*)y, rows, cols, b_period);
  });
  return check_launch("add_rowvec_mask");
}

extern "C" int ofa_embedding_fwd(const void* weight, const int64_t* ids, void* out, int64_t n, int D, int64_t V, uint8_t* is_pad,
                                 int64_t pad_id, int dtype, void* stream) {
  OFA_DT_CHECK("embedding_fwd");
  OFA_REQUIRE(!is_pad || D % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "embedding_fwd: the pad mask rides with the vector kernel (D = %d)", D);
  OFA_REQUIRE(n >= 0 && D > 0 && V > 0 && weight && ids && out, OFA_ERR_INVALID, "embedding_fwd: bad argument");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (D % dt_vecn(dtype) != 0) {
    dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((embedding_fwd_scalar_kernel<T>), dim3(grid_for(n * D)), dim3(256), 0, st, (const T*)weight, ids, (T*)out,
                         n, D, V);
    });
    return check_launch("embedding_fwd_scalar");
  }
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((embedding_fwd_kernel<T>), dim3(grid_for(n * D / Vec<T>::N)), dim3(256), 0, st, (const T*)weight, ids,
                       (T*)out, n, D, V, is_pad, pad_id);
  });
  return check_launch("embedding_fwd");
}

extern "C" int ofa_gather_rows(const void* src, const int64_t* index, void* out, int64_t n, int D, int64_t src_rows, int dtype,
                               void* stream) {
  OFA_DT_CHECK("gather_rows");
  OFA_REQUIRE(n >= 0 && D > 0 && src_rows > 0 && src && index && out, OFA_ERR_INVALID, "gather_rows: bad argument");
  OFA_REQUIRE(D % dt_vecn(dtype) == 0, OFA_ERR_INVALID, "gather_rows: D=%d must be a multiple of the 16-byte vector width", D);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(grid_for(n * D / Vec<T>::N)), dim3(256), 0, st, (const T*)src, index, (T*)out,
                       n, D, src_rows);
  });
  return check_launch("gather_rows");
}

extern "C" int ofa_gather_rows_parts(const void* const* srcs, const int* lens, int nparts, const int64_t* index, void* out, int64_t n, int D,
                                     int64_t batch, int dtype, void* stream) {
  OFA_DT_CHECK("gather_rows_parts");
  OFA_REQUIRE(srcs && lens && index && out && nparts >= 1 && nparts <= 8 && n >= 0 && D > 0 && batch > 0, OFA_ERR_INVALID, "gather_rows_parts: bad argument");
  OFA_REQUIRE(D % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "gather_rows_parts: D=%d not vectorizable", D);
  if (n == 0) return 0;
  GatherParts gp;
  gp.n = nparts;
  gp.start[0] = 0;
  for (int k = 0; k < 8; ++k) {
    gp.src[k] = srcs[k < nparts ? k : 0];
    if (k < nparts) {
      OFA_REQUIRE(srcs[k] && lens[k] > 0 && !((uintptr_t)srcs[k] & 15), OFA_ERR_INVALID, "gather_rows_parts: part %d is NULL, empty or not 16-byte aligned", k);
      gp.start[k + 1] = gp.start[k] + lens[k];
    } else {
      gp.start[k + 1] = gp.start[k];
    }
  }
  const int Ttot = gp.start[nparts];
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((gather_rows_parts_kernel<T>), dim3(grid_for(n * D / Vec<T>::N)), dim3(256), 0, st, gp, index, (T*)out, n, D, Ttot, batch);
  });
  return check_launch("gather_rows_parts");
}

extern "C" int ofa_scatter_rows_part(const void* src, const int64_t* inverse, void* out, int64_t batch, int nk, int Ttot, int start, int D,
                                     int64_t src_rows, int dtype, void* stream) {
  OFA_DT_CHECK("scatter_rows_part");
  OFA_REQUIRE(src && inverse && out && batch > 0 && nk > 0 && start >= 0 && start + nk <= Ttot && D > 0 && src_rows > 0, OFA_ERR_INVALID,
              "scatter_rows_part: bad argument");
  OFA_REQUIRE(D % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "scatter_rows_part: D=%d not vectorizable", D);
  hipStream_t st = (hipStream_t)stream;
  const int64_t work = batch * nk * D / dt_vecn(dtype);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((scatter_rows_part_kernel<T>), dim3(grid_for(work)), dim3(256), 0, st, (const T*)src, inverse, (T*)out, batch, nk, Ttot, start, D, src_rows);
  });
  return check_launch("scatter_rows_part");
}

// Narrow-table scatter-add with a PRECOMPUTED segment plan: the ids of a rel-pos bias lookup (bucket[i][j], adaptor/text.py:101-104,
// image_resnet.py:116-128) are the same every step, a few hundred distinct values over 10^4..10^6 positions, so the positions are
// sorted by id once on the host side of the op (order / seg_off / seg_row, cached per lookup) and one wave sums one segment:
// 64 / CPL positions per trip x CPL columns (CPL = D rounded up to a power of two), fixed order, no atomics, no scan of the id list
// (embedding_bwd_scalar_kernel lets every table row sweep ALL ids: 47 us per [252 x 252] lookup, 0.85 ms per cfg-2b step).
template <typename T, int CPL>
__global__ __launch_bounds__(256) void segment_rowsum_kernel(const T* __restrict__ dout, const int* __restrict__ order,
                                                             const int* __restrict__ seg_off, const int* __restrict__ seg_row,
                                                             T* __restrict__ dw, int nseg, int D, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= nseg) return;
  constexpr int G = 64 / CPL;
  const int g = lane / CPL, c = lane % CPL;
  const int lo = seg_off[sg], hi = seg_off[sg + 1];
  float acc = 0.f;
  int p = lo + g;
  for (; p + 3 * G < hi; p += 4 * G) {                    // four dependent index -> row gathers in flight per lane
    const int64_t r0 = order[p], r1 = order[p + G], r2 = order[p + 2 * G], r3 = order[p + 3 * G];
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (c < D) {
      v0 = ld1<T>(dout + r0 * D + c);
      v1 = ld1<T>(dout + r1 * D + c);
      v2 = ld1<T>(dout + r2 * D + c);
      v3 = ld1<T>(dout + r3 * D + c);
    }
    acc += (v0 + v1) + (v2 + v3);
  }
  for (; p < hi; p += G) {
    const int64_t row = order[p];
    if (c < D) acc += ld1<T>(dout + row * D + c);
  }
#pragma unroll
  for (int off = CPL; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
  if (g == 0 && c < D) {
    T* o = dw + (int64_t)seg_row[sg] * D + c;
    st1<T>(o, (accumulate ? ld1<T>(o) : 0.f) + acc);
  }
}

// slices for a table of V rows of D columns (<= 64 slices)
extern "C" int ofa_embedding_bwd_slices(int64_t V, int D) {
  if (V <= 0 || D <= 0) return 1;
  const int64_t by_rows = 8192 / V;                 // wide tables: <= 8192 partial rows
  const int64_t by_bytes = ((int64_t)1 << 21) / (V * D);   // narrow ones (rel-pos tables [~7000, heads]): <= 8 MB of partials
  int64_t s = by_rows > by_bytes ? by_rows : by_bytes;
  return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

template <typename T>
static void launch_segment_rowsum(const void* dout, const int32_t* order, const int32_t* seg_off, const int32_t* seg_row, void* dw, int nseg,
                                  int D, int accumulate, hipStream_t st) {
  const dim3 grid(cdiv(nseg, 4)), block(256);
  if (D <= 8) hipLaunchKernelGGL((segment_rowsum_kernel<T, 8>), grid, block, 0, st, (const T*)dout, order, seg_off, seg_row, (T*)dw, nseg, D, accumulate);
  else if (D <= 16) hipLaunchKernelGGL((segment_rowsum_kernel<T, 16>), grid, block, 0, st, (const T*)dout, order, seg_off, seg_row, (T*)dw, nseg, D, accumulate);
  else if (D <= 32) hipLaunchKernelGGL((segment_rowsum_kernel<T, 32>), grid, block, 0, st, (const T*)dout, order, seg_off, seg_row, (T*)dw, nseg, D, accumulate);
  else hipLaunchKernelGGL((segment_rowsum_kernel<T, 64>), grid, block, 0, st, (const T*)dout, order, seg_off, seg_row, (T*)dw, nseg, D, accumulate);
}

extern "C" int ofa_segment_rowsum(const void* dout, const int32_t* order, const int32_t* seg_off, const int32_t* seg_row, void* dweight,
                                  int nseg, int D, int accumulate, int dtype, void* stream) {
  OFA_DT_CHECK("segment_rowsum");
  OFA_REQUIRE(dout && order && seg_off && seg_row && dweight && nseg >= 0 && D > 0 && D <= 64, OFA_ERR_INVALID,
              "segment_rowsum: bad argument (D = %d, at most 64 columns)", D);
  if (nseg == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    launch_segment_rowsum<typename decltype(tag)::type>(dout, order, seg_off, seg_row, dweight, nseg, D, accumulate, st);
  });
  return check_launch("segment_rowsum");
}

extern "C" int ofa_embedding_bwd(const void* dout, const int64_t* ids, void* dweight, int64_t n, int D, int64_t V,
                                 int64_t padding_idx, uint8_t* present_ws, float* slice_ws, int dtype, void* stream) {
  OFA_DT_CHECK("embedding_bwd");
  OFA_REQUIRE(n >= 0 && D > 0 && V > 0 && dout && ids && dweight, OFA_ERR_INVALID, "embedding_bwd: bad argument");
  const int vecn = dt_vecn(dtype);
  OFA_REQUIRE(D <= 2048, OFA_ERR_UNSUPPORTED, "embedding_bwd: D=%d exceeds 2048", D);
  const bool vec_ok = D % vecn == 0 && D <= 64 * vecn * 4 && (((uintptr_t)dout | (uintptr_t)dweight) & 15) == 0;
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (present_ws) {                                   // optional V-byte scratch: mark the rows that occur
    (void)hipMemsetAsync(present_ws, 0, (size_t)V, st);
    hipLaunchKernelGGL(embedding_mark_kernel, dim3(grid_for(n)), dim3(256), 0, st, ids, present_ws, n, V);
  }
  const int S = slice_ws ? ofa_embedding_bwd_slices(V, D) : 1;
  const int nv = cdiv(D, 64 * vecn);
  dim3 grid((unsigned)((V + 3) / 4), S), block(256);
#define EMB_LAUNCH(T, NV)                                                                                               \
  hipLaunchKernelGGL((embedding_bwd_kernel<T, NV>), grid, block, 0, st, (const T*)dout, ids, (T*)dweight, slice_ws, n, D, V, \
                     padding_idx, (const uint8_t*)present_ws, S)
  if (!vec_ok)
    dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((embedding_bwd_scalar_kernel<T>), grid, block, 0, st, (const T*)dout, ids, (T*)dweight, slice_ws, n, D, V,
                         padding_idx, (const uint8_t*)present_ws, S);
    });
  else
    dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (nv <= 1) EMB_LAUNCH(T, 1);
      else if (nv <= 2) EMB_LAUNCH(T, 2);
      else EMB_LAUNCH(T, 4);
    });
#undef EMB_LAUNCH
  int rc = check_launch("embedding_bwd");
  if (rc || S == 1) return rc;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((embedding_fold_kernel<T>), dim3((unsigned)V), dim3(256), 0, st, slice_ws, (T*)dweight, D, V, padding_idx,
                       (const uint8_t*)present_ws, S);
  });
  return check_launch("embedding_fold");
}

// debug builds: OFA_STEP_EDGES_OLD = a bit mask of OFA_EDGE_* items whose callers take the path they took before (A/B runs, the tests
// that compare the two); the product library has one path
extern "C" int ofa_step_edges_old(int item) {
#ifdef OFA_DEBUG_SWITCHES
  if (const char* e = getenv("OFA_STEP_EDGES_OLD")) return (atoi(e) >> item) & 1;
#endif
  return 0;
}

// debug builds: OFA_STEP_TAIL_OLD = a bit mask of OFA_TAIL_* items (the gradient plumbing around the optimizer) that run as they did
// before; the product library has one path
extern "C" int ofa_step_tail_old(int item) {
#ifdef OFA_DEBUG_SWITCHES
  if (const char* e = getenv("OFA_STEP_TAIL_OLD")) return (atoi(e) >> item) & 1;
#endif
  return 0;
}

extern "C" int ofa_embedding_bwd_ids_ok(int64_t n, int D, int64_t V, int dtype) {
  const int vecn = dt_vecn(dtype);
  return OFA_DT_OK(dtype) && n >= 0 && n <= OFA_EMBEDDING_IDS_MAX && V > 0 && V < ((int64_t)1 << 31) && D > 0 && D % vecn == 0 &&
         D <= 64 * vecn * 4;
}

extern "C" int ofa_embedding_bwd_ids(const void* dout, const int64_t* ids, void* dweight, int64_t n, int D, int64_t V,
                                     int64_t padding_idx, int slices, int dtype, void* stream) {
  OFA_DT_CHECK("embedding_bwd_ids");
  OFA_REQUIRE(n >= 0 && D > 0 && V > 0 && slices >= 1 && dout && ids && dweight, OFA_ERR_INVALID, "embedding_bwd_ids: bad argument");
  OFA_REQUIRE(ofa_embedding_bwd_ids_ok(n, D, V, dtype), OFA_ERR_UNSUPPORTED,
              "embedding_bwd_ids: n=%lld ids (at most %d), D=%d (whole 16-byte vectors, at most 256 of them): use ofa_embedding_bwd",
              (long long)n, OFA_EMBEDDING_IDS_MAX, D);
  OFA_REQUIRE((((uintptr_t)dout | (uintptr_t)dweight) & 15) == 0, OFA_ERR_UNSUPPORTED, "embedding_bwd_ids: buffers not 16-byte aligned");
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int vecn = dt_vecn(dtype);
  const int nv = cdiv(D, 64 * vecn);
  const int per = (int)(((n + slices - 1) / slices + 63) / 64 * 64);         // embedding_bwd_kernel's slice length
  const int blocks = cdiv(n, EMB_IDS_WAVES) < 1024 ? cdiv(n, EMB_IDS_WAVES) : 1024;      // a position per wave and sweep
  const size_t lds = (size_t)((n + 63) / 64 * 64 + EMB_IDS_WAVES * 64) * sizeof(int);
#define EMB_LAUNCH(T, NV, SL)                                                                                       \
  hipLaunchKernelGGL((embedding_bwd_ids_kernel<T, NV, SL>), dim3(blocks), dim3(EMB_IDS_WAVES * 64), lds, st, (const T*)dout, ids, \
                     (T*)dweight, (int)n, D, V, padding_idx, per)
  if (slices > 1)
    dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (nv <= 1) EMB_LAUNCH(T, 1, true);
      else if (nv <= 2) EMB_LAUNCH(T, 2, true);
      else EMB_LAUNCH(T, 4, true);
    });
  else
    dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (nv <= 1) EMB_LAUNCH(T, 1, false);
      else if (nv <= 2) EMB_LAUNCH(T, 2, false);
      else EMB_LAUNCH(T, 4, false);
    });
#undef EMB_LAUNCH
  return check_launch("embedding_bwd_ids");
}

extern "C" int ofa_embedding_range_bwd(const void* dout, void* dweight, int batch, int64_t T, int D, int64_t V, int64_t r0, int dtype,
                                       void* stream) {
  OFA_DT_CHECK("embedding_range_bwd");
  OFA_REQUIRE(dout && dweight && batch >= 1 && T >= 0 && D > 0 && V > 0 && r0 >= 0 && r0 + T <= V, OFA_ERR_INVALID,
              "embedding_range_bwd: bad argument (rows %lld .. %lld of %lld)", (long long)r0, (long long)(r0 + T), (long long)V);
  OFA_REQUIRE(D % dt_vecn(dtype) == 0 && (((uintptr_t)dout | (uintptr_t)dweight) & 15) == 0, OFA_ERR_UNSUPPORTED,
              "embedding_range_bwd: D=%d / buffers not whole 16-byte vectors: use ofa_embedding_bwd", D);
  if (T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = T * D;
  dispatch_dtype(dtype, [&](auto tag) {
    using TT = typename decltype(tag)::type;             // (T is the row count here)
    hipLaunchKernelGGL((embedding_range_bwd_kernel<TT>), dim3(grid_for(n / Vec<TT>::N)), dim3(256), 0, st, (const TT*)dout,
                       (TT*)dweight + r0 * D, batch, n);
  });
  return check_launch("embedding_range_bwd");
}

extern "C" int ofa_im2col_patch(const void* img, void* col, int B, int C, int H, int W, int p, int Kpad, int lead, int dtype,
                                void* stream) {
  OFA_DT_CHECK("im2col_patch");
  OFA_REQUIRE(img && col && B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0 && Kpad >= C * p * p && lead >= 0, OFA_ERR_INVALID,
              "im2col_patch: bad argument (H=%d W=%d p=%d Kpad=%d)", H, W, p, Kpad);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * (lead + (int64_t)(H / p) * (W / p)) * Kpad;
  if (total == 0) return 0;
  // 16-bit images with even p: whole runs as dwords (im2col_patch_runs_kernel); odd p, fp32, unaligned buffers: element by element
  if (dtype != OFA_F32 && p % 2 == 0 && Kpad % 8 == 0 && ((uintptr_t)img & 3) == 0 && ((uintptr_t)col & 15) == 0 &&
      total / 8 < ((int64_t)1 << 31) && !ofa_step_edges_old(OFA_EDGE_IM2COL)) {
    dispatch_dtype16(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((im2col_patch_runs_kernel<T>), dim3(grid_for(total / 8)), dim3(256), 0, st, (const T*)img, (T*)col, B, C,
                         H, W, p, Kpad, lead);
    });
    return check_launch("im2col_patch_runs");
  }
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((im2col_patch_kernel<T>), dim3(grid_for(total)), dim3(256), 0, st, (const T*)img, (T*)col, B, C, H, W, p,
                       Kpad, lead);
  });
  return check_launch("im2col_patch");
}

extern "C" int ofa_colsum_ws_floats(int cols) { return 128 * cols; }

extern "C" int ofa_colsum_slots(int64_t rows) {
  int64_t groups = (rows + 63) / 64;
  return (int)(groups < 1 ? 1 : (groups > 128 ? 128 : groups));
}

extern "C" int ofa_colsum(const void* x, void* out, float* ws, int64_t rows, int cols, int64_t ld, float alpha,
                          int accumulate, int dtype, int out_dtype, void* stream) {
  OFA_DT_CHECK("colsum");
  OFA_REQUIRE(OFA_DT_OK(out_dtype), OFA_ERR_INVALID, "colsum: bad out dtype %d", out_dtype);
  OFA_REQUIRE(rows >= 0 && cols > 0 && ld >= cols && x && (out || accumulate == OFA_DEFER_FOLD) && ws, OFA_ERR_INVALID,
              "colsum: bad argument");
  const int n = dt_vecn(dtype);
  OFA_REQUIRE(cols % n == 0 && ld % n == 0, OFA_ERR_UNSUPPORTED, "colsum: cols=%d / ld not vectorizable", cols);
  hipStream_t st = (hipStream_t)stream;
  const int groups = ofa_colsum_slots(rows);
  dim3 grid(cdiv(cols / n, 32), groups), block(256);
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((colsum_partial_kernel<T>), grid, block, 0, st, (const T*)x, ws, rows, cols, ld);
  });
  int rc = check_launch("colsum_partial");
  if (rc || accumulate == OFA_DEFER_FOLD) return rc;          // deferred: the caller folds ws (ofa_fold_batched)
  dispatch_dtype(out_dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((colsum_final_kernel<T>), dim3(cdiv(cols, 64)), dim3(1024), 0, st, (const float*)ws, (T*)out, cols, groups,
                       alpha, accumulate);
  });
  return check_launch("colsum_final");
}

// ---- y = a * b  (b same shape, or a row vector broadcast over rows)
namespace ofa {
template <typename T>
__global__ __launch_bounds__(256) void mul_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y,
                                                  int64_t rows, int cols, int b_rowvec) {
  constexpr int N = Vec<T>::N;
  const int vpr = cols / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    float x[N], t[N];
    load_vec<T>(a + r * cols + c, x);
    load_vec<T>(b_rowvec ? b + c : b + r * cols + c, t);
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] *= t[j];
    store_vec<T>(y + r * cols + c, x);
  }
}
// y[r, :] = x[r, :] * scale[r / group]   (DropPath: one keep/scale factor per sample = per group of T batch-major rows)
template <typename T>
__global__ __launch_bounds__(256) void scale_row_groups_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                               T* __restrict__ y, int64_t rows, int cols, int64_t group) {
  constexpr int N = Vec<T>::N;
  const int vpr = cols / N;
  const int64_t total = rows * vpr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t r = v / vpr;
    const int c = (int)(v % vpr) * N;
    const float s = scale[r / group];
    float a[N];
    load_vec<T>(x + r * cols + c, a);
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] *= s;
    store_vec<T>(y + r * cols + c, a);
  }
}
// out[0] = sum(x[0..n))   single block, deterministic
__global__ __launch_bounds__(256) void reduce_sum_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n) {
  __shared__ float sw[4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sw[0] + sw[1] + sw[2] + sw[3];
}
// out[h] = sum_b sum_t x[(b*heads + h)*ld + t], t < T     one block per head
__global__ __launch_bounds__(256) void head_sum_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int heads,
                                                       int T, int ld) {
  __shared__ float sw[4];
  const int h = blockIdx.x;
  float s = 0.f;
  for (int b = 0; b < B; ++b)
    for (int t = threadIdx.x; t < T; t += 256) s += x[((int64_t)b * heads + h) * ld + t];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[h] = sw[0] + sw[1] + sw[2] + sw[3];
}
// out[i] = sum_{k < n} in_k[i]   (fp32 accumulation, one rounding): the gradient of a tensor that n consumers read (ops.fan_out: the
// abs-position bias every layer of a stack assembles its attention bias from) in ONE launch instead of autograd's n - 1 pairwise adds
struct AddNArgs { const void* in[16]; int n; };
template <typename T>
__global__ __launch_bounds__(256) void add_n_kernel(AddNArgs a, T* __restrict__ out, int64_t numel) {
  constexpr int N = Vec<T>::N;
  const int64_t nvec = numel / N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (int k = 0; k < a.n; ++k) {
      float t[N];
      load_vec<T>((const T*)a.in[k] + v * N, t);
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += t[j];
    }
    store_vec<T>(out + v * N, acc);
  }
  if (blockIdx.x == 0) {                                   // the tail that is not a whole 16-byte vector
    for (int64_t i = nvec * N + threadIdx.x; i < numel; i += 256) {
      float t = 0.f;
      for (int k = 0; k < a.n; ++k) t += ld1<T>((const T*)a.in[k] + i);
      st1<T>(out + i, t);
    }
  }
}
}  // namespace ofa

extern "C" int ofa_add_n(const void* const* inputs, int n, void* out, int64_t numel, int dtype, void* stream) {
  OFA_DT_CHECK("add_n");
  OFA_REQUIRE(inputs && out && n >= 1 && n <= 16 && numel >= 0, OFA_ERR_INVALID, "add_n: 1..16 inputs (got %d)", n);
  if (numel == 0) return 0;
  AddNArgs a;
  for (int k = 0; k < 16; ++k) a.in[k] = inputs[k < n ? k : 0];
  for (int k = 0; k < n; ++k) OFA_REQUIRE(inputs[k] && !((uintptr_t)inputs[k] & 15), OFA_ERR_INVALID, "add_n: input %d is NULL or not 16-byte aligned", k);
  OFA_REQUIRE(!((uintptr_t)out & 15), OFA_ERR_INVALID, "add_n: out is not 16-byte aligned");
  a.n = n;
  hipStream_t st = (hipStream_t)stream;
  const int64_t work = numel / dt_vecn(dtype) + 1;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((add_n_kernel<T>), dim3(grid_for(work)), dim3(256), 0, st, a, (T*)out, numel);
  });
  return check_launch("add_n");
}

// out[i] (+)= sum_b x[b * n + i]: the gradient of a tensor every sample of the batch read (batch-invariant position embeddings)
template <typename T>
__global__ __launch_bounds__(256) void batch_sum_kernel(const T* __restrict__ x, T* __restrict__ out, int batch, int64_t n, int accumulate) {
  constexpr int N = Vec<T>::N;
  const int64_t total = n / N;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    float acc[N], t[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    if (accumulate) load_vec<T>(out + v * N, acc);
    for (int b = 0; b < batch; ++b) {
      load_vec<T>(x + (int64_t)b * n + v * N, t);
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] += t[j];
    }
    store_vec<T>(out + v * N, acc);
  }
}

extern "C" int ofa_batch_sum(const void* x, void* out, int batch, int64_t n, int accumulate, int dtype, void* stream) {
  OFA_DT_CHECK("batch_sum");
  OFA_REQUIRE(x && out && batch >= 1 && n >= 0, OFA_ERR_INVALID, "batch_sum: bad argument");
  OFA_REQUIRE(n % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "batch_sum: n=%lld not vectorizable", (long long)n);
  if (n == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((batch_sum_kernel<T>), dim3(grid_for(n / Vec<T>::N)), dim3(256), 0, st, (const T*)x, (T*)out, batch, n, accumulate);
  });
  return check_launch("batch_sum");
}

extern "C" int ofa_mul(const void* a, const void* b, void* y, int64_t rows, int cols, int b_rowvec, int dtype, void* stream) {
  OFA_DT_CHECK("mul");
  OFA_REQUIRE(rows >= 0 && cols > 0 && a && b && y, OFA_ERR_INVALID, "mul: bad argument");
  OFA_REQUIRE(cols % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "mul: cols=%d not vectorizable", cols);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((mul_kernel<T>), dim3(grid_for(rows * cols / Vec<T>::N)), dim3(256), 0, st, (const T*)a, (const T*)b, (T*)y, rows, cols, b_rowvec);
  });
  return check_launch("mul");
}

extern "C" int ofa_scale_row_groups(const void* x, const float* scale, void* y, int64_t rows, int cols, int64_t group, int dtype,
                                    void* stream) {
  OFA_DT_CHECK("scale_row_groups");
  OFA_REQUIRE(rows >= 0 && cols > 0 && group > 0 && x && scale && y, OFA_ERR_INVALID, "scale_row_groups: bad argument");
  OFA_REQUIRE(cols % dt_vecn(dtype) == 0, OFA_ERR_UNSUPPORTED, "scale_row_groups: cols=%d not vectorizable", cols);
  if (rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((scale_row_groups_kernel<T>), dim3(grid_for(rows * cols / Vec<T>::N)), dim3(256), 0, st, (const T*)x, scale, (T*)y, rows, cols, group);
  });
  return check_launch("scale_row_groups");
}

extern "C" int ofa_reduce_sum_f32(const float* x, float* out, int64_t n, void* stream) {
  OFA_REQUIRE(n >= 0 && out && (n == 0 || x), OFA_ERR_INVALID, "reduce_sum_f32: bad argument");
  hipLaunchKernelGGL(reduce_sum_f32_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, out, n);
  return check_launch("reduce_sum_f32");
}

extern "C" int ofa_head_sum_f32(const float* x, float* out, int B, int heads, int T, int ld, void* stream) {
  OFA_REQUIRE(x && out && B > 0 && heads > 0 && T > 0 && ld >= T, OFA_ERR_INVALID, "head_sum_f32: bad argument");
  hipLaunchKernelGGL(head_sum_kernel, dim3(heads), dim3(256), 0, (hipStream_t)stream, x, out, B, heads, T, ld);
  return check_launch("head_sum_f32");
}

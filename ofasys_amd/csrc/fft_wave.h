// The one-wave FFT that the audio kernels share (griffin_lim.hip, audio_features.hip): complex helpers, the wave-level LDS hand-over and the
// forward radix-2^2 transform of M = 2^LOGM complex points that one wave runs in its own LDS buffer.
#pragma once
#include "common.h"

namespace ofa {

__device__ __forceinline__ float2 gl_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 gl_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 gl_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 gl_mulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)

// what one wave wrote to its LDS buffer is what all of its lanes read next
__device__ __forceinline__ void gl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// In-place complex FFT of M = 2^LOGM points, natural order in, bit-reversed order out.  Stage h: (a, b) at distance h -> (a + b, (a - b) W_{2h}^j);
// W_{2h}^j = tw[j M / h].
template <int LOGM> __device__ __forceinline__ void gl_fft_forward(float2* z, const float2* tw, int lane) {
  constexpr int M = 1 << LOGM;
  int lh = LOGM - 1;
#pragma unroll
  for (; lh >= 1; lh -= 2) {                                    // stages h and h / 2
    const int h = 1 << lh, hh = h >> 1;
    for (int q = lane; q < M / 4; q += WAVE) {
      const int j = q & (hh - 1), i0 = ((q >> (lh - 1)) << (lh + 1)) + j;
      const float2 a0 = z[i0], a1 = z[i0 + hh], a2 = z[i0 + h], a3 = z[i0 + h + hh];
      const float2 b0 = gl_add(a0, a2), b2 = gl_mul(gl_sub(a0, a2), tw[j << (LOGM - lh)]);
      const float2 b1 = gl_add(a1, a3), b3 = gl_mul(gl_sub(a1, a3), tw[(j + hh) << (LOGM - lh)]);
      const float2 w2 = tw[j << (LOGM - lh + 1)];
      z[i0] = gl_add(b0, b1);
      z[i0 + hh] = gl_mul(gl_sub(b0, b1), w2);
      z[i0 + h] = gl_add(b2, b3);
      z[i0 + h + hh] = gl_mul(gl_sub(b2, b3), w2);
    }
    gl_wave_sync();
  }
  if (lh == 0) {                                                // LOGM odd: the last stage alone, h = 1
    for (int q = lane; q < M / 2; q += WAVE) {
      const float4 v = *reinterpret_cast<const float4*>(z + 2 * q);
      *reinterpret_cast<float4*>(z + 2 * q) = make_float4(v.x + v.z, v.y + v.w, v.x - v.z, v.y - v.w);
    }
    gl_wave_sync();
  }
}

}  // namespace ofa

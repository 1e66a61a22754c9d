// What every observer kernel (the three element sweeps of bt_q8_observe.hip; the fused forward's OBS form in bt_fused_fwd.h, launched
// by bt_fused_flipout_obs.hip) shares: a running (min, max) pair, the two float atomics and the workgroup merge; and what the sweeps
// share besides: the head / quads / tail walk over one fp32 run, and on the host their grid rule, alignment check and launch by draw source.
// Reduction: per thread, wavefront shuffles, one LDS step per workgroup, then at most ONE vector atomic per statistic and workgroup on
// the value's bit pattern (none when a plain load shows that the value would not widen the statistic). The bits of a non-negative float order like a signed integer's and those of a negative float in reverse like
// an unsigned integer's, so a float maximum is a signed-integer atomic max for v >= 0 and an unsigned-integer atomic min for v < 0
// (the minimum: the mirror image); -0 is made +0 first and non-finite values never reach the atomics (they are counted instead).
// Minimum and maximum have no order: the result does not depend on how the workgroups are scheduled. A pair starts at (+inf, -inf)
// and a call can only widen it.
#pragma once
#include "bt_api_internal.h"

namespace bt {

constexpr int kObsThreads = 256;
constexpr int kObsGrid = 2048;   // workgroups of a launch, at most (256 CUs x 8)

__device__ __forceinline__ bool obs_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

struct Range {
  float lo, hi;
  __device__ __forceinline__ void take(float v, unsigned& bad) {
    if (obs_finite(v)) {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    } else {
      ++bad;
    }
  }
};

template <int K>
__device__ __forceinline__ void obs_init(Range (&r)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) r[k].lo = INFINITY, r[k].hi = -INFINITY;
}

// A grid row's walk over one fp32 run x[0, n): one(i, x[i]) before the first 16-byte boundary, quad(i0, x[i0 .. i0 + 4)) on 16-byte loads, one() for the rest.
template <typename One, typename Quad>
__device__ __forceinline__ void obs_walk(const float* x, long long n, One one, Quad quad) {
  long long head = (long long)(((16u - (unsigned)(((uintptr_t)x) & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const long long nquad = (n - head) >> 2;
  const long long tail0 = head + 4 * nquad;
  const long long tid = (long long)blockIdx.x * kObsThreads + threadIdx.x, stride = (long long)gridDim.x * kObsThreads;
  const float4* const x4 = reinterpret_cast<const float4*>(x + head);
  for (long long g = tid; g < nquad; g += stride) {
    const float4 v = x4[g];   // (a value, not a reference into memory: ONE 16-byte load)
    quad(head + 4 * g, v);
  }
  if (tid < head) one(tid, x[tid]);                             // head < 4
  if (tid < n - tail0) one(tail0 + tid, x[tail0 + tid]);        // n - tail0 < 4
}

__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
  v = __fadd_rn(v, 0.0f);   // -0 -> +0
  if (v >= 0.0f)
    __hip_atomic_fetch_min(reinterpret_cast<int*>(addr), __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    __hip_atomic_fetch_max(reinterpret_cast<unsigned*>(addr), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
  v = __fadd_rn(v, 0.0f);
  if (v >= 0.0f)
    __hip_atomic_fetch_max(reinterpret_cast<int*>(addr), __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    __hip_atomic_fetch_min(reinterpret_cast<unsigned*>(addr), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The workgroup's ranges r[0 .. K) and its count of non-finite values -> dst[k] (a (min, max) pair each) and *nonfinite.
// NWAVES: the wavefronts of the workgroup (the sweeps' 256 threads: four); a wave with nothing to say brings (+inf, -inf) and 0.
// lds: NWAVES * (2 * K + 1) words. Every thread of the workgroup calls it (one workgroup barrier inside).
template <int K, int NWAVES = kObsThreads / 64>
__device__ __forceinline__ void obs_merge(Range (&r)[K], unsigned bad, float* const (&dst)[K], unsigned* nonfinite, float* lds) {
  constexpr int W = 2 * K + 1;
  static_assert(2 * K + 1 <= 64 * NWAVES, "one thread per statistic");
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      r[k].lo = fminf(r[k].lo, __shfl_xor(r[k].lo, o, 64));
      r[k].hi = fmaxf(r[k].hi, __shfl_xor(r[k].hi, o, 64));
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[wv * W + 2 * k] = r[k].lo, lds[wv * W + 2 * k + 1] = r[k].hi;
    lds[wv * W + 2 * K] = __uint_as_float(bad);
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * K) {
    const bool is_max = t & 1;
    float v = lds[t];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) v = is_max ? fmaxf(v, lds[w * W + t]) : fminf(v, lds[w * W + t]);
    // (still +-inf: the workgroup met no finite value.) A statistic only ever widens, so a value that does not widen what a plain
    // load sees -- however stale -- cannot widen the current one: most workgroups issue no atomic at all, and the ones that do are
    // not queued behind thousands of others on the same ten words.
    if (obs_finite(v)) {
      float* const p = dst[t >> 1] + (is_max ? 1 : 0);
      const float cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (is_max ? v > cur : v < cur) {
        if (is_max)
          atomic_max_f32(p, v);
        else
          atomic_min_f32(p, v);
      }
    }
  } else if (t == 2 * K) {
    unsigned b = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) b += __float_as_uint(lds[w * W + 2 * K]);
    if (b) __hip_atomic_fetch_add(nonfinite, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// A supplied sign as the observers (and the INT8 Flipout forward) read it: a negative value is -1, anything else +1.
__device__ __forceinline__ float obs_sign(float v) { return v < 0.0f ? -1.0f : 1.0f; }

// ---------------------------------------------------------------------------- host side of the element sweeps
// `rows` grid rows (samples, segments) of at most `cap` workgroups, a thread taking at least one quad of its row's n elements; every
// workgroup ends in a merge, so equal rows share about kObsGrid of them (obs_cap).
inline dim3 obs_grid(long long n, int rows, long long cap) {
  long long gx = (n + 4 * kObsThreads - 1) / (4 * kObsThreads);
  return dim3((unsigned)(gx > cap ? cap : gx), (unsigned)rows);
}
inline long long obs_cap(int rows) { return (kObsGrid + rows - 1) / rows; }

template <typename... T>
inline bool obs_aligned4(const T*... p) {   // (a null pointer is aligned)
  return ((((uintptr_t)p) | ...) & 3u) == 0;
}

// The <true> (draws regenerated on chip) or the <false> (draws supplied) instantiation of a sweep, under its name.
template <typename Args>
inline int obs_launch(bool on_chip, void (*kt)(Args), const char* name_t, void (*kf)(Args), const char* name_f, const char* who, dim3 grid, bt_stream_t stream,
                      const Args& a) {
  return launch_kernel(on_chip ? kt : kf, on_chip ? name_t : name_f, who, grid, dim3(kObsThreads), 0, 0, (hipStream_t)stream, a);
}

}  // namespace bt

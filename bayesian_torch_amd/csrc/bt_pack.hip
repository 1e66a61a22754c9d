// bt_pack_sync: keep the tap-major (mu, softplus(rho)) copies the fast kernels read in step with the parameters WITHOUT trusting
// the host to notice a change.
//
// The reference's own idioms write parameters through `.data` (models/dnn_to_bnn.py:65-71,95-101 `mu_kernel.data.copy_`,
// utils/util.py:102-117 in MOPED()), which no host-side version counter sees. So the check is made on the device, every time, in
// the stream: launch 1 sweeps the natural-layout (mu, rho) of up to 64 layers (8 B/weight, HBM-bound: ResNet18's 89 MB ~ 25 us)
// into one 64-bit fingerprint per layer -- the wrapping sum over the elements of a 64-bit mix of (index, mu bits, rho bits);
// integer addition commutes, so the value does not depend on the order the blocks arrive in -- and its last block compares each
// layer's fingerprint with the one stored when its pack was last built. Launch 2 rebuilds the packs of exactly the layers that
// differ (its blocks return at once for the others). Nothing comes back to the host, so both launches sit inside a captured
// HIP graph like any other kernel: a replay follows parameter updates.
//
// bt_pack_sync_kl: launch 1 also reads the priors of the layers that ask for it and produces their KL terms (the fused forwards'
// closed form and per-element order; one double partial per block, summed in block order by the last block: deterministic).
// The forwards of those layers then run without a KL sweep of their own: 8 B/weight read here instead of 16 B/weight there.
#include "bt_segments.h"

namespace bt {

// pack_dirty_kernel's argument block: what it packs from and to (t.n: elements of the natural tensors).
struct PackSegs {
  const float* src_mu[kMaxSegs];
  const float* src_rho[kMaxSegs];
  float* mu_p[kMaxSegs];
  float* sg_p[kMaxSegs];
  unsigned long long* state[kMaxSegs];
  long long C[kMaxSegs], T[kMaxSegs], np[kMaxSegs];   // pack geometry: channels, taps, packed elements
  SegTable t;
  unsigned long long force;                 // bit i: rebuild segment i whatever its fingerprint says
};
inline uint64_t digest_arg(uint64_t h, const PackSegs& a) {
  return digest_arg(digest_segs(h, a.t, a.src_mu, a.src_rho, a.mu_p, a.sg_p, a.state, a.C, a.T, a.np), a.force);
}

// The fingerprint launch's own argument block (what it reads).
struct FpSegs {
  const float* mu[kMaxSegs];
  const float* rho[kMaxSegs];
  unsigned long long* state[kMaxSegs];
  // KL (bt_pack_sync_kl): kl_out[i] == nullptr -> segment i produces none
  const float* pmu[kMaxSegs];
  const float* psig[kMaxSegs];
  const float* mu_b[kMaxSegs];
  const float* rho_b[kMaxSegs];
  const float* pmu_b[kMaxSegs];
  const float* psig_b[kMaxSegs];
  float* kl_out[kMaxSegs];
  int n_bias[kMaxSegs];
  SegTable t;
  unsigned long long force;
  int any_kl;
};
inline uint64_t digest_arg(uint64_t h, const FpSegs& a) {
  h = digest_segs(h, a.t, a.mu, a.rho, a.state, a.pmu, a.psig, a.mu_b, a.rho_b, a.pmu_b, a.psig_b, a.kl_out, a.n_bias);
  return digest_arg(digest_arg(h, a.force), a.any_kl);
}
static_assert(sizeof(PackSegs) <= kMaxSegArgBytes && sizeof(FpSegs) <= kMaxSegArgBytes, "argument block larger than kl_hier_bwd_kernel's");

constexpr int kFpThreads = 256;
constexpr int kFpElemsPerBlock = kFpThreads * 4 * 4;

__device__ __forceinline__ unsigned long long fp_mix(unsigned long long i, float m, float r) {
  unsigned long long h = (((unsigned long long)__float_as_uint(m)) << 32 | (unsigned long long)__float_as_uint(r)) + i * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h;
}

template <bool KL>
__device__ __forceinline__ void fp_sweep(const FpSegs& sg, int seg, int nb, int lb, unsigned long long& acc, double& kacc) {
  const long long n = sg.t.n[seg];
  const float* __restrict__ mu = sg.mu[seg];
  const float* __restrict__ rho = sg.rho[seg];
  const float* __restrict__ pm = sg.pmu[seg];
  const float* __restrict__ ps = sg.psig[seg];
  uintptr_t align = (uintptr_t)mu | (uintptr_t)rho;
  if (KL) align |= (uintptr_t)pm | (uintptr_t)ps;
  const bool vec_ok = (align & 15u) == 0;
  const long long n4 = vec_ok ? (n >> 2) : 0;
  for (long long base = (long long)lb * (kFpThreads * 4); base < n4; base += (long long)nb * (kFpThreads * 4)) {
    float4 m[4], r[4], p[4], q[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long long i = base + v * kFpThreads + threadIdx.x;
      if (i < n4) {
        m[v] = reinterpret_cast<const float4*>(mu)[i], r[v] = reinterpret_cast<const float4*>(rho)[i];
        if (KL) p[v] = reinterpret_cast<const float4*>(pm)[i], q[v] = reinterpret_cast<const float4*>(ps)[i];
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long long i = base + v * kFpThreads + threadIdx.x;
      if (i < n4) {
        const unsigned long long e = (unsigned long long)i * 4ull;
        acc += fp_mix(e, m[v].x, r[v].x) + fp_mix(e + 1, m[v].y, r[v].y) + fp_mix(e + 2, m[v].z, r[v].z) + fp_mix(e + 3, m[v].w, r[v].w);
        if (KL) kacc += kl_quad(m[v], r[v], p[v], q[v]);
      }
    }
  }
  for (long long i = (n4 << 2) + (long long)lb * kFpThreads + threadIdx.x; i < n; i += (long long)nb * kFpThreads) {
    const float mi = mu[i], ri = rho[i];
    acc += fp_mix((unsigned long long)i, mi, ri);
    if (KL) kacc += (double)kl_term(mi, softplus(ri), pm[i], ps[i]);
  }
}

__global__ __launch_bounds__(kFpThreads) void pack_fingerprint_kernel(FpSegs sg, unsigned* counter, double* slots, int total_blocks) {
  __shared__ int is_last;
  __shared__ double kred[kFpThreads / 64];
  int seg, nb, lb;
  seg_locate(sg.t, seg, nb, lb);
  const bool kl = sg.kl_out[seg] != nullptr;
  unsigned long long acc = 0ull;
  double kacc = 0.0;
  if (kl) fp_sweep<true>(sg, seg, nb, lb, acc, kacc);
  else fp_sweep<false>(sg, seg, nb, lb, acc, kacc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  // One agent-scope add per wave (performed at L2), drained before the block's ticket: the last arriver's agent-scope loads see
  // every add (MI355X_MICROARCH.md "Valid forms": all handed-off words written and read with agent-scope atomics).
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(&sg.state[seg][0], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (kl) {
    kacc = wave_sum(kacc);
    if ((threadIdx.x & 63) == 0) kred[threadIdx.x >> 6] = kacc;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (kl) {   // the block's KL partial, stored write-through (agent scope) and drained before the ticket: the same hand-off as the adds
      __hip_atomic_store(&slots[blockIdx.x], (kred[0] + kred[1]) + (kred[2] + kred[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    is_last = (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)total_blocks - 1u) ? 1 : 0;
  }
  __syncthreads();
  if (!is_last) return;
  if ((int)threadIdx.x < sg.t.nseg) {
    unsigned long long* const st = sg.state[threadIdx.x];
    const unsigned long long fp = __hip_atomic_load(&st[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long old = __hip_atomic_load(&st[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool dirty = ((sg.force >> threadIdx.x) & 1ull) || fp != old;
    __hip_atomic_store(&st[1], fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&st[2], dirty ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&st[3], st[3] + (dirty ? 1ull : 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // rebuild count (diagnostic, tests)
    __hip_atomic_store(&st[0], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // accumulator left zeroed for the next call
  }
  if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!sg.any_kl) return;
  // KL finish: one wave per segment, the block partials in block order (fixed lane split + fixed butterfly: deterministic)
  const int lane = threadIdx.x & 63;
  for (int s = threadIdx.x >> 6; s < sg.t.nseg; s += kFpThreads / 64) {
    if (sg.kl_out[s] == nullptr) continue;
    double t = 0.0;
    for (int b = sg.t.first_block[s] + lane; b < sg.t.first_block[s + 1]; b += 64) {
      t += __hip_atomic_load(&slots[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&slots[b], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
    }
    t = wave_sum(t);
    double bt_ = 0.0;
    const float *mb = sg.mu_b[s], *rb = sg.rho_b[s], *pb = sg.pmu_b[s], *qb = sg.psig_b[s];
    if (mb)
      for (int c = lane; c < sg.n_bias[s]; c += 64) bt_ += (double)kl_term(mb[c], softplus(rb[c]), pb[c], qb[c]);
    bt_ = wave_sum(bt_);
    if (lane == 0) {
      float v = (float)(t / (double)sg.t.n[s]);
      if (mb) v += (float)(bt_ / (double)sg.n_bias[s]);
      sg.kl_out[s][0] = v;
    }
  }
}

// packed[(co*T + t)*C4 + c] <- natural[co][c][t] for the segments marked dirty (the layout of bt_pack_params). A work item is (row co,
// chunk of 64 channels): its 64 x T natural floats are one contiguous run -- read coalesced, transposed through LDS, written as T runs
// of 64 packed floats (a training step rebuilds every pack: read straight in packed order the natural tensors were fetched at a
// stride of T floats, 99 us per ResNet18 step).
constexpr int kPackCh = 64;
__global__ __launch_bounds__(256) void pack_dirty_kernel(PackSegs sg) {
  extern __shared__ float2 tile[];   // [T][64 + 1] (mu, sigma)
  int seg, nb, lb;
  seg_locate(sg.t, seg, nb, lb);
  if (__hip_atomic_load(&sg.state[seg][2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull) return;
  const long long C = sg.C[seg], T = sg.T[seg], C4 = (C + 3) & ~3ll;
  const long long Co = sg.np[seg] / (T * C4);
  const long long cchunks = (C4 + kPackCh - 1) / kPackCh, items = Co * cchunks;
  const float* __restrict__ mu = sg.src_mu[seg];
  const float* __restrict__ rho = sg.src_rho[seg];
  float* __restrict__ mu_p = sg.mu_p[seg];
  float* __restrict__ sg_p = sg.sg_p[seg];
  const int Ti = (int)T;
  for (long long it = lb; it < items; it += nb) {
    const long long co = it / cchunks, c0 = (it - co * cchunks) * kPackCh;
    const int nc = (int)((C - c0) < kPackCh ? (C - c0 > 0 ? C - c0 : 0) : kPackCh);      // real channels of this chunk
    const int nc4 = (int)((C4 - c0) < kPackCh ? (C4 - c0) : kPackCh);                     // packed channels (padding holds zeros)
    const long long src0 = (co * C + c0) * T;
    __syncthreads();   // (the previous item's tile has been written out)
    for (int i = threadIdx.x; i < nc * Ti; i += 256) {
      const int c = i / Ti, t = i - c * Ti;
      tile[t * (kPackCh + 1) + c] = make_float2(mu[src0 + i], softplus(rho[src0 + i]));
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Ti * nc4; j += 256) {
      const int t = j / nc4, c = j - t * nc4;
      const float2 v = c < nc ? tile[t * (kPackCh + 1) + c] : make_float2(0.f, 0.f);
      const long long dst = (co * T + t) * C4 + c0 + c;
      mu_p[dst] = v.x;
      sg_p[dst] = v.y;
    }
  }
}

// bt_pack_eps: eps_packed[r][t][c] <- eps[r][c][t], r = (sample, row) -- pack_dirty_kernel's transpose for a draw: a work item is
// (r, chunk of 64 channels), its 64 x T natural floats one contiguous run read coalesced, transposed through LDS, written as T runs
// of packed floats; the padding channels hold 0.0.
__global__ __launch_bounds__(256) void pack_eps_kernel(const float* __restrict__ eps, float* __restrict__ out, long long rows, long long C, int T) {
  extern __shared__ float etile[];   // [T][64 + 1]
  const long long C4 = (C + 3) & ~3ll;
  const long long cchunks = (C4 + kPackCh - 1) / kPackCh, items = rows * cchunks;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long r = it / cchunks, c0 = (it - r * cchunks) * kPackCh;
    const int nc = (int)((C - c0) < kPackCh ? (C - c0 > 0 ? C - c0 : 0) : kPackCh);
    const int nc4 = (int)((C4 - c0) < kPackCh ? (C4 - c0) : kPackCh);
    const long long src0 = (r * C + c0) * T;
    __syncthreads();   // (the previous item's tile has been written out)
    for (int i = threadIdx.x; i < nc * T; i += 256) {
      const int c = i / T, t = i - c * T;
      etile[t * (kPackCh + 1) + c] = eps[src0 + i];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < T * nc4; j += 256) {
      const int t = j / nc4, c = j - t * nc4;
      out[(r * T + t) * C4 + c0 + c] = c < nc ? etile[t * (kPackCh + 1) + c] : 0.f;
    }
  }
}

// bt_pack_signs: out[s][i] <- 0x80 where signs[s][i] < 0, else 0x00; a thread writes one dword = four consecutive elements of a sample's
// image (the image stride is a multiple of 16 bytes; bytes past n hold 0). Elements that are not exactly +1 / -1 -- zeros, NaNs,
// anything else -- are counted: one vector atomic per wave that met one, on the word the host zeroed in front of this launch.
__global__ __launch_bounds__(256) void pack_signs_kernel(const float* __restrict__ signs, uint32_t* __restrict__ out, long long n, long long words_per_sample,
                                                         long long words, unsigned* __restrict__ not_pm1) {
  unsigned bad = 0;
  for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long long)gridDim.x * 256) {
    const long long smp = w / words_per_sample, e0 = 4 * (w - smp * words_per_sample);
    const float* const src = signs + smp * n;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e0 + k < n) {
        const float v = src[e0 + k];
        word |= (v < 0.f ? 0x80u : 0u) << (8 * k);
        bad += (v == 1.f || v == -1.f) ? 0u : 1u;
      }
    }
    out[w] = word;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(not_pm1, bad);
}

}  // namespace bt

extern "C" int bt_pack_signs(const float* signs, int32_t S, int64_t n, uint8_t* signs_packed, uint32_t* not_pm1_count, bt_stream_t stream) {
  using namespace bt;
  if (!signs || !signs_packed || !not_pm1_count) return set_error(BT_ERR_BAD_ARG, "bt_pack_signs: null argument");
  if (S <= 0 || n <= 0) return set_error(BT_ERR_BAD_ARG, "bt_pack_signs: non-positive dimension");
  if ((((uintptr_t)signs_packed) & 15u) != 0) return set_error(BT_ERR_BAD_ARG, "bt_pack_signs: signs_packed must be 16-byte aligned");
  if (n >= (1ll << 30)) return set_error(BT_ERR_UNSUPPORTED, "bt_pack_signs: a sample of 2^30 elements or more exceeds the kernels' 32-bit offsets");
  const long long wps = BT_SIGNS_PACKED_STRIDE(n) / 4, words = (long long)S * wps;
  if (!plan_only() && hipMemsetAsync(not_pm1_count, 0, sizeof(uint32_t), (hipStream_t)stream) != hipSuccess)
    return set_error(BT_ERR_HIP_BASE, "bt_pack_signs: hipMemsetAsync failed");
  long long blocks = (words + 255) / 256;
  if (blocks > 4096) blocks = 4096;   // (the rest in the kernel's loop)
  return launch_kernel(pack_signs_kernel, nullptr, "bt_pack_signs", dim3((unsigned)blocks), dim3(256), 0, 0, (hipStream_t)stream, signs,
                       reinterpret_cast<uint32_t*>(signs_packed), (long long)n, wps, words, not_pm1_count);
}

extern "C" int bt_pack_eps(const float* eps_w, int32_t S, int64_t Co, int64_t Ci, int64_t taps, float* eps_packed, bt_stream_t stream) {
  using namespace bt;
  if (!eps_w || !eps_packed) return set_error(BT_ERR_BAD_ARG, "bt_pack_eps: null argument");
  if (S <= 0 || Co <= 0 || Ci <= 0 || taps <= 0) return set_error(BT_ERR_BAD_ARG, "bt_pack_eps: non-positive dimension");
  if (taps > 128) return set_error(BT_ERR_UNSUPPORTED, "bt_pack_eps: kernels larger than 128 taps are not supported");
  const long long rows = (long long)S * Co, C4 = (Ci + 3) & ~3ll;
  if (rows >= (1ll << 40) / (taps * C4)) return set_error(BT_ERR_UNSUPPORTED, "bt_pack_eps: draw too large");
  long long blocks = rows * ((C4 + kPackCh - 1) / kPackCh);
  if (blocks > 8192) blocks = 8192;   // (the rest in the kernel's item loop)
  const int lds = (int)(taps * (kPackCh + 1) * sizeof(float));
  return launch_kernel(pack_eps_kernel, nullptr, "bt_pack_eps", dim3((unsigned)blocks), dim3(256), lds, 128 * (kPackCh + 1) * (int)sizeof(float), (hipStream_t)stream,
                       eps_w, eps_packed, rows, (long long)Ci, (int)taps);
}

extern "C" int bt_pack_sync_kl(int32_t n_segments, const bt_pack_seg* segs, const bt_pack_kl* kls, void* workspace, size_t workspace_bytes,
                               bt_stream_t stream) {
  using namespace bt;
  if (n_segments <= 0 || n_segments > BT_PACK_MAX_SEGMENTS) return set_error(BT_ERR_BAD_ARG, "bt_pack_sync: n_segments must be in [1, 64]");
  if (!segs) return set_error(BT_ERR_BAD_ARG, "bt_pack_sync: null argument");
  if (!workspace || workspace_bytes < BT_WORKSPACE_BYTES) return set_error(BT_ERR_WORKSPACE, "bt_pack_sync: workspace smaller than BT_WORKSPACE_BYTES");
  FpSegs fs = {};
  PackSegs pk = {};
  for (int i = 0; i < n_segments; ++i) {
    const bt_pack_kl* k = kls ? &kls[i] : nullptr;
    if (!k || !k->kl_out) continue;
    if (!k->prior_mu_w || !k->prior_sigma_w) return set_error(BT_ERR_BAD_ARG, "bt_pack_sync_kl: kl_out given but weight priors are NULL");
    const bool b = k->mu_b != nullptr;
    if (b != (k->rho_b != nullptr) || b != (k->prior_mu_b != nullptr) || b != (k->prior_sigma_b != nullptr))
      return set_error(BT_ERR_BAD_ARG, "bt_pack_sync_kl: give all four bias tensors or none");
    if (b && (k->n_bias <= 0 || k->n_bias >= (1ll << 30))) return set_error(BT_ERR_BAD_ARG, "bt_pack_sync_kl: bad n_bias");
    fs.pmu[i] = k->prior_mu_w, fs.psig[i] = k->prior_sigma_w, fs.kl_out[i] = k->kl_out;
    fs.mu_b[i] = k->mu_b, fs.rho_b[i] = k->rho_b, fs.pmu_b[i] = k->prior_mu_b, fs.psig_b[i] = k->prior_sigma_b;
    fs.n_bias[i] = b ? (int)k->n_bias : 0;
    fs.any_kl = 1;
  }
  int64_t elems[kMaxSegs], items[kMaxSegs];   // a segment's work: elements to fingerprint, (row, 64-channel chunk) items to pack
  long long max_taps = 1;
  for (int i = 0; i < n_segments; ++i) {
    const bt_pack_seg& s = segs[i];
    if (!s.mu_w || !s.rho_w || !s.mu_packed || !s.sigma_packed || !s.state || s.Co <= 0 || s.Ci <= 0 || s.taps <= 0)
      return set_error(BT_ERR_BAD_ARG, "bt_pack_sync: null pointer or non-positive dimension in a segment");
    if ((s.src_mu == nullptr) != (s.src_rho == nullptr)) return set_error(BT_ERR_BAD_ARG, "bt_pack_sync: src_mu and src_rho must both be given or both be NULL");
    const long long C4 = (s.Ci + 3) & ~3ll;
    fs.mu[i] = s.mu_w, fs.rho[i] = s.rho_w;
    pk.src_mu[i] = s.src_mu ? s.src_mu : s.mu_w, pk.src_rho[i] = s.src_rho ? s.src_rho : s.rho_w;
    pk.mu_p[i] = s.mu_packed, pk.sg_p[i] = s.sigma_packed;
    fs.state[i] = pk.state[i] = reinterpret_cast<unsigned long long*>(s.state);
    fs.t.n[i] = pk.t.n[i] = elems[i] = s.Co * s.Ci * s.taps;
    pk.C[i] = s.Ci, pk.T[i] = s.taps, pk.np[i] = s.Co * s.taps * C4;
    items[i] = s.Co * ((C4 + kPackCh - 1) / kPackCh);
    if (s.force) pk.force |= 1ull << i;
    if (s.taps > max_taps) max_taps = s.taps;
  }
  fs.force = pk.force;
  // At most 128 fingerprint blocks per segment (more are slower: every wave ends in one 64-bit atomic on the segment's accumulator --
  // 1024 blocks: 14 -> 25 us for 1.5 M weights), and with a KL one slot per block in the workspace; at most 256 pack blocks.
  const int fcap = fs.any_kl && kMaxSlots / n_segments < 128 ? kMaxSlots / n_segments : 128;
  const int fblocks = seg_partition(fs.t, n_segments, elems, kFpElemsPerBlock, fcap, 0, "bt_pack_sync");
  const int pblocks = seg_partition(pk.t, n_segments, items, 1, 256, 0, "bt_pack_sync");
  // Everything that can refuse the call is checked before the first launch: the fingerprint launch stores every segment's new
  // fingerprint and dirty flag, so a refusal after it would leave the packs stale against fingerprints that say they are current.
  const size_t lds = (size_t)max_taps * (kPackCh + 1) * sizeof(float2);
  if (max_taps > 128) return set_error(BT_ERR_UNSUPPORTED, "bt_pack_sync: kernels larger than 128 taps are not supported");
  const int lds_limit = 128 * (kPackCh + 1) * (int)sizeof(float2);   // (above the default dynamic-LDS limit: 11 x 11 kernels and larger)
  if (!plan_only())
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(pack_dirty_kernel), lds_limit, "bt_pack_sync")) return rc;
  if (int rc = launch_kernel(pack_fingerprint_kernel, nullptr, "bt_pack_sync (fingerprint)", dim3(fblocks), dim3(kFpThreads), 0, 0, (hipStream_t)stream, fs,
                             ws_counter(workspace), ws_slots(workspace), fblocks))
    return rc;
  return launch_kernel(pack_dirty_kernel, nullptr, "bt_pack_sync (pack)", dim3(pblocks), dim3(256), (int)lds, lds_limit, (hipStream_t)stream, pk);
}

extern "C" int bt_pack_sync(int32_t n_segments, const bt_pack_seg* segs, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  return bt_pack_sync_kl(n_segments, segs, nullptr, workspace, workspace_bytes, stream);
}

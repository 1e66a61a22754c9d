// The segmented hand-off: one launch over a list of up to 64 tensors (the KL kernels, their gradients, the pack check). A SegTable
// says which blocks of the grid work on which segment; it is built on the host by seg_partition / seg_layers and read on the device by
// seg_locate (every block) and seg_finish (the last arriver of a reduction: the one fixed-order finish, reasoned about here only).
#pragma once
#include <stdio.h>

#include "bt_api_internal.h"

namespace bt {

static_assert(BT_KL_MAX_SEGMENTS == 64 && BT_PACK_MAX_SEGMENTS == 64, "SegTable holds 64 segments and new_layer one bit for each");
constexpr int kMaxSegs = 64;

struct SegTable {
  long long n[kMaxSegs];            // elements of segment i
  int first_block[kMaxSegs + 1];    // blocks [first_block[i], first_block[i+1]) work on segment i
  unsigned long long new_layer;     // bit i: segment i starts a new layer (fp32 summation grouping); 0 where nothing is summed
  int nseg;
};
// A kernel's argument block is a SegTable plus its own pointer arrays and scalars; none is larger than kl_hier_bwd_kernel's eleven arrays.
constexpr size_t kMaxSegArgBytes = 11 * kMaxSegs * sizeof(void*) + sizeof(SegTable);

// Blocks over segments: segment i gets ceil(work[i] / per_block) blocks, at most max_per_seg (0: no cap; the kernel's loop strides over
// the rest). -> the grid, or the refusal's (negative) code: more than max_slots blocks (a reduction's workspace holds one slot per
// block), or with max_slots == 0 more than a grid holds.
inline int seg_partition(SegTable& t, int nseg, const int64_t* work, int per_block, long long max_per_seg, int max_slots, const char* who) {
  char buf[160];
  long long blocks = 0;
  for (int i = 0; i < nseg; ++i) {
    long long nb = (work[i] + per_block - 1) / per_block;
    if (max_per_seg && nb > max_per_seg) nb = max_per_seg;
    t.first_block[i] = (int)blocks;
    blocks += nb;
    if (blocks > (max_slots ? max_slots : 0x7FFFFFFFll)) {
      snprintf(buf, sizeof(buf), max_slots ? "%s: too many blocks for the workspace; split the call" : "%s: too many elements for one launch", who);
      return set_error(BT_ERR_UNSUPPORTED, buf);
    }
  }
  t.first_block[nseg] = (int)blocks;
  t.nseg = nseg;
  return (int)blocks;
}

// layer_of_segment (null: every segment a layer of its own) -> new_layer; BT_OK or the refusal.
inline int seg_layers(SegTable& t, int nseg, const int32_t* layer_of_segment, const char* who) {
  t.new_layer = 0;
  for (int i = 0; i < nseg; ++i) {
    if (layer_of_segment && i && layer_of_segment[i] < layer_of_segment[i - 1]) {
      char buf[160];
      snprintf(buf, sizeof(buf), "%s: layer_of_segment must be non-decreasing", who);
      return set_error(BT_ERR_BAD_ARG, buf);
    }
    if (i == 0 || !layer_of_segment || layer_of_segment[i] != layer_of_segment[i - 1]) t.new_layer |= 1ull << i;
  }
  return BT_OK;
}

// Plan-only digest of a segmented argument block: what the launch means, not the block's bytes (entries past nseg are never read).
// Per segment every per_seg array's entry, n and first_block; then the table's tail. The block's own scalars follow in its overload.
template <typename... Arr>
uint64_t digest_segs(uint64_t h, const SegTable& t, const Arr&... per_seg) {
  for (int i = 0; i < t.nseg; ++i) {
    ((h = digest_arg(h, per_seg[i])), ...);
    h = digest_arg(digest_arg(h, t.n[i]), t.first_block[i]);
  }
  return digest_arg(digest_arg(digest_arg(h, t.first_block[t.nseg]), t.nseg), t.new_layer);
}

// This block's segment, the number of blocks on it and this block's index among them (nseg <= 64: a linear scan on scalars).
__device__ __forceinline__ void seg_locate(const SegTable& t, int& seg, int& nb, int& lb) {
  seg = 0;
  while (seg + 1 < t.nseg && (int)blockIdx.x >= t.first_block[seg + 1]) ++seg;
  nb = t.first_block[seg + 1] - t.first_block[seg];
  lb = blockIdx.x - t.first_block[seg];
}

// The last arriver (all 256 threads of it, after publish_and_ticket_wt) turns the blocks' fp64 partials into the result: a fixed-ORDER
// finish, in parallel. A segment's partials are summed in a fixed tree (thread t adds the slots t, t + 256, ... in increasing order;
// then the wave butterflies and the four wave sums in index order): the same tree every time, so the result is deterministic -- and a
// whole model's ~2,700 slots do not pass through ONE thread's serial chain of agent-scope loads (429 us of a 3.95 ms ResNet18 training
// step, and of every get_kl_loss()). The partials were stored write-through at agent scope and drained before each block's ticket, so
// agent-scope loads see them; slots and counter are left zeroed for the next call. to_f32(fp64 segment sum, n) is the segment's fp32
// value (also seg_out[s] when given); the segments of a layer are added in fp32, then the layers in order (the reference adds fp32
// 0-dim tensors: kl_weight + kl_bias, then += across layers). red: the kernel's four doubles of LDS, free again.
template <typename F>
__device__ __forceinline__ void seg_finish(const SegTable& t, double* slots, unsigned* counter, double* red, float* kl_out, float* seg_out, F to_f32) {
  __shared__ double seg_sum[kMaxSegs];
  for (int s = 0; s < t.nseg; ++s) {
    double v = 0.0;
    for (int b = t.first_block[s] + (int)threadIdx.x; b < t.first_block[s + 1]; b += 256) {
      v += __hip_atomic_load(&slots[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&slots[b], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
    }
    v = wave_sum(v);
    __syncthreads();   // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) seg_sum[s] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f, layer = 0.0f;
    for (int s = 0; s < t.nseg; ++s) {
      const float v = to_f32(seg_sum[s], t.n[s]);
      if (seg_out) seg_out[s] = v;
      if ((t.new_layer >> s) & 1ull) {
        if (s) total += layer;  // 0.0f + x is exact, so the first layer enters unrounded
        layer = v;
      } else {
        layer += v;
      }
    }
    kl_out[0] = total + layer;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
  }
}

}  // namespace bt

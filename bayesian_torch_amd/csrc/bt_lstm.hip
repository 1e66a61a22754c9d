// The LSTM cell's gate arithmetic behind the two fused Linear launches of a time step (layers/_lstm.py): one element-wise forward
// launch and one backward launch, both memory-bound. Gate order i, f, g, o over the 4H columns, as the reference's
// rnn_variational.py:107-153.
//
// A thread owns FOUR consecutive hidden units j .. j + 3 of one row. In the vector form that is four 16-byte gate loads at columns
// j, H + j, 2H + j, 3H + j of each of a and b, one for c_prev, and 16-byte stores; it is legal only when H % 4 == 0, every pointer
// handed over is 16-byte aligned and every row stride is a multiple of 4 (vec_ok below, checked on the host per call). Otherwise
// the element-wise form walks the same four units with 4-byte accesses and computes the same values. No LDS, no scratch.
#include "bt_api_internal.h"

namespace bt {

constexpr float kLog2e = 1.4426950408889634f;

// 1 / (1 + e^-x) on v_exp_f32 / v_rcp_f32. e^-x overflows to +inf for x < -88.7: rcp(inf) = 0, the limit; it underflows to 0 for
// large x: rcp(1) = 1. Never inf / inf.
__device__ __forceinline__ float sigmoid_hw(float x) {
  const float e = __builtin_amdgcn_exp2f(__fmul_rn(x, -kLog2e));
  return __builtin_amdgcn_rcpf(__fadd_rn(1.0f, e));
}

// tanh x = 1 - 2 / (e^2x + 1). e^2x = +inf gives 1 - 2 * 0 = 1, e^2x = 0 gives 1 - 2 = -1. (The (e - 1) / (e + 1) form would be
// inf * 0 there.)
__device__ __forceinline__ float tanh_hw(float x) {
  const float e = __builtin_amdgcn_exp2f(__fmul_rn(x, 2.0f * kLog2e));
  return __fsub_rn(1.0f, __fmul_rn(2.0f, __builtin_amdgcn_rcpf(__fadd_rn(e, 1.0f))));
}

// Four consecutive floats at p; the element-wise form reads / writes the first n (1..4) of them, the rest are zero / dropped.
template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int n, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, int n, const float (&v)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = v[k];
  }
}

// Item `it` of rows * H4 (H4 = ceil(H / 4)): row r, hidden units j .. j + n - 1.
__device__ __forceinline__ bool cell_item(long long items, int H4, long long H, long long& r, long long& j, int& n) {
  const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
  if (it >= items) return false;
  r = it / H4;
  j = (it - r * H4) * 4;
  n = H - j < 4 ? (int)(H - j) : 4;
  return true;
}

// h = o * tanh(c), c = f * c_prev + i * g over z = a (+ b). c_prev row r reads row r % c_rows (an initial state shared by the MC
// samples). ACT: the four activated gates go to act [rows][4H] for the backward.
template <bool VEC, bool ACT>
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(long long items, int H4, long long H, const float* __restrict__ a,
                                                             const float* __restrict__ b, const float* c_prev, long long c_rows, long long ld_c,
                                                             float* h_out, float* c_out, long long ld_out, float* __restrict__ act) {
  long long r, j;
  int n;
  if (!cell_item(items, H4, H, r, j, n)) return;
  const long long zrow = r * 4 * H + j;
  float z[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) load4<VEC>(a + zrow + q * H, n, z[q]);
  if (b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float t[4];
      load4<VEC>(b + zrow + q * H, n, t);
#pragma unroll
      for (int k = 0; k < 4; ++k) z[q][k] = __fadd_rn(z[q][k], t[k]);
    }
  }
  float cp[4], h[4], c[4];
  load4<VEC>(c_prev + (r % c_rows) * ld_c + j, n, cp);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    z[0][k] = sigmoid_hw(z[0][k]);
    z[1][k] = sigmoid_hw(z[1][k]);
    z[2][k] = tanh_hw(z[2][k]);
    z[3][k] = sigmoid_hw(z[3][k]);
    c[k] = __fadd_rn(__fmul_rn(z[1][k], cp[k]), __fmul_rn(z[0][k], z[2][k]));
    h[k] = __fmul_rn(z[3][k], tanh_hw(c[k]));
  }
  store4<VEC>(c_out + r * ld_out + j, n, c);
  store4<VEC>(h_out + r * ld_out + j, n, h);
  if constexpr (ACT) {
#pragma unroll
    for (int q = 0; q < 4; ++q) store4<VEC>(act + zrow + q * H, n, z[q]);
  }
}

// The closed form on the saved activations (never the derivative of the exponential formulas above: a saturated gate gives exactly 0):
//   dc = grad_c + grad_h o (1 - tanh^2 c)      di = dc g i (1 - i)     df = dc c_prev f (1 - f)     dg = dc i (1 - g^2)
//   do = grad_h tanh(c) o (1 - o)              dc_prev = dc f
// grad_h / grad_c null: zero. dz [rows][4H] is the gradient of a and of b alike; dc_prev [rows][H] is per row (a shared c_prev's is
// the sum over the samples, done by the caller).
template <bool VEC>
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(long long items, int H4, long long H, const float* __restrict__ act, const float* c_prev,
                                                             long long c_rows, long long ld_c, const float* c_new, long long ld_cn,
                                                             const float* grad_h, long long ld_gh, const float* grad_c, long long ld_gc,
                                                             float* __restrict__ dz, float* __restrict__ dc_prev) {
  long long r, j;
  int n;
  if (!cell_item(items, H4, H, r, j, n)) return;
  const long long zrow = r * 4 * H + j;
  float g4[4][4], cp[4], cn[4], gh[4] = {0.f, 0.f, 0.f, 0.f}, gc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 4; ++q) load4<VEC>(act + zrow + q * H, n, g4[q]);
  load4<VEC>(c_prev + (r % c_rows) * ld_c + j, n, cp);
  load4<VEC>(c_new + r * ld_cn + j, n, cn);
  if (grad_h) load4<VEC>(grad_h + r * ld_gh + j, n, gh);
  if (grad_c) load4<VEC>(grad_c + r * ld_gc + j, n, gc);
  float d[4][4], dcp[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float i = g4[0][k], f = g4[1][k], g = g4[2][k], o = g4[3][k];
    const float tc = tanh_hw(cn[k]);
    const float dc = __fadd_rn(gc[k], __fmul_rn(__fmul_rn(gh[k], o), __fsub_rn(1.0f, __fmul_rn(tc, tc))));
    d[0][k] = __fmul_rn(__fmul_rn(dc, g), __fmul_rn(i, __fsub_rn(1.0f, i)));
    d[1][k] = __fmul_rn(__fmul_rn(dc, cp[k]), __fmul_rn(f, __fsub_rn(1.0f, f)));
    d[2][k] = __fmul_rn(__fmul_rn(dc, i), __fsub_rn(1.0f, __fmul_rn(g, g)));
    d[3][k] = __fmul_rn(__fmul_rn(gh[k], tc), __fmul_rn(o, __fsub_rn(1.0f, o)));
    dcp[k] = __fmul_rn(dc, f);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) store4<VEC>(dz + zrow + q * H, n, d[q]);
  store4<VEC>(dc_prev + r * H + j, n, dcp);
}

// The vector form's guard: whole quads per row, every pointer on a 16-byte boundary, every row stride a multiple of 4.
static bool vec_ok(int64_t H, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> strides) {
  if (H % 4) return false;
  for (const void* p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15u)) return false;
  for (int64_t s : strides)
    if (s % 4) return false;
  return true;
}

// rows * ceil(H / 4) items in blocks of 256 -> false when the grid would not fit.
static bool cell_grid(int64_t rows, int64_t H, long long& items, int& H4, unsigned& blocks) {
  if (H > (int64_t)INT_MAX - 3 || rows > LLONG_MAX / ((H + 3) / 4)) return false;
  H4 = (int)((H + 3) / 4);
  items = (long long)rows * H4;
  const long long nb = (items + 255) / 256;
  if (nb > INT_MAX) return false;
  blocks = (unsigned)nb;
  return true;
}

}  // namespace bt

extern "C" int bt_lstm_cell_fwd(int64_t rows, int64_t H, const float* a, const float* b, const float* c_prev, int64_t c_rows, int64_t ld_c,
                                float* h_out, float* c_out, int64_t ld_out, float* act, bt_stream_t stream) {
  using namespace bt;
  if (rows < 1 || H < 1 || !a || !c_prev || !h_out || !c_out || c_rows < 1 || rows % c_rows || ld_c < H || ld_out < H)
    return set_error(BT_ERR_BAD_ARG, "bt_lstm_cell_fwd: bad argument");
  long long items;
  int H4;
  unsigned blocks;
  if (!cell_grid(rows, H, items, H4, blocks)) return set_error(BT_ERR_UNSUPPORTED, "bt_lstm_cell_fwd: too many elements for one launch");
  const bool vec = vec_ok(H, {a, b, c_prev, h_out, c_out, act}, {ld_c, ld_out});
  auto launch = [&](auto kern, const char* name) {
    return launch_kernel(kern, name, "bt_lstm_cell_fwd", dim3(blocks), dim3(256), 0, 0, (hipStream_t)stream, items, H4, (long long)H, a, b, c_prev,
                         (long long)c_rows, (long long)ld_c, h_out, c_out, (long long)ld_out, act);
  };
  if (vec) return act ? launch(lstm_cell_fwd_kernel<true, true>, "lstm_cell_fwd_kernel<vec4,act=1>") : launch(lstm_cell_fwd_kernel<true, false>, "lstm_cell_fwd_kernel<vec4,act=0>");
  return act ? launch(lstm_cell_fwd_kernel<false, true>, "lstm_cell_fwd_kernel<elem,act=1>") : launch(lstm_cell_fwd_kernel<false, false>, "lstm_cell_fwd_kernel<elem,act=0>");
}

extern "C" int bt_lstm_cell_bwd(int64_t rows, int64_t H, const float* act, const float* c_prev, int64_t c_rows, int64_t ld_c, const float* c_new,
                                int64_t ld_cn, const float* grad_h, int64_t ld_gh, const float* grad_c, int64_t ld_gc, float* dz, float* dc_prev,
                                bt_stream_t stream) {
  using namespace bt;
  if (rows < 1 || H < 1 || !act || !c_prev || !c_new || !dz || !dc_prev || c_rows < 1 || rows % c_rows || ld_c < H || ld_cn < H ||
      (grad_h && ld_gh < H) || (grad_c && ld_gc < H))
    return set_error(BT_ERR_BAD_ARG, "bt_lstm_cell_bwd: bad argument");
  long long items;
  int H4;
  unsigned blocks;
  if (!cell_grid(rows, H, items, H4, blocks)) return set_error(BT_ERR_UNSUPPORTED, "bt_lstm_cell_bwd: too many elements for one launch");
  const bool vec = vec_ok(H, {act, c_prev, c_new, grad_h, grad_c, dz, dc_prev}, {ld_c, ld_cn, grad_h ? ld_gh : 0, grad_c ? ld_gc : 0});
  auto launch = [&](auto kern, const char* name) {
    return launch_kernel(kern, name, "bt_lstm_cell_bwd", dim3(blocks), dim3(256), 0, 0, (hipStream_t)stream, items, H4, (long long)H, act, c_prev,
                         (long long)c_rows, (long long)ld_c, c_new, (long long)ld_cn, grad_h, (long long)ld_gh, grad_c, (long long)ld_gc, dz, dc_prev);
  };
  return vec ? launch(lstm_cell_bwd_kernel<true>, "lstm_cell_bwd_kernel<vec4>") : launch(lstm_cell_bwd_kernel<false>, "lstm_cell_bwd_kernel<elem>");
}

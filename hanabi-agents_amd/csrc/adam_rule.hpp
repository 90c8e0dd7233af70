// adam_rule.hpp — the per-element optimizer rule of a merged NoisyLinear tensor W = w + w_mu + w_sigma * noise, shared by the
// Adam kernels of learner.hip and by the launch of learner2.hip that runs the output layer's step beside the dW1 product
// (learner_tail_l2_dw1_kernel): ONE copy of the rule, so that every kernel that steps a tensor produces the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#include "../../include/hanabi_hip.h"
#include "common.hpp"

namespace hb {
namespace adam {

struct AdamArgs {
  float *w, *w_mu, *w_sigma;
  const float* noise;  // eps of the layer (same shape); bias noise for bias tensors
  const void* grad;    // d loss / d (merged tensor): fp32 / bf16 / f16 (grad_dtype), rows grad_ld elements apart
  float *m_w, *v_w, *m_mu, *v_mu, *m_sg, *v_sg;
  const float* step;   // number of completed Adam steps (device scalar)
  void* eff;           // merged tensor in the GEMM dtype for the next forward
  long long n;
  int cols, eff_ld;    // parameter tensors are [n/cols, cols] row-major; eff rows are eff_ld >= cols elements apart
  int grad_dtype, grad_ld;
  float lr, b1, b2, eps;
  float step_offset;   // this step's number t = *step + step_offset
};

// all merged tensors of the network in ONE launch: workgroup b belongs to tensor t where first[t] <= b < first[t+1]
struct AdamMulti {
  AdamArgs t[8];
  int first[9];
  int count;
};

template <typename T> __device__ __forceinline__ void store_eff(T* p, long long i, float v);
template <> __device__ __forceinline__ void store_eff<float>(float* p, long long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void store_eff<__hip_bfloat16>(__hip_bfloat16* p, long long i, float v) { p[i] = __float2bfloat16(v); }
template <> __device__ __forceinline__ void store_eff<__half>(__half* p, long long i, float v) { p[i] = __float2half(v); }

__device__ __forceinline__ float load_grad(const void* g, int dtype, long long i) {
  if (dtype == 1) return __bfloat162float(static_cast<const __hip_bfloat16*>(g)[i]);
  if (dtype == 2) return __half2float(static_cast<const __half*>(g)[i]);
  return static_cast<const float*>(g)[i];
}

__device__ __forceinline__ float adam1(float p, float g, float& m, float& v, float b1, float b2, float bc1, float bc2s,
                                       float lr, float eps) {
  // explicit roundings (no compiler-chosen FMA contraction): the scalar and the 4-wide kernels must agree bit for bit
  m = __fmaf_rn(b1, m, __fmul_rn(1.f - b1, g));
  v = __fmaf_rn(b2, v, __fmul_rn(__fmul_rn(1.f - b2, g), g));
  // torch.optim.Adam / optix.adam: eps outside the sqrt
  return __fsub_rn(p, __fdiv_rn(__fmul_rn(lr / bc1, m), __fadd_rn(__fdiv_rn(sqrtf(v), bc2s), eps)));
}
// The step Adam takes for moments (m, v): p_new = p - adam_step(...). w and w_mu of a NoisyLinear always see the same
// gradient, so their moments are equal for ever; a caller may pass the SAME moment arrays for both (m_mu == m_w,
// v_mu == v_w) and the kernels then apply w's step to w_mu without touching the moments a second time.
__device__ __forceinline__ float adam_step(float m, float v, float bc1, float bc2s, float lr, float eps) {
  return __fdiv_rn(__fmul_rn(lr / bc1, m), __fadd_rn(__fdiv_rn(sqrtf(v), bc2s), eps));
}
__device__ __forceinline__ float merged(float w, float mu, float sg, float nz) {  // W = w + w_mu + w_sigma * noise
  return __fadd_rn(__fadd_rn(w, mu), __fmul_rn(sg, nz));
}

// this step's bias corrections: 1 - b1^t and sqrt(1 - b2^t), t = *step + step_offset
__device__ __forceinline__ void bias_corrections(const AdamArgs& a, float& bc1, float& bc2s) {
  const float t = *a.step + a.step_offset;
  bc1 = 1.f - powf(a.b1, t);
  bc2s = sqrtf(1.f - powf(a.b2, t));
}

// ONE element i of tensor a: the three parameters, their moments and the next effective weight
template <typename T>
__device__ __forceinline__ void step_element(const AdamArgs& a, long long i, float bc1, float bc2s) {
  const long long row = i / a.cols, col = i - row * a.cols;
  const float g = load_grad(a.grad, a.grad_dtype, row * a.grad_ld + col), nz = a.noise[i];
  float m, v;
  m = a.m_w[i]; v = a.v_w[i];
  const float w = adam1(a.w[i], g, m, v, a.b1, a.b2, bc1, bc2s, a.lr, a.eps);
  a.m_w[i] = m; a.v_w[i] = v; a.w[i] = w;
  float mu;
  if (a.m_mu == a.m_w) {  // shared moments: (m, v) are w's, already advanced
    mu = __fsub_rn(a.w_mu[i], adam_step(m, v, bc1, bc2s, a.lr, a.eps));
  } else {
    m = a.m_mu[i]; v = a.v_mu[i];
    mu = adam1(a.w_mu[i], g, m, v, a.b1, a.b2, bc1, bc2s, a.lr, a.eps);
    a.m_mu[i] = m; a.v_mu[i] = v;
  }
  a.w_mu[i] = mu;
  m = a.m_sg[i]; v = a.v_sg[i];
  const float sg = adam1(a.w_sigma[i], __fmul_rn(g, nz), m, v, a.b1, a.b2, bc1, bc2s, a.lr, a.eps);
  a.m_sg[i] = m; a.v_sg[i] = v; a.w_sigma[i] = sg;
  store_eff<T>(static_cast<T*>(a.eff), row * a.eff_ld + col, merged(w, mu, sg, nz));
}

// W consecutive elements per thread (one 16- or 8-byte access per array); every tensor has cols % 4 == 0, n < 2^30 and
// 16-byte aligned rows (checked on the host), so a group never straddles a row. W = 4 (16-byte accesses, 72 registers) is the
// form that runs; W = 2 (8-byte accesses, 44 registers) fits into the 48 registers per SIMD lane the one-kernel actor
// (csrc/actor_fused.hip) leaves free and so runs BESIDE the policy kernel instead of waiting for it — measured slower in the
// loop (hb_noisy_adam_multi; DESIGN section 5c "Co-residency"), kept for measurements. Same arithmetic per element in every
// form (adam1's explicit roundings).
template <int W> struct VecW;
template <> struct VecW<4> { typedef float4 type; };
template <> struct VecW<2> { typedef float2 type; };
// (element offsets are 32-bit unsigned — the host checks n < 2^30 — so every access is "scalar base + 32-bit lane offset": one
//  address register per thread instead of a 64-bit pair per array)
template <int W>
__device__ __forceinline__ void ldw(const float* p, uint32_t off, float out[W]) {
  const typename VecW<W>::type v = *reinterpret_cast<const typename VecW<W>::type*>(reinterpret_cast<const char*>(p) + static_cast<uint64_t>(off << 2));
  const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
  for (int k = 0; k < W; ++k) out[k] = f[k];
}
template <int W>
__device__ __forceinline__ void stw(float* p, uint32_t off, const float in[W]) {
  typename VecW<W>::type v;
  float* f = reinterpret_cast<float*>(&v);
#pragma unroll
  for (int k = 0; k < W; ++k) f[k] = in[k];
  *reinterpret_cast<typename VecW<W>::type*>(reinterpret_cast<char*>(p) + static_cast<uint64_t>(off << 2)) = v;
}
template <int W>
__device__ __forceinline__ void load_gradw(const void* g, int dtype, uint32_t i, float out[W]) {
  if (dtype == 0) {
    ldw<W>(static_cast<const float*>(g), i, out);
  } else if (dtype == 1) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(static_cast<const char*>(g) + static_cast<uint64_t>(i << 1));
    if constexpr (W == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      out[0] = __uint_as_float(v.x << 16); out[1] = __uint_as_float(v.x & 0xFFFF0000u);
      out[2] = __uint_as_float(v.y << 16); out[3] = __uint_as_float(v.y & 0xFFFF0000u);
    } else {
      const uint32_t v = *p;
      out[0] = __uint_as_float(v << 16); out[1] = __uint_as_float(v & 0xFFFF0000u);
    }
  } else {
    const __half* h = reinterpret_cast<const __half*>(static_cast<const char*>(g) + static_cast<uint64_t>(i << 1));
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = __half2float(h[k]);
  }
}

// group q of tensor a: its W consecutive elements q * W .. q * W + W - 1 (the caller checks q < n / W)
template <typename T, int W>
__device__ __forceinline__ void step_group(const AdamArgs& a, int q, float bc1, float bc2s) {
  constexpr int SH = W == 4 ? 2 : 1;
  T* eff = static_cast<T*>(a.eff);
  const int cw = a.cols >> SH;
  const int row = q / cw, col = (q - row * cw) << SH;
  const uint32_t i = static_cast<uint32_t>(q) << SH;
  float g[W], nz[W];
  load_gradw<W>(a.grad, a.grad_dtype, static_cast<uint32_t>(row) * static_cast<uint32_t>(a.grad_ld) + col, g);
  ldw<W>(a.noise, i, nz);
  float res[3][W], lm[W], lv[W];
  auto one = [&](float* p, float* mp, float* vp, int which) {
    float pa[W], ma[W], va[W];
    ldw<W>(p, i, pa); ldw<W>(mp, i, ma); ldw<W>(vp, i, va);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      pa[k] = adam1(pa[k], which == 2 ? __fmul_rn(g[k], nz[k]) : g[k], ma[k], va[k], a.b1, a.b2, bc1, bc2s, a.lr, a.eps);
      res[which][k] = pa[k];
      lm[k] = ma[k];
      lv[k] = va[k];
    }
    stw<W>(p, i, pa); stw<W>(mp, i, ma); stw<W>(vp, i, va);
  };
  one(a.w, a.m_w, a.v_w, 0);

  if (a.m_mu == a.m_w) {  // shared moments: apply w's step to w_mu
    float pv[W];
    ldw<W>(a.w_mu, i, pv);
#pragma unroll
    for (int k = 0; k < W; ++k) res[1][k] = pv[k] = __fsub_rn(pv[k], adam_step(lm[k], lv[k], bc1, bc2s, a.lr, a.eps));
    stw<W>(a.w_mu, i, pv);
  } else {
    one(a.w_mu, a.m_mu, a.v_mu, 1);
  }

  one(a.w_sigma, a.m_sg, a.v_sg, 2);
  const uint32_t e = static_cast<uint32_t>(row) * static_cast<uint32_t>(a.eff_ld) + col;
#pragma unroll
  for (int k = 0; k < W; ++k) store_eff<T>(eff, e + k, merged(res[0][k], res[1][k], res[2][k], nz[k]));
}

// The workgroup's share of a multi-tensor step, 256 threads per workgroup: block (an index into m.first) of the W-wide form
// takes one group per thread; W = 1 is the scalar form, whose nb workgroups of a tensor stride over it.
template <typename T, int W>
__device__ __forceinline__ void step_block(const AdamMulti& m, int block, int tid) {
  int ti = 0;
  while (ti + 1 < m.count && block >= m.first[ti + 1]) ++ti;
  const AdamArgs& a = m.t[ti];
  float bc1, bc2s;
  bias_corrections(a, bc1, bc2s);
  if constexpr (W == 1) {
    const int nb = m.first[ti + 1] - m.first[ti];
    for (long long i = static_cast<long long>(block - m.first[ti]) * 256 + tid; i < a.n; i += static_cast<long long>(nb) * 256)
      step_element<T>(a, i, bc1, bc2s);
  } else {
    // (no grid-stride loop: the host launches one thread per group, so no address becomes a loop-carried 64-bit pointer)
    const int nw = static_cast<int>(a.n >> (W == 4 ? 2 : 1));
    const int q = (block - m.first[ti]) * 256 + tid;
    if (q < nw) step_group<T, W>(a, q, bc1, bc2s);
  }
}

// Host side of a multi-tensor launch: checks `count` entries of the caller's table and lays their workgroups out from block 0
// on (m.first). `width` = elements per thread asked for (4, 2 or 1); returns the width that runs — 1, the scalar form, when
// some tensor does not allow 16-byte accesses — or a negative error code. *blocks = workgroups of 256 threads in all.
inline int plan_multi(const hb_adam_tensor* tensors, int count, const float* step_dev, float step_offset, float lr, float beta1,
                      float beta2, float eps, int width, AdamMulti& m, int* blocks) {
  m.count = count;
  bool vec4 = width != 1;  // several elements per thread when every tensor allows 16-byte accesses
  for (int i = 0; i < count; ++i) {
    const hb_adam_tensor& d = tensors[i];
    const int gl = d.grad_ld ? d.grad_ld : d.cols;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    // (32-bit element offsets inside the vector kernels: n < 2^30, rows * row stride < 2^31)
    vec4 = vec4 && d.cols > 0 && d.cols % 4 == 0 && d.n % 4 == 0 && d.n < (1LL << 30) &&
           (d.n / d.cols) * static_cast<long long>(d.eff_ld > gl ? d.eff_ld : gl) < (1LL << 31) && d.eff_ld % 4 == 0 && gl % 4 == 0 && al16(d.w) &&
           al16(d.w_mu) && al16(d.w_sigma) && al16(d.noise) && al16(d.grad) && al16(d.m_w) && al16(d.v_w) && al16(d.m_mu) &&
           al16(d.v_mu) && al16(d.m_sigma) && al16(d.v_sigma);
  }
  if (!vec4) width = 1;
  int nblk = 0;
  for (int i = 0; i < count; ++i) {
    const hb_adam_tensor& d = tensors[i];
    if (!d.w || !d.w_mu || !d.w_sigma || !d.noise || !d.grad || !d.m_w || !d.v_w || !d.m_mu || !d.v_mu || !d.m_sigma ||
        !d.v_sigma || !d.eff)
      return hb::fail(HB_ERR_INVALID, "null pointer in tensor %d", i);
    if (d.n <= 0 || d.cols < 1 || d.eff_ld < d.cols || d.n % d.cols) return hb::fail(HB_ERR_INVALID, "bad shape in tensor %d", i);
    if (d.grad_dtype < 0 || d.grad_dtype > 2 || (d.grad_ld != 0 && d.grad_ld < d.cols))
      return hb::fail(HB_ERR_INVALID, "bad gradient dtype / row stride in tensor %d", i);
    m.t[i] = AdamArgs{d.w, d.w_mu, d.w_sigma, d.noise, d.grad, d.m_w, d.v_w, d.m_mu, d.v_mu, d.m_sigma, d.v_sigma,
                      step_dev, d.eff, d.n, d.cols, d.eff_ld, d.grad_dtype, d.grad_ld ? d.grad_ld : d.cols, lr, beta1, beta2, eps, step_offset};
    m.first[i] = nblk;
    long long nb = ((vec4 ? d.n / width : d.n) + 255) / 256;
    if (!vec4 && nb > 1024) nb = 1024;   // (the vector kernels take one group per thread, the scalar one strides)
    nblk += static_cast<int>(nb);
  }
  m.first[count] = nblk;
  *blocks = nblk;
  return width;
}

// learner2.hip: hb_noisy_adam_multi with a gradient-product entry (hb_adam_tensor.gx != NULL) — learner_tail_l2_dw1_kernel
int launch_tail(const hb_adam_tensor* steps, int n_steps, const hb_adam_tensor& prod, const float* step_dev, float step_offset,
                int eff_dtype, float lr, float beta1, float beta2, float eps, void* stream);

}  // namespace adam
}  // namespace hb

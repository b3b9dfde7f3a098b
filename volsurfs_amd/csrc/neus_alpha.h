// The NeuS alpha of one sample and its backward (volume_rendering_modules.py VolumeRenderingNeuS
// compute_alphas_from_logistic_beta), shared by surf_render.hip and offsets_render.hip so that both
// methods' fused kernels perform the same fp32 operations in the same order.  The build has
// -ffp-contract=off.
#pragma once
#include "ray_scan.h"

namespace vsa_ray {

// compute_alphas_from_logistic_beta (volume_rendering_modules.py) of one sample, each line one
// torch elementwise op of the reference in its order:
//   tc   = (d_0 g_0 + d_1 g_1) + d_2 g_2              (dirs * grad).sum(-1)
//   r1   = relu((-tc) 0.5 + 0.5),  r2 = relu(-tc)
//   ic   = -(r1 omc + r2 car)                          omc = fl32(1 - cos_anneal_ratio) on the host
//   h    = (ic dt) 0.5;  next = sdf + h;  prev = sdf - h
//   pc   = 1 / (1 + exp(-(prev beta))),  nc likewise  torch.sigmoid
//   q    = ((pc - nc) + 1e-6) / (pc + 1e-6);  alpha = min(max(q, 0), 1)
struct NeusAlpha {
  float tc, r1, r2, h, pc, nc, num, den, q, alpha;
};

__device__ __forceinline__ float alpha_value(const NeusAlpha& a) { return a.alpha; }  // ray_sweep.h

__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float sigmoid_torch(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ NeusAlpha neus_alpha(float sdf, const float* g, const float* dir, float dt,
                                                float car, float omc, float beta) {
  NeusAlpha a;
  float tc = dir[0] * g[0];
  tc = tc + dir[1] * g[1];
  a.tc = tc + dir[2] * g[2];
  a.r1 = relu((-a.tc) * 0.5f + 0.5f);
  a.r2 = relu(-a.tc);
  const float ic = -(a.r1 * omc + a.r2 * car);
  a.h = (ic * dt) * 0.5f;
  const float next = sdf + a.h, prev = sdf - a.h;
  a.pc = sigmoid_torch(prev * beta);
  a.nc = sigmoid_torch(next * beta);
  a.num = (a.pc - a.nc) + 1e-6f;
  a.den = a.pc + 1e-6f;
  a.q = a.num / a.den;
  a.alpha = fminf(fmaxf(a.q, 0.0f), 1.0f);
  return a;
}

// The autograd backward of neus_alpha from g_alpha, each line the derivative torch applies to the
// op above it (clamp passes the gradient where 0 <= q <= 1; relu passes none where its output is 0;
// a / b gives g / b and (-g) ((a / b) / b); sigmoid gives (g (1 - y)) y):
//   g_q  = clip mask;  g_num = g_q / den;  g_den = (-g_q) (q / den);  g_pc = g_num + g_den;  g_nc = -g_num
//   g_xp = (g_pc (1 - pc)) pc;  g_xn = (g_nc (1 - nc)) nc;  g_prev = g_xp beta;  g_next = g_xn beta
//   g_sdf = g_next + g_prev;  g_h = g_next + (-g_prev);  g_ic = (g_h 0.5) dt;  g_s = -g_ic
//   g_tc = (-((relu' (g_s omc)) 0.5)) + (-(relu' (g_s car)));  g_grad_d = g_tc d_d
__device__ __forceinline__ void neus_alpha_bwd(const NeusAlpha& a, float g_alpha, const float* dir,
                                               float dt, float car, float omc, float beta,
                                               float& g_sdf, float g_grad[3]) {
  const float g_q = (a.q >= 0.0f && a.q <= 1.0f) ? g_alpha : 0.0f;
  const float g_num = g_q / a.den;
  const float g_den = (-g_q) * (a.q / a.den);
  const float g_pc = g_num + g_den;
  const float g_nc = -g_num;
  const float g_prev = ((g_pc * (1.0f - a.pc)) * a.pc) * beta;
  const float g_next = ((g_nc * (1.0f - a.nc)) * a.nc) * beta;
  g_sdf = g_next + g_prev;
  const float g_h = g_next + (-g_prev);
  const float g_s = -((g_h * 0.5f) * dt);
  const float g_u1 = a.r1 > 0.0f ? g_s * omc : 0.0f;
  const float g_u2 = a.r2 > 0.0f ? g_s * car : 0.0f;
  const float g_tc = (-(g_u1 * 0.5f)) + (-g_u2);
#pragma unroll
  for (int d = 0; d < 3; ++d) g_grad[d] = g_tc * dir[d];
}

}  // namespace vsa_ray

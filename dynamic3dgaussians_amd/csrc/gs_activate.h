// gs_activate.h -- F.normalize of a quaternion row, forward and backward, in
// the operation order of torch's kernels for the same ops.  Shared by the
// preprocess kernels' GS_FLAG_ACTIVATE path (gs_preprocess.hip) and the scene
// regularisers' raw-rotation path (gs_scene_loss.hip); both files are compiled
// without fma contraction, so the two agree bit for bit.
//
// F.normalize = q / max(|q|, 1e-12) (torch.nn.functional.normalize, p = 2,
// dim = 1).  The squared norm is summed pairwise, (x^2 + y^2) + (z^2 + w^2):
// the order that reproduces torch's GPU reduction bit for bit
// (tools/act_probe.py on an MI355X: 100 % of 400k quaternions vs 88 % for the
// sequential sum, profiles/r04b/act_probe.txt).
#pragma once

#include <hip/hip_runtime.h>

namespace gs {

constexpr float NORMALIZE_EPS = 1e-12f;
__device__ inline float act_norm(float4 q) { return sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w)); }
__device__ inline float4 act_normalize(float4 q) {
  const float d = fmaxf(act_norm(q), NORMALIZE_EPS);
  return make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}
// dL/dq of q_hat = q / max(|q|, eps) for the upstream gradient gq of q_hat:
// DivBackward (g / d for q, -g (q / d) / d summed for the denominator),
// ClampMinBackward (passes where |q| >= eps), NormBackward (q (g_n / |q|)).
__device__ inline float4 act_normalize_bwd(float4 q, float4 gq) {
  const float n = act_norm(q);
  const float d = fmaxf(n, NORMALIZE_EPS);
  const float gd = (-gq.x * ((q.x / d) / d) + -gq.y * ((q.y / d) / d)) +
                   (-gq.z * ((q.z / d) / d) + -gq.w * ((q.w / d) / d));
  const float gn = (n >= NORMALIZE_EPS && n != 0.0f) ? gd / n : 0.0f;
  return make_float4(gq.x / d + q.x * gn, gq.y / d + q.y * gn, gq.z / d + q.z * gn, gq.w / d + q.w * gn);
}

}  // namespace gs

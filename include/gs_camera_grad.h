/*
 * gs_camera_grad.h -- gradients of a camera batch's view matrices, projection
 * matrices and camera positions (no reference analogue: the reference's
 * rasterizer treats its cameras as constants; its pose metric,
 * metrics.py:46-79 compute_pose_errors, is fed by poses estimated elsewhere).
 *
 * gs_backward_batch(_window) leaves, in its scratch, one accumulation record
 * per (camera, Gaussian): the blend backward's sums, from which the preprocess
 * backward forms the gradient of the NDC mean, of the depth, of the EWA matrix
 * rows and of the SH view direction, multiplies them by the camera and writes
 * them per Gaussian.  gs_camera_grad_batch multiplies the same quantities by
 * the homogeneous mean instead and reduces them over the Gaussians: the exact
 * derivative of the compat = fixed forward with respect to the 16 + 16 + 3
 * camera numbers of every camera.
 *
 * With p = (x, y, z, 1) the mean at the camera's frame, v / pr the camera's
 * view / projection matrix (v[4 i + j]: input i, output j), t_j = sum_i p_i
 * v[4 i + j], h_j = sum_i p_i pr[4 i + j] and mw = 1 / (h_3 + 1e-7), every
 * pair with radius > 0 adds
 *
 *   dL_dproj[4 i + 0] += p_i mw am0          (am: gradient of the NDC mean)
 *   dL_dproj[4 i + 1] += p_i mw am1
 *   dL_dproj[4 i + 3] -= p_i mw^2 (h_0 am0 + h_1 am1)
 *   dL_dview[4 i + j] += p_i dL/dt_j         (i = 0..3, j = 0..2; dL/dt =
 *                                             (dtx, dty, dtz + dL/ddepth))
 *   dL_dview[4 r + 0] += j00 dT0[r]          (r = 0..2: the EWA rows A = J W,
 *   dL_dview[4 r + 1] += j11 dT1[r]           dT0 / dT1 the gradients of A's
 *   dL_dview[4 r + 2] += j02 dT0[r] + j12 dT1[r]                   two rows)
 *   dL_dcampos        -= the SH view-direction term of the mean gradient
 *
 * dtx, dty, dtz, dT0, dT1 are the preprocess backward's, with one difference:
 * for a mean inside the frustum clamp (Q9) dtz carries the exact derivative of
 * the clamped Jacobian entry (one h t / t_z^3 where the per-Gaussian backward
 * keeps the reference's two), so that the result is the derivative there too.
 * Column 3 of dL_dview and column 2 of dL_dproj are 0: the forward reads
 * neither.  The tan(fov / 2) and principal point scalars of gs_camera are not
 * differentiated (the EWA focal lengths are constants), so dL_dproj serves the
 * chain view -> view @ P of a pose, not the refinement of intrinsics.  With a
 * tile window (gs_camera tile_*) the gradient is that of the window's pixels.
 * grad_mask (the Q12 label) masks per-Gaussian gradients and is not applied.
 *
 * Sums: each thread adds its pairs in fp64, the workgroup's threads are summed
 * in a fixed order into one fp64 record per (camera, workgroup) in the
 * workspace, a second kernel adds each camera's records in index order and
 * rounds once to fp32.  No atomics: the result does not depend on scheduling.
 *
 * GS_ABI_VERSION does not change: no existing struct or entry point does.
 */
#ifndef GS_CAMERA_GRAD_H
#define GS_CAMERA_GRAD_H

#include "gs_window.h"
#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_CAMERA_GRAD_MAX_CAMS 64 /* the camera batch's limit */

/* Bytes of gs_camera_grad_batch's workspace for P Gaussians and C cameras
 * (0 when P <= 0 or C is outside 1..GS_CAMERA_GRAD_MAX_CAMS). */
size_t gs_camera_grad_workspace_bytes(int64_t P, int32_t C);

/* Host-only validation of gs_camera_grad_batch's own arguments (what it runs
 * first): rejects P < 0, C outside 1..GS_CAMERA_GRAD_MAX_CAMS, compat =
 * reference (0: its backward runs on the wrapper's swapped camera scalars and
 * its EWA terms are not derivatives of its forward), a null or misaligned
 * output and a workspace that is missing, misaligned or smaller than
 * gs_camera_grad_workspace_bytes(P, C).  0 when valid; else nonzero with the
 * message in gs_last_error(). */
int gs_check_camera_grad(int64_t P, int32_t C, int compat, const void *workspace, uint64_t workspace_bytes,
                         const float *dL_dview, const float *dL_dproj, const float *dL_dcampos);

/* After gs_backward_batch(_window) on the same stream, with the same
 * Gaussians, cameras, window (NULL = none), radii, compat, geometry buffer and
 * the backward's scratch as that call left it (nothing else may have written
 * it since).  Writes EVERY element of dL_dview [C,16], dL_dproj [C,16] and
 * dL_dcampos [C,3] (fp32, the layout of the inputs): zeros for a camera that
 * sees nothing, for P = 0 (no state buffer is then read) and, for dL_dcampos,
 * without SHs.  Of gs_gaussians it reads P, D, M, means3D, shs and
 * cov3D_precomp. */
int gs_camera_grad_batch(const gs_gaussians *g, const gs_camera *cams, int32_t C, const gs_window *win,
                         const int32_t *radii, int compat, const void *geom_buffer, const void *scratch,
                         void *workspace, uint64_t workspace_bytes, float *dL_dview, float *dL_dproj,
                         float *dL_dcampos, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_CAMERA_GRAD_H */

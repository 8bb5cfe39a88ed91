/*
 * gs_window.h -- temporal-window camera batches (no reference analogue as an
 * interface; the reference's motion-basis loop renders frame t's cameras at
 * positions[:, t] one call at a time, dyn_train.py:422-457).
 *
 * A camera batch (gsplat_hip.h gs_*_batch) may carry a window of B frames:
 *
 *  - g->means3D is P x B x 3 fp32, contiguous, Gaussian-major -- frame b of
 *    Gaussian i at 3 (i B + b), the layout gs_motion_forward writes
 *    (gs_motion.h `positions`).
 *  - camera c reads frame win->cam_frame[c].  It is projected, culled, binned
 *    and blended exactly as gs_*_batch would do it with means3D holding that
 *    frame's P x 3 means.  Every other per-Gaussian input (opacities, scales,
 *    rotations, cov3D_precomp, colours or SH, semantic features, grad_mask,
 *    GS_FLAG_ACTIVATE) is shared by all frames: the window moves the means
 *    only.
 *  - cam_frame is non-decreasing: the cameras are grouped by frame, so the
 *    backward's one thread per Gaussian walks them once and stores a frame's
 *    mean gradient when the frame changes.  The outputs are stacked in the
 *    caller's camera order; the caller sorts its cameras by frame.
 *  - Backward: dL_dmeans3D is P x B x 3, every element written once (added to
 *    with GS_FLAG_ACCUMULATE).  Frame b receives the sum over the cameras of
 *    frame b, in camera order, the first of them that sees the Gaussian
 *    assigning; frames without a camera and Gaussians unseen in a frame
 *    receive zeros (times grad_mask, like every masked gradient).  All other
 *    gradients are summed over all cameras of all frames, as in
 *    gs_backward_batch, and so are the densification statistics
 *    (gs_gaussians.densify_*): a Gaussian seen by cameras of several frames
 *    counts once per camera.
 *
 * GS_ABI_VERSION does not change: gs_gaussians, gs_camera and gs_batch_hint
 * are untouched and every existing entry point keeps its meaning (it is the
 * win == NULL case of its *_window form: B = 1, every frame 0).
 *
 * gs_forward_render_batch has no window form: binning, sort and blend work
 * from the per-camera records the plan wrote and never read the means, so it
 * serves both cases (the retry of gs_forward_batch_window included).
 * gs_spatial_order likewise: hand it one frame's P x 3 means.
 */
#ifndef GS_WINDOW_H
#define GS_WINDOW_H

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_WINDOW_MAX_FRAMES 64

typedef struct gs_window {
  int32_t B;                /* frames per Gaussian in means3D, 1 .. GS_WINDOW_MAX_FRAMES */
  const int32_t *cam_frame; /* host, C entries, each in [0, B), non-decreasing */
} gs_window;

/* Host-only validation of a window for a batch of C cameras (what the entry
 * points below run first): rejects a null window or frame array, B outside
 * [1, GS_WINDOW_MAX_FRAMES], C < 1, a frame outside [0, B) and a decreasing
 * sequence.  0 when valid; else nonzero with the message in gs_last_error(). */
int gs_check_window(const gs_window *w, int32_t C);

/* gs_forward_plan_batch / gs_forward_batch / gs_backward_batch with a window
 * (`win`, before the stream; NULL = the call without one). */
int gs_forward_plan_batch_window(const gs_gaussians *g, const gs_camera *cams, int32_t C,
                                 int prefiltered, int debug, int compat, void *geom_buffer,
                                 void *image_buffer, int32_t *radii, int64_t *num_rendered,
                                 int64_t *num_instances, const gs_window *win, gs_stream_t stream);

int gs_forward_batch_window(const gs_gaussians *g, const gs_camera *cams, int32_t C, int prefiltered,
                            int compat, void *geom_buffer, void *image_buffer, void *binning_buffer,
                            const int64_t *capacity, gs_batch_hint *hint, int32_t *radii,
                            int64_t *num_rendered, int64_t *num_instances, int32_t *fits,
                            float *out_color, float *out_feature, float *out_depth, float *out_alpha,
                            const gs_window *win, gs_stream_t stream);

int gs_backward_batch_window(const gs_gaussians *g, const gs_camera *cams, int32_t C,
                             const int32_t *radii, int debug, int compat, const void *geom_buffer,
                             const void *binning_buffer, const void *image_buffer,
                             const int64_t *num_instances, const float *alphas,
                             const float *dL_dout_color, const float *dL_dout_feature,
                             const float *dL_dout_depth, const float *dL_dout_alpha, void *scratch,
                             float *dL_dmeans2D, float *dL_dcolors, float *dL_dsemantic,
                             float *dL_dopacity, float *dL_dmeans3D, float *dL_dcov3D, float *dL_dsh,
                             float *dL_dscales, float *dL_drotations, const gs_window *win,
                             gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_WINDOW_H */

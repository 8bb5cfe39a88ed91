/*
 * gs_track.h -- point tracking on a rendered camera batch: which Gaussians a
 * pixel is made of (top-K contributor maps) and where chosen Gaussians land in
 * every camera at every timestep (track projection).  The evaluation side of
 * the reference's tracking (metrics.py:489-520 PCK, dyn_som.py:171-230
 * get_tracks_3d) needs 2-D tracks; the reference has no kernel that produces
 * them: its forward throws the blended ids away like ours.
 *
 * Contributor maps.  The forward blends, per pixel, the entries of the pixel's
 * tile list that pass its decision chain: an entry is skipped when power > 0
 * or alpha < 1/255, the walk ends at the first entry whose test_T = T (1 -
 * alpha) < 1e-4 (that entry is not blended), every other entry blends with the
 * weight w = alpha T.  gs_contributors_batch repeats that walk on the state
 * the forward left, with the forward's own expressions, and keeps for every
 * pixel the K entries of largest w:
 *
 *   top_id[c, k, y, x]  the Gaussian with the k-th largest w, -1 when fewer
 *                       than k + 1 entries blended
 *   top_w [c, k, y, x]  that w, 0 where the id is -1
 *
 * Between equal weights the entry earlier in the tile list (the nearer one)
 * ranks first.  Pixels outside a camera's tile window (gs_camera tile_*) hold
 * -1 / 0 at every rank.  Both compat modes blend the same entries, so the maps
 * do not depend on compat.  No atomics: two runs give the same bits.  In
 * compat = fixed the forward's alpha image is the sum of ALL blended w of the
 * pixel, so sum_k top_w <= alpha up to the rounding of that sum.
 *
 * Track projection.  For timestep t, camera c and track n the mean
 * means3D[t, ids[n]] goes through camera c exactly as the forward's preprocess
 * projects it: uv [t, c, n] is what the forward stores as means2D (pixel
 * centres at integers) and depth [t, c, n] its view-space z, bit for bit.
 * inside [t, c, n] is 1 when the point is in front of the camera (the
 * forward's frustum test, z > 0) and floor(uv + 0.5) lies in [0, W) x [0, H).
 * ids[n] < 0 (no Gaussian: a query on empty background) writes uv = depth = 0
 * and inside = 0.  An id >= P is a caller's error that only a host-visible id
 * array could be checked for; on the device it is clamped to P - 1 and flagged
 * inside = 0, never dereferenced out of range.
 *
 * GS_ABI_VERSION does not change: no existing struct or entry point does.
 */
#ifndef GS_TRACK_H
#define GS_TRACK_H

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_TRACK_MAX_K 4     /* ranks kept per pixel */
#define GS_TRACK_MAX_CAMS 64 /* the camera batch's limit */

/* Host-only validation of gs_contributors_batch's own arguments (what it runs
 * first): rejects P outside [0, 2^31), C outside 1..GS_TRACK_MAX_CAMS, K
 * outside 1..GS_TRACK_MAX_K, W or H < 0, C K H W beyond 2^62 elements (the
 * kernel indexes with 64 bits) and, when there is an element to write, a null
 * or misaligned output.  0 when valid; else nonzero with the message in
 * gs_last_error(). */
int gs_check_contributors(int64_t P, int32_t C, int32_t W, int32_t H, int32_t K, const int32_t *top_id,
                          const float *top_w);

/* After gs_forward_render(_batch) / gs_forward_batch (fits = 1, or its retry)
 * on the same stream, with the same cameras and with the state buffers and
 * num_instances as that call left them (what gs_backward_batch takes).  Writes
 * EVERY element of top_id and top_w [C, K, H, W].  P = 0 or no instance at
 * all: -1 / 0 everywhere, and no state buffer is read.  The single-camera
 * state is the C = 1 case.  `compat` is validated (0 or 1) and otherwise
 * unused. */
int gs_contributors_batch(const gs_camera *cams, int32_t C, int64_t P, int compat, const void *geom_buffer,
                          const void *binning_buffer, const void *image_buffer, const int64_t *num_instances,
                          int32_t K, int32_t *top_id, float *top_w, gs_stream_t stream);

/* Host-only validation of gs_track_project's own arguments: rejects P outside
 * [0, 2^31), T < 0, N < 0, C outside 1..GS_TRACK_MAX_CAMS, T C N beyond 2^62
 * and, when there is an element to write, null ids or a null or misaligned
 * output (uv 8-byte, depth 4-byte aligned). */
int gs_check_track_project(int64_t P, int32_t T, int32_t C, int64_t N, const int32_t *ids, const float *uv,
                           const float *depth, const uint8_t *inside);

/* means3D [T, P, 3] and ids [N] on the device; the cameras as a batch takes
 * them (matrices contiguous [C,16] / [C,16], one image size).  Writes EVERY
 * element of uv [T, C, N, 2], depth [T, C, N] and inside [T, C, N].  P = 0:
 * zeros, means3D is not read. */
int gs_track_project(const gs_camera *cams, int32_t C, int64_t P, int32_t T, const float *means3D,
                     const int32_t *ids, int64_t N, float *uv, float *depth, uint8_t *inside, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_TRACK_H */

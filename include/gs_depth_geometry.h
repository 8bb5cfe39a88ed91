/* gs_depth_geometry.h -- C ABI of the geometry on depth maps: the point
 * z-buffer and the mMDE score, dense unprojection, depth-induced optical flow
 * and one bilinear border sampler.  Exported by the same libgsplat_hip.so as
 * gsplat_hip.h.  Forward only.
 *
 * Replaces the PyTorch of the reference's unproject_image / mMDE
 * (metrics.py:131-213, 254-292), depth2point_cam / depth2point_world
 * (dyn_utils.py:442-480), pixel_to_camera_coordinates,
 * camera_to_world_coordinates, compute_optical_flow, warp_flow and
 * accumulate_flows (ideaII.py:102-206) and the track lifting of
 * dyn_som.py:268-286.
 *
 * Conventions.  All device data is contiguous fp32 unless stated.  Matrices
 * are row-major as torch stores them: K and Kinv are [B, 3, 3] (9 floats per
 * camera), w2c, c2w and T are [B, 4, 4] (16 floats; only the first three rows
 * are read).  A pixel's coordinates are (x, y) = (column, row).  Every struct
 * shares its name with its entry point (the struct is always written
 * `struct gs_...`).  Every call is asynchronous on `stream`, reads nothing
 * back, allocates nothing, uses no floating-point atomic and returns 0 or an
 * error code with gs_last_error() set (as gsplat_hip.h).  Each call runs its
 * _validate function (host code, no device access) first.
 *
 * gs_point_depth: the nearest point per pixel.  Per camera b and point p, in
 * fp32:
 *
 *   c = w2c[b] (p, 1);  rejected unless c.z > 0
 *   q = K[b] c;  u = q.x / q.z,  v = q.y / q.z
 *   px = rintf(u), py = rintf(v)   (round half to even, as torch.round)
 *   rejected unless 0 <= px < W and 0 <= py < H, tested in float before the
 *   conversion to int with comparisons that are false for NaN (so NaN, inf
 *   and values beyond the int range never become an index)
 *   depth[b][py][px] = min(depth[b][py][px], c.z)
 *
 * depth is first filled with +inf (one launch); a second launch runs one
 * thread per (camera, point) and takes the minimum with a 32-bit integer
 * atomic on the bit pattern of c.z: positive floats order as their bits and
 * +inf is the largest of them, so the integer minimum is the float minimum.
 * It does not depend on the order of arrival: reruns are bit-identical.
 * points is [P, 3] shared by all cameras (points_batch_stride 0) or
 * [B, P, 3], one cloud per camera (points_batch_stride P * 3).  P = 0 gives
 * an all-inf map.  Bytes from shapes: 4 B H W written by the fill, 12 B P
 * read and up to B P four-byte atomics by the second launch.  Time model:
 * none derived -- the rate of integer min atomics is not a documented figure
 * of the chip, so the launch's time is a measurement only
 * (tools/depth_geometry_bench.py, profiles/depth_geometry/bench.json: 0.32 ms
 * for 300k points x 27 cameras of 800 x 800, 7.96 M atomics issued, about
 * 10 % of the streaming rate under the byte model: bound by the atomics).
 *
 * gs_depth_abs_rel: the mMDE score's sums.  A pixel is valid iff est is
 * finite, gt > 0 and exclude != 1 (the reference's (1 - mask).bool();
 * exclude is optional, [H, W] with exclude_batch_stride 0 or [B, H, W] with
 * H * W).  Its term |gt - est| / gt is taken in fp32; a workgroup adds its
 * terms in fp64 and writes one partial, and a second kernel adds an image's
 * partials in index order in fp64.  out[b] = {sum, count} as fp64; the
 * caller divides (0 / 0 = NaN for an image with no valid pixel, as
 * torch.mean of an empty tensor).  Two calls give the same bits.  Bytes: 8
 * or 12 per pixel read.
 *
 * gs_depth_unproject: xyz = c2w (depth * Kinv (x, y, 1), 1) per pixel,
 * [B, H, W, 3].  With xy == NULL, (x, y) is the pixel's (column, row).  With
 * xy [B, H * W, 2] the coordinates are read from it (sparse form: H = 1,
 * W = N points, depth [B, N] sampled by the caller).  Bytes: 4 read (12 with
 * xy), 12 written per pixel.
 *
 * gs_depth_flow: c2 = T (depth1 * Kinv1 (x, y, 1), 1), q = K2 c2,
 * uv = q.xy / max(q.z, 1e-7) (the reference's clamp(min=1e-7), kept),
 * flow[b][0] = uv.x - x, flow[b][1] = uv.y - y; valid[b] (uint8, optional)
 * = depth1 > 0 && q.z > 1e-7.  T = w2c2 c2w1 is composed by the caller.
 * Bytes: 4 read, 8 (9 with valid) written per pixel.
 *
 * gs_sample_bilinear: src [B, Ch, H, W] sampled as
 * F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True)
 * at pixel coordinates: x is clamped to [0, W - 1] and y to [0, H - 1],
 * x0 = min(floor(x), W - 2) (0 when W == 1), likewise y0, and the four taps
 * are blended with weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty.
 * A NaN coordinate gives a NaN output (and reads src[..][0][0] only).
 * mode GS_SAMPLE_POINTS: coords is xy [B, N, 2], out is [B, Ch, N].
 * mode GS_SAMPLE_DISPLACEMENT: coords is disp [B, 2, h, w], the coordinate of
 * output pixel (x, y) is (x + disp[b][0][y][x], y + disp[b][1][y][x]), out is
 * [B, Ch, h, w] and N must be h * w; with add_displacement != 0 (Ch == 2
 * only) out = disp + sample, one step of the reference's accumulate_flows.
 * Bytes: 8 read per output position, 4 Ch written, and 16 Ch gathered (the
 * taps; neighbours share cache lines, so this is an upper bound). */
#ifndef GS_DEPTH_GEOMETRY_H
#define GS_DEPTH_GEOMETRY_H

#include <stddef.h>
#include <stdint.h>

#include "gsplat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GS_SAMPLE_POINTS 0
#define GS_SAMPLE_DISPLACEMENT 1

struct gs_point_depth {
  int64_t P;                    /* points per cloud (>= 0) */
  int32_t B, H, W;              /* cameras, rows, columns (all > 0) */
  int32_t _pad;
  const float *points;          /* [P, 3] or [B, P, 3]; may be NULL when P == 0 */
  int64_t points_batch_stride;  /* floats between the clouds of two cameras: 0 or P*3 */
  const float *w2c;             /* [B, 16] */
  const float *K;               /* [B, 9] */
  float *depth;                 /* [B, H, W], +inf where no point lands */
};

struct gs_depth_abs_rel {
  int32_t B, H, W;              /* images, rows, columns (all > 0) */
  int32_t _pad;
  const float *est;             /* [B, H, W] */
  const float *gt;              /* [B, H, W] */
  const float *exclude;         /* optional [H, W] or [B, H, W]; a pixel with exclude == 1 is left out */
  int64_t exclude_batch_stride; /* floats between the masks of two images: 0 or H*W */
  double *out;                  /* [B, 2] fp64: sum of terms, count of valid pixels */
  void *workspace;              /* gs_depth_abs_rel_workspace_bytes(B, H, W) bytes */
  uint64_t workspace_bytes;     /* size of the buffer behind `workspace` */
};

struct gs_depth_unproject {
  int32_t B, H, W;              /* cameras, rows, columns (all > 0) */
  int32_t _pad;
  const float *depth;           /* [B, H, W] */
  const float *xy;              /* optional [B, H*W, 2]: coordinates in place of (column, row) */
  const float *Kinv;            /* [B, 9] */
  const float *c2w;             /* [B, 16] */
  float *xyz;                   /* [B, H, W, 3] */
};

struct gs_depth_flow {
  int32_t B, H, W;              /* camera pairs, rows, columns (all > 0) */
  int32_t _pad;
  const float *depth1;          /* [B, H, W] */
  const float *Kinv1;           /* [B, 9] */
  const float *T;               /* [B, 16]: w2c2 c2w1 */
  const float *K2;              /* [B, 9] */
  float *flow;                  /* [B, 2, H, W] */
  uint8_t *valid;               /* optional [B, H, W] */
};

struct gs_sample_bilinear {
  int32_t B, Ch, H, W;          /* the source (all > 0) */
  int32_t mode;                 /* GS_SAMPLE_POINTS or GS_SAMPLE_DISPLACEMENT */
  int32_t add_displacement;     /* DISPLACEMENT and Ch == 2 only: out = disp + sample */
  int64_t N;                    /* output positions per image (> 0); h*w in DISPLACEMENT mode */
  int32_t h, w;                 /* DISPLACEMENT: the output grid (> 0); POINTS: ignored */
  const float *src;             /* [B, Ch, H, W] */
  const float *coords;          /* POINTS: xy [B, N, 2]; DISPLACEMENT: disp [B, 2, h, w] */
  float *out;                   /* [B, Ch, N] */
};

/* sizeof each struct as the library was compiled (for binding mirrors). */
size_t gs_point_depth_struct_bytes(void);
size_t gs_depth_abs_rel_struct_bytes(void);
size_t gs_depth_unproject_struct_bytes(void);
size_t gs_depth_flow_struct_bytes(void);
size_t gs_sample_bilinear_struct_bytes(void);

/* Workspace of one gs_depth_abs_rel call: one fp64 sum and one fp64 count per
 * workgroup.  0 for non-positive shapes. */
size_t gs_depth_abs_rel_workspace_bytes(int32_t B, int32_t H, int32_t W);

/* The argument checks the entry points run first (host code, no device access). */
int gs_point_depth_validate(const struct gs_point_depth *args);
int gs_depth_abs_rel_validate(const struct gs_depth_abs_rel *args);
int gs_depth_unproject_validate(const struct gs_depth_unproject *args);
int gs_depth_flow_validate(const struct gs_depth_flow *args);
int gs_sample_bilinear_validate(const struct gs_sample_bilinear *args);

int gs_point_depth(const struct gs_point_depth *args, gs_stream_t stream);
int gs_depth_abs_rel(const struct gs_depth_abs_rel *args, gs_stream_t stream);
int gs_depth_unproject(const struct gs_depth_unproject *args, gs_stream_t stream);
int gs_depth_flow(const struct gs_depth_flow *args, gs_stream_t stream);
int gs_sample_bilinear(const struct gs_sample_bilinear *args, gs_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GS_DEPTH_GEOMETRY_H */

// gs_track.hip -- point tracking on a rendered camera batch
// (include/gs_track.h): the top-K contributor maps and the track projection.
// No reference analogue: the reference's forward (DGR/cuda_rasterizer/
// forward.cu:274-408) keeps no ids either, and its tracking evaluation
// (metrics.py:489-520, dyn_som.py:171-230) is fed from elsewhere.
//
// contributors_kernel is render_fwd_kernel (gs_render.hip) at F = 0 with the
// colour sums replaced by a K-entry insertion: the same geometry (a wave per
// 8x8 strip, lane = pixel, a strip per workgroup), the same dispatch
// (strip_of_block over the plan's order table), the same chunked walk (records
// staged through LDS, prefetched one chunk ahead, ids two), the same strip
// cull and the same power / alpha / test_T expressions (gs_blend.h), so every
// lane takes the forward's decisions and forms the forward's w = alpha T bit
// for bit.  It reads no colour, depth or feature and writes 8 K bytes per
// pixel; the matrix cores are not used.  The K best (w, id) pairs of a lane
// live in registers: K is a template parameter and the insertion is a chain of
// selects over named array elements in fully unrolled loops (a dynamically
// indexed array would go to scratch).  No atomics.
//
// track_project_kernel: a thread per (t, c, n), n fastest; the projection is
// preprocess_fwd_kernel's (gs_preprocess.hip) through the functions of
// gs_project.h.  Compiled with -ffp-contract=off like that file, so uv and
// depth are its means2D and depths bit for bit; the walk helpers of gs_blend.h
// contain no contractable expression (their multiply-adds are explicit fmaf),
// and neither does the decision chain below.
#include "gs_blend.h"
#include "gs_common.h"
#include "gs_kernels.h"
#include "gs_project.h"

namespace gs {

// Waves per SIMD asked of the register allocator: 8 (<= 64 VGPRs), which every
// K fits without scratch (DESIGN.md 9.14 has the compiler's report).
template <int K>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void contributors_kernel(ContribArgs a0,
                                                                                                      CamBatch cb) {
  int cam, item;
  strip_of_block(blockIdx.x, cb.C, num_tiles_of(a0), cam, item);
  const int W = a0.W, H = a0.H, grid_x = a0.grid_x, ks = a0.K;  // ks <= K ranks are stored
  const size_t HW = (size_t)H * W;
  const uint4* __restrict__ order = shift_bytes(a0.order, cam * cb.img_stride);
  const uint32_t* __restrict__ point_list = shift_bytes(a0.point_list, cb.bin_off[cam]);
  const float* __restrict__ rec = shift_bytes(a0.rec, cam * cb.geom_stride);
  int32_t* __restrict__ top_id = a0.top_id + (size_t)cam * ks * HW;
  float* __restrict__ top_w = a0.top_w + (size_t)cam * ks * HW;
  // per record: (x, y, -a/2, -b) (-c/2, opacity, id bits, -)
  __shared__ float4 s_rec[CHUNK][2];

  const int lane = threadIdx.x & 63;
  const uint4 trec = tile_rec(order, item >> 2);
  const int tile = (int)trec.x, wave = item & 3;
  const int tx = tile % grid_x, ty = tile / grid_x;
  const int qx0 = strip_x0(tx, wave), qy0 = strip_y0(ty, wave);
  const int px = qx0 + lane % STRIP_W, py = qy0 + lane / STRIP_W;
  const bool inside = px < W && py < H;
  const float pfx = (float)px, pfy = (float)py;
  const float sx0 = (float)qx0, sx1 = sx0 + (float)(STRIP_W - 1);
  const float sy0 = (float)qy0, sy1 = sy0 + (float)(STRIP_H - 1);
  const uint2 range = make_uint2(trec.y, trec.z);

  float tw[K];
  int32_t ti[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    tw[k] = 0.f;
    ti[k] = -1;
  }
  float T = 1.0f;
  uint32_t live = inside ? 1u : 0u;  // the forward's `live`: an integer, so that it stays in a VGPR

  // One survivor at the pixel: the forward's blend_step without the sums.
  // A blending entry has w >= 1e-4 / 255 > 0 and every kept w is >= 0, so a
  // lane that does not blend (w = 0) inserts nothing; `>`: between equal
  // weights the earlier entry keeps its rank.
  auto step = [&](float power, float alpha, int32_t gid) {
    const float test_T = T * (1 - alpha);
    const bool cand = live != 0u && !(power > 0.0f) && !(alpha < ALPHA_MIN);
    const bool fin = cand && test_T < 0.0001f;  // saturated: not blended, lane done
    const bool blend = cand && !fin;
    live = fin ? 0u : live;
    const float w = blend ? alpha * T : 0.0f;
    T = blend ? test_T : T;
    bool gt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gt[k] = w > tw[k];
#pragma unroll
    for (int k = K - 1; k > 0; --k) {
      tw[k] = gt[k - 1] ? tw[k - 1] : (gt[k] ? w : tw[k]);
      ti[k] = gt[k - 1] ? ti[k - 1] : (gt[k] ? gid : ti[k]);
    }
    tw[0] = gt[0] ? w : tw[0];
    ti[0] = gt[0] ? gid : ti[0];
  };

  if (in_window(cb, cam, tx, ty) && range.y > range.x) {
    const uint32_t lastv = range.y - 1;
    RecRegs q = load_rec(point_list, rec, range.x + lane, lastv);
    uint32_t gnext = load_gid(point_list, range.x + CHUNK + lane, lastv);
    if (wave_any(live != 0u)) {
      for (uint32_t c0 = range.x; c0 < range.y; c0 += CHUNK) {
        const bool keep = (c0 + lane < range.y) && !strip_culled(q, sx0, sx1, sy0, sy1);
        {
          const float4 h = half_conic(q.q0, q.q1);
          s_rec[lane][0] = make_float4(q.q0.x, q.q0.y, h.x, h.y);
          s_rec[lane][1] = make_float4(h.z, q.q1.y, __uint_as_float(q.gid), 0.f);
        }
        uint64_t mask = __ballot(keep);
        q = load_rec_gid(rec, gnext);                                // next chunk (clamped)
        gnext = load_gid(point_list, c0 + 2 * CHUNK + lane, lastv);   // the one after
        bool done = false;
        // two survivors per iteration, evaluated side by side and blended in
        // order; a missing second survivor gets power = +1 (never blends)
        while (mask) {
          const int ja = __builtin_ctzll(mask);
          mask &= mask - 1;
          const bool two = mask != 0;
          const int jb = two ? __builtin_ctzll(mask) : ja;
          if (two) mask &= mask - 1;
          const float4 r0a = s_rec[ja][0], r1a = s_rec[ja][1];
          const float4 r0b = s_rec[jb][0], r1b = s_rec[jb][1];
          const float pa = gauss_power(r0a.x - pfx, r0a.y - pfy, make_float4(r0a.z, r0a.w, r1a.x, 0.f));
          float pb = gauss_power(r0b.x - pfx, r0b.y - pfy, make_float4(r0b.z, r0b.w, r1b.x, 0.f));
          pb = two ? pb : 1.0f;
          const float ala = fminf(0.99f, r1a.y * gauss_exp(pa));
          const float alb = fminf(0.99f, r1b.y * gauss_exp(pb));
          step(pa, ala, (int32_t)__float_as_uint(r1a.z));
          step(pb, alb, (int32_t)__float_as_uint(r1b.z));
          if (!wave_any(live != 0u)) {
            done = true;
            break;
          }
        }
        if (done) break;
      }
    }
  }
  // planar stores, a strip row (8 pixels, 32 B) contiguous per rank; a pixel
  // outside the window or with an empty list stores the initial -1 / 0
  if (inside) {
    const size_t pix = (size_t)py * W + px;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k < ks) {
        top_id[(size_t)k * HW + pix] = ti[k];
        top_w[(size_t)k * HW + pix] = tw[k];
      }
  }
}

// -1 / 0 everywhere: P = 0 or a batch without a single instance
__global__ __launch_bounds__(256) void contributors_fill_kernel(int64_t n, int32_t* __restrict__ top_id,
                                                                float* __restrict__ top_w) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    top_id[i] = -1;
    top_w[i] = 0.f;
  }
}
// blocks of 256 threads for n elements, capped (the kernels stride over the rest)
static unsigned blocks_for(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

void launch_contributors(const ContribArgs& a, const CamBatch& cb, bool walk, hipStream_t s) {
  const int64_t n = (int64_t)cb.C * a.K * a.H * a.W;
  if (n <= 0) return;
  if (!walk) {
    hipLaunchKernelGGL(contributors_fill_kernel, dim3(blocks_for(n)), dim3(256), 0, s, n, a.top_id, a.top_w);
    return;
  }
  const dim3 grid(a.num_tiles * 4 * cb.C), block(64);
  if (a.K == 1) hipLaunchKernelGGL(contributors_kernel<1>, grid, block, 0, s, a, cb);
  else if (a.K == 2) hipLaunchKernelGGL(contributors_kernel<2>, grid, block, 0, s, a, cb);
  else hipLaunchKernelGGL(contributors_kernel<4>, grid, block, 0, s, a, cb);  // K = 3: the last rank is not stored
}

// ------------------------------------------------------------------ projection

__global__ __launch_bounds__(256) void track_project_kernel(TrackProjectArgs a, CamBatch cb) {
  const int64_t per_t = (int64_t)cb.C * a.N, total = per_t * a.T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / per_t, r = i - t * per_t;
    const int c = (int)(r / a.N);
    const int64_t n = r - (int64_t)c * a.N;
    const int32_t id0 = a.ids[n];
    float u = 0.f, v = 0.f, z = 0.f;
    uint8_t in = 0;
    if (id0 >= 0 && a.P > 0) {
      const int32_t id = id0 < a.P ? id0 : a.P - 1;  // an id >= P: clamped, flagged outside
      const V3 p = ld3(a.means3D + 3 * ((size_t)t * a.P + id));
      const V3 pv = xf43(cb.view + 16 * c, p);
      const float4 ph = xf44(cb.proj + 16 * c, p);
      const float pw = 1.0f / (ph.w + 0.0000001f);
      u = ndc_to_pix(ph.x * pw, a.W);
      v = ndc_to_pix(ph.y * pw, a.H);
      z = pv.z;
      const float ru = floorf(u + 0.5f), rv = floorf(v + 0.5f);
      in = (id0 < a.P && pv.z > 0.0f && ru >= 0.f && ru < (float)a.W && rv >= 0.f && rv < (float)a.H) ? 1 : 0;
    }
    reinterpret_cast<float2*>(a.uv)[i] = make_float2(u, v);
    a.depth[i] = z;
    a.inside[i] = in;
  }
}

void launch_track_project(const TrackProjectArgs& a, const CamBatch& cb, hipStream_t s) {
  const int64_t n = (int64_t)a.T * cb.C * a.N;
  if (n <= 0) return;
  hipLaunchKernelGGL(track_project_kernel, dim3(blocks_for(n)), dim3(256), 0, s, a, cb);
}

}  // namespace gs

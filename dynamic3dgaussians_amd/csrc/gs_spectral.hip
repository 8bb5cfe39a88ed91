// gs_spectral.hip -- spectral embedding of a sparse symmetric graph by
// Chebyshev-filtered subspace iteration (C ABI, definition and method:
// include/gs_spectral.h; sizes and the workspace: gs_spectral_layout.h; the
// small problems: gs_spectral_small.h).
//
//   sp_degree_kernel   a thread per row: row_ptr, col and val checked before
//                      anything is used as an address, d in CSR order, g
//   sp_begin_kernel    the bad-input verdict (code 2) and the done flag
//   sp_start_kernel    the counter-based start block
//   sp_spmm_kernel     Y = a g_i sum_j val_ij g_j X[j, :] + b X[i, :] + c Z[i, :]:
//                      a row walked in CSR order by a group of lanes across
//                      the B columns (16, 32 or 64 lanes: several rows per
//                      wave at the small tiers; two columns per lane at
//                      B = 72), four entries' loads in flight
//   sp_gram_kernel     a slab of rows per workgroup: the upper triangle of
//                      X^T Y, 16 x 16 threads with up to 15 accumulators each,
//                      rows added in order
//   sp_gram_reduce_kernel  the slabs added in index order, mirrored
//   sp_svqb_kernel / sp_ritz_kernel  one workgroup on gs_sym_eig.h
//   sp_rotate_kernel   X <- X R (and W <- W R in the same launch), R in LDS
//   sp_resid_kernel    per-slab column sums of (W - theta X)^2, rows in order
//   sp_check_kernel    the slabs in order, the residual test, the done flag
//   sp_embed_kernel    vectors, g V, the optional row normalisation, one fp32
//                      rounding
//
// Every kernel of the iteration reads the done flag first.  No float atomics:
// every sum is sequential in an order fixed by the sizes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_spectral.h"
#include "gs_launch.h"
#include "gs_spectral_layout.h"
#include "gs_spectral_small.h"

using namespace gs;

namespace {

__device__ inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(SP_THREADS) void sp_degree_kernel(int n, int64_t nnz, const int64_t* row_ptr,
                                                               const int32_t* col, const double* val, double* d,
                                                               double* g, int32_t* ctrl) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t lo = row_ptr[i], hi = row_ptr[i + 1];
  bool bad = lo < 0 || hi < lo || hi > nnz || (i == 0 && lo != 0) || (i == n - 1 && hi != nnz);
  double sum = 0.0;
  if (!bad) {
#pragma unroll 4
    for (int64_t p = lo; p < hi; ++p) {
      const int32_t c = col[p];
      const double v = val[p];
      bad |= c < 0 || c >= n || !(v >= 0.0) || !sp_finite(v);
      sum += v;
    }
    bad |= !sp_finite(sum);
  }
  if (bad) {
    atomicMax(&ctrl[SP_CTRL_BAD], 1);
    sum = 0.0;
  }
  d[i] = sum;
  g[i] = sum > 0.0 ? 1.0 / sqrt(sum) : 0.0;
}

__global__ void sp_begin_kernel(int B, int32_t* ctrl, int32_t* status) {
  if (threadIdx.x != 0) return;
  if (ctrl[SP_CTRL_BAD]) {
    ctrl[SP_CTRL_DONE] = 1;
    status[0] = 2;
  }
  status[3] = B;
}

__global__ __launch_bounds__(SP_THREADS) void sp_start_kernel(int n, int B, uint64_t seed, const int32_t* ctrl,
                                                              double* X) {
  if (ctrl[SP_CTRL_DONE]) return;
  const int64_t e = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (e >= (int64_t)n * B) return;
  X[e] = sp_start(seed, 0, e / B, (int)(e % B));
}

struct SpSpmm {
  int n, B, lpr, step;  // lanes per row; step 0: Y = S X, else step `step` of the filter
  int64_t nnz;
  const int64_t* row_ptr;
  const int32_t* col;
  const double *val, *g, *theta, *X, *Z;
  double* Y;
  const int32_t* ctrl;
};

template <int CPT>
__global__ __launch_bounds__(SP_THREADS) void sp_spmm_kernel(const SpSpmm a) {
  if (a.ctrl[SP_CTRL_DONE]) return;
  const int B = a.B;
  const int64_t gt = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  const int64_t row = gt / a.lpr;
  const int lane = (int)(gt % a.lpr);
  if (row >= a.n) return;
  ChebStep cs{1.0, 0.0, 0.0};
  if (a.step > 0) cs = sp_cheb_step(a.theta[0], a.theta[B - 1], a.step);
  const int64_t lo = clamp64(a.row_ptr[row], 0, a.nnz), hi = clamp64(a.row_ptr[row + 1], lo, a.nnz);
  int cq[CPT];
  bool on[CPT];
  double acc[CPT];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    cq[q] = lane + q * a.lpr;
    on[q] = cq[q] < B;
    if (!on[q]) cq[q] = 0;  // a valid address; the value is never stored
    acc[q] = 0.0;
  }
  const int last = a.n - 1;
  int64_t p = lo;
  for (; p + 4 <= hi; p += 4) {  // four entries' loads in flight, added in CSR order
    int64_t j[4];
    double w[4], x[4][CPT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int32_t c = a.col[p + u];
      j[u] = c < 0 ? 0 : (c > last ? last : c);
      w[u] = a.val[p + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u] = w[u] * a.g[j[u]];
#pragma unroll
      for (int q = 0; q < CPT; ++q) x[u][q] = a.X[j[u] * B + cq[q]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < CPT; ++q) acc[q] += w[u] * x[u][q];
  }
  for (; p < hi; ++p) {
    const int32_t c = a.col[p];
    const int64_t j = c < 0 ? 0 : (c > last ? last : c);
    const double w = a.val[p] * a.g[j];
#pragma unroll
    for (int q = 0; q < CPT; ++q) acc[q] += w * a.X[j * B + cq[q]];
  }
  const double gi = a.g[row];
#pragma unroll
  for (int q = 0; q < CPT; ++q) {
    if (!on[q]) continue;
    const int64_t o = row * B + cq[q];
    double y = cs.alpha * (gi * acc[q]);
    if (a.step > 0) y += cs.beta * a.X[o];
    if (a.step > 1) y += cs.gamma * a.Z[o];
    a.Y[o] = y;
  }
}

// part[slab][i][j], i <= j: sum over the slab's rows of X[r, i] Y[r, j], rows ascending.
__global__ __launch_bounds__(SP_THREADS) void sp_gram_kernel(int n, int B, int64_t slab_rows, const double* X,
                                                             const double* Y, double* part, const int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  __shared__ double xs[SP_CHUNK * SP_MAX_B];
  __shared__ double ys[SP_CHUNK * SP_MAX_B];
  constexpr int T = (SP_MAX_B + 15) / 16;  // 5 tiles of 16 a side
  const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
  double acc[T][T];
#pragma unroll
  for (int p = 0; p < T; ++p)
#pragma unroll
    for (int q = 0; q < T; ++q) acc[p][q] = 0.0;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  for (int64_t rc = r0; rc < r1; rc += SP_CHUNK) {
    const int rows = (int)(r1 - rc < SP_CHUNK ? r1 - rc : SP_CHUNK);
    for (int e = tid; e < rows * B; e += SP_THREADS) {
      xs[e] = X[rc * B + e];
      ys[e] = Y[rc * B + e];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      double xv[T], yv[T];
#pragma unroll
      for (int p = 0; p < T; ++p) {
        xv[p] = ti + 16 * p < B ? xs[r * B + ti + 16 * p] : 0.0;
        yv[p] = tj + 16 * p < B ? ys[r * B + tj + 16 * p] : 0.0;
      }
#pragma unroll
      for (int p = 0; p < T; ++p)
#pragma unroll
        for (int q = p; q < T; ++q) acc[p][q] += xv[p] * yv[q];  // tiles under the diagonal are never needed
    }
    __syncthreads();
  }
  double* out = part + (int64_t)blockIdx.x * B * B;
#pragma unroll
  for (int p = 0; p < T; ++p)
#pragma unroll
    for (int q = p; q < T; ++q) {
      const int i = ti + 16 * p, j = tj + 16 * q;
      if (i < B && j < B && i <= j) out[i * B + j] = acc[p][q];
    }
}

__global__ __launch_bounds__(SP_THREADS) void sp_gram_reduce_kernel(int B, int64_t slabs, const double* part,
                                                                    double* G, const int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  const int e = blockIdx.x * SP_THREADS + threadIdx.x;
  if (e >= B * B) return;
  const int i = e / B, j = e % B;
  if (i > j) return;
  double s = 0.0;
  for (int64_t b = 0; b < slabs; ++b) s += part[b * B * B + e];
  G[i * B + j] = s;
  G[j * B + i] = s;
}

struct SpSmallLds {
  double A[2 * SP_MAX_B * (SP_MAX_B + 1)];
  double rot[3 * SP_MAX_B / 2];
  double red[2 * SP_EIG_THREADS];
  double scale[SP_MAX_B];
  int pq[SP_MAX_B];
};

__global__ __launch_bounds__(SP_EIG_THREADS) void sp_svqb_kernel(int B, const double* G, double* T, int32_t* replaced,
                                                                 const int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  __shared__ SpSmallLds l;
  SymEigScratch w{l.rot, l.pq, l.red, 0};
  sp_svqb(B, G, l.A, l.A + sp_even(B) * sp_ld(B), w, l.scale, T, replaced, threadIdx.x, SP_EIG_THREADS);
}

__global__ __launch_bounds__(SP_EIG_THREADS) void sp_ritz_kernel(int B, const double* H, double* evecs, double* theta,
                                                                 double* Q, const int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  __shared__ SpSmallLds l;
  SymEigScratch w{l.rot, l.pq, l.red, 0};
  sp_ritz(B, H, l.A, l.A + sp_even(B) * sp_ld(B), w, evecs, theta, Q, threadIdx.x, SP_EIG_THREADS);
}

// out[r, k] = sum_i X[r, i] R[i, k], i ascending; blockIdx.y picks the pair
// (X0, out0) or (X1, out1).  A replaced column k takes the fresh values of
// epoch `epoch` instead.
struct SpRotate {
  int n, B;
  uint32_t epoch;
  uint64_t seed;
  const double *R, *X0, *X1;
  double *out0, *out1;
  const int32_t *replaced, *ctrl;
};

__global__ __launch_bounds__(SP_THREADS) void sp_rotate_kernel(const SpRotate a) {
  if (a.ctrl[SP_CTRL_DONE]) return;
  __shared__ double rs[SP_MAX_B * SP_MAX_B];
  __shared__ double xs[SP_CHUNK * SP_MAX_B];
  const int tid = threadIdx.x, B = a.B;
  const double* X = blockIdx.y ? a.X1 : a.X0;
  double* out = blockIdx.y ? a.out1 : a.out0;
  const int64_t r0 = (int64_t)blockIdx.x * SP_CHUNK;
  const int rows = (int)(a.n - r0 < SP_CHUNK ? a.n - r0 : SP_CHUNK);
  for (int e = tid; e < B * B; e += SP_THREADS) rs[e] = a.R[e];
  for (int e = tid; e < rows * B; e += SP_THREADS) xs[e] = X[r0 * B + e];
  __syncthreads();
  for (int e = tid; e < rows * B; e += SP_THREADS) {
    const int r = e / B, k = e % B;
    double s = 0.0;
    if (a.replaced && a.replaced[k]) {
      s = sp_start(a.seed, a.epoch, r0 + r, k);
    } else {
      for (int i = 0; i < B; ++i) s += xs[r * B + i] * rs[i * B + k];
    }
    out[r0 * B + e] = s;
  }
}

__global__ __launch_bounds__(128) void sp_resid_kernel(int n, int B, int64_t slab_rows, const double* X,
                                                       const double* W, const double* theta, double* rpart,
                                                       const int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  const int j = threadIdx.x;
  if (j >= B) return;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  const double th = theta[j];
  double s = 0.0;
#pragma unroll 4
  for (int64_t r = r0; r < r1; ++r) {
    const double v = W[r * B + j] - th * X[r * B + j];
    s += v * v;
  }
  rpart[(int64_t)blockIdx.x * B + j] = s;
}

// Outer iteration t: the residual norms, the test, the flag.  The outputs of
// the K leading pairs are written when the call ends here.
__global__ __launch_bounds__(128) void sp_check_kernel(int t, int max_outer, int B, int K, double tol, int64_t slabs,
                                                       const double* rpart, const double* theta, double* eigenvalues,
                                                       double* residuals, int32_t* status, int32_t* ctrl) {
  if (ctrl[SP_CTRL_DONE]) return;
  __shared__ double res[128];
  const int j = threadIdx.x;
  if (j < B) {
    double s = 0.0;
    for (int64_t b = 0; b < slabs; ++b) s += rpart[b * B + j];
    res[j] = sp_finite(s) ? sqrt(s) : 1.7976931348623157e308;
  }
  __syncthreads();
  if (j != 0) return;
  int conv = 0;
  for (int k = 0; k < K; ++k) conv += res[k] <= tol ? 1 : 0;
  status[1] = t + 1;
  status[2] = conv;
  const bool end = conv == K || t + 1 == max_outer;
  if (!end) return;
  for (int k = 0; k < K; ++k) {
    const double th = theta[k];
    eigenvalues[k] = sp_finite(th) ? th : 0.0;
    residuals[k] = res[k];
  }
  status[0] = conv == K ? 0 : 1;
  ctrl[SP_CTRL_FINAL] = t + 1;
  ctrl[SP_CTRL_DONE] = 1;
}

__global__ __launch_bounds__(SP_THREADS) void sp_embed_kernel(int t, int n, int B, int K, int row_normalize,
                                                              const double* X, const double* g, double* vectors,
                                                              float* embedding, const int32_t* ctrl) {
  if (ctrl[SP_CTRL_FINAL] != t + 1) return;
  const int64_t r = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (r >= n) return;
  const double gi = g[r];
  double scale = 1.0;
  if (row_normalize) {
    double ss = 0.0;
    for (int k = 0; k < K; ++k) {
      const double u = gi * X[r * B + k];
      ss += u * u;
    }
    const double nrm = sqrt(ss);
    if (nrm > 0.0 && sp_finite(nrm)) scale = nrm;
  }
  for (int k = 0; k < K; ++k) {
    double v = X[r * B + k];
    if (!sp_finite(v)) v = 0.0;
    vectors[r * K + k] = v;
    const double u = gi * v;
    embedding[r * K + k] = gi > 0.0 ? (float)(row_normalize ? u / scale : u) : 0.f;
  }
}

int lanes_per_row(int B, int cpt) {
  const int need = (B + cpt - 1) / cpt;
  int l = 1;
  while (l < need) l *= 2;
  return l;
}

void launch_spmm(hipStream_t s, SpSpmm k) {
  const int cpt = k.B > 64 ? 2 : 1;
  k.lpr = lanes_per_row(k.B, cpt);
  const int64_t threads = (int64_t)k.n * k.lpr;
  const dim3 grid((unsigned)((threads + SP_THREADS - 1) / SP_THREADS));
  if (cpt == 2)
    hipLaunchKernelGGL(sp_spmm_kernel<2>, grid, dim3(SP_THREADS), 0, s, k);
  else
    hipLaunchKernelGGL(sp_spmm_kernel<1>, grid, dim3(SP_THREADS), 0, s, k);
}

}  // namespace

extern "C" int gs_spectral_embedding(const gs_spectral_args* g, gs_stream_t stream) {
  if (int rc = gs_spectral_validate(g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int n = g->n, K = g->num_vectors;
  const SpectralLayout L(n, K);
  const int B = L.B;
  void* ws = g->workspace;
  double* d = at<double>(ws, L.off_d);
  double* gv = at<double>(ws, L.off_g);
  double* P[4];
  for (int i = 0; i < 4; ++i) P[i] = at<double>(ws, L.off_blk[i]);
  double* part = at<double>(ws, L.off_part);
  double* rpart = at<double>(ws, L.off_rpart);
  double* gram = at<double>(ws, L.off_gram);
  double* rot = at<double>(ws, L.off_rot);
  double* evec = at<double>(ws, L.off_evec);
  double* theta = at<double>(ws, L.off_theta);
  int32_t* repl = at<int32_t>(ws, L.off_repl);
  int32_t* ctrl = at<int32_t>(ws, L.off_ctrl);

  hipError_t e = hipMemsetAsync(ctrl, 0, SP_CTRL_WORDS * sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(g->eigenvalues, 0, (size_t)K * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(g->residuals, 0, (size_t)K * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(g->vectors, 0, (size_t)n * K * sizeof(double), s);
  if (e == hipSuccess) e = hipMemsetAsync(g->embedding, 0, (size_t)n * K * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(g->status, 0, 4 * sizeof(int32_t), s);
  if (e != hipSuccess) return gs_set_error((int)e, "spectral embedding: %s", hipGetErrorString(e));

  const dim3 tb(SP_THREADS);
  const dim3 row_grid((unsigned)(((int64_t)n + SP_THREADS - 1) / SP_THREADS));
  const dim3 elem_grid((unsigned)(((int64_t)n * B + SP_THREADS - 1) / SP_THREADS));
  const dim3 slab_grid((unsigned)L.slabs);
  const dim3 bb_grid((unsigned)((B * B + SP_THREADS - 1) / SP_THREADS));
  const unsigned chunks = (unsigned)(((int64_t)n + SP_CHUNK - 1) / SP_CHUNK);

  hipLaunchKernelGGL(sp_degree_kernel, row_grid, tb, 0, s, n, g->nnz, g->row_ptr, g->col, g->val, d, gv, ctrl);
  hipLaunchKernelGGL(sp_begin_kernel, dim3(1), dim3(64), 0, s, B, ctrl, g->status);
  hipLaunchKernelGGL(sp_start_kernel, elem_grid, tb, 0, s, n, B, g->seed, ctrl, P[0]);

  SpSpmm mm;
  mm.n = n; mm.B = B; mm.lpr = 0; mm.step = 0; mm.nnz = g->nnz;
  mm.row_ptr = g->row_ptr; mm.col = g->col; mm.val = g->val; mm.g = gv; mm.theta = theta;
  mm.X = nullptr; mm.Z = nullptr; mm.Y = nullptr; mm.ctrl = ctrl;
  SpRotate ro;
  ro.n = n; ro.B = B; ro.epoch = 0; ro.seed = g->seed; ro.R = rot;
  ro.X0 = ro.X1 = nullptr; ro.out0 = ro.out1 = nullptr; ro.replaced = nullptr; ro.ctrl = ctrl;

  for (int t = 0; t < g->max_outer; ++t) {
    // SVQB, twice: P[0] -> P[1] -> P[0]
    for (int pass = 0; pass < 2; ++pass) {
      double* src = P[pass];
      double* dst = P[1 - pass];
      hipLaunchKernelGGL(sp_gram_kernel, slab_grid, tb, 0, s, n, B, L.slab_rows, src, src, part, ctrl);
      hipLaunchKernelGGL(sp_gram_reduce_kernel, bb_grid, tb, 0, s, B, L.slabs, part, gram, ctrl);
      hipLaunchKernelGGL(sp_svqb_kernel, dim3(1), dim3(SP_EIG_THREADS), 0, s, B, gram, rot, repl, ctrl);
      SpRotate r = ro;
      r.epoch = (uint32_t)(1 + 2 * t + pass);
      r.X0 = src; r.out0 = dst; r.replaced = repl;
      hipLaunchKernelGGL(sp_rotate_kernel, dim3(chunks, 1), tb, 0, s, r);
    }
    // Rayleigh-Ritz: W = S X in P[1], the rotated pair in P[2], P[3]
    SpSpmm w = mm;
    w.X = P[0]; w.Y = P[1];
    launch_spmm(s, w);
    hipLaunchKernelGGL(sp_gram_kernel, slab_grid, tb, 0, s, n, B, L.slab_rows, P[0], P[1], part, ctrl);
    hipLaunchKernelGGL(sp_gram_reduce_kernel, bb_grid, tb, 0, s, B, L.slabs, part, gram, ctrl);
    hipLaunchKernelGGL(sp_ritz_kernel, dim3(1), dim3(SP_EIG_THREADS), 0, s, B, gram, evec, theta, rot, ctrl);
    SpRotate r = ro;
    r.X0 = P[0]; r.out0 = P[2]; r.X1 = P[1]; r.out1 = P[3];
    hipLaunchKernelGGL(sp_rotate_kernel, dim3(chunks, 2), tb, 0, s, r);
    hipLaunchKernelGGL(sp_resid_kernel, slab_grid, dim3(128), 0, s, n, B, L.slab_rows, P[2], P[3], theta, rpart, ctrl);
    hipLaunchKernelGGL(sp_check_kernel, dim3(1), dim3(128), 0, s, t, g->max_outer, B, K, g->tol, L.slabs, rpart, theta,
                       g->eigenvalues, g->residuals, g->status, ctrl);
    hipLaunchKernelGGL(sp_embed_kernel, row_grid, tb, 0, s, t, n, B, K, g->row_normalize, P[2], gv, g->vectors,
                       g->embedding, ctrl);
    if (t + 1 == g->max_outer) break;
    // the filter: Y_0 = P[2]; a step writes the block that holds neither Y_{s-1} nor Y_{s-2}
    int cur = 2, prev = -1;
    for (int step = 1; step <= g->degree; ++step) {
      int out = 0;
      while (out == cur || out == prev) ++out;
      SpSpmm f = mm;
      f.step = step;
      f.X = P[cur]; f.Z = prev >= 0 ? P[prev] : nullptr; f.Y = P[out];
      launch_spmm(s, f);
      prev = cur;
      cur = out;
    }
    double* x = P[cur];
    P[cur] = P[0];
    P[0] = x;
  }
  return launch_status("spectral embedding", 0, s);
}

// gs_torch_binding.cpp -- the C++ binding behind `_C`.
//
// The reference binds its rasterizer with a C++ torch extension
// (DGR/rasterize_points.cu:35-246, RasterizeGaussiansCUDA /
// RasterizeGaussiansBackwardCUDA, DGR/ext.cpp:15-19).  This file is our
// counterpart on top of the C ABI (include/gsplat_hip.h) and the one place a
// rasterizer call's arguments are handled: tensor checks, output allocation,
// struct packing and the ABI calls, tens of microseconds of host time per
// camera.  dynamic3dgaussians_amd/_C.py in front of it keeps the reference's
// positional signatures, answers an empty scene and host tensors, and does
// the sync-free plan's bookkeeping.  Built with torch.utils.cpp_extension by
// build.py into lib/ next to the library it is linked against (found through
// rpath $ORIGIN).  No device code: every kernel runs through the C ABI.
#include <torch/extension.h>

#include <stdexcept>
#include <string>
#include <tuple>

#include "gs_camera_grad.h"
#include "gs_track.h"
#include "gs_window.h"
#include "gsplat_hip.h"

namespace {

using at::Tensor;
using OptT = c10::optional<Tensor>;

const int kSupportedF[] = {0, 4, 8, 16, 32, 36, 64};

bool present(const OptT& t) { return t.has_value() && t->defined() && t->numel() > 0; }

Tensor dev_f32(const Tensor& t, const at::Device& dev, const char* name) {
  if (t.device() != dev)
    throw std::runtime_error(std::string(name) + " must be on the rasterizer's HIP device");
  Tensor u = t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
  return u.contiguous();
}

void check(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + gs_last_error() + " (code " + std::to_string(rc) + ")");
}

int feature_width(int64_t F) {
  for (int k : kSupportedF)
    if (k >= F) return k;
  throw std::runtime_error("semantic feature width " + std::to_string(F) + " exceeds the largest compiled width 64");
}

struct Inputs {
  at::Device dev{at::kCUDA};
  int64_t P = 0, M = 0, F = 0, F_user = 0;
  int64_t B = 1;  // frames per Gaussian in means3D (a temporal window, gs_window.h), else 1
  int D = 0;
  float scale_modifier = 1.f;
  Tensor means3D, colors, opacity, scales, rotations, cov3D, sh, sem;
  gs_gaussians g{};

  Inputs(const Tensor& means3D_, const OptT& colors_, const OptT& sem_, const OptT& opacity_, const OptT& scales_,
         const OptT& rotations_, double scale_mod, const OptT& cov3D_, const OptT& sh_, int64_t degree,
         bool windowed = false) {
    if (windowed) {
      if (means3D_.dim() != 3 || means3D_.size(2) != 3)
        throw std::runtime_error("means3D must have dimensions (num_points, frames, 3) with cam_frames");
      B = means3D_.size(1);
    } else if (means3D_.dim() != 2 || means3D_.size(1) != 3) {
      throw std::runtime_error("means3D must have dimensions (num_points, 3)");  // rasterize_points.cu:60-62
    }
    dev = means3D_.device();
    P = means3D_.size(0);
    means3D = dev_f32(means3D_, dev, "means3D");
    if (present(colors_)) colors = dev_f32(*colors_, dev, "colors_precomp");
    if (present(opacity_)) opacity = dev_f32(*opacity_, dev, "opacities");
    if (present(scales_)) scales = dev_f32(*scales_, dev, "scales");
    if (present(rotations_)) rotations = dev_f32(*rotations_, dev, "rotations");
    if (present(cov3D_)) cov3D = dev_f32(*cov3D_, dev, "cov3D_precomp");
    if (present(sh_)) {
      sh = dev_f32(*sh_, dev, "sh");
      M = sh.size(1);
    }
    D = (int)degree;
    scale_modifier = (float)scale_mod;
    if (present(sem_)) {
      sem = dev_f32(*sem_, dev, "semantic_feature").reshape({P, -1});
      F_user = sem.size(1);
      F = feature_width(F_user);
      if (F != F_user) sem = at::constant_pad_nd(sem, {0, F - F_user}, 0.0);
      sem = sem.contiguous();
    }
    auto ptr = [](const Tensor& t) -> const float* { return t.defined() ? t.data_ptr<float>() : nullptr; };
    g.P = (int32_t)P;
    g.D = D;
    g.M = (int32_t)M;
    g.F = (int32_t)F;
    g.means3D = ptr(means3D);
    g.shs = ptr(sh);
    g.colors_precomp = ptr(colors);
    g.semantic_feature = ptr(sem);
    g.opacities = ptr(opacity);
    g.scales = ptr(scales);
    g.rotations = ptr(rotations);
    g.cov3D_precomp = ptr(cov3D);
    g.scale_modifier = scale_modifier;
    g.flags = 0;
    g.grad_mask = nullptr;
    g.densify_accum = g.densify_denom = g.max_radius = nullptr;
    g.feature_ready = nullptr;
    g.walk_order = nullptr;
  }
};

void* nz(const Tensor& t) { return (t.defined() && t.numel()) ? t.data_ptr() : nullptr; }

// One forward and one backward body over the gs_*_batch entry points, for any
// number of cameras, called by _C.rasterize_gaussians_batch and _C._backward.
// A single camera (_C.rasterize_gaussians / _backward) is a batch of one,
// wrapped and unwrapped in Python.  The forward's one host
// round trip (the plan header) sits between the two ABI calls, so the host
// work around it is on the step's critical path.

// The C cameras of a call; the ABI checks that 1 <= C <= its camera limit.
struct Cameras {
  Tensor view, proj, cpos, bg;
  std::vector<gs_camera> cams;
  Cameras(const at::Device& dev, const Tensor& bg_, const Tensor& views, const Tensor& projs, const Tensor& campos,
          const std::vector<double>& cx, const std::vector<double>& cy, const std::vector<double>& tx,
          const std::vector<double>& ty, int64_t W, int64_t H, const std::vector<std::vector<int64_t>>& windows) {
    const int64_t C = (int64_t)cx.size();
    if (C < 1) throw std::runtime_error("camera batch size 0: a call takes at least one camera");
    if ((int64_t)cy.size() != C || (int64_t)tx.size() != C || (int64_t)ty.size() != C)
      throw std::runtime_error("per-camera scalars must all have C entries");
    view = dev_f32(views, dev, "viewmatrices").reshape({C, 16}).contiguous();
    proj = dev_f32(projs, dev, "projmatrices").reshape({C, 16}).contiguous();
    cpos = dev_f32(campos, dev, "campos").reshape({C, 3}).contiguous();
    bg = dev_f32(bg_, dev, "bg").reshape({-1});
    if (!windows.empty() && (int64_t)windows.size() != C)
      throw std::runtime_error("tile windows: one (x0, y0, x1, y1) per camera");
    cams.assign(C, gs_camera{});
    for (int64_t c = 0; c < C; ++c) {
      gs_camera& k = cams[c];
      if (!windows.empty()) {
        if (windows[c].size() != 4) throw std::runtime_error("a tile window is (x0, y0, x1, y1)");
        k.tile_x0 = (int32_t)windows[c][0];
        k.tile_y0 = (int32_t)windows[c][1];
        k.tile_x1 = (int32_t)windows[c][2];
        k.tile_y1 = (int32_t)windows[c][3];
      }
      k.viewmatrix = view.data_ptr<float>() + 16 * c;
      k.projmatrix = proj.data_ptr<float>() + 16 * c;
      k.campos = cpos.data_ptr<float>() + 3 * c;
      k.background = bg.data_ptr<float>();
      k.c_x = (float)cx[c];
      k.c_y = (float)cy[c];
      k.tan_fovx = (float)tx[c];
      k.tan_fovy = (float)ty[c];
      k.image_width = (int32_t)W;
      k.image_height = (int32_t)H;
    }
  }
};

// The temporal window of a call (gs_window.h): cam_frames empty = none.
struct Window {
  std::vector<int32_t> frames;
  gs_window w{};
  const gs_window* ptr = nullptr;
  Window(const std::vector<int64_t>& cam_frames, int64_t C, int64_t B) {
    if (cam_frames.empty()) return;
    if ((int64_t)cam_frames.size() != C) throw std::runtime_error("cam_frames must have C entries");
    frames.assign(cam_frames.begin(), cam_frames.end());
    w.B = (int32_t)B;
    w.cam_frame = frames.data();
    ptr = &w;
    check(gs_check_window(ptr, (int32_t)C), "camera frames");
  }
  Window(const Window&) = delete;
};

// capacity: empty = the two-phase path (plan, host read, render); else the
// sync-free gs_forward_batch with a binning buffer of capacity[c] instances
// per camera and `hint` (gs_batch_hint as {valid, p1, q1, p2, max_len,
// total}), retried with the exact lengths when they do not fit.  Returns the
// reference's counts, the images and state, the exact num_instances, the
// per-camera lengths the binning buffer is laid out with (what the backward
// takes), the updated hint and whether the first attempt fitted.
// cam_frames: empty = the call without a temporal window; else (gs_window.h)
// means3D is (P, B, 3) and camera c renders frame cam_frames[c].
std::tuple<std::vector<int64_t>, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, std::vector<int64_t>,
           std::vector<int64_t>, std::vector<int64_t>, bool>
forward_batch(const Tensor& bg, const Tensor& means3D, const OptT& colors, const OptT& sem, const OptT& opacity,
              const OptT& scales, const OptT& rotations, double scale_modifier, const OptT& cov3D, const Tensor& views,
              const Tensor& projs, const std::vector<double>& cx, const std::vector<double>& cy,
              const std::vector<double>& tx, const std::vector<double>& ty, int64_t H, int64_t W, const OptT& sh,
              int64_t degree, const Tensor& campos, bool prefiltered, bool debug, int64_t compat, bool activate,
              const std::vector<std::vector<int64_t>>& windows, int64_t feature_ready,
              const std::vector<int64_t>& capacity, const std::vector<int64_t>& hint, const OptT& walk_order,
              const OptT& zero_fill, const std::vector<int64_t>& cam_frames, int64_t stream) {
  Inputs in(means3D, colors, sem, opacity, scales, rotations, scale_modifier, cov3D, sh, degree, !cam_frames.empty());
  if (activate) in.g.flags |= GS_FLAG_ACTIVATE;
  in.g.feature_ready = reinterpret_cast<gs_event_t>(feature_ready);
  if (present(zero_fill)) {  // the backward's scratch, zeroed by the blend (gs_gaussians.zero_fill)
    const Tensor& z = *zero_fill;
    if (z.device() != in.dev || !z.is_contiguous())
      throw std::runtime_error("zero_fill must be a contiguous device tensor");
    in.g.zero_fill = z.data_ptr();
    in.g.zero_fill_bytes = (int64_t)(z.numel() * z.element_size()) & ~(int64_t)15;
  }
  if (present(walk_order)) {
    const Tensor& w = *walk_order;
    if (w.scalar_type() != at::kInt || w.device() != in.dev || !w.is_contiguous() || w.numel() != in.P)
      throw std::runtime_error("walk_order must be a contiguous int32 device tensor of P ids");
    in.g.walk_order = w.data_ptr<int32_t>();
  }
  Cameras k(in.dev, bg, views, projs, campos, cx, cy, tx, ty, W, H, windows);
  const int32_t C = (int32_t)k.cams.size();
  const Window win(cam_frames, C, in.B);
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(in.dev);
  const auto u8 = at::TensorOptions().dtype(at::kByte).device(in.dev);
  Tensor out_color = at::empty({C, 3, H, W}, f32);
  Tensor out_feature = at::empty({C, in.F, H, W}, f32);
  Tensor out_depth = at::empty({C, 1, H, W}, f32);
  Tensor out_alpha = at::empty({C, 1, H, W}, f32);
  Tensor radii = at::empty({C, in.P}, f32.dtype(at::kInt));
  Tensor geom = at::empty({(int64_t)gs_batch_geom_buffer_bytes(in.P, C)}, u8);
  Tensor img = at::empty({(int64_t)gs_batch_image_buffer_bytes((int32_t)W, (int32_t)H, C)}, u8);
  std::vector<int64_t> NR(C, 0), NI(C, 0);
  gs_stream_t s = reinterpret_cast<gs_stream_t>(stream);
  float* oc = out_color.data_ptr<float>();
  float* of = in.F ? out_feature.data_ptr<float>() : nullptr;
  float* od = out_depth.data_ptr<float>();
  float* oa = out_alpha.data_ptr<float>();
  Tensor binning;
  bool fitted = false;
  gs_batch_hint h{};
  if (!capacity.empty() && !debug) {
    if ((int64_t)capacity.size() != C) throw std::runtime_error("capacity must have C entries");
    if (hint.size() == 6) {
      h.valid = (int32_t)hint[0];
      h.p1 = (int32_t)hint[1];
      h.q1 = (int32_t)hint[2];
      h.p2 = (int32_t)hint[3];
      h.max_len = hint[4];
      h.total = hint[5];
    }
    const int64_t nb = (int64_t)gs_batch_binning_buffer_bytes(C, capacity.data());
    binning = at::empty({nb > 1 ? nb : 1}, u8);
    int32_t fits = 0;
    check(gs_forward_batch_window(&in.g, k.cams.data(), C, prefiltered ? 1 : 0, (int)compat, geom.data_ptr(),
                                  img.data_ptr(), binning.data_ptr(), capacity.data(), &h,
                                  radii.data_ptr<int32_t>(), NR.data(), NI.data(), &fits, oc, of, od, oa, win.ptr, s),
          "rasterize_gaussians_batch (sync-free forward)");
    fitted = fits != 0;
  } else {
    check(gs_forward_plan_batch_window(&in.g, k.cams.data(), C, prefiltered ? 1 : 0, debug ? 1 : 0, (int)compat,
                                       geom.data_ptr(), img.data_ptr(), radii.data_ptr<int32_t>(), NR.data(),
                                       NI.data(), win.ptr, s),
          "rasterize_gaussians_batch (preprocess)");
  }
  std::vector<int64_t> layout = NI;
  if (fitted) {
    layout = capacity;
  } else {
    // two-phase, or the sync-free attempt's retry with the exact lengths
    const int64_t nb = (int64_t)gs_batch_binning_buffer_bytes(C, NI.data());
    binning = at::empty({nb > 1 ? nb : 1}, u8);
    check(gs_forward_render_batch(&in.g, k.cams.data(), C, debug ? 1 : 0, (int)compat, geom.data_ptr(),
                                  binning.data_ptr(), img.data_ptr(), NI.data(), radii.data_ptr<int32_t>(), oc, of, od,
                                  oa, s),
          "rasterize_gaussians_batch (render)");
  }
  Tensor feature_map = in.F_user != in.F ? out_feature.narrow(1, 0, in.F_user) : out_feature;
  std::vector<int64_t> hint_out = {h.valid, h.p1, h.q1, h.p2, h.max_len, h.total};
  return {NR, out_color, feature_map, out_depth, out_alpha, radii, geom, binning, img, NI, layout, hint_out, fitted};
}

// [C, ch, H, W] fp32 of an upstream gradient (channels zero-padded to ch), or undefined
Tensor batch_image(const OptT& t, int64_t C, int64_t ch, int64_t H, int64_t W, const at::Device& dev,
                   const char* name) {
  if (!present(t)) return Tensor();
  Tensor u = dev_f32(*t, dev, name).reshape({C, -1, H, W});
  if (u.size(1) < ch)
    u = at::cat({u, at::zeros({C, ch - u.size(1), H, W}, u.options())}, 1);
  return u.contiguous();
}

void set_grad_mask(Inputs& in, const OptT& grad_mask, Tensor& keep) {
  if (!grad_mask.has_value() || !grad_mask->defined()) return;
  keep = grad_mask->to(in.dev, at::kFloat).reshape({-1}).contiguous();
  if (keep.numel() != in.P)
    throw std::runtime_error("grad_mask must have " + std::to_string(in.P) + " elements, got " +
                             std::to_string(keep.numel()));
  in.g.grad_mask = keep.data_ptr<float>();
}

// (accum, denom, max_radius): this call's densification statistics
void set_densify(Inputs& in, const c10::optional<std::vector<Tensor>>& densify) {
  if (!densify.has_value()) return;
  const auto& d = *densify;
  if (d.size() != 3) throw std::runtime_error("densify must hold (accum, denom, max_radius)");
  for (const auto& t : d)
    if (t.dim() != 1 || t.size(0) != in.P || t.scalar_type() != at::kFloat || t.device() != in.dev || !t.is_contiguous())
      throw std::runtime_error("densify statistics must be contiguous fp32 (" + std::to_string(in.P) +
                               ",) tensors on the device");
  in.g.densify_accum = d[0].data_ptr<float>();
  in.g.densify_denom = d[1].data_ptr<float>();
  in.g.max_radius = d[2].data_ptr<float>();
}

// The backward's nine gradients in the order of its return tuple (_C.py
// _buffer_shapes): fresh tensors, or the caller's `out` (empty, or nine
// entries) -- with `exact` each in its exact shape (the GradientSink
// contract), else an empty entry = allocate and the others matched by element
// count and viewed in their shapes (a gradient bucket's flat views).
std::vector<Tensor> gradient_outputs(const Inputs& in, const std::vector<Tensor>& out, bool exact, bool windowed) {
  static const char* const names[9] = {"dmeans2D", "dcolors", "dsem", "dopacity", "dmeans3D",
                                       "dcov3D", "dsh", "dscales", "drot"};
  const int64_t P = in.P;
  // dmeans3D of a temporal window: one row per frame, (P, B, 3)
  const std::vector<int64_t> dmeans = windowed ? std::vector<int64_t>{P, in.B, 3} : std::vector<int64_t>{P, 3};
  const std::vector<int64_t> shapes[9] = {{P, 3}, {P, 3}, {P, in.F}, {P, 1}, dmeans, {P, 6}, {P, in.M, 3}, {P, 3}, {P, 4}};
  if (!out.empty() && out.size() != 9) throw std::runtime_error("out must hold the 9 gradient buffers");
  std::vector<Tensor> o;
  for (int i = 0; i < 9; ++i) {
    if (out.empty() || (!exact && out[i].numel() == 0)) {
      o.push_back(at::empty(shapes[i], at::TensorOptions().dtype(at::kFloat).device(in.dev)));
      continue;
    }
    const Tensor& d = out[i];
    const int64_t n = c10::multiply_integers(shapes[i]);
    const bool fits = exact ? d.sizes() == at::IntArrayRef(shapes[i]) : d.numel() == n;
    if (!fits || d.scalar_type() != at::kFloat || d.device() != in.dev || !d.is_contiguous())
      throw std::runtime_error(std::string("gradient buffer ") + names[i] + " must be a contiguous fp32 device tensor of " +
                               (exact ? "its exact shape" : std::to_string(n) + " elements"));
    o.push_back(d.view(shapes[i]));
  }
  return o;
}

// `exact_out`, `accumulate`: _C._backward.  Returns the gradients summed over
// the cameras, in gradient_outputs' order.
std::vector<Tensor> backward_batch(
    const Tensor& bg, const Tensor& means3D, const Tensor& radii, const OptT& colors, const OptT& sem,
    const OptT& scales, const OptT& rotations, double scale_modifier, const OptT& cov3D, const Tensor& views,
    const Tensor& projs, const std::vector<double>& cx, const std::vector<double>& cy, const std::vector<double>& tx,
    const std::vector<double>& ty, const OptT& dL_color, const OptT& dL_feature, const OptT& dL_depth,
    const OptT& dL_alpha, const OptT& sh, int64_t degree, const Tensor& campos, const Tensor& geom,
    const std::vector<int64_t>& num_instances, const OptT& binning, const Tensor& img, const Tensor& alphas,
    bool debug, int64_t compat, const OptT& grad_mask, c10::optional<std::vector<Tensor>> densify,
    const OptT& opacity, bool activate, const std::vector<std::vector<int64_t>>& windows,
    const std::vector<Tensor>& out, bool exact_out, bool accumulate, const OptT& scratch_in, bool scratch_zeroed,
    const std::vector<int64_t>& cam_frames, int64_t stream) {
  if (activate && !present(opacity)) throw std::runtime_error("activate=True needs the raw opacities");
  if (accumulate && out.empty()) throw std::runtime_error("accumulate needs the caller's gradient buffers");
  Inputs in(means3D, colors, sem, activate ? opacity : c10::nullopt, scales, rotations, scale_modifier, cov3D, sh,
            degree, !cam_frames.empty());
  if (activate) in.g.flags |= GS_FLAG_ACTIVATE;
  if (accumulate) in.g.flags |= GS_FLAG_ACCUMULATE;
  const int64_t C = (int64_t)cx.size(), P = in.P;
  // rasterize_points.cu:160-161 takes H, W from dL_dout_color; an absent
  // upstream gradient counts as zeros, sized from the alpha image
  const Tensor& img_ref = present(dL_color) ? *dL_color : alphas;
  const int64_t H = img_ref.size(-2), W = img_ref.size(-1);
  Cameras k(in.dev, bg, views, projs, campos, cx, cy, tx, ty, W, H, windows);
  const Window win(cam_frames, C, in.B);
  Tensor gm;
  set_grad_mask(in, grad_mask, gm);
  Tensor dLc = batch_image(dL_color, C, 3, H, W, in.dev, "dL_dout_color");
  Tensor dLd = batch_image(dL_depth, C, 1, H, W, in.dev, "dL_dout_depth");
  Tensor dLa = batch_image(dL_alpha, C, 1, H, W, in.dev, "dL_dout_alpha");
  Tensor dLf = in.F ? batch_image(dL_feature, C, in.F, H, W, in.dev, "dL_dout_feature") : Tensor();
  Tensor alphas_c = dev_f32(alphas, in.dev, "alpha");
  Tensor radii_c = radii.to(in.dev, at::kInt).contiguous();
  if (radii_c.dim() != 2 || radii_c.size(0) != C || radii_c.size(1) != P)
    throw std::runtime_error("radii must be [C=" + std::to_string(C) + ", P=" + std::to_string(P) + "]");
  if ((int64_t)num_instances.size() != C) throw std::runtime_error("num_instances must have C entries");
  std::vector<Tensor> o = gradient_outputs(in, out, exact_out, win.ptr != nullptr);
  set_densify(in, densify);
  // the scratch: the caller's (kept from the forward, which may have zeroed
  // it: scratch_zeroed -> GS_FLAG_SCRATCH_ZEROED) or a fresh one
  const int64_t nscr = (int64_t)gs_batch_backward_scratch_bytes(P, (int32_t)in.F, (int32_t)C);
  Tensor scratch;
  if (present(scratch_in)) {
    scratch = *scratch_in;
    if (scratch.device() != in.dev || !scratch.is_contiguous() || scratch.numel() * scratch.element_size() < nscr)
      throw std::runtime_error("scratch must be a contiguous device tensor of " + std::to_string(nscr) + " bytes");
    if (scratch_zeroed) in.g.flags |= GS_FLAG_SCRATCH_ZEROED;
  } else {
    scratch = at::empty({nscr}, at::TensorOptions().dtype(at::kByte).device(in.dev));
  }
  const Tensor bin = binning.has_value() ? *binning : Tensor();
  auto fp = [](const Tensor& t) -> const float* { return t.defined() ? t.data_ptr<float>() : nullptr; };
  check(gs_backward_batch_window(&in.g, k.cams.data(), (int32_t)C, radii_c.data_ptr<int32_t>(), debug ? 1 : 0,
                                 (int)compat, geom.data_ptr(), nz(bin), img.data_ptr(), num_instances.data(),
                                 alphas_c.data_ptr<float>(), fp(dLc), fp(dLf), fp(dLd), fp(dLa), scratch.data_ptr(),
                                 o[0].data_ptr<float>(), o[1].data_ptr<float>(), static_cast<float*>(nz(o[2])),
                                 o[3].data_ptr<float>(), o[4].data_ptr<float>(), o[5].data_ptr<float>(),
                                 static_cast<float*>(nz(o[6])), o[7].data_ptr<float>(), o[8].data_ptr<float>(), win.ptr,
                                 reinterpret_cast<gs_stream_t>(stream)),
        "rasterize_gaussians_batch_backward");
  if (in.F_user != in.F) o[2] = o[2].narrow(1, 0, in.F_user);
  return o;
}

// The gradients of the C cameras (gs_camera_grad.h), after backward_batch on
// the same stream with the same inputs, from the `scratch` that call wrote:
// (dL_dview [C,16], dL_dproj [C,16], dL_dcampos [C,3]).
std::tuple<Tensor, Tensor, Tensor> camera_grad_batch(
    const Tensor& bg, const Tensor& means3D, const Tensor& radii, const OptT& cov3D, const Tensor& views,
    const Tensor& projs, const std::vector<double>& cx, const std::vector<double>& cy, const std::vector<double>& tx,
    const std::vector<double>& ty, int64_t H, int64_t W, const OptT& sh, int64_t degree, const Tensor& campos,
    const Tensor& geom, const Tensor& scratch, int64_t compat, const std::vector<std::vector<int64_t>>& windows,
    const std::vector<int64_t>& cam_frames, int64_t stream) {
  Inputs in(means3D, c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt, c10::nullopt, 1.0, cov3D, sh, degree,
            !cam_frames.empty());
  const int64_t C = (int64_t)cx.size(), P = in.P;
  Cameras k(in.dev, bg, views, projs, campos, cx, cy, tx, ty, W, H, windows);
  const Window win(cam_frames, C, in.B);
  Tensor radii_c = radii.to(in.dev, at::kInt).contiguous();
  if (P > 0 && (radii_c.dim() != 2 || radii_c.size(0) != C || radii_c.size(1) != P))
    throw std::runtime_error("radii must be [C=" + std::to_string(C) + ", P=" + std::to_string(P) + "]");
  if (P > 0) {
    const int64_t nscr = (int64_t)gs_batch_backward_scratch_bytes(P, 0, (int32_t)C);
    if (scratch.device() != in.dev || !scratch.is_contiguous() || scratch.numel() * scratch.element_size() < nscr ||
        geom.device() != in.dev || geom.numel() < (int64_t)gs_batch_geom_buffer_bytes(P, (int32_t)C))
      throw std::runtime_error("camera_grad_batch: geom and scratch must be the forward's and the backward's buffers");
  }
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(in.dev);
  Tensor dview = at::empty({C, 16}, f32), dproj = at::empty({C, 16}, f32), dcpos = at::empty({C, 3}, f32);
  const int64_t nws = (int64_t)gs_camera_grad_workspace_bytes(P, (int32_t)C);
  Tensor ws = at::empty({nws > 16 ? nws : 16}, f32.dtype(at::kByte));
  check(gs_camera_grad_batch(&in.g, k.cams.data(), (int32_t)C, win.ptr, P ? radii_c.data_ptr<int32_t>() : nullptr,
                             (int)compat, nz(geom), nz(scratch), ws.data_ptr(), (uint64_t)ws.numel(),
                             dview.data_ptr<float>(), dproj.data_ptr<float>(), dcpos.data_ptr<float>(),
                             reinterpret_cast<gs_stream_t>(stream)),
        "camera_grad_batch");
  return {dview, dproj, dcpos};
}

// The K largest blend weights of every pixel and their Gaussians
// (gs_track.h), after forward_batch on the same stream from the state buffers
// that call returned: (top_id int32 [C,K,H,W], top_w [C,K,H,W]).
std::tuple<Tensor, Tensor> contributors_batch(
    const Tensor& geom, const OptT& binning, const Tensor& img, const std::vector<int64_t>& num_instances,
    const Tensor& bg, const Tensor& views, const Tensor& projs, const std::vector<double>& cx,
    const std::vector<double>& cy, const std::vector<double>& tx, const std::vector<double>& ty, int64_t H, int64_t W,
    const Tensor& campos, int64_t P, int64_t K, int64_t compat, const std::vector<std::vector<int64_t>>& windows,
    int64_t stream) {
  const at::Device dev = views.device();
  Cameras k(dev, bg, views, projs, campos, cx, cy, tx, ty, W, H, windows);
  const int64_t C = (int64_t)k.cams.size();
  if ((int64_t)num_instances.size() != C) throw std::runtime_error("num_instances must have C entries");
  if (K < 1 || K > GS_TRACK_MAX_K)
    throw std::runtime_error("K = " + std::to_string(K) + " outside 1.." + std::to_string(GS_TRACK_MAX_K));
  const Tensor bin = binning.has_value() ? *binning : Tensor();
  if (P > 0) {
    if (geom.device() != dev || img.device() != dev || (bin.defined() && bin.numel() && bin.device() != dev))
      throw std::runtime_error("contributors_batch: the state buffers must be on the cameras' device");
    if (geom.numel() < (int64_t)gs_batch_geom_buffer_bytes(P, (int32_t)C) ||
        img.numel() < (int64_t)gs_batch_image_buffer_bytes((int32_t)W, (int32_t)H, (int32_t)C) ||
        (bin.defined() ? bin.numel() : 0) < (int64_t)gs_batch_binning_buffer_bytes((int32_t)C, num_instances.data()))
      throw std::runtime_error("contributors_batch: geom, binning and img must be the forward's buffers for P, the "
                               "image size and num_instances");
  }
  const auto opt = at::TensorOptions().device(dev);
  Tensor top_id = at::empty({C, K, H, W}, opt.dtype(at::kInt));
  Tensor top_w = at::empty({C, K, H, W}, opt.dtype(at::kFloat));
  check(gs_contributors_batch(k.cams.data(), (int32_t)C, P, (int)compat, nz(geom), nz(bin), nz(img),
                              num_instances.data(), (int32_t)K, static_cast<int32_t*>(nz(top_id)),
                              static_cast<float*>(nz(top_w)), reinterpret_cast<gs_stream_t>(stream)),
        "contributors_batch");
  return {top_id, top_w};
}

// means3D [T,P,3] and ids [N] through the C cameras (gs_track.h):
// (uv [T,C,N,2], depth [T,C,N], inside bool [T,C,N]).
std::tuple<Tensor, Tensor, Tensor> track_project(
    const Tensor& means3D, const Tensor& ids, const Tensor& bg, const Tensor& views, const Tensor& projs,
    const std::vector<double>& cx, const std::vector<double>& cy, const std::vector<double>& tx,
    const std::vector<double>& ty, int64_t H, int64_t W, const Tensor& campos, int64_t stream) {
  if (means3D.dim() != 3 || means3D.size(2) != 3)
    throw std::runtime_error("means3D must have dimensions (timesteps, num_points, 3)");
  const at::Device dev = means3D.device();
  Tensor m = dev_f32(means3D, dev, "means3D");
  if (ids.device() != dev || ids.dim() != 1) throw std::runtime_error("ids must be a 1-D tensor on means3D's device");
  Tensor id32 = ids.to(at::kInt).contiguous();
  Cameras k(dev, bg, views, projs, campos, cx, cy, tx, ty, W, H, {});
  const int64_t C = (int64_t)k.cams.size(), T = m.size(0), P = m.size(1), N = id32.size(0);
  const auto opt = at::TensorOptions().device(dev);
  Tensor uv = at::empty({T, C, N, 2}, opt.dtype(at::kFloat));
  Tensor depth = at::empty({T, C, N}, opt.dtype(at::kFloat));
  Tensor inside = at::empty({T, C, N}, opt.dtype(at::kBool));
  check(gs_track_project(k.cams.data(), (int32_t)C, P, (int32_t)T, static_cast<const float*>(nz(m)),
                         static_cast<const int32_t*>(nz(id32)), N, static_cast<float*>(nz(uv)),
                         static_cast<float*>(nz(depth)), static_cast<uint8_t*>(nz(inside)),
                         reinterpret_cast<gs_stream_t>(stream)),
        "track_project");
  return {uv, depth, inside};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "the binding of dynamic3dgaussians_amd._C (C++ over the gsplat_hip C ABI)";
  m.def("abi_version", []() { return gs_version(); });
  m.def("forward_batch", &forward_batch);
  m.def("backward_batch", &backward_batch);
  m.def("camera_grad_batch", &camera_grad_batch);
  m.def("contributors_batch", &contributors_batch);
  m.def("track_project", &track_project);
}

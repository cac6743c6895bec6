// torch.ops.be.*: the C entry points of libblurry_edges_hip registered as PyTorch operators (north_star: "hand-written HIP C++
// kernels ... exposed as torch extensions").  This file is host-only glue over the C ABI of include/blurry_edges_hip.h - it
// allocates outputs with torch, takes the current stream from torch and calls the same symbols the ctypes binding
// (be_hip/native.py) calls; the C ABI stays the language-neutral boundary.  Registered for the LocalStage hot path: the packed
// inference forward (models/local_stage.py:63-73), pass-A colours and the depth solve (bench.py's step), and the training
// units, pooling, loss and optimizer tail of the training step (local_training.py:103-108).
// Host structs of the C ABI (be_render_opts, be_depth_consts, the device-side job tables) travel as byte tensors.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../include/blurry_edges_hip.h"

namespace {

using at::Tensor;
using c10::optional;

void* stream_of(const Tensor& t) {
    // arguments are evaluated in any order: refuse a CPU tensor here too, before its device index reaches the HIP runtime
    TORCH_CHECK(t.is_cuda(), "expected a tensor on the GPU; the HIP path has no CPU fallback");
    return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

const float* fp(const Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda(), what, ": expected a tensor on the GPU; the HIP path has no CPU fallback");
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous(), what, ": expected a contiguous float32 tensor");
    return t.data_ptr<float>();
}
float* fpm(const Tensor& t, const char* what) { return const_cast<float*>(fp(t, what)); }
const float* fpo(const optional<Tensor>& t, const char* what) { return t.has_value() && t->defined() ? fp(*t, what) : nullptr; }

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, what, ": ", be_last_error()); }

template <class T>
const T* host_struct(const Tensor& bytes, const char* what) {
    TORCH_CHECK(!bytes.is_cuda() && bytes.scalar_type() == at::kByte && bytes.is_contiguous() && (size_t)bytes.numel() >= sizeof(T), what,
                ": expected a CPU uint8 tensor holding the C struct");
    return reinterpret_cast<const T*>(bytes.data_ptr<uint8_t>());
}

// ---- inference -----------------------------------------------------------------------------------------------------------
Tensor local_stage_pack(at::TensorList tensors, double eps) {
    TORCH_CHECK(tensors.size() == 86, "local_stage_pack: 86 tensors expected (native.local_stage_pack order)");
    std::vector<const float*> ptrs;
    std::vector<Tensor> keep;
    for (const Tensor& t : tensors) { keep.push_back(t.contiguous()); ptrs.push_back(fp(keep.back(), "local_stage_pack")); }
    Tensor packed = at::empty({(int64_t)be_local_stage_packed_floats()}, keep[0].options());
    check(be_local_stage_pack_f32(ptrs.data(), (float)eps, packed.data_ptr<float>(), stream_of(packed)), "be_local_stage_pack_f32");
    return packed;
}

std::tuple<Tensor, Tensor> local_stage_forward(const Tensor& packed, const Tensor& x, const optional<Tensor>& out_,
                                               const optional<Tensor>& workspace_, bool winograd, int64_t chunk) {
    TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 && x.size(2) == BE_R && x.size(3) == BE_R, "local_stage_forward: x must be [N,3,21,21]");
    const int64_t n = x.size(0);
    Tensor out = out_.has_value() && out_->defined() ? *out_ : at::empty({n, 10}, x.options());
    const size_t need = be_local_stage_workspace_bytes(n, (int64_t)chunk);
    Tensor ws = workspace_.has_value() && workspace_->defined() && (size_t)workspace_->numel() * 4 >= need
                    ? *workspace_ : at::empty({(int64_t)((need + 3) / 4)}, x.options());
    be_local_stage_opts o{winograd ? 1 : 0, (int)chunk};
    check(be_local_stage_forward_f32(fp(packed, "packed"), fp(x, "x"), fpm(out, "out"), n, ws.data_ptr<float>(), (size_t)ws.numel() * 4, &o,
                                     stream_of(x)), "be_local_stage_forward_f32");
    return {out, ws};
}

Tensor render_colors(const Tensor& opts, const Tensor& params10, const Tensor& patches, const optional<Tensor>& colors_) {
    TORCH_CHECK(params10.is_cuda() && patches.is_cuda(), "render_colors: expected tensors on the GPU; the HIP path has no CPU fallback");
    const int64_t n = params10.size(0);
    TORCH_CHECK(params10.dim() == 2 && params10.size(1) == 10 && patches.numel() == n * 3 * BE_NPIX, "render_colors: params10 [N,10], patches [N,3,21,21]");
    Tensor colors = colors_.has_value() && colors_->defined() ? *colors_ : at::empty({n, 3, 3}, params10.options());
    check(be_render_colors_f32(host_struct<be_render_opts>(opts, "render_colors(opts)"), fp(params10, "params10"), fp(patches, "patches"),
                               fpm(colors, "colors"), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n, stream_of(params10)),
          "be_render_colors_f32");
    return colors;
}

Tensor local_depth(const Tensor& consts, const Tensor& params10, const optional<Tensor>& out_) {
    TORCH_CHECK(params10.is_cuda(), "local_depth: expected a tensor on the GPU; the HIP path has no CPU fallback");
    TORCH_CHECK(params10.dim() == 2 && params10.size(1) == 10 && params10.size(0) % 2 == 0, "local_depth: params10 [2P,10]");
    const int64_t p = params10.size(0) / 2;
    Tensor out = out_.has_value() && out_->defined() ? *out_ : at::empty({p, 2}, params10.options());
    check(be_local_depth_f32(host_struct<be_depth_consts>(consts, "local_depth(consts)"), fp(params10, "params10"), fpm(out, "out"), p,
                             stream_of(params10)), "be_local_depth_f32");
    return out;
}

// ---- training ------------------------------------------------------------------------------------------------------------
// conv / linear + BatchNorm (batch statistics) [+ res] [+ Smish]: -> (out, y, mean, invstd, s_in or an empty tensor)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> train_unit_fwd(const Tensor& x, const Tensor& pw, const Tensor& pb, const Tensor& gamma,
                                                                  const Tensor& beta, const optional<Tensor>& res, Tensor run_mean,
                                                                  Tensor run_var, int64_t cout, int64_t ksize, bool act, double eps,
                                                                  double momentum, Tensor scratch) {
    TORCH_CHECK(x.dim() == 4, "train_unit_fwd: x must be NHWC [N,H,W,C]");
    const int64_t n = x.size(0), h = x.size(1), w = x.size(2), cin = x.size(3);
    Tensor y = at::empty({n, h, w, cout}, x.options()), out = at::empty_like(y);
    Tensor s_in = act ? at::empty_like(y) : at::empty({0}, x.options());
    Tensor mean = at::empty({cout}, x.options()), invstd = at::empty({cout}, x.options());
    be_conv_desc d{(int)n, (int)h, (int)w, (int)cin, (int)cout, (int)ksize, 0};
    check(be_train_unit_fwd_f32(&d, fp(x, "x"), fp(pw, "packed_w"), fp(pb, "packed_bias"), fp(gamma, "gamma"), fp(beta, "beta"), fpo(res, "res"),
                                (float)eps, (float)momentum, fpm(run_mean, "run_mean"), fpm(run_var, "run_var"), y.data_ptr<float>(),
                                mean.data_ptr<float>(), invstd.data_ptr<float>(), act ? s_in.data_ptr<float>() : nullptr,
                                out.data_ptr<float>(), act ? 1 : 0, scratch.data_ptr<float>(), (size_t)scratch.numel() * 4, stream_of(x)),
          "be_train_unit_fwd_f32");
    return {out, y, mean, invstd, s_in};
}

// backward of the unit; the four parameter gradients are written into the given slices of the flat gradient buffer
std::tuple<Tensor, Tensor> train_unit_bwd(const Tensor& x, const Tensor& dout, const optional<Tensor>& s_in, const Tensor& y, const Tensor& mean,
                                          const Tensor& invstd, const Tensor& gamma, const optional<Tensor>& dg_pw,
                                          const optional<Tensor>& dg_pb, const optional<Tensor>& dx_add, int64_t ksize, int64_t chw_hw,
                                          Tensor dgamma, Tensor dbeta, Tensor dw, Tensor db, Tensor scratch) {
    const int64_t n = x.size(0), h = x.size(1), w = x.size(2), cin = x.size(3), cout = y.size(-1);
    Tensor ds = at::empty_like(y), dy = at::empty_like(y);
    const bool want_dx = dg_pw.has_value() && dg_pw->defined();
    Tensor dx = want_dx ? at::empty({n, h, w, cin}, x.options()) : at::empty({0}, x.options());
    be_conv_desc d{(int)n, (int)h, (int)w, (int)cin, (int)cout, (int)ksize, 0};
    const bool has_s = s_in.has_value() && s_in->defined() && s_in->numel() > 0;
    check(be_train_unit_bwd_f32(&d, fp(x, "x"), fp(dout, "dout"), has_s ? fp(*s_in, "s_in") : nullptr, fp(y, "y"), fp(mean, "mean"),
                                fp(invstd, "invstd"), fp(gamma, "gamma"), want_dx ? fp(*dg_pw, "dgrad_w") : nullptr,
                                want_dx ? fpo(dg_pb, "dgrad_b") : nullptr, fpo(dx_add, "dx_add"), (int)chw_hw, ds.data_ptr<float>(),
                                dy.data_ptr<float>(), fpm(dgamma, "dgamma"), fpm(dbeta, "dbeta"), fpm(dw, "dw"), fpm(db, "db"),
                                want_dx ? dx.data_ptr<float>() : nullptr, scratch.data_ptr<float>(), (size_t)scratch.numel() * 4, stream_of(x)),
          "be_train_unit_bwd_f32");
    return {ds, dx};
}

// two units on one input with shared launches (a residual block's 3x3 convolution and 1x1 downsample): the outputs of two
// train_unit_fwd calls, a's five then b's five
std::vector<Tensor> train_unit_pair_fwd(const Tensor& x, const Tensor& pw_a, const Tensor& pb_a, const Tensor& gamma_a, const Tensor& beta_a,
                                        Tensor rm_a, Tensor rv_a, int64_t cout_a, int64_t ks_a, bool act_a, const Tensor& pw_b,
                                        const Tensor& pb_b, const Tensor& gamma_b, const Tensor& beta_b, Tensor rm_b, Tensor rv_b,
                                        int64_t cout_b, int64_t ks_b, bool act_b, double eps, double momentum, Tensor scratch) {
    TORCH_CHECK(x.dim() == 4, "train_unit_pair_fwd: x must be NHWC [N,H,W,C]");
    const int64_t n = x.size(0), h = x.size(1), w = x.size(2), cin = x.size(3);
    std::vector<Tensor> r;
    be_train_unit_fwd u[2];
    const Tensor* pw[2] = {&pw_a, &pw_b}; const Tensor* pb[2] = {&pb_a, &pb_b};
    const Tensor* ga[2] = {&gamma_a, &gamma_b}; const Tensor* be[2] = {&beta_a, &beta_b};
    Tensor* rm[2] = {&rm_a, &rm_b}; Tensor* rv[2] = {&rv_a, &rv_b};
    const int64_t cout[2] = {cout_a, cout_b}, ks[2] = {ks_a, ks_b};
    const bool act[2] = {act_a, act_b};
    for (int j = 0; j < 2; ++j) {
        Tensor y = at::empty({n, h, w, cout[j]}, x.options()), out = at::empty_like(y);
        Tensor s_in = act[j] ? at::empty_like(y) : at::empty({0}, x.options());
        Tensor mean = at::empty({cout[j]}, x.options()), invstd = at::empty({cout[j]}, x.options());
        u[j] = be_train_unit_fwd{be_conv_desc{(int)n, (int)h, (int)w, (int)cin, (int)cout[j], (int)ks[j], 0}, fp(x, "x"), fp(*pw[j], "packed_w"),
                                 fp(*pb[j], "packed_bias"), fp(*ga[j], "gamma"), fp(*be[j], "beta"), nullptr, fpm(*rm[j], "run_mean"),
                                 fpm(*rv[j], "run_var"), y.data_ptr<float>(), mean.data_ptr<float>(), invstd.data_ptr<float>(),
                                 act[j] ? s_in.data_ptr<float>() : nullptr, out.data_ptr<float>(), act[j] ? 1 : 0};
        r.insert(r.end(), {out, y, mean, invstd, s_in});
    }
    check(be_train_unit_pair_fwd_f32(&u[0], &u[1], (float)eps, (float)momentum, scratch.data_ptr<float>(), (size_t)scratch.numel() * 4,
                                     stream_of(x)), "be_train_unit_pair_fwd_f32");
    return r;
}

// backward of the pair: -> (ds_a, ds_b, dx) with dx = the sum of the two units' input gradients
std::vector<Tensor> train_unit_pair_bwd(const Tensor& x, const Tensor& dout_a, const optional<Tensor>& s_in_a, const Tensor& y_a,
                                        const Tensor& mean_a, const Tensor& invstd_a, const Tensor& gamma_a, const Tensor& dg_pw_a,
                                        const Tensor& dg_pb_a, int64_t ks_a, Tensor dgamma_a, Tensor dbeta_a, Tensor dw_a, Tensor db_a,
                                        const Tensor& dout_b, const optional<Tensor>& s_in_b, const Tensor& y_b, const Tensor& mean_b,
                                        const Tensor& invstd_b, const Tensor& gamma_b, const Tensor& dg_pw_b, const Tensor& dg_pb_b,
                                        int64_t ks_b, Tensor dgamma_b, Tensor dbeta_b, Tensor dw_b, Tensor db_b, Tensor scratch) {
    const int64_t n = x.size(0), h = x.size(1), w = x.size(2), cin = x.size(3);
    const Tensor* dout[2] = {&dout_a, &dout_b}; const optional<Tensor>* s_in[2] = {&s_in_a, &s_in_b};
    const Tensor* y[2] = {&y_a, &y_b}; const Tensor* mean[2] = {&mean_a, &mean_b}; const Tensor* invstd[2] = {&invstd_a, &invstd_b};
    const Tensor* gamma[2] = {&gamma_a, &gamma_b}; const Tensor* pw[2] = {&dg_pw_a, &dg_pw_b}; const Tensor* pb[2] = {&dg_pb_a, &dg_pb_b};
    Tensor* dgamma[2] = {&dgamma_a, &dgamma_b}; Tensor* dbeta[2] = {&dbeta_a, &dbeta_b}; Tensor* dw[2] = {&dw_a, &dw_b};
    Tensor* db[2] = {&db_a, &db_b};
    const int64_t ks[2] = {ks_a, ks_b};
    be_train_unit_bwd u[2];
    std::vector<Tensor> ds, dy, dx;
    for (int j = 0; j < 2; ++j) {
        ds.push_back(at::empty_like(*y[j])); dy.push_back(at::empty_like(*y[j])); dx.push_back(at::empty({n, h, w, cin}, x.options()));
        const bool has_s = s_in[j]->has_value() && (*s_in[j])->defined() && (*s_in[j])->numel() > 0;
        u[j] = be_train_unit_bwd{be_conv_desc{(int)n, (int)h, (int)w, (int)cin, (int)y[j]->size(-1), (int)ks[j], 0}, fp(x, "x"), fp(*dout[j], "dout"),
                                 has_s ? fp(**s_in[j], "s_in") : nullptr, fp(*y[j], "y"), fp(*mean[j], "mean"), fp(*invstd[j], "invstd"),
                                 fp(*gamma[j], "gamma"), fp(*pw[j], "dgrad_w"), fp(*pb[j], "dgrad_b"), nullptr, 0, ds[j].data_ptr<float>(),
                                 dy[j].data_ptr<float>(), fpm(*dgamma[j], "dgamma"), fpm(*dbeta[j], "dbeta"), fpm(*dw[j], "dw"), fpm(*db[j], "db"),
                                 dx[j].data_ptr<float>()};
    }
    check(be_train_unit_pair_bwd_f32(&u[0], &u[1], scratch.data_ptr<float>(), (size_t)scratch.numel() * 4, stream_of(x)),
          "be_train_unit_pair_bwd_f32");
    return {ds[0], ds[1], dx[0]};
}

std::tuple<Tensor, Tensor> maxpool_fwd_idx(const Tensor& x, int64_t k, int64_t stride, int64_t pad) {
    TORCH_CHECK(x.dim() == 4, "maxpool_fwd_idx: x must be NHWC [N,H,W,C]");
    const int64_t n = x.size(0), h = x.size(1), w = x.size(2), c = x.size(3);
    const int64_t oh = (h + 2 * pad - k) / stride + 1, ow = (w + 2 * pad - k) / stride + 1;
    Tensor y = at::empty({n, oh, ow, c}, x.options()), idx = at::empty({n, oh, ow, c}, x.options().dtype(at::kByte));
    check(be_maxpool_nhwc_fwd_idx_f32(fp(x, "x"), y.data_ptr<float>(), idx.data_ptr<uint8_t>(), (int)n, (int)h, (int)w, (int)c, (int)k, (int)stride,
                                      (int)pad, stream_of(x)), "be_maxpool_nhwc_fwd_idx_f32");
    return {y, idx};
}

Tensor maxpool_bwd_idx(const Tensor& idx, const Tensor& dout, int64_t h, int64_t w, int64_t k, int64_t stride, int64_t pad) {
    TORCH_CHECK(dout.dim() == 4 && idx.is_cuda() && idx.scalar_type() == at::kByte && idx.is_contiguous() && idx.numel() == dout.numel(),
                "maxpool_bwd_idx: dout [N,oh,ow,C] float32 and idx = the uint8 winners of maxpool_fwd_idx (same shape) on the GPU");
    const int64_t n = dout.size(0), c = dout.size(3);
    Tensor dx = at::empty({n, h, w, c}, dout.options());
    check(be_maxpool_nhwc_bwd_idx_f32(idx.data_ptr<uint8_t>(), fp(dout, "dout"), dx.data_ptr<float>(), (int)n, (int)h, (int)w, (int)c, (int)k,
                                      (int)stride, (int)pad, stream_of(dout)), "be_maxpool_nhwc_bwd_idx_f32");
    return dx;
}

// clip_grad_norm_(max_norm) + AdamW over the flat gradient buffer; returns nothing (grad_norm is written in place)
void clip_adamw(const Tensor& table, int64_t nentries, Tensor grad_flat, Tensor partial, double max_norm, double grad_scale, double lr,
                double beta1, double beta2, double eps, double weight_decay, Tensor step, Tensor grad_norm, bool write_back) {
    TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kByte && partial.scalar_type() == at::kDouble, "clip_adamw: table (uint8) / partial (float64)");
    check(be_clip_adamw_f32(reinterpret_cast<const be_adam_entry*>(table.data_ptr<uint8_t>()), (int)nentries, fpm(grad_flat, "grad_flat"),
                            grad_flat.numel(), partial.data_ptr<double>(), (int)partial.numel(), (float)max_norm, (float)grad_scale, lr, beta1,
                            beta2, eps, weight_decay, fpm(step, "step"), fpm(grad_norm, "grad_norm"), write_back ? 1 : 0, stream_of(grad_flat)),
          "be_clip_adamw_f32");
}


// ---- the fine-grained PostProcess / DepthEtas methods and their adjoints (be_compat.hip, be_compat_bwd.hip, be_elementwise.hip) ------
// flat one-row-per-patch layouts; the Python classes permute the reference's [B,K,...,Hp,Wp] layout to and from them
Tensor params2etas(const Tensor& p) {
    Tensor out = at::empty_like(p);
    check(be_params2etas_f32(fp(p, "params"), out.data_ptr<float>(), p.numel(), stream_of(p)), "be_params2etas_f32");
    return out;
}
Tensor params2etas_bwd(const Tensor& p, const Tensor& geta) {
    TORCH_CHECK(geta.numel() == p.numel(), "params2etas_bwd: cotangent size");
    Tensor gp = at::empty_like(p);
    check(be_params2etas_bwd_f32(fp(p, "params"), fp(geta, "geta"), gp.data_ptr<float>(), p.numel(), stream_of(p)), "be_params2etas_bwd_f32");
    return gp;
}
Tensor params2dists(const Tensor& opts, const Tensor& params8) {
    TORCH_CHECK(params8.dim() == 2 && params8.size(1) == 8, "params2dists: params8 [N,8]");
    const int64_t n = params8.size(0);
    fp(params8, "params8");
    Tensor out = at::empty({n, 2, BE_R, BE_R}, params8.options());
    check(be_params2dists_f32(host_struct<be_render_opts>(opts, "params2dists(opts)"), params8.data_ptr<float>(), out.data_ptr<float>(), n,
                              stream_of(params8)), "be_params2dists_f32");
    return out;
}
Tensor params2dists_bwd(const Tensor& opts, const Tensor& params8, const Tensor& gdists) {
    TORCH_CHECK(params8.dim() == 2 && params8.size(1) == 8, "params2dists_bwd: params8 [N,8]");
    const int64_t n = params8.size(0);
    TORCH_CHECK(gdists.numel() == n * 2 * BE_NPIX, "params2dists_bwd: gdists [N,2,21,21]");
    fp(params8, "params8");
    Tensor g = at::empty_like(params8);
    check(be_params2dists_bwd_f32(host_struct<be_render_opts>(opts, "params2dists_bwd(opts)"), params8.data_ptr<float>(), fp(gdists, "gdists"),
                                  g.data_ptr<float>(), n, stream_of(params8)), "be_params2dists_bwd_f32");
    return g;
}
Tensor dists2indicators(const Tensor& dists, const Tensor& etas) {
    const int64_t n = etas.numel() / 2;
    TORCH_CHECK(dists.numel() == n * 2 * BE_NPIX && etas.numel() == 2 * n, "dists2indicators: dists [N,2,21,21], etas [N,2]");
    Tensor out = at::empty({n, 3, BE_R, BE_R}, dists.options());
    check(be_dists2indicators_f32(fp(dists, "dists"), fp(etas, "etas"), out.data_ptr<float>(), n, stream_of(dists)), "be_dists2indicators_f32");
    return out;
}
std::tuple<Tensor, Tensor> dists2indicators_bwd(const Tensor& dists, const Tensor& etas, const Tensor& gw) {
    const int64_t n = etas.numel() / 2;
    TORCH_CHECK(dists.numel() == n * 2 * BE_NPIX && gw.numel() == n * 3 * BE_NPIX, "dists2indicators_bwd: dists [N,2,21,21], gwedges [N,3,21,21]");
    Tensor gd = at::empty_like(dists), ge = at::empty_like(etas);
    check(be_dists2indicators_bwd_f32(fp(dists, "dists"), fp(etas, "etas"), fp(gw, "gwedges"), gd.data_ptr<float>(), ge.data_ptr<float>(), n,
                                      stream_of(dists)), "be_dists2indicators_bwd_f32");
    return {gd, ge};
}
Tensor inverse3x3(const Tensor& a) {
    TORCH_CHECK(a.numel() % 9 == 0, "inverse3x3: [...,3,3]");
    Tensor out = at::empty_like(a);
    check(be_inverse3x3_f32(fp(a, "A"), out.data_ptr<float>(), a.numel() / 9, stream_of(a)), "be_inverse3x3_f32");
    return out;
}
Tensor inverse3x3_bwd(const Tensor& inv, const Tensor& gout) {
    TORCH_CHECK(inv.numel() % 9 == 0 && gout.numel() == inv.numel(), "inverse3x3_bwd: [...,3,3]");
    Tensor ga = at::empty_like(inv);
    check(be_inverse3x3_bwd_f32(fp(inv, "inv"), fp(gout, "gout"), ga.data_ptr<float>(), inv.numel() / 9, stream_of(inv)), "be_inverse3x3_bwd_f32");
    return ga;
}
Tensor image_derivative(const Tensor& img) {
    TORCH_CHECK(img.dim() == 4, "image_derivative: img [N,C,H,W]");
    const int64_t n = img.size(0), c = img.size(1), h = img.size(2), w = img.size(3);
    Tensor out = at::empty({n, c, h - 2, w - 2}, img.options());
    check(be_image_derivative_f32(fp(img, "img"), out.data_ptr<float>(), n * c, (int)h, (int)w, stream_of(img)), "be_image_derivative_f32");
    return out;
}
Tensor image_derivative_bwd(const Tensor& img, const Tensor& gout) {
    TORCH_CHECK(img.dim() == 4, "image_derivative_bwd: img [N,C,H,W]");
    const int64_t n = img.size(0), c = img.size(1), h = img.size(2), w = img.size(3);
    TORCH_CHECK(gout.numel() == n * c * (h - 2) * (w - 2), "image_derivative_bwd: gout [N,C,H-2,W-2]");
    Tensor g = at::empty_like(img);
    check(be_image_derivative_bwd_f32(fp(img, "img"), fp(gout, "gout"), g.data_ptr<float>(), n * c, (int)h, (int)w, stream_of(img)),
          "be_image_derivative_bwd_f32");
    return g;
}
Tensor normalized_gaussian(const Tensor& x, double delta_sq) {
    Tensor y = at::empty_like(x);
    check(be_normalized_gaussian_f32(fp(x, "x"), y.data_ptr<float>(), (float)delta_sq, x.numel(), stream_of(x)), "be_normalized_gaussian_f32");
    return y;
}
Tensor normalized_gaussian_bwd(const Tensor& x, const Tensor& gy, double delta_sq) {
    TORCH_CHECK(gy.numel() == x.numel(), "normalized_gaussian_bwd: cotangent size");
    Tensor gx = at::empty_like(x);
    check(be_normalized_gaussian_bwd_f32(fp(x, "x"), fp(gy, "gy"), gx.data_ptr<float>(), (float)delta_sq, x.numel(), stream_of(x)),
          "be_normalized_gaussian_bwd_f32");
    return gx;
}
Tensor etas2depth(const Tensor& consts, const Tensor& eta1, const Tensor& eta2) {
    TORCH_CHECK(eta1.numel() == eta2.numel(), "etas2depth: eta1 / eta2 sizes");
    fp(eta1, "eta1");
    Tensor z = at::empty_like(eta1);
    check(be_etas2depth_f32(host_struct<be_depth_consts>(consts, "etas2depth(consts)"), eta1.data_ptr<float>(), fp(eta2, "eta2"), z.data_ptr<float>(),
                            nullptr, eta1.numel(), stream_of(eta1)), "be_etas2depth_f32");
    return z;
}
std::tuple<Tensor, Tensor> etas2depth_bwd(const Tensor& consts, const Tensor& eta1, const Tensor& eta2, const Tensor& gz) {
    TORCH_CHECK(eta1.numel() == eta2.numel() && gz.numel() == eta1.numel(), "etas2depth_bwd: sizes");
    fp(eta1, "eta1");
    Tensor g1 = at::empty_like(eta1), g2 = at::empty_like(eta1);
    check(be_etas2depth_bwd_f32(host_struct<be_depth_consts>(consts, "etas2depth_bwd(consts)"), eta1.data_ptr<float>(), fp(eta2, "eta2"),
                                fp(gz, "gdepth"), g1.data_ptr<float>(), g2.data_ptr<float>(), eta1.numel(), stream_of(eta1)), "be_etas2depth_bwd_f32");
    return {g1, g2};
}
Tensor depth2sigma(const Tensor& consts, const Tensor& depth, double rho_prime) {
    fp(depth, "depth");
    Tensor out = at::empty_like(depth);
    check(be_depth2sigma_f32(host_struct<be_depth_consts>(consts, "depth2sigma(consts)"), depth.data_ptr<float>(), (float)rho_prime,
                             out.data_ptr<float>(), depth.numel(), stream_of(depth)), "be_depth2sigma_f32");
    return out;
}
Tensor depth2sigma_bwd(const Tensor& consts, const Tensor& depth, double rho_prime, const Tensor& geta) {
    TORCH_CHECK(geta.numel() == depth.numel(), "depth2sigma_bwd: cotangent size");
    fp(depth, "depth");
    Tensor g = at::empty_like(depth);
    check(be_depth2sigma_bwd_f32(host_struct<be_depth_consts>(consts, "depth2sigma_bwd(consts)"), depth.data_ptr<float>(), (float)rho_prime,
                                 fp(geta, "geta"), g.data_ptr<float>(), depth.numel(), stream_of(depth)), "be_depth2sigma_bwd_f32");
    return g;
}
// nn.Fold of a [B,C,21,21,Hp,Wp] patch tensor (contiguous) -> [B,C,H,W]; mode 0 sum, 1 mean, 2 count of positive entries
Tensor fold_patches(const Tensor& src, int64_t B, int64_t C, int64_t hp, int64_t wp, int64_t H, int64_t W, int64_t stride, int64_t mode) {
    TORCH_CHECK(src.is_cuda() && src.is_contiguous(), "fold_patches: expected a contiguous tensor on the GPU; the HIP path has no CPU fallback");
    const int64_t p = hp * wp;
    TORCH_CHECK(src.numel() == B * C * BE_NPIX * p, "fold_patches: src [B,C,21,21,Hp,Wp]");
    const bool is_int = src.scalar_type() == at::kInt;
    TORCH_CHECK(is_int ? mode == 2 : src.scalar_type() == at::kFloat, "fold_patches: float32 source (int32 only for mode 2)");
    Tensor out = at::empty({B, C, H, W}, src.options().dtype(at::kFloat));
    check(be_fold_patches_f32(is_int ? nullptr : src.data_ptr<float>(), is_int ? src.data_ptr<int32_t>() : nullptr, out.data_ptr<float>(), (int)B,
                              (int)C, (int)hp, (int)wp, (int)H, (int)W, (int)stride, C * BE_NPIX * p, BE_NPIX * p, BE_R * p, p, wp, 1, (int)mode,
                              stream_of(src)), "be_fold_patches_f32");
    return out;
}
Tensor fold_patches_bwd(const Tensor& gout, int64_t hp, int64_t wp, int64_t stride, int64_t mode) {
    TORCH_CHECK(gout.dim() == 4, "fold_patches_bwd: gout [B,C,H,W]");
    const int64_t B = gout.size(0), C = gout.size(1), H = gout.size(2), W = gout.size(3), p = hp * wp;
    Tensor g = at::empty({B, C, BE_R, BE_R, hp, wp}, gout.options());
    check(be_fold_patches_bwd_f32(fp(gout, "gout"), g.data_ptr<float>(), (int)B, (int)C, (int)hp, (int)wp, (int)H, (int)W, (int)stride,
                                  C * BE_NPIX * p, BE_NPIX * p, BE_R * p, p, wp, 1, (int)mode, stream_of(gout)), "be_fold_patches_bwd_f32");
    return g;
}
void wrap_angles_(Tensor est, int64_t col0, int64_t col1) {
    TORCH_CHECK(est.dim() == 2, "wrap_angles_: est [N,ld]");
    check(be_wrap_angles_inplace_f32(fpm(est, "est"), est.size(0), (int)est.size(1), (int)col0, (int)col1, stream_of(est)),
          "be_wrap_angles_inplace_f32");
}


// ---- pass B, folds, the two fused losses, attention (the rest of north_star's "exposed as torch extensions") ----------
// a be_patch_view travels as its bytes (it holds the device pointer of `pixels`, which is passed next to it so that the operator
// sees - and keeps alive - the tensor the view points into)
std::vector<Tensor> render_full(const Tensor& opts, const Tensor& consts, double rho_prime, bool densify_w, const Tensor& params12,
                                const Tensor& view, const Tensor& pixels, int64_t want) {
    TORCH_CHECK(params12.dim() == 2 && params12.size(1) == 12, "render_full: params12 [P,12]");
    TORCH_CHECK(pixels.is_cuda(), "render_full: expected the viewed pixels on the GPU; the HIP path has no CPU fallback");
    fp(params12, "params12");
    const int64_t n = params12.size(0);
    const be_patch_view* v = host_struct<be_patch_view>(view, "render_full(view)");
    auto o = params12.options();
    Tensor rec = at::empty({n, BE_RECORD_FLOATS}, o);
    Tensor t[6];
    if (want & 1) t[0] = at::empty({n, 2, 3, BE_R, BE_R}, o);
    if (want & 2) t[1] = at::empty({n, 3, BE_R, BE_R}, o);
    if (want & 4) t[2] = at::empty({n, 3, BE_R, BE_R}, o);
    if (want & 8) t[3] = at::empty({n, BE_R, BE_R}, o);
    if (want & 16) t[4] = at::empty({n, BE_R, BE_R}, o);
    if (want & 32) t[5] = at::empty({n, BE_R, BE_R}, o.dtype(at::kInt));
    auto f = [&](int i) { return t[i].defined() ? t[i].data_ptr<float>() : nullptr; };
    check(be_render_full_f32(host_struct<be_render_opts>(opts, "render_full(opts)"), host_struct<be_depth_consts>(consts, "render_full(consts)"),
                             (float)rho_prime, densify_w ? 1 : 0, params12.data_ptr<float>(), v, rec.data_ptr<float>(), f(0), f(1), f(2), f(3), f(4),
                             t[5].defined() ? t[5].data_ptr<int32_t>() : nullptr, n, stream_of(params12)), "be_render_full_f32");
    std::vector<Tensor> r{rec};
    for (int i = 0; i < 6; ++i) if (t[i].defined()) r.push_back(t[i]);
    return r;
}

// ---- the record folds.  What the operators share: the maps a `want` mask names, the optional origin tables and the checks of
// records / rho_primes / points.  Every message starts with the operator's name (`who`).

// the maps named by `want` (bit 0 image, 1 shpd, 2 refoc, 3 bndry, 4 depth, 5 conf): [batch.., channels.., tail..] with channels
// {2,3} (image; {6} when `flat`), {3} (shpd, refoc) or none (bndry, depth, conf); the others stay undefined (a null pointer)
struct FoldMaps {
    Tensor t[6];
    FoldMaps(int64_t want, const Tensor& like, const std::vector<int64_t>& batch, const std::vector<int64_t>& tail, bool flat = false) {
        const std::vector<int64_t> channels[6] = {flat ? std::vector<int64_t>{6} : std::vector<int64_t>{2, 3}, {3}, {3}, {}, {}, {}};
        for (int i = 0; i < 6; ++i) {
            if (!(want & (1 << i))) continue;
            std::vector<int64_t> s(batch);
            s.insert(s.end(), channels[i].begin(), channels[i].end());
            s.insert(s.end(), tail.begin(), tail.end());
            t[i] = at::empty(s, like.options());
        }
    }
    float* operator[](int i) const { return t[i].defined() ? t[i].data_ptr<float>() : nullptr; }
    std::vector<Tensor> list() const {                          // the requested maps, in bit order
        std::vector<Tensor> r;
        for (int i = 0; i < 6; ++i) if (t[i].defined()) r.push_back(t[i]);
        return r;
    }
};

// a patch grid given by origin tables (ys [HP], xs [WP]: int32 on the GPU) instead of one stride
static const int32_t* origin_table(const Tensor& t, const std::string& what) {
    TORCH_CHECK(t.is_cuda(), what, ": expected the origin table on the GPU; the HIP path has no CPU fallback");
    TORCH_CHECK(t.dim() == 1 && t.numel() > 0 && t.scalar_type() == at::kInt && t.is_contiguous(), what, ": a contiguous int32 vector");
    return t.data_ptr<int32_t>();
}

// ys / xs both given = origin tables, both absent = the uniform grid of `stride` (null pointers)
struct OriginTables { const int32_t* ys = nullptr; const int32_t* xs = nullptr; };
static OriginTables optional_tables(const std::string& who, const optional<Tensor>& ys, const optional<Tensor>& xs, int64_t hp, int64_t wp) {
    OriginTables g;
    if (ys.has_value()) {
        g.ys = origin_table(*ys, who + "(ys)");
        g.xs = origin_table(*xs, who + "(xs)");
        TORCH_CHECK(ys->numel() == hp && xs->numel() == wp, who, ": ys [hp], xs [wp]");
    }
    return g;
}

// what the operators over an optional-table grid check first: the table pair, then the records
static void check_grid_records(const std::string& who, const optional<Tensor>& ys, const optional<Tensor>& xs, const Tensor& records, int64_t hp,
                               int64_t wp) {
    TORCH_CHECK(ys.has_value() == xs.has_value(), who, ": ys and xs must both be given (origin tables) or both be None");
    TORCH_CHECK(records.dim() == 2 && records.size(0) == hp * wp && records.size(1) == BE_RECORD_FLOATS, who, ": records [hp*wp,32]");
}
static void check_rho_primes(const std::string& who, const Tensor& rho_primes, const Tensor& records) {
    TORCH_CHECK(rho_primes.dim() == 1 && rho_primes.numel() > 0, who, ": rho_primes [K], K >= 1");
    TORCH_CHECK(rho_primes.device() == records.device(), who, ": rho_primes and records on one device");
}
static void check_points(const std::string& who, const Tensor& points, const Tensor& records) {
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 2 && points.size(0) > 0, who, ": points [N,2], N >= 1");
    TORCH_CHECK(points.device() == records.device(), who, ": points and records on one device");
}
static void check_lattice(const std::string& who, int64_t scale, int64_t h, int64_t w, int64_t H, int64_t W) {
    TORCH_CHECK(scale >= 1 && scale <= BE_RENDER_AT_MAX_SCALE && h >= 1 && w >= 1 && h <= H && w <= W, who, ": bad scale or window");
}
static const be_render_opts* fold_opts(const std::string& who, const Tensor& opts) { return host_struct<be_render_opts>(opts, (who + "(opts)").c_str()); }
static const be_depth_consts* fold_consts(const std::string& who, const Tensor& consts) {
    return host_struct<be_depth_consts>(consts, (who + "(consts)").c_str());
}

// records [P,32] or [B,P,32] -> the maps named by `want`, in bit order
std::vector<Tensor> fold_records(const Tensor& opts, const Tensor& records, int64_t hp, int64_t wp, int64_t H, int64_t W, int64_t stride,
                                 bool densify_w, int64_t want) {
    fp(records, "records");
    const bool batched = records.dim() == 3;
    TORCH_CHECK((batched || records.dim() == 2) && records.size(-1) == BE_RECORD_FLOATS && records.size(-2) == hp * wp,
                "fold_records: records [P,32] or [B,P,32] with P = hp * wp");
    const int64_t B = batched ? records.size(0) : 1;
    const FoldMaps m(want, records, batched ? std::vector<int64_t>{B} : std::vector<int64_t>{}, {H, W});
    const be_render_opts* ro = fold_opts("fold_records", opts);
    if (batched)
        check(be_fold_records_batch_f32(ro, records.data_ptr<float>(), (int)B, (int)hp, (int)wp, (int)H, (int)W, (int)stride, densify_w ? 1 : 0, m[0],
                                        m[1], m[2], m[3], m[4], m[5], stream_of(records)), "be_fold_records_batch_f32");
    else
        check(be_fold_records_f32(ro, records.data_ptr<float>(), (int)hp, (int)wp, (int)H, (int)W, (int)stride, densify_w ? 1 : 0, m[0], m[1], m[2],
                                  m[3], m[4], m[5], stream_of(records)), "be_fold_records_f32");
    return m.list();
}

// the two passes over a patch grid given by origin tables
Tensor render_full_grid(const Tensor& opts, const Tensor& consts, double rho_prime, bool densify_w, const Tensor& params12,
                        const Tensor& img, const Tensor& ys, const Tensor& xs) {
    TORCH_CHECK(img.dim() == 4 && img.size(0) == 2 && img.size(1) == 3, "render_full_grid: img [2,3,H,W]");
    const int64_t HP = ys.numel(), WP = xs.numel();
    TORCH_CHECK(params12.dim() == 2 && params12.size(0) == HP * WP && params12.size(1) == 12, "render_full_grid: params12 [HP*WP,12]");
    Tensor rec = at::empty({HP * WP, BE_RECORD_FLOATS}, params12.options());
    check(be_render_full_grid_f32(host_struct<be_render_opts>(opts, "render_full_grid(opts)"),
                                  host_struct<be_depth_consts>(consts, "render_full_grid(consts)"), (float)rho_prime, densify_w ? 1 : 0,
                                  fp(params12, "params12"), fp(img, "img"), (int)img.size(2), (int)img.size(3),
                                  origin_table(ys, "render_full_grid(ys)"), origin_table(xs, "render_full_grid(xs)"), (int)HP, (int)WP,
                                  rec.data_ptr<float>(), stream_of(params12)), "be_render_full_grid_f32");
    return rec;
}
std::vector<Tensor> fold_records_grid(const Tensor& opts, const Tensor& records, const Tensor& ys, const Tensor& xs, int64_t H, int64_t W,
                                      bool densify_w, int64_t want) {
    const int64_t HP = ys.numel(), WP = xs.numel();
    TORCH_CHECK(records.dim() == 2 && records.size(0) == HP * WP && records.size(1) == BE_RECORD_FLOATS,
                "fold_records_grid: records [HP*WP,32]");
    fp(records, "records");
    const FoldMaps m(want, records, {}, {H, W});
    check(be_fold_records_grid_f32(fold_opts("fold_records_grid", opts), records.data_ptr<float>(), (int)HP, (int)WP, (int)H, (int)W,
                                   origin_table(ys, "fold_records_grid(ys)"), origin_table(xs, "fold_records_grid(xs)"), densify_w ? 1 : 0,
                                   m[0], m[1], m[2], m[3], m[4], m[5], stream_of(records)), "be_fold_records_grid_f32");
    return m.list();
}

// focal stack: records [hp*wp,32] + rho_primes [K] (fp32 on the GPU) -> [K,3,H,W]
Tensor fold_refocus_stack(const Tensor& opts, const Tensor& consts, const Tensor& records, const Tensor& rho_primes,
                          const c10::optional<Tensor>& ys, const c10::optional<Tensor>& xs, int64_t hp, int64_t wp, int64_t H, int64_t W,
                          int64_t stride) {
    const char* who = "fold_refocus_stack";
    check_grid_records(who, ys, xs, records, hp, wp);
    check_rho_primes(who, rho_primes, records);
    const OriginTables g = optional_tables(who, ys, xs, hp, wp);
    const int64_t K = rho_primes.numel();
    fp(records, "records");
    Tensor out = at::empty({K, 3, H, W}, records.options());
    check(be_fold_refocus_stack_f32(fold_opts(who, opts), fold_consts(who, consts), records.data_ptr<float>(), (int)hp, (int)wp, (int)H, (int)W,
                                    (int)stride, g.ys, g.xs, fp(rho_primes, "rho_primes"), (int)K, out.data_ptr<float>(), stream_of(records)),
          "be_fold_refocus_stack_f32");
    return out;
}

// the folds on a lattice `scale` times finer over the window (top, left, h, w); maps [..,Ho,Wo]
std::vector<Tensor> fold_records_at(const Tensor& opts, const Tensor& records, const c10::optional<Tensor>& ys, const c10::optional<Tensor>& xs,
                                    int64_t hp, int64_t wp, int64_t H, int64_t W, int64_t stride, int64_t scale, int64_t top, int64_t left,
                                    int64_t h, int64_t w, bool densify_w, int64_t want) {
    const char* who = "fold_records_at";
    check_grid_records(who, ys, xs, records, hp, wp);
    check_lattice(who, scale, h, w, H, W);
    const OriginTables g = optional_tables(who, ys, xs, hp, wp);
    fp(records, "records");
    const FoldMaps m(want, records, {}, {(h - 1) * scale + 1, (w - 1) * scale + 1});
    check(be_fold_records_at_f32(fold_opts(who, opts), records.data_ptr<float>(), (int)hp, (int)wp, (int)H, (int)W, (int)stride, g.ys, g.xs,
                                 (int)scale, (int)top, (int)left, (int)h, (int)w, densify_w ? 1 : 0, m[0], m[1], m[2], m[3], m[4], m[5],
                                 stream_of(records)), "be_fold_records_at_f32");
    return m.list();
}

Tensor fold_refocus_stack_at(const Tensor& opts, const Tensor& consts, const Tensor& records, const Tensor& rho_primes,
                             const c10::optional<Tensor>& ys, const c10::optional<Tensor>& xs, int64_t hp, int64_t wp, int64_t H, int64_t W,
                             int64_t stride, int64_t scale, int64_t top, int64_t left, int64_t h, int64_t w) {
    const char* who = "fold_refocus_stack_at";
    check_grid_records(who, ys, xs, records, hp, wp);
    check_rho_primes(who, rho_primes, records);
    check_lattice(who, scale, h, w, H, W);
    const OriginTables g = optional_tables(who, ys, xs, hp, wp);
    const int64_t K = rho_primes.numel();
    fp(records, "records");
    Tensor out = at::empty({K, 3, (h - 1) * scale + 1, (w - 1) * scale + 1}, records.options());
    check(be_fold_refocus_stack_at_f32(fold_opts(who, opts), fold_consts(who, consts), records.data_ptr<float>(), (int)hp, (int)wp, (int)H, (int)W,
                                       (int)stride, g.ys, g.xs, (int)scale, (int)top, (int)left, (int)h, (int)w, fp(rho_primes, "rho_primes"),
                                       (int)K, out.data_ptr<float>(), stream_of(records)), "be_fold_refocus_stack_at_f32");
    return out;
}

// the folds at arbitrary positions: points [N,2] (y, x) float32 on the records' device; maps channel-major over the points
// ([6,N], [3,N], [N])
std::vector<Tensor> fold_records_points(const Tensor& opts, const Tensor& records, const c10::optional<Tensor>& ys, const c10::optional<Tensor>& xs,
                                        int64_t hp, int64_t wp, int64_t H, int64_t W, int64_t stride, const Tensor& points, bool densify_w,
                                        int64_t want) {
    const char* who = "fold_records_points";
    check_grid_records(who, ys, xs, records, hp, wp);
    check_points(who, points, records);
    const OriginTables g = optional_tables(who, ys, xs, hp, wp);
    fp(records, "records");
    const int64_t N = points.size(0);
    const FoldMaps m(want, records, {}, {N}, true);
    check(be_fold_records_points_f32(fold_opts(who, opts), records.data_ptr<float>(), (int)hp, (int)wp, (int)H, (int)W, (int)stride, g.ys, g.xs,
                                     fp(points, "points"), N, densify_w ? 1 : 0, m[0], m[1], m[2], m[3], m[4], m[5], stream_of(records)),
          "be_fold_records_points_f32");
    return m.list();
}

Tensor fold_refocus_stack_points(const Tensor& opts, const Tensor& consts, const Tensor& records, const Tensor& rho_primes,
                                 const c10::optional<Tensor>& ys, const c10::optional<Tensor>& xs, int64_t hp, int64_t wp, int64_t H, int64_t W,
                                 int64_t stride, const Tensor& points) {
    const char* who = "fold_refocus_stack_points";
    check_grid_records(who, ys, xs, records, hp, wp);
    check_rho_primes(who, rho_primes, records);
    check_points(who, points, records);
    const OriginTables g = optional_tables(who, ys, xs, hp, wp);
    const int64_t K = rho_primes.numel(), N = points.size(0);
    fp(records, "records");
    Tensor out = at::empty({K, 3, N}, records.options());
    check(be_fold_refocus_stack_points_f32(fold_opts(who, opts), fold_consts(who, consts), records.data_ptr<float>(), (int)hp, (int)wp, (int)H,
                                           (int)W, (int)stride, g.ys, g.xs, fp(points, "points"), N, fp(rho_primes, "rho_primes"), (int)K,
                                           out.data_ptr<float>(), stream_of(records)), "be_fold_refocus_stack_points_f32");
    return out;
}

// forward reprojection: depth [Hs,Ws] on the GPU; cam_src / cam_dst [4] (fy, fx, cy, cx) and pose [12] (R row-major, t) are CPU
// float32 tensors, read on the host as the C entries read them
static const float* host_floats(const Tensor& t, int64_t n, const char* what) {
    TORCH_CHECK(!t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n, what, ": expected a CPU float32 tensor of ",
                n, " numbers");
    return t.data_ptr<float>();
}

// The three argument checks the geometry operators share (be_hip/native.py states the same three for the ctypes binding).
// A depth map: float32 [H,W] on the GPU, contiguous, 1 .. 2^31 - 1 samples (the index maps are int32) -> its data.
static const float* depth_map(const char* who, const Tensor& depth, const char* name = "depth", const char* dims = "[Hs,Ws]") {
    TORCH_CHECK(depth.dim() == 2 && depth.numel() > 0 && depth.numel() <= 0x7fffffff, who, ": ", name, " ", dims, ", 1 .. 2^31 - 1 samples");
    return fp(depth, name);
}

// A target image of Ho x Wo pixels: sides in 1 .. 2^24, pixel indices int32.
static void target_size(const char* who, int64_t Ho, int64_t Wo) {
    TORCH_CHECK(Ho >= 1 && Wo >= 1 && Ho <= (1 << 24) && Wo <= (1 << 24) && Ho * Wo <= 0x7fffffff, who, ": bad target size");
}

static bool given(const optional<Tensor>& t) { return t.has_value() && t->defined(); }

// An optional map that rides on a depth map (weight, edge): depth's sizes, on depth's device -> its data, nullptr when absent.
static const float* map_like(const char* who, const optional<Tensor>& t, const Tensor& depth, const char* name, const char* dims = "[Hs,Ws]",
                             const char* of = "depth") {
    if (!given(t)) return nullptr;
    TORCH_CHECK(t->sizes() == depth.sizes() && t->device() == depth.device(), who, ": ", name, " ", dims, " on ", of, "'s device");
    return fp(*t, name);
}

Tensor unproject(const Tensor& depth, const Tensor& cam_src, const Tensor& pose, int64_t scale, int64_t top, int64_t left) {
    depth_map("unproject", depth);
    Tensor xyz = at::empty({3, depth.size(0), depth.size(1)}, depth.options());
    check(be_unproject_f32(depth.data_ptr<float>(), (int)depth.size(0), (int)depth.size(1), (int)scale, (int)top, (int)left,
                           host_floats(cam_src, 4, "unproject(cam_src)"), host_floats(pose, 12, "unproject(pose)"), xyz.data_ptr<float>(),
                           stream_of(depth)), "be_unproject_f32");
    return xyz;
}

// -> (depth [Ho,Wo], index [Ho,Wo] int32, feat_out [C,Ho,Wo] or an empty tensor when feat is None)
std::tuple<Tensor, Tensor, Tensor> reproject(const Tensor& depth, const Tensor& cam_src, const Tensor& cam_dst, const Tensor& pose, double near,
                                             int64_t Ho, int64_t Wo, const c10::optional<Tensor>& feat, int64_t scale, int64_t top,
                                             int64_t left) {
    depth_map("reproject", depth);
    target_size("reproject", Ho, Wo);
    const int64_t Ns = depth.numel();
    int64_t C = 0;
    const float* pf = nullptr;
    if (given(feat)) {
        TORCH_CHECK(feat->dim() == 2 && feat->size(1) == Ns, "reproject: feat [C,Hs*Ws]");
        TORCH_CHECK(feat->device() == depth.device(), "reproject: feat and depth on one device");
        C = feat->size(0);
        if (C > 0) pf = fp(*feat, "feat");
    }
    auto o = depth.options();
    Tensor zbuf = at::empty({Ho * Wo}, o.dtype(at::kLong));
    Tensor dout = at::empty({Ho, Wo}, o), index = at::empty({Ho, Wo}, o.dtype(at::kInt));
    Tensor fout = given(feat) ? at::empty({C, Ho, Wo}, o) : at::empty({0}, o);
    check(be_reproject_f32(depth.data_ptr<float>(), (int)depth.size(0), (int)depth.size(1), (int)scale, (int)top, (int)left,
                           host_floats(cam_src, 4, "reproject(cam_src)"), host_floats(cam_dst, 4, "reproject(cam_dst)"),
                           host_floats(pose, 12, "reproject(pose)"), (float)near, (int)Ho, (int)Wo, pf, (int)C,
                           reinterpret_cast<uint64_t*>(zbuf.data_ptr<int64_t>()), dout.data_ptr<float>(), index.data_ptr<int32_t>(),
                           C > 0 ? fout.data_ptr<float>() : nullptr, stream_of(depth)), "be_reproject_f32");
    return {dout, index, fout};
}

// multi-view depth fusion: depth[v] [Hs,Ws] on the GPU, weight[v] of the same shape or an empty tensor (1 everywhere), feat[v] [C,Hs*Ws]
// (an empty list when C == 0); cam_src [V,4], pose [V,12], cam_dst [4] CPU float32; scale / top / left one int per view
// -> (depth, weight [Ho,Wo], views, count, layer [Ho,Wo] int32, feat [C,Ho,Wo]); the per-pixel state is scratch allocated here
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> fuse_views(at::TensorList depth, at::TensorList weight, at::TensorList feat,
                                                                      const Tensor& cam_src, const Tensor& pose, const Tensor& cam_dst,
                                                                      double near, int64_t Ho, int64_t Wo, at::IntArrayRef scale,
                                                                      at::IntArrayRef top, at::IntArrayRef left, double tau, int64_t min_views,
                                                                      bool recentre, int64_t peel) {
    const int64_t V = (int64_t)depth.size();
    TORCH_CHECK(V >= 1 && V <= BE_FUSE_MAX_VIEWS, "fuse_views: 1 .. ", BE_FUSE_MAX_VIEWS, " views");
    TORCH_CHECK((int64_t)weight.size() == V && (feat.size() == 0 || (int64_t)feat.size() == V), "fuse_views: weight and feat hold one entry per view");
    TORCH_CHECK((int64_t)scale.size() == V && (int64_t)top.size() == V && (int64_t)left.size() == V, "fuse_views: scale, top, left hold one entry per view");
    target_size("fuse_views", Ho, Wo);
    const int64_t C = feat.size() == 0 ? 0 : feat[0].size(0);
    std::vector<const float*> pd(V), pw(V), pf(V);
    std::vector<int> hs(V), ws(V), sc(V), tp(V), lf(V);
    for (int64_t v = 0; v < V; ++v) {
        const Tensor& d = depth[v];
        pd[v] = depth_map("fuse_views", d);
        TORCH_CHECK(d.device() == depth[0].device(), "fuse_views: every view on one device");
        pw[v] = weight[v].numel() > 0 ? map_like("fuse_views", weight[v], d, "weight") : nullptr;     // an empty tensor: 1 everywhere
        pf[v] = nullptr;
        if (C > 0) {
            TORCH_CHECK(feat[v].dim() == 2 && feat[v].size(0) == C && feat[v].size(1) == d.numel() && feat[v].device() == d.device(),
                        "fuse_views: feat [C,Hs*Ws] on depth's device, the same C in every view");
            pf[v] = fp(feat[v], "feat");
        }
        hs[v] = (int)d.size(0); ws[v] = (int)d.size(1); sc[v] = (int)scale[v]; tp[v] = (int)top[v]; lf[v] = (int)left[v];
    }
    const int64_t bytes = be_fuse_scratch_bytes((int)Ho, (int)Wo, (int)C);
    TORCH_CHECK(bytes > 0, "fuse_views: no scratch size for ", Ho, " x ", Wo, " with ", C, " channels");
    auto o = depth[0].options();
    Tensor scratch = at::empty({bytes / 8 + 1}, o.dtype(at::kLong));
    Tensor dout = at::empty({Ho, Wo}, o), wout = at::empty({Ho, Wo}, o), fout = at::empty({C, Ho, Wo}, o);
    Tensor views = at::empty({Ho, Wo}, o.dtype(at::kInt)), count = at::empty({Ho, Wo}, o.dtype(at::kInt)), layer = at::empty({Ho, Wo}, o.dtype(at::kInt));
    check(be_fuse_views_f32((int)V, pd.data(), pw.data(), C > 0 ? pf.data() : nullptr, (int)C, hs.data(), ws.data(), sc.data(), tp.data(), lf.data(),
                            host_floats(cam_src, 4 * V, "fuse_views(cam_src)"), host_floats(pose, 12 * V, "fuse_views(pose)"),
                            host_floats(cam_dst, 4, "fuse_views(cam_dst)"), (float)near, (int)Ho, (int)Wo, (float)tau, (int)min_views,
                            recentre ? 1 : 0, (int)peel, scratch.data_ptr<int64_t>(), dout.data_ptr<float>(), wout.data_ptr<float>(),
                            views.data_ptr<int32_t>(), count.data_ptr<int32_t>(), layer.data_ptr<int32_t>(),
                            C > 0 ? fout.data_ptr<float>() : nullptr, stream_of(depth[0])), "be_fuse_views_f32");
    return {dout, wout, views, count, layer, fout};
}

// TSDF volumes: the sums sw int32 [Nz,Ny,Nx], swd int64 [Nz,Ny,Nx], swf int64 [C,Nz,Ny,Nx] on the GPU; origin, voxel [3], cam [4]
// and pose [12] CPU float32 tensors.  tsdf_integrate adds one view to the sums in place.
static void tsdf_dims(const Tensor& a, const char* what, int dims[3]) {
    TORCH_CHECK(a.dim() == 3 && a.is_cuda() && a.is_contiguous(), what, ": expected a contiguous tensor [Nz,Ny,Nx] on the GPU");
    for (int i = 0; i < 3; ++i) {
        TORCH_CHECK(a.size(i) >= 1 && a.size(i) <= BE_TSDF_MAX_DIM, what, ": each of (Nz, Ny, Nx) must be in [1, ", BE_TSDF_MAX_DIM, "]");
        dims[i] = (int)a.size(i);
    }
}

static int64_t tsdf_sums(const Tensor& sw, const Tensor& swd, const Tensor& swf, const char* what, int dims[3]) {
    tsdf_dims(sw, what, dims);
    TORCH_CHECK(sw.scalar_type() == at::kInt && swd.scalar_type() == at::kLong && swf.scalar_type() == at::kLong, what,
                ": sw must be int32, swd and swf int64");
    TORCH_CHECK(swd.sizes() == sw.sizes() && swd.device() == sw.device() && swd.is_contiguous(), what, ": swd [Nz,Ny,Nx] on sw's device");
    TORCH_CHECK(swf.dim() == 4 && swf.sizes().slice(1) == sw.sizes() && swf.device() == sw.device() && swf.is_contiguous(), what,
                ": swf [C,Nz,Ny,Nx] on sw's device");
    return swf.size(0);
}

void tsdf_integrate(const Tensor& depth, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& feat, const Tensor& cam_src,
                    const Tensor& pose, double near, int64_t scale, int64_t top, int64_t left, const Tensor& origin, const Tensor& voxel,
                    double trunc, Tensor& sw, Tensor& swd, Tensor& swf) {
    depth_map("tsdf_integrate", depth);
    int dims[3];
    const int64_t C = tsdf_sums(sw, swd, swf, "tsdf_integrate", dims);
    TORCH_CHECK(sw.device() == depth.device(), "tsdf_integrate: the volume and depth on one device");
    const float* pw = map_like("tsdf_integrate", weight, depth, "weight");
    const bool has_feat = given(feat);
    TORCH_CHECK((has_feat ? feat->size(0) : 0) == C, "tsdf_integrate: feat must hold the volume's ", C, " channels");
    if (has_feat)
        TORCH_CHECK(feat->dim() == 2 && feat->size(1) == depth.numel() && feat->device() == depth.device(), "tsdf_integrate: feat [C,Hs*Ws] on depth's device");
    check(be_tsdf_integrate_f32(depth.data_ptr<float>(), pw, C > 0 ? fp(*feat, "feat") : nullptr, (int)C, (int)depth.size(0),
                                (int)depth.size(1), (int)scale, (int)top, (int)left, host_floats(cam_src, 4, "tsdf_integrate(cam_src)"),
                                host_floats(pose, 12, "tsdf_integrate(pose)"), (float)near, dims, host_floats(origin, 3, "tsdf_integrate(origin)"),
                                host_floats(voxel, 3, "tsdf_integrate(voxel)"), (float)trunc, sw.data_ptr<int32_t>(), swd.data_ptr<int64_t>(),
                                C > 0 ? swf.data_ptr<int64_t>() : nullptr, stream_of(depth)), "be_tsdf_integrate_f32");
}

// -> (D, W [Nz,Ny,Nx], Fm [C,Nz,Ny,Nx]) float32
std::tuple<Tensor, Tensor, Tensor> tsdf_mean(const Tensor& sw, const Tensor& swd, const Tensor& swf) {
    int dims[3];
    const int64_t C = tsdf_sums(sw, swd, swf, "tsdf_mean", dims);
    auto o = sw.options().dtype(at::kFloat);
    Tensor D = at::empty(sw.sizes(), o), W = at::empty(sw.sizes(), o), Fm = at::empty(swf.sizes(), o);
    check(be_tsdf_mean_f32(dims, (int)C, sw.data_ptr<int32_t>(), swd.data_ptr<int64_t>(), C > 0 ? swf.data_ptr<int64_t>() : nullptr,
                           D.data_ptr<float>(), W.data_ptr<float>(), C > 0 ? Fm.data_ptr<float>() : nullptr, stream_of(sw)), "be_tsdf_mean_f32");
    return {D, W, Fm};
}

// D, W [Nz,Ny,Nx], Fm [C,Nz,Ny,Nx] as tsdf_mean returns them -> (depth, weight [Ho,Wo], feat [C,Ho,Wo])
std::tuple<Tensor, Tensor, Tensor> tsdf_raycast(const Tensor& D, const Tensor& W, const Tensor& Fm, const Tensor& origin, const Tensor& voxel,
                                                const Tensor& cam_dst, const Tensor& pose, int64_t Ho, int64_t Wo, double z_near, double step,
                                                int64_t n) {
    int dims[3];
    tsdf_dims(D, "tsdf_raycast", dims);
    fp(D, "D");
    fp(W, "W");
    TORCH_CHECK(W.sizes() == D.sizes() && W.device() == D.device(), "tsdf_raycast: W [Nz,Ny,Nx] on D's device");
    TORCH_CHECK(Fm.dim() == 4 && Fm.sizes().slice(1) == D.sizes() && Fm.device() == D.device(), "tsdf_raycast: Fm [C,Nz,Ny,Nx] on D's device");
    target_size("tsdf_raycast", Ho, Wo);
    TORCH_CHECK(n >= 1 && n <= BE_TSDF_MAX_STEPS, "tsdf_raycast: n must be in [1, ", BE_TSDF_MAX_STEPS, "]");
    const int64_t C = Fm.size(0);
    Tensor dout = at::empty({Ho, Wo}, D.options()), wout = at::empty({Ho, Wo}, D.options()), fout = at::empty({C, Ho, Wo}, D.options());
    check(be_tsdf_raycast_f32(D.data_ptr<float>(), W.data_ptr<float>(), C > 0 ? fp(Fm, "Fm") : nullptr, (int)C, dims,
                              host_floats(origin, 3, "tsdf_raycast(origin)"), host_floats(voxel, 3, "tsdf_raycast(voxel)"),
                              host_floats(cam_dst, 4, "tsdf_raycast(cam_dst)"), host_floats(pose, 12, "tsdf_raycast(pose)"), (int)Ho, (int)Wo,
                              (float)z_near, (float)step, (int)n, dout.data_ptr<float>(), wout.data_ptr<float>(),
                              C > 0 ? fout.data_ptr<float>() : nullptr, stream_of(D)), "be_tsdf_raycast_f32");
    return {dout, wout, fout};
}

// counts [n] uint8 on the GPU -> (offsets [n] int32 = the exclusive prefix sums, total [1] int64 on the device)
std::tuple<Tensor, Tensor> exclusive_scan(const Tensor& counts) {
    TORCH_CHECK(counts.is_cuda() && counts.dim() == 1 && counts.scalar_type() == at::kByte && counts.is_contiguous(),
                "exclusive_scan: counts must be a contiguous uint8 tensor [n] on the GPU");
    const int64_t n = counts.numel();
    TORCH_CHECK(n <= 0x7fffffff, "exclusive_scan: at most 2^31 - 1 counts");
    Tensor offsets = at::empty({n}, counts.options().dtype(at::kInt)), total = at::empty({1}, counts.options().dtype(at::kLong));
    const size_t bytes = be_exclusive_scan_workspace_bytes(n);
    Tensor ws = at::empty({(int64_t)(bytes / 8)}, counts.options().dtype(at::kLong));
    check(be_exclusive_scan_u8_i32(counts.data_ptr<uint8_t>(), n, offsets.data_ptr<int32_t>(), total.data_ptr<int64_t>(), ws.data_ptr<int64_t>(),
                                   bytes, stream_of(counts)), "be_exclusive_scan_u8_i32");
    return {offsets, total};
}

// D, W [Nz,Ny,Nx], Fm [C,Nz,Ny,Nx] as tsdf_mean returns them -> [vertices [V,3], faces [T,3] int32, weight [V], feat [C,V],
// normal [V,3], normal_valid [V] bool (both empty without normals), edge [V] int64, totals [2] int64 on the CPU = (V, T)].  Count,
// one read-back of the totals (the synchronisation a result of variable length costs), allocation, emit.  A total >= 2^31 emits
// nothing: every output is empty beside totals, which the caller refuses (mesh.check_totals).
std::vector<Tensor> tsdf_mesh(const Tensor& D, const Tensor& W, const Tensor& Fm, const Tensor& origin, const Tensor& voxel, double min_weight,
                              bool normals) {
    int dims[3];
    tsdf_dims(D, "tsdf_mesh", dims);
    fp(D, "D");
    fp(W, "W");
    TORCH_CHECK(W.sizes() == D.sizes() && W.device() == D.device(), "tsdf_mesh: W [Nz,Ny,Nx] on D's device");
    TORCH_CHECK(Fm.dim() == 4 && Fm.sizes().slice(1) == D.sizes() && Fm.device() == D.device(), "tsdf_mesh: Fm [C,Nz,Ny,Nx] on D's device");
    const int64_t C = Fm.size(0), n = D.numel();
    const float* fm = C > 0 ? fp(Fm, "Fm") : nullptr;
    const float* org = host_floats(origin, 3, "tsdf_mesh(origin)");
    const float* vox = host_floats(voxel, 3, "tsdf_mesh(voxel)");
    auto ob = D.options().dtype(at::kByte), oi = D.options().dtype(at::kInt), ol = D.options().dtype(at::kLong);
    Tensor nt = at::empty({n}, ob), mask = at::empty({n}, ob), voff = at::empty({n}, oi), toff = at::empty({n}, oi), totals = at::empty({2}, ol);
    const size_t bytes = be_tsdf_mesh_workspace_bytes(n);
    Tensor ws = at::empty({(int64_t)(bytes / 8)}, ol);
    void* stream = stream_of(D);
    check(be_tsdf_mesh_count_f32(D.data_ptr<float>(), W.data_ptr<float>(), dims, (float)min_weight, nt.data_ptr<uint8_t>(), mask.data_ptr<uint8_t>(),
                                 voff.data_ptr<int32_t>(), toff.data_ptr<int32_t>(), totals.data_ptr<int64_t>(), ws.data_ptr<int64_t>(), bytes,
                                 stream), "be_tsdf_mesh_count_f32");
    Tensor host = totals.cpu();                                         // synchronises with the current stream
    int64_t V = host.data_ptr<int64_t>()[0], T = host.data_ptr<int64_t>()[1];
    const bool fits = V >= 0 && T >= 0 && V <= 0x7fffffff && T <= 0x7fffffff;
    if (!fits) V = T = 0;
    Tensor vertices = at::empty({V, 3}, D.options()), faces = at::empty({T, 3}, oi), weight = at::empty({V}, D.options());
    Tensor feat = at::empty({C, V}, D.options()), edge = at::empty({V}, ol);
    Tensor normal = at::empty({normals ? V : 0, 3}, D.options()), normal_valid = at::empty({normals ? V : 0}, D.options().dtype(at::kBool));
    if (fits && (V > 0 || T > 0))
        check(be_tsdf_mesh_emit_f32(D.data_ptr<float>(), W.data_ptr<float>(), fm, (int)C, dims, org, vox, (float)min_weight, nt.data_ptr<uint8_t>(),
                                    mask.data_ptr<uint8_t>(), voff.data_ptr<int32_t>(), toff.data_ptr<int32_t>(), V, T, vertices.data_ptr<float>(),
                                    faces.data_ptr<int32_t>(), weight.data_ptr<float>(), C > 0 ? feat.data_ptr<float>() : nullptr,
                                    normals ? normal.data_ptr<float>() : nullptr,
                                    normals ? reinterpret_cast<uint8_t*>(normal_valid.data_ptr<bool>()) : nullptr, edge.data_ptr<int64_t>(), stream),
              "be_tsdf_mesh_emit_f32");
    return {vertices, faces, weight, feat, normal, normal_valid, edge, host};
}

// vertices [V,3], faces [T,3] int32 and the optional per-vertex maps weight [V], feat [C,V], normal [V,3], normal_valid [V] bool on
// the GPU; cam_dst [4] and pose [12] (mesh frame -> camera frame) CPU float32 tensors -> [depth [Ho,Wo], face [Ho,Wo] int32,
// weight [Ho,Wo], feat [C,Ho,Wo], normal [3,Ho,Wo], normal_valid [Ho,Wo] bool, bary [3,Ho,Wo]]; an output whose input is absent
// (bary: want_bary false) is an empty tensor.  Nothing synchronises with the host.
std::vector<Tensor> mesh_raster(const Tensor& vertices, const Tensor& faces, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& feat,
                                const c10::optional<Tensor>& normal, const c10::optional<Tensor>& normal_valid, const Tensor& cam_dst,
                                const Tensor& pose, double near, int64_t cull, int64_t Ho, int64_t Wo, bool want_bary) {
    fp(vertices, "mesh_raster(vertices)");
    TORCH_CHECK(vertices.dim() == 2 && vertices.size(1) == 3, "mesh_raster: vertices [V,3]");
    TORCH_CHECK(faces.is_cuda() && faces.dim() == 2 && faces.size(1) == 3 && faces.scalar_type() == at::kInt && faces.is_contiguous() &&
                faces.device() == vertices.device(), "mesh_raster: faces must be a contiguous int32 tensor [T,3] on vertices' device");
    TORCH_CHECK(Ho >= 1 && Wo >= 1 && Ho <= BE_RASTER_MAX_SIZE && Wo <= BE_RASTER_MAX_SIZE, "mesh_raster: size must be in [1, ", BE_RASTER_MAX_SIZE, "]");
    const int64_t V = vertices.size(0), T = faces.size(0);
    const bool has_w = given(weight), has_f = given(feat), has_n = given(normal), has_nv = given(normal_valid);
    if (has_w) TORCH_CHECK(weight->dim() == 1 && weight->size(0) == V && weight->device() == vertices.device(), "mesh_raster: weight [V] on vertices' device");
    if (has_f) TORCH_CHECK(feat->dim() == 2 && feat->size(1) == V && feat->device() == vertices.device(), "mesh_raster: feat [C,V] on vertices' device");
    if (has_n) TORCH_CHECK(normal->dim() == 2 && normal->size(0) == V && normal->size(1) == 3 && normal->device() == vertices.device(),
                           "mesh_raster: normal [V,3] on vertices' device");
    TORCH_CHECK(!has_nv || has_n, "mesh_raster: normal_valid needs normal");
    if (has_nv) TORCH_CHECK(normal_valid->is_cuda() && normal_valid->dim() == 1 && normal_valid->size(0) == V && normal_valid->scalar_type() == at::kBool &&
                            normal_valid->is_contiguous() && normal_valid->device() == vertices.device(),
                            "mesh_raster: normal_valid must be a contiguous bool tensor [V] on vertices' device");
    const int64_t C = has_f ? feat->size(0) : 0;
    auto of = vertices.options();
    Tensor depth = at::empty({Ho, Wo}, of), face = at::empty({Ho, Wo}, of.dtype(at::kInt));
    Tensor wout = at::empty({has_w ? Ho : 0, has_w ? Wo : 0}, of), fout = at::empty({C, has_f ? Ho : 0, has_f ? Wo : 0}, of);
    Tensor nout = at::empty({has_n ? 3 : 0, has_n ? Ho : 0, has_n ? Wo : 0}, of);
    Tensor nvout = at::empty({has_n ? Ho : 0, has_n ? Wo : 0}, of.dtype(at::kBool));
    Tensor bary = at::empty({want_bary ? 3 : 0, want_bary ? Ho : 0, want_bary ? Wo : 0}, of);
    const size_t bytes = be_mesh_raster_workspace_bytes(V, (int)Ho, (int)Wo);
    TORCH_CHECK(bytes > 0, "mesh_raster: at most 2^31 - 1 vertices");
    Tensor ws = at::empty({(int64_t)((bytes + 15) / 16), 2}, of.dtype(at::kLong));
    check(be_mesh_raster_f32(vertices.data_ptr<float>(), V, faces.data_ptr<int32_t>(), T, has_w ? fp(*weight, "mesh_raster(weight)") : nullptr,
                             has_f && C > 0 ? fp(*feat, "mesh_raster(feat)") : nullptr, (int)C, has_n ? fp(*normal, "mesh_raster(normal)") : nullptr,
                             has_nv ? reinterpret_cast<const uint8_t*>(normal_valid->data_ptr<bool>()) : nullptr,
                             host_floats(cam_dst, 4, "mesh_raster(cam_dst)"), host_floats(pose, 12, "mesh_raster(pose)"), (float)near, (int)cull,
                             (int)Ho, (int)Wo, depth.data_ptr<float>(), face.data_ptr<int32_t>(), has_w ? wout.data_ptr<float>() : nullptr,
                             has_f && C > 0 ? fout.data_ptr<float>() : nullptr, has_n ? nout.data_ptr<float>() : nullptr,
                             has_n ? reinterpret_cast<uint8_t*>(nvout.data_ptr<bool>()) : nullptr, want_bary ? bary.data_ptr<float>() : nullptr,
                             ws.data_ptr<int64_t>(), bytes, stream_of(vertices)), "be_mesh_raster_f32");
    return {depth, face, wout, fout, nout, nvout, bary};
}

// ---- mesh cleaning: the five steps of be_mesh_components_* / be_mesh_select_*, none of which synchronises with the host; the
// read-backs between them are native.py's, the same for both bindings
static void mesh_faces(const char* who, const Tensor& faces, int64_t V) {
    TORCH_CHECK(faces.is_cuda() && faces.dim() == 2 && faces.size(1) == 3 && faces.scalar_type() == at::kInt && faces.is_contiguous(), who,
                ": faces must be a contiguous int32 tensor [T,3] on the GPU");
    TORCH_CHECK(V >= 0 && V <= 0x7fffffff && faces.size(0) <= 0x7fffffff, who, ": at most 2^31 - 1 vertices and triangles");
}

template <typename T>
static T* on_device(const char* who, const char* name, const Tensor& t, at::ScalarType dtype, const Tensor& like, int64_t numel = -1) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == dtype && t.is_contiguous() && t.device() == like.device() && (numel < 0 || t.numel() == numel), who,
                ": ", name, " must be a contiguous ", c10::toString(dtype), " tensor", numel < 0 ? "" : " of the mesh's size", " on the mesh's device");
    return reinterpret_cast<T*>(t.data_ptr());
}

// faces [T,3] int32 over V vertices -> [label [V], component [V], face_component [T] int32, total [1] int64 on the device = K]
std::vector<Tensor> mesh_components(const Tensor& faces, int64_t V) {
    mesh_faces("mesh_components", faces, V);
    const int64_t T = faces.size(0);
    auto oi = faces.options();
    Tensor label = at::empty({V}, oi), component = at::empty({V}, oi), face_component = at::empty({T}, oi), total = at::empty({1}, oi.dtype(at::kLong));
    const size_t bytes = be_mesh_components_workspace_bytes(V);
    Tensor ws = at::empty({(int64_t)((bytes + 7) / 8)}, oi.dtype(at::kLong));
    check(be_mesh_components_i32(faces.data_ptr<int32_t>(), V, T, label.data_ptr<int32_t>(), component.data_ptr<int32_t>(),
                                 face_component.data_ptr<int32_t>(), total.data_ptr<int64_t>(), ws.data_ptr<int64_t>(), bytes, stream_of(faces)),
          "be_mesh_components_i32");
    return {label, component, face_component, total};
}

// -> [triangles [Kcap] int32, vertices [Kcap] int32, area_q [Kcap] int64]
std::vector<Tensor> mesh_components_stats(const Tensor& vertices, const Tensor& faces, const Tensor& component, int64_t Kcap) {
    fp(vertices, "mesh_components_stats(vertices)");
    TORCH_CHECK(vertices.dim() == 2 && vertices.size(1) == 3, "mesh_components_stats: vertices [V,3]");
    const int64_t V = vertices.size(0), T = faces.size(0);
    mesh_faces("mesh_components_stats", faces, V);
    const int32_t* comp = on_device<int32_t>("mesh_components_stats", "component", component, at::kInt, vertices, V);
    TORCH_CHECK(faces.device() == vertices.device() && Kcap >= 0 && Kcap <= V, "mesh_components_stats: faces on vertices' device, Kcap in [0, V]");
    auto oi = faces.options();
    Tensor triangles = at::empty({Kcap}, oi), nvertices = at::empty({Kcap}, oi), area_q = at::empty({Kcap}, oi.dtype(at::kLong));
    check(be_mesh_components_stats(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, comp, Kcap, triangles.data_ptr<int32_t>(),
                                   nvertices.data_ptr<int32_t>(), area_q.data_ptr<int64_t>(), stream_of(vertices)), "be_mesh_components_stats");
    return {triangles, nvertices, area_q};
}

// -> [keep [Kcap] bool (0 from K on), vertex_keep [V] bool (empty without component)]
std::vector<Tensor> mesh_components_decide(const Tensor& triangles, const Tensor& area_q, const Tensor& total, int64_t min_triangles, double min_area,
                                           bool largest, const c10::optional<Tensor>& component) {
    const int64_t Kcap = triangles.numel();
    TORCH_CHECK(triangles.is_cuda() && triangles.scalar_type() == at::kInt && triangles.is_contiguous(),
                "mesh_components_decide: triangles must be a contiguous int32 tensor on the GPU");
    const int64_t* aq = on_device<int64_t>("mesh_components_decide", "area_q", area_q, at::kLong, triangles, Kcap);
    const int64_t* tot = on_device<int64_t>("mesh_components_decide", "total", total, at::kLong, triangles, 1);
    const bool has_c = given(component);
    const int64_t V = has_c ? component->numel() : 0;
    const int32_t* comp = has_c ? on_device<int32_t>("mesh_components_decide", "component", *component, at::kInt, triangles) : nullptr;
    auto ob = triangles.options().dtype(at::kBool);
    Tensor keep = at::zeros({Kcap}, ob), vertex_keep = at::empty({V}, ob);
    Tensor ws = at::empty({BE_COMPONENTS_DECIDE_WORKSPACE_BYTES / 8}, triangles.options().dtype(at::kLong));
    check(be_mesh_components_decide(triangles.data_ptr<int32_t>(), aq, tot, Kcap, min_triangles, (float)min_area, largest ? 1 : 0,
                                    reinterpret_cast<uint8_t*>(keep.data_ptr<bool>()), comp, V,
                                    has_c ? reinterpret_cast<uint8_t*>(vertex_keep.data_ptr<bool>()) : nullptr, ws.data_ptr<int64_t>(),
                                    BE_COMPONENTS_DECIDE_WORKSPACE_BYTES, stream_of(triangles)), "be_mesh_components_decide");
    return {keep, vertex_keep};
}

// faces [T,3], vertex_keep [V] bool -> [voff [V], foff [T] int32, totals [2] int64 on the device = (V', T')]
std::vector<Tensor> mesh_select_count(const Tensor& faces, const Tensor& vertex_keep) {
    const int64_t V = vertex_keep.numel(), T = faces.size(0);
    mesh_faces("mesh_select_count", faces, V);
    const uint8_t* vk = on_device<uint8_t>("mesh_select_count", "vertex_keep", vertex_keep, at::kBool, faces);
    auto oi = faces.options();
    Tensor voff = at::empty({V}, oi), foff = at::empty({T}, oi), totals = at::empty({2}, oi.dtype(at::kLong));
    const size_t bytes = be_mesh_select_workspace_bytes(V, T);
    Tensor ws = at::empty({(int64_t)((bytes + 7) / 8)}, oi.dtype(at::kLong));
    check(be_mesh_select_count(faces.data_ptr<int32_t>(), V, T, vk, voff.data_ptr<int32_t>(), foff.data_ptr<int32_t>(), totals.data_ptr<int64_t>(),
                               ws.data_ptr<int64_t>(), bytes, stream_of(faces)), "be_mesh_select_count");
    return {voff, foff, totals};
}

// the emit phase -> [vertices [V2,3], faces [T2,3], weight [V2], feat [C,V2], normal [V2,3], normal_valid [V2] bool, edge [V2] int64,
// component [V2] int32, vertex_index [V2], face_index [T2] int32]; an output whose input is absent is an empty tensor
std::vector<Tensor> mesh_select(const Tensor& vertices, const Tensor& faces, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& feat,
                                const c10::optional<Tensor>& normal, const c10::optional<Tensor>& normal_valid, const c10::optional<Tensor>& edge,
                                const c10::optional<Tensor>& component, const Tensor& vertex_keep, const Tensor& voff, const Tensor& foff, int64_t V2,
                                int64_t T2) {
    const char* who = "mesh_select";
    fp(vertices, "mesh_select(vertices)");
    TORCH_CHECK(vertices.dim() == 2 && vertices.size(1) == 3, "mesh_select: vertices [V,3]");
    const int64_t V = vertices.size(0), T = faces.size(0);
    mesh_faces(who, faces, V);
    TORCH_CHECK(V2 >= 0 && V2 <= V && T2 >= 0 && T2 <= T, "mesh_select: V2 in [0, V] and T2 in [0, T]");
    const bool has_w = given(weight), has_f = given(feat), has_n = given(normal), has_nv = given(normal_valid), has_e = given(edge), has_c = given(component);
    if (has_f) TORCH_CHECK(feat->dim() == 2 && feat->size(1) == V, "mesh_select: feat [C,V]");
    const int64_t C = has_f ? feat->size(0) : 0;
    const float* pw = has_w ? on_device<float>(who, "weight", *weight, at::kFloat, vertices, V) : nullptr;
    const float* pf = has_f && C > 0 ? on_device<float>(who, "feat", *feat, at::kFloat, vertices, C * V) : nullptr;
    const float* pn = has_n ? on_device<float>(who, "normal", *normal, at::kFloat, vertices, 3 * V) : nullptr;
    const uint8_t* pnv = has_nv ? on_device<uint8_t>(who, "normal_valid", *normal_valid, at::kBool, vertices, V) : nullptr;
    const int64_t* pe = has_e ? on_device<int64_t>(who, "edge", *edge, at::kLong, vertices, V) : nullptr;
    const int32_t* pc = has_c ? on_device<int32_t>(who, "component", *component, at::kInt, vertices, V) : nullptr;
    const uint8_t* vk = on_device<uint8_t>(who, "vertex_keep", vertex_keep, at::kBool, vertices, V);
    const int32_t* pvo = on_device<int32_t>(who, "voff", voff, at::kInt, vertices, V);
    const int32_t* pfo = on_device<int32_t>(who, "foff", foff, at::kInt, vertices, T);
    auto of = vertices.options(), oi = faces.options();
    Tensor vout = at::empty({V2, 3}, of), fout = at::empty({T2, 3}, oi), wout = at::empty({has_w ? V2 : 0}, of), ftout = at::empty({C, has_f ? V2 : 0}, of);
    Tensor nout = at::empty({has_n ? V2 : 0, 3}, of), nvout = at::empty({has_nv ? V2 : 0}, of.dtype(at::kBool));
    Tensor eout = at::empty({has_e ? V2 : 0}, of.dtype(at::kLong)), cout = at::empty({has_c ? V2 : 0}, oi);
    Tensor vindex = at::empty({V2}, oi), findex = at::empty({T2}, oi);
    check(be_mesh_select_emit(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, pw, pf, (int)C, pn, pnv, pe, pc, vk, pvo, pfo, V2, T2,
                              vout.data_ptr<float>(), fout.data_ptr<int32_t>(), has_w ? wout.data_ptr<float>() : nullptr,
                              pf ? ftout.data_ptr<float>() : nullptr, has_n ? nout.data_ptr<float>() : nullptr,
                              has_nv ? reinterpret_cast<uint8_t*>(nvout.data_ptr<bool>()) : nullptr, has_e ? eout.data_ptr<int64_t>() : nullptr,
                              has_c ? cout.data_ptr<int32_t>() : nullptr, vindex.data_ptr<int32_t>(), findex.data_ptr<int32_t>(), stream_of(vertices)),
          "be_mesh_select_emit");
    return {vout, fout, wout, ftout, nout, nvout, eout, cout, vindex, findex};
}

// ---- mesh simplification: the three steps of be_mesh_cluster_f32 / be_mesh_simplify_*, none of which synchronises with the host; the
// one read-back between count and emit is native.py's, the same for both bindings.  cell, origin: CPU float32 tensors [3].
static int64_t mesh_vertices(const char* who, const Tensor& vertices) {
    fp(vertices, who);
    TORCH_CHECK(vertices.dim() == 2 && vertices.size(1) == 3, who, ": vertices [V,3]");
    return vertices.size(0);
}

// -> [label [V], cluster [V], members [V] int32 (0 from V' on), totals [2] int64 on the device = (V', overflow)]
std::vector<Tensor> mesh_cluster(const Tensor& vertices, const c10::optional<Tensor>& weight, const Tensor& cell, const Tensor& origin) {
    const char* who = "mesh_cluster";
    const int64_t V = mesh_vertices(who, vertices);
    const float* pw = given(weight) ? on_device<float>(who, "weight", *weight, at::kFloat, vertices, V) : nullptr;
    auto oi = vertices.options().dtype(at::kInt), ol = vertices.options().dtype(at::kLong);
    Tensor label = at::empty({V}, oi), cluster = at::empty({V}, oi), members = at::empty({V}, oi), totals = at::empty({2}, ol);
    const size_t bytes = be_mesh_cluster_workspace_bytes(V);
    TORCH_CHECK(bytes > 0, "mesh_cluster: at most 2^29 vertices");
    Tensor ws = at::empty({(int64_t)((bytes + 7) / 8)}, ol);
    check(be_mesh_cluster_f32(vertices.data_ptr<float>(), pw, V, host_floats(cell, 3, "mesh_cluster(cell)"), host_floats(origin, 3, "mesh_cluster(origin)"),
                              label.data_ptr<int32_t>(), cluster.data_ptr<int32_t>(), members.data_ptr<int32_t>(), totals.data_ptr<int64_t>(),
                              ws.data_ptr<int64_t>(), bytes, stream_of(vertices)), "be_mesh_cluster_f32");
    return {label, cluster, members, totals};
}

// -> [sums [rows,V] int64, fflag [T] uint8, foff [T] int32, totals [2] int64 on the device = (T', overflow)]
std::vector<Tensor> mesh_simplify_count(const Tensor& vertices, const Tensor& faces, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& feat,
                                        const c10::optional<Tensor>& normal, const c10::optional<Tensor>& normal_valid, const Tensor& cell,
                                        const Tensor& origin, const Tensor& cluster, bool flaps) {
    const char* who = "mesh_simplify_count";
    const int64_t V = mesh_vertices(who, vertices), T = faces.size(0);
    mesh_faces(who, faces, V);
    const bool has_w = given(weight), has_f = given(feat), has_n = given(normal), has_nv = given(normal_valid);
    if (has_f) TORCH_CHECK(feat->dim() == 2 && feat->size(1) == V, "mesh_simplify_count: feat [C,V]");
    TORCH_CHECK(!has_nv || has_n, "mesh_simplify_count: normal_valid needs normal");
    const int64_t C = has_f ? feat->size(0) : 0;
    const int rows = be_mesh_simplify_sum_rows((int)C, has_n ? 1 : 0);
    TORCH_CHECK(rows > 0, "mesh_simplify_count: too many channels");
    const float* pw = has_w ? on_device<float>(who, "weight", *weight, at::kFloat, vertices, V) : nullptr;
    const float* pf = has_f && C > 0 ? on_device<float>(who, "feat", *feat, at::kFloat, vertices, C * V) : nullptr;
    const float* pn = has_n ? on_device<float>(who, "normal", *normal, at::kFloat, vertices, 3 * V) : nullptr;
    const uint8_t* pnv = has_nv ? on_device<uint8_t>(who, "normal_valid", *normal_valid, at::kBool, vertices, V) : nullptr;
    const int32_t* pc = on_device<int32_t>(who, "cluster", cluster, at::kInt, vertices, V);
    auto oi = faces.options(), ol = oi.dtype(at::kLong);
    Tensor sums = at::empty({rows, V}, ol), fflag = at::empty({T}, oi.dtype(at::kByte)), foff = at::empty({T}, oi), totals = at::empty({2}, ol);
    const size_t bytes = be_mesh_simplify_workspace_bytes(T);
    TORCH_CHECK(bytes > 0, "mesh_simplify_count: at most 2^29 triangles");
    Tensor ws = at::empty({(int64_t)((bytes + 7) / 8)}, ol);
    check(be_mesh_simplify_count(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, pw, pf, (int)C, pn, pnv,
                                 host_floats(cell, 3, "mesh_simplify_count(cell)"), host_floats(origin, 3, "mesh_simplify_count(origin)"), pc,
                                 flaps ? 1 : 0, sums.data_ptr<int64_t>(), fflag.data_ptr<uint8_t>(), foff.data_ptr<int32_t>(),
                                 totals.data_ptr<int64_t>(), ws.data_ptr<int64_t>(), bytes, stream_of(vertices)), "be_mesh_simplify_count");
    return {sums, fflag, foff, totals};
}

// the emit phase -> [vertices [V2,3], faces [T2,3] int32, weight [V2], feat [C,V2], normal [V2,3], normal_valid [V2] bool, face_index
// [T2] int32]; weight without want_weight and the normals without normal rows in sums are empty tensors
std::vector<Tensor> mesh_simplify(const Tensor& vertices, const Tensor& faces, const Tensor& cell, const Tensor& origin, const Tensor& label,
                                  const Tensor& cluster, const Tensor& members, const Tensor& sums, int64_t C, bool normals, bool want_weight,
                                  const Tensor& fflag, const Tensor& foff, int64_t V2, int64_t T2) {
    const char* who = "mesh_simplify";
    const int64_t V = mesh_vertices(who, vertices), T = faces.size(0);
    mesh_faces(who, faces, V);
    TORCH_CHECK(V2 >= 0 && V2 <= V && T2 >= 0 && T2 <= T, "mesh_simplify: V2 in [0, V] and T2 in [0, T]");
    const int rows = be_mesh_simplify_sum_rows((int)C, normals ? 1 : 0);
    TORCH_CHECK(C >= 0 && rows > 0, "mesh_simplify: too many channels");
    const int32_t* pl = on_device<int32_t>(who, "label", label, at::kInt, vertices, V);
    const int32_t* pc = on_device<int32_t>(who, "cluster", cluster, at::kInt, vertices, V);
    const int32_t* pm = on_device<int32_t>(who, "members", members, at::kInt, vertices, V);
    const int64_t* ps = on_device<int64_t>(who, "sums", sums, at::kLong, vertices, rows * V);
    const uint8_t* pff = on_device<uint8_t>(who, "fflag", fflag, at::kByte, vertices, T);
    const int32_t* pfo = on_device<int32_t>(who, "foff", foff, at::kInt, vertices, T);
    auto of = vertices.options(), oi = faces.options();
    Tensor vout = at::empty({V2, 3}, of), fout = at::empty({T2, 3}, oi), wout = at::empty({want_weight ? V2 : 0}, of), ftout = at::empty({C, V2}, of);
    Tensor nout = at::empty({normals ? V2 : 0, 3}, of), nvout = at::empty({normals ? V2 : 0}, of.dtype(at::kBool)), findex = at::empty({T2}, oi);
    check(be_mesh_simplify_emit(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, host_floats(cell, 3, "mesh_simplify(cell)"),
                                host_floats(origin, 3, "mesh_simplify(origin)"), pl, pc, pm, ps, (int)C, normals ? 1 : 0, pff, pfo, V2, T2,
                                vout.data_ptr<float>(), fout.data_ptr<int32_t>(), want_weight ? wout.data_ptr<float>() : nullptr,
                                C > 0 ? ftout.data_ptr<float>() : nullptr, normals ? nout.data_ptr<float>() : nullptr,
                                normals ? reinterpret_cast<uint8_t*>(nvout.data_ptr<bool>()) : nullptr, findex.data_ptr<int32_t>(),
                                stream_of(vertices)), "be_mesh_simplify_emit");
    return {vout, fout, wout, ftout, nout, nvout, findex};
}

// ---- mesh smoothing: be_mesh_adjacency_f32 / be_mesh_smooth_f32 / be_mesh_normals_f32; nothing synchronises with the host
static Tensor smooth_workspace(const char* who, const Tensor& vertices, int64_t V, int64_t T, size_t* bytes) {
    *bytes = be_mesh_smooth_workspace_bytes(V, T);
    TORCH_CHECK(*bytes > 0 || (V == 0 && T == 0), who, ": at most 2^29 vertices and triangles");
    return at::empty({(int64_t)((*bytes + 7) / 8)}, vertices.options().dtype(at::kLong));
}

// -> [valence [V] int32, boundary [V] bool]
std::vector<Tensor> mesh_adjacency(const Tensor& vertices, const Tensor& faces) {
    const char* who = "mesh_adjacency";
    const int64_t V = mesh_vertices(who, vertices), T = faces.size(0);
    mesh_faces(who, faces, V);
    Tensor valence = at::empty({V}, faces.options()), boundary = at::empty({V}, faces.options().dtype(at::kBool));
    size_t bytes;
    Tensor ws = smooth_workspace(who, vertices, V, T, &bytes);
    check(be_mesh_adjacency_f32(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, valence.data_ptr<int32_t>(),
                                reinterpret_cast<uint8_t*>(boundary.data_ptr<bool>()), ws.data_ptr<int64_t>(), bytes, stream_of(vertices)),
          "be_mesh_adjacency_f32");
    return {valence, boundary};
}

// -> [vertices [V,3], displacement [V], valence [V] int32, boundary [V] bool]
std::vector<Tensor> mesh_smooth(const Tensor& vertices, const Tensor& faces, int64_t iters, double lam, double mu, bool free_boundary) {
    const char* who = "mesh_smooth";
    const int64_t V = mesh_vertices(who, vertices), T = faces.size(0);
    mesh_faces(who, faces, V);
    TORCH_CHECK(iters >= 0 && iters <= BE_SMOOTH_MAX_ITERS, "mesh_smooth: iters must be in [0, ", BE_SMOOTH_MAX_ITERS, "]");
    Tensor out = at::empty({V, 3}, vertices.options()), displacement = at::empty({V}, vertices.options());
    Tensor valence = at::empty({V}, faces.options()), boundary = at::empty({V}, faces.options().dtype(at::kBool));
    size_t bytes;
    Tensor ws = smooth_workspace(who, vertices, V, T, &bytes);
    check(be_mesh_smooth_f32(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, (int)iters, lam, mu, free_boundary ? 1 : 0,
                             out.data_ptr<float>(), displacement.data_ptr<float>(), valence.data_ptr<int32_t>(),
                             reinterpret_cast<uint8_t*>(boundary.data_ptr<bool>()), ws.data_ptr<int64_t>(), bytes, stream_of(vertices)),
          "be_mesh_smooth_f32");
    return {out, displacement, valence, boundary};
}

// -> [normal [V,3], normal_valid [V] bool]
std::vector<Tensor> mesh_normals(const Tensor& vertices, const Tensor& faces) {
    const char* who = "mesh_normals";
    const int64_t V = mesh_vertices(who, vertices), T = faces.size(0);
    mesh_faces(who, faces, V);
    Tensor normal = at::empty({V, 3}, vertices.options()), valid = at::empty({V}, vertices.options().dtype(at::kBool));
    size_t bytes;
    Tensor ws = smooth_workspace(who, vertices, V, T, &bytes);
    check(be_mesh_normals_f32(vertices.data_ptr<float>(), faces.data_ptr<int32_t>(), V, T, normal.data_ptr<float>(),
                              reinterpret_cast<uint8_t*>(valid.data_ptr<bool>()), ws.data_ptr<int64_t>(), bytes, stream_of(vertices)),
          "be_mesh_normals_f32");
    return {normal, valid};
}

// depth registration: normal [3,H,W] of depth [H,W]; cam [4] a CPU float32 tensor as for unproject
Tensor depth_normals(const Tensor& depth, const Tensor& cam, int64_t step, double max_jump, int64_t scale, int64_t top, int64_t left) {
    depth_map("depth_normals", depth, "depth", "[H,W]");
    Tensor normal = at::empty({3, depth.size(0), depth.size(1)}, depth.options());
    check(be_depth_normals_f32(depth.data_ptr<float>(), (int)depth.size(0), (int)depth.size(1), (int)scale, (int)top, (int)left,
                               host_floats(cam, 4, "depth_normals(cam)"), (int)step, (float)max_jump, normal.data_ptr<float>(),
                               stream_of(depth)), "be_depth_normals_f32");
    return normal;
}

// the linearised point-to-plane step: depth_s [Hs,Ws] (weight_s or None) against depth_d [Hd,Wd], normal_d [3,Hd,Wd] (weight_d or
// None) -> (sums [32] float64, rows [8,Hs*Ws] or an empty tensor when rows is false); the partial sums are scratch allocated here
std::tuple<Tensor, Tensor> icp_linearize(const Tensor& depth_s, const c10::optional<Tensor>& weight_s, const Tensor& cam_src, int64_t scale,
                                         int64_t top, int64_t left, const Tensor& depth_d, const Tensor& normal_d,
                                         const c10::optional<Tensor>& weight_d, const Tensor& cam_dst, const Tensor& pose, double near,
                                         double max_dist, double huber, bool rows) {
    const float* ps = depth_map("icp_linearize", depth_s, "depth_s");
    const float* pd = depth_map("icp_linearize", depth_d, "depth_d", "[Hd,Wd]");
    const int64_t Hs = depth_s.size(0), Ws = depth_s.size(1), Hd = depth_d.size(0), Wd = depth_d.size(1);
    TORCH_CHECK(normal_d.numel() == 3 * Hd * Wd && normal_d.size(0) == 3 && normal_d.device() == depth_s.device() && depth_d.device() == depth_s.device(),
                "icp_linearize: normal_d [3,Hd,Wd] and depth_d on depth_s's device");
    const float* pws = map_like("icp_linearize", weight_s, depth_s, "weight_s", "[Hs,Ws]", "depth_s");
    const float* pwd = map_like("icp_linearize", weight_d, depth_d, "weight_d", "[Hd,Wd]", "depth_s");   // depth_d is on depth_s's device
    const int64_t bytes = be_icp_scratch_bytes((int)Hs, (int)Ws);
    TORCH_CHECK(bytes > 0, "icp_linearize: no scratch size for ", Hs, " x ", Ws);
    auto o = depth_s.options();
    Tensor scratch = at::empty({bytes / 8}, o.dtype(at::kDouble)), sums = at::empty({32}, o.dtype(at::kDouble));
    Tensor rout = rows ? at::empty({8, Hs * Ws}, o) : at::empty({0}, o);
    check(be_icp_linearize_f32(ps, pws, (int)Hs, (int)Ws, (int)scale, (int)top, (int)left,
                               host_floats(cam_src, 4, "icp_linearize(cam_src)"), pd, fp(normal_d, "normal_d"), pwd,
                               (int)Hd, (int)Wd, host_floats(cam_dst, 4, "icp_linearize(cam_dst)"),
                               host_floats(pose, 12, "icp_linearize(pose)"), (float)near, (float)max_dist, (float)huber,
                               scratch.data_ptr<double>(), sums.data_ptr<double>(), rows ? rout.data_ptr<float>() : nullptr,
                               stream_of(depth_s)), "be_icp_linearize_f32");
    return {sums, rout};
}

// nearest-sample flood fill: depth [H,W], weight [H,W] or None -> (depth_out [H,W], index [H,W] int32, dist2 [H,W] int32); the seed
// maps and the per-seed means are scratch allocated here
std::tuple<Tensor, Tensor, Tensor> fill_nearest(const Tensor& depth, const c10::optional<Tensor>& weight, int64_t smooth_r, double sigma_z,
                                                bool fuse) {
    TORCH_CHECK(depth.dim() == 2 && depth.numel() > 0 && depth.size(0) <= 16384 && depth.size(1) <= 16384,
                "fill_nearest: depth [H,W], 1 <= H, W <= 16384");
    TORCH_CHECK(smooth_r >= 0 && smooth_r <= 8, "fill_nearest: smooth_r must be in [0, 8]");
    fp(depth, "depth");
    const int64_t H = depth.size(0), W = depth.size(1);
    const float* pw = map_like("fill_nearest", weight, depth, "weight", "[H,W]");
    auto o = depth.options();
    Tensor scratch = at::empty({smooth_r > 0 ? 3 : 2, H, W}, o.dtype(at::kInt));
    Tensor dout = at::empty({H, W}, o), index = at::empty({H, W}, o.dtype(at::kInt)), dist2 = at::empty({H, W}, o.dtype(at::kInt));
    check(be_fill_nearest_f32(depth.data_ptr<float>(), pw, (int)H, (int)W, (int)smooth_r, (float)sigma_z, fuse ? 1 : 0,
                              scratch.data_ptr<int32_t>(), dout.data_ptr<float>(), index.data_ptr<int32_t>(), dist2.data_ptr<int32_t>(),
                              stream_of(depth)), "be_fill_nearest_f32");
    return {dout, index, dist2};
}

// diffusion depth completion: depth [H,W], weight / edge [H,W] or None -> (depth_out [H,W], index [H,W] int32, dist2 [H,W] int32,
// residual [1]); iters 0: the default schedule; the pyramid is scratch allocated here
std::tuple<Tensor, Tensor, Tensor, Tensor> fill_diffuse(const Tensor& depth, const c10::optional<Tensor>& weight,
                                                        const c10::optional<Tensor>& edge, int64_t smooth_r, double sigma_z, double leak,
                                                        int64_t iters, bool fuse) {
    TORCH_CHECK(depth.dim() == 2 && depth.numel() > 0 && depth.size(0) <= 16384 && depth.size(1) <= 16384,
                "fill_diffuse: depth [H,W], 1 <= H, W <= 16384");
    TORCH_CHECK(smooth_r >= 0 && smooth_r <= 8, "fill_diffuse: smooth_r must be in [0, 8]");
    TORCH_CHECK(iters >= 0 && iters <= 4096, "fill_diffuse: iters must be in [0, 4096]");
    fp(depth, "depth");
    const int64_t H = depth.size(0), W = depth.size(1);
    const float* pw = map_like("fill_diffuse", weight, depth, "weight", "[H,W]");
    const float* pe = map_like("fill_diffuse", edge, depth, "edge", "[H,W]");
    auto o = depth.options();
    const int64_t bytes = be_fill_diffuse_scratch_bytes((int)H, (int)W);
    TORCH_CHECK(bytes > 0, "fill_diffuse: no scratch size for ", H, " x ", W);
    Tensor scratch = at::empty({bytes / 4}, o.dtype(at::kInt));
    Tensor dout = at::empty({H, W}, o), index = at::empty({H, W}, o.dtype(at::kInt)), dist2 = at::empty({H, W}, o.dtype(at::kInt));
    Tensor residual = at::empty({1}, o);
    check(be_fill_diffuse_f32(depth.data_ptr<float>(), pw, pe, (int)H, (int)W, (int)smooth_r,
                              (float)sigma_z, (float)leak, (int)iters, fuse ? 1 : 0, scratch.data_ptr<int32_t>(), dout.data_ptr<float>(),
                              index.data_ptr<int32_t>(), dist2.data_ptr<int32_t>(), residual.data_ptr<float>(), stream_of(depth)),
          "be_fill_diffuse_f32");
    return {dout, index, dist2, residual};
}

// LocalLoss forward + analytic backward in one launch -> (partial [B,3], grad_est [B,10] or an empty tensor)
std::tuple<Tensor, Tensor> local_loss(const Tensor& opts, const Tensor& est, const Tensor& img_fit, const Tensor& gt, const Tensor& bdist,
                                      const Tensor& deri, double beta_b, double beta_s, bool want_grad) {
    TORCH_CHECK(est.dim() == 2 && est.size(1) == 10, "local_loss: est [B,10]");
    fp(est, "est");
    const int64_t b = est.size(0);
    TORCH_CHECK(img_fit.numel() == b * BE_NPIX * 3 && gt.numel() == b * BE_NPIX * 3 && bdist.numel() == b * BE_NPIX && deri.numel() == b * 361 * 3,
                "local_loss: img / gt [B,21,21,3], bdist [B,21,21], deri [B,19,19,3]");
    Tensor partial = at::empty({b, 3}, est.options());
    Tensor grad = want_grad ? at::empty({b, 10}, est.options()) : at::empty({0}, est.options());
    check(be_local_loss_f32(host_struct<be_render_opts>(opts, "local_loss(opts)"), est.data_ptr<float>(), fp(img_fit, "img_fit"), fp(gt, "gt"),
                            fp(bdist, "bdist"), fp(deri, "deri"), (float)beta_b, (float)beta_s, partial.data_ptr<float>(),
                            want_grad ? grad.data_ptr<float>() : nullptr, nullptr, nullptr, b, stream_of(est)), "be_local_loss_f32");
    return {partial, grad};
}
Tensor local_loss_finish(const Tensor& partial, double beta_b, double beta_s) {
    TORCH_CHECK(partial.dim() == 2 && partial.size(1) == 3, "local_loss_finish: partial [B,3]");
    Tensor out = at::empty({1}, partial.options());
    check(be_local_loss_finish_f32(fp(partial, "partial"), (int)partial.size(0), (float)beta_b, (float)beta_s, out.data_ptr<float>(),
                                   stream_of(partial)), "be_local_loss_finish_f32");
    return out;
}

// GlobalLoss terms + analytic gradient in one launch -> (partial [B*P,8], grad [B*P,12], grad_depth [B*P,4])
std::tuple<Tensor, Tensor, Tensor> global_loss(const Tensor& opts, const Tensor& consts, const Tensor& est, const Tensor& img_fit, const Tensor& img_gt,
                                               const Tensor& G, const Tensor& Gd, const Tensor& Gb, const Tensor& bdist, const Tensor& deri,
                                               const Tensor& bdepth, at::ArrayRef<double> gamma6, int64_t hp, int64_t wp, int64_t stride) {
    TORCH_CHECK(est.dim() == 3 && est.size(2) == 12 && est.size(1) == hp * wp, "global_loss: est [B,P,12] with P = hp * wp");
    TORCH_CHECK(img_gt.dim() == 5 && gamma6.size() == 6, "global_loss: img_gt [B,2,H,W,3], six gammas");
    fp(est, "est");
    const int64_t B = est.size(0), P = est.size(1), H = img_gt.size(2), W = img_gt.size(3);
    float g6[6];
    for (int i = 0; i < 6; ++i) g6[i] = (float)gamma6[i];
    Tensor partial = at::empty({B * P, 8}, est.options()), grad = at::empty({B * P, 12}, est.options()), gdep = at::empty({B * P, 4}, est.options());
    check(be_global_loss_f32(host_struct<be_render_opts>(opts, "global_loss(opts)"), host_struct<be_depth_consts>(consts, "global_loss(consts)"),
                             est.data_ptr<float>(), fp(img_fit, "img_fit"), fp(img_gt, "img_gt"), fp(G, "G"), fp(Gd, "Gderi"), fp(Gb, "Gbndry"),
                             fp(bdist, "bdist"), fp(deri, "deri"), fp(bdepth, "bdepth"), g6, partial.data_ptr<float>(), grad.data_ptr<float>(),
                             gdep.data_ptr<float>(), (int)B, (int)hp, (int)wp, (int)H, (int)W, (int)stride, stream_of(est)), "be_global_loss_f32");
    return {partial, grad, gdep};
}

// multi-head self-attention (head dim 16), inference / training forward / backward; workspaces are the caller's (reused across layers)
std::tuple<Tensor, Tensor> attention(const Tensor& qkv, int64_t B, int64_t L, int64_t l_valid, int64_t H, const optional<Tensor>& workspace_) {
    fp(qkv, "qkv");
    const size_t need = be_attention_workspace_floats((int)B, (int)L, (int)H);
    Tensor ws = workspace_.has_value() && workspace_->defined() && (size_t)workspace_->numel() >= need ? *workspace_
                                                                                                        : at::empty({(int64_t)need}, qkv.options());
    Tensor out = at::empty({B * L, H * 16}, qkv.options());
    check(be_attention_f32(qkv.data_ptr<float>(), out.data_ptr<float>(), fpm(ws, "workspace"), (int)B, (int)L, (int)l_valid, (int)H, stream_of(qkv)),
          "be_attention_f32");
    return {out, ws};
}
std::tuple<Tensor, Tensor> attention_train_fwd(const Tensor& qkv, Tensor workspace, int64_t B, int64_t L, int64_t l_valid, int64_t H, double p,
                                               int64_t seed) {
    fp(qkv, "qkv");
    TORCH_CHECK((size_t)workspace.numel() >= be_attention_train_workspace_floats((int)B, (int)L, (int)H), "attention_train_fwd: workspace too small");
    Tensor out = at::empty({B * L, H * 16}, qkv.options()), lse = at::empty({B * H, L}, qkv.options());
    check(be_attention_train_fwd_f32(qkv.data_ptr<float>(), out.data_ptr<float>(), lse.data_ptr<float>(), fpm(workspace, "workspace"), (int)B, (int)L,
                                     (int)l_valid, (int)H, (float)p, (uint32_t)seed, stream_of(qkv)), "be_attention_train_fwd_f32");
    return {out, lse};
}
Tensor attention_bwd(const Tensor& qkv, const Tensor& out, const Tensor& lse, const Tensor& dout, Tensor workspace, Tensor scratch,
                     bool operands_ready, int64_t B, int64_t L, int64_t l_valid, int64_t H, double p, int64_t seed) {
    fp(qkv, "qkv");
    TORCH_CHECK((size_t)workspace.numel() >= be_attention_train_workspace_floats((int)B, (int)L, (int)H) &&
                (size_t)scratch.numel() >= be_attention_bwd_scratch_floats((int)B, (int)L, (int)H), "attention_bwd: workspace / scratch too small");
    Tensor dqkv = at::empty_like(qkv);
    check(be_attention_bwd_f32(qkv.data_ptr<float>(), fp(out, "out"), fp(lse, "lse"), fp(dout, "dout"), dqkv.data_ptr<float>(),
                               fpm(workspace, "workspace"), fpm(scratch, "scratch"), operands_ready ? 1 : 0, (int)B, (int)L, (int)l_valid, (int)H,
                               (float)p, (uint32_t)seed, stream_of(qkv)), "be_attention_bwd_f32");
    return dqkv;
}

}  // namespace

TORCH_LIBRARY(be, m) {
    m.def("local_stage_pack(Tensor[] tensors, float eps) -> Tensor");
    m.def("local_stage_forward(Tensor packed, Tensor x, Tensor(a!)? out, Tensor(b!)? workspace, bool winograd, int chunk) -> (Tensor(a!), Tensor(b!))");
    m.def("render_colors(Tensor opts, Tensor params10, Tensor patches, Tensor(a!)? colors) -> Tensor(a!)");
    m.def("local_depth(Tensor consts, Tensor params10, Tensor(a!)? out) -> Tensor(a!)");
    m.def("train_unit_fwd(Tensor x, Tensor pw, Tensor pb, Tensor gamma, Tensor beta, Tensor? res, Tensor(a!) run_mean, Tensor(b!) run_var, "
          "int cout, int ksize, bool act, float eps, float momentum, Tensor(c!) scratch) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("train_unit_bwd(Tensor x, Tensor dout, Tensor? s_in, Tensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor? dg_pw, Tensor? dg_pb, "
          "Tensor? dx_add, int ksize, int chw_hw, Tensor(a!) dgamma, Tensor(b!) dbeta, Tensor(c!) dw, Tensor(d!) db, Tensor(e!) scratch) -> (Tensor, Tensor)");
    m.def("train_unit_pair_fwd(Tensor x, Tensor pw_a, Tensor pb_a, Tensor gamma_a, Tensor beta_a, Tensor(a!) rm_a, Tensor(b!) rv_a, int cout_a, "
          "int ks_a, bool act_a, Tensor pw_b, Tensor pb_b, Tensor gamma_b, Tensor beta_b, Tensor(c!) rm_b, Tensor(d!) rv_b, int cout_b, int ks_b, "
          "bool act_b, float eps, float momentum, Tensor(e!) scratch) -> Tensor[]");
    m.def("train_unit_pair_bwd(Tensor x, Tensor dout_a, Tensor? s_in_a, Tensor y_a, Tensor mean_a, Tensor invstd_a, Tensor gamma_a, Tensor dg_pw_a, "
          "Tensor dg_pb_a, int ks_a, Tensor(a!) dgamma_a, Tensor(b!) dbeta_a, Tensor(c!) dw_a, Tensor(d!) db_a, Tensor dout_b, Tensor? s_in_b, "
          "Tensor y_b, Tensor mean_b, Tensor invstd_b, Tensor gamma_b, Tensor dg_pw_b, Tensor dg_pb_b, int ks_b, Tensor(e!) dgamma_b, "
          "Tensor(f!) dbeta_b, Tensor(g!) dw_b, Tensor(h!) db_b, Tensor(i!) scratch) -> Tensor[]");
    m.def("maxpool_fwd_idx(Tensor x, int k, int stride, int pad) -> (Tensor, Tensor)");
    m.def("maxpool_bwd_idx(Tensor idx, Tensor dout, int h, int w, int k, int stride, int pad) -> Tensor");
    m.def("clip_adamw(Tensor table, int nentries, Tensor(a!) grad_flat, Tensor(b!) partial, float max_norm, float grad_scale, float lr, float beta1, "
          "float beta2, float eps, float weight_decay, Tensor(c!) step, Tensor(d!) grad_norm, bool write_back) -> ()");
    m.def("params2etas(Tensor p) -> Tensor");
    m.def("params2etas_bwd(Tensor p, Tensor geta) -> Tensor");
    m.def("params2dists(Tensor opts, Tensor params8) -> Tensor");
    m.def("params2dists_bwd(Tensor opts, Tensor params8, Tensor gdists) -> Tensor");
    m.def("dists2indicators(Tensor dists, Tensor etas) -> Tensor");
    m.def("dists2indicators_bwd(Tensor dists, Tensor etas, Tensor gwedges) -> (Tensor, Tensor)");
    m.def("inverse3x3(Tensor a) -> Tensor");
    m.def("inverse3x3_bwd(Tensor inv, Tensor gout) -> Tensor");
    m.def("image_derivative(Tensor img) -> Tensor");
    m.def("image_derivative_bwd(Tensor img, Tensor gout) -> Tensor");
    m.def("normalized_gaussian(Tensor x, float delta_sq) -> Tensor");
    m.def("normalized_gaussian_bwd(Tensor x, Tensor gy, float delta_sq) -> Tensor");
    m.def("etas2depth(Tensor consts, Tensor eta1, Tensor eta2) -> Tensor");
    m.def("etas2depth_bwd(Tensor consts, Tensor eta1, Tensor eta2, Tensor gz) -> (Tensor, Tensor)");
    m.def("depth2sigma(Tensor consts, Tensor depth, float rho_prime) -> Tensor");
    m.def("depth2sigma_bwd(Tensor consts, Tensor depth, float rho_prime, Tensor geta) -> Tensor");
    m.def("fold_patches(Tensor src, int B, int C, int hp, int wp, int H, int W, int stride, int mode) -> Tensor");
    m.def("fold_patches_bwd(Tensor gout, int hp, int wp, int stride, int mode) -> Tensor");
    m.def("wrap_angles_(Tensor(a!) est, int col0, int col1) -> ()");
    m.def("render_full(Tensor opts, Tensor consts, float rho_prime, bool densify_w, Tensor params12, Tensor view, Tensor pixels, int want) -> Tensor[]");
    m.def("fold_records(Tensor opts, Tensor records, int hp, int wp, int H, int W, int stride, bool densify_w, int want) -> Tensor[]");
    m.def("render_full_grid(Tensor opts, Tensor consts, float rho_prime, bool densify_w, Tensor params12, Tensor img, Tensor ys, Tensor xs) -> Tensor");
    m.def("fold_records_grid(Tensor opts, Tensor records, Tensor ys, Tensor xs, int H, int W, bool densify_w, int want) -> Tensor[]");
    m.def("fold_refocus_stack(Tensor opts, Tensor consts, Tensor records, Tensor rho_primes, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride) -> Tensor");
    m.def("fold_records_at(Tensor opts, Tensor records, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride, int scale, int top, int left, int h, int w, bool densify_w, int want) -> Tensor[]");
    m.def("fold_refocus_stack_at(Tensor opts, Tensor consts, Tensor records, Tensor rho_primes, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride, int scale, int top, int left, int h, int w) -> Tensor");
    m.def("fold_records_points(Tensor opts, Tensor records, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride, Tensor points, bool densify_w, int want) -> Tensor[]");
    m.def("fold_refocus_stack_points(Tensor opts, Tensor consts, Tensor records, Tensor rho_primes, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride, Tensor points) -> Tensor");
    m.def("unproject(Tensor depth, Tensor cam_src, Tensor pose, int scale, int top, int left) -> Tensor");
    m.def("reproject(Tensor depth, Tensor cam_src, Tensor cam_dst, Tensor pose, float near, int Ho, int Wo, Tensor? feat, int scale, int top, int left) -> (Tensor, Tensor, Tensor)");
    m.def("fuse_views(Tensor[] depth, Tensor[] weight, Tensor[] feat, Tensor cam_src, Tensor pose, Tensor cam_dst, float near, int Ho, int Wo, "
          "int[] scale, int[] top, int[] left, float tau, int min_views, bool recentre, int peel) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("tsdf_integrate(Tensor depth, Tensor? weight, Tensor? feat, Tensor cam_src, Tensor pose, float near, int scale, int top, int left, "
          "Tensor origin, Tensor voxel, float trunc, Tensor(a!) sw, Tensor(b!) swd, Tensor(c!) swf) -> ()");
    m.def("tsdf_mean(Tensor sw, Tensor swd, Tensor swf) -> (Tensor, Tensor, Tensor)");
    m.def("exclusive_scan(Tensor counts) -> (Tensor, Tensor)");
    m.def("tsdf_mesh(Tensor D, Tensor W, Tensor Fm, Tensor origin, Tensor voxel, float min_weight, bool normals) -> Tensor[]");
    m.def("mesh_raster(Tensor vertices, Tensor faces, Tensor? weight, Tensor? feat, Tensor? normal, Tensor? normal_valid, Tensor cam_dst, "
          "Tensor pose, float near, int cull, int Ho, int Wo, bool want_bary) -> Tensor[]");
    m.def("mesh_components(Tensor faces, int V) -> Tensor[]");
    m.def("mesh_components_stats(Tensor vertices, Tensor faces, Tensor component, int Kcap) -> Tensor[]");
    m.def("mesh_components_decide(Tensor triangles, Tensor area_q, Tensor total, int min_triangles, float min_area, bool largest, "
          "Tensor? component) -> Tensor[]");
    m.def("mesh_select_count(Tensor faces, Tensor vertex_keep) -> Tensor[]");
    m.def("mesh_select(Tensor vertices, Tensor faces, Tensor? weight, Tensor? feat, Tensor? normal, Tensor? normal_valid, Tensor? edge, "
          "Tensor? component, Tensor vertex_keep, Tensor voff, Tensor foff, int V2, int T2) -> Tensor[]");
    m.def("mesh_cluster(Tensor vertices, Tensor? weight, Tensor cell, Tensor origin) -> Tensor[]");
    m.def("mesh_simplify_count(Tensor vertices, Tensor faces, Tensor? weight, Tensor? feat, Tensor? normal, Tensor? normal_valid, Tensor cell, "
          "Tensor origin, Tensor cluster, bool flaps) -> Tensor[]");
    m.def("mesh_simplify(Tensor vertices, Tensor faces, Tensor cell, Tensor origin, Tensor label, Tensor cluster, Tensor members, Tensor sums, int C, "
          "bool normals, bool want_weight, Tensor fflag, Tensor foff, int V2, int T2) -> Tensor[]");
    m.def("mesh_adjacency(Tensor vertices, Tensor faces) -> Tensor[]");
    m.def("mesh_smooth(Tensor vertices, Tensor faces, int iters, float lam, float mu, bool free_boundary) -> Tensor[]");
    m.def("mesh_normals(Tensor vertices, Tensor faces) -> Tensor[]");
    m.def("tsdf_raycast(Tensor D, Tensor W, Tensor Fm, Tensor origin, Tensor voxel, Tensor cam_dst, Tensor pose, int Ho, int Wo, float z_near, "
          "float step, int n) -> (Tensor, Tensor, Tensor)");
    m.def("depth_normals(Tensor depth, Tensor cam, int step, float max_jump, int scale, int top, int left) -> Tensor");
    m.def("icp_linearize(Tensor depth_s, Tensor? weight_s, Tensor cam_src, int scale, int top, int left, Tensor depth_d, Tensor normal_d, "
          "Tensor? weight_d, Tensor cam_dst, Tensor pose, float near, float max_dist, float huber, bool rows) -> (Tensor, Tensor)");
    m.def("fill_nearest(Tensor depth, Tensor? weight, int smooth_r, float sigma_z, bool fuse) -> (Tensor, Tensor, Tensor)");
    m.def("fill_diffuse(Tensor depth, Tensor? weight, Tensor? edge, int smooth_r, float sigma_z, float leak, int iters, bool fuse) -> "
          "(Tensor, Tensor, Tensor, Tensor)");
    m.def("local_loss(Tensor opts, Tensor est, Tensor img_fit, Tensor gt, Tensor bdist, Tensor deri, float beta_b, float beta_s, bool want_grad) -> (Tensor, Tensor)");
    m.def("local_loss_finish(Tensor partial, float beta_b, float beta_s) -> Tensor");
    m.def("global_loss(Tensor opts, Tensor consts, Tensor est, Tensor img_fit, Tensor img_gt, Tensor G, Tensor Gd, Tensor Gb, Tensor bdist, Tensor deri, "
          "Tensor bdepth, float[] gamma6, int hp, int wp, int stride) -> (Tensor, Tensor, Tensor)");
    m.def("attention(Tensor qkv, int B, int L, int l_valid, int H, Tensor(a!)? workspace) -> (Tensor, Tensor(a!))");
    m.def("attention_train_fwd(Tensor qkv, Tensor(a!) workspace, int B, int L, int l_valid, int H, float p, int seed) -> (Tensor, Tensor)");
    m.def("attention_bwd(Tensor qkv, Tensor out, Tensor lse, Tensor dout, Tensor(a!) workspace, Tensor(b!) scratch, bool operands_ready, int B, int L, "
          "int l_valid, int H, float p, int seed) -> Tensor");
}

// on ROCm builds of PyTorch the GPU dispatch key is named CUDA (HIP masquerades as it); ops that take only host structs + GPU tensors
// dispatch on the GPU tensors
TORCH_LIBRARY_IMPL(be, CUDA, m) {
    m.impl("local_stage_pack", local_stage_pack);
    m.impl("local_stage_forward", local_stage_forward);
    m.impl("train_unit_fwd", train_unit_fwd);
    m.impl("train_unit_bwd", train_unit_bwd);
    m.impl("train_unit_pair_fwd", train_unit_pair_fwd);
    m.impl("train_unit_pair_bwd", train_unit_pair_bwd);
    m.impl("maxpool_fwd_idx", maxpool_fwd_idx);
    m.impl("maxpool_bwd_idx", maxpool_bwd_idx);
    m.impl("clip_adamw", clip_adamw);
}
// registered for every backend: these check their GPU arguments themselves, so that a CPU tensor raises the library's own
// "no CPU fallback" error instead of the dispatcher's missing-kernel message (some also take a CPU byte tensor - the host struct -
// next to their GPU tensors)
TORCH_LIBRARY_IMPL(be, CompositeExplicitAutograd, m) {
    m.impl("render_colors", render_colors);
    m.impl("local_depth", local_depth);
    m.impl("params2dists", params2dists);
    m.impl("params2dists_bwd", params2dists_bwd);
    m.impl("etas2depth", etas2depth);
    m.impl("etas2depth_bwd", etas2depth_bwd);
    m.impl("depth2sigma", depth2sigma);
    m.impl("depth2sigma_bwd", depth2sigma_bwd);
    m.impl("params2etas", params2etas);
    m.impl("params2etas_bwd", params2etas_bwd);
    m.impl("dists2indicators", dists2indicators);
    m.impl("dists2indicators_bwd", dists2indicators_bwd);
    m.impl("inverse3x3", inverse3x3);
    m.impl("inverse3x3_bwd", inverse3x3_bwd);
    m.impl("image_derivative", image_derivative);
    m.impl("image_derivative_bwd", image_derivative_bwd);
    m.impl("normalized_gaussian", normalized_gaussian);
    m.impl("normalized_gaussian_bwd", normalized_gaussian_bwd);
    m.impl("fold_patches", fold_patches);
    m.impl("fold_patches_bwd", fold_patches_bwd);
    m.impl("wrap_angles_", wrap_angles_);
    m.impl("render_full", render_full);
    m.impl("fold_records", fold_records);
    m.impl("render_full_grid", render_full_grid);
    m.impl("fold_records_grid", fold_records_grid);
    m.impl("fold_refocus_stack", fold_refocus_stack);
    m.impl("fold_records_at", fold_records_at);
    m.impl("fold_refocus_stack_at", fold_refocus_stack_at);
    m.impl("fold_records_points", fold_records_points);
    m.impl("fold_refocus_stack_points", fold_refocus_stack_points);
    m.impl("unproject", unproject);
    m.impl("reproject", reproject);
    m.impl("fuse_views", fuse_views);
    m.impl("tsdf_integrate", tsdf_integrate);
    m.impl("tsdf_mean", tsdf_mean);
    m.impl("tsdf_raycast", tsdf_raycast);
    m.impl("exclusive_scan", exclusive_scan);
    m.impl("tsdf_mesh", tsdf_mesh);
    m.impl("mesh_raster", mesh_raster);
    m.impl("mesh_components", mesh_components);
    m.impl("mesh_components_stats", mesh_components_stats);
    m.impl("mesh_components_decide", mesh_components_decide);
    m.impl("mesh_select_count", mesh_select_count);
    m.impl("mesh_select", mesh_select);
    m.impl("mesh_cluster", mesh_cluster);
    m.impl("mesh_simplify_count", mesh_simplify_count);
    m.impl("mesh_simplify", mesh_simplify);
    m.impl("mesh_adjacency", mesh_adjacency);
    m.impl("mesh_smooth", mesh_smooth);
    m.impl("mesh_normals", mesh_normals);
    m.impl("depth_normals", depth_normals);
    m.impl("icp_linearize", icp_linearize);
    m.impl("fill_nearest", fill_nearest);
    m.impl("fill_diffuse", fill_diffuse);
    m.impl("local_loss", local_loss);
    m.impl("local_loss_finish", local_loss_finish);
    m.impl("global_loss", global_loss);
    m.impl("attention", attention);
    m.impl("attention_train_fwd", attention_train_fwd);
    m.impl("attention_bwd", attention_bwd);
}

// msm_gfft.hpp -- transforms of vectors of curve points over a radix-2 domain (included by msm_engine.hip, after msm_pmul.hpp and
// msm_ntt.hpp): the C ABI mi355_msm_fft_points[_device] of include/mi355_msm.h over the kernels of group_fft.hpp.
//
// Reference: ARK poly/src/domain/mod.rs:99-170 (fft, ifft, coset_fft, coset_ifft over any DomainCoeff<F>).
// A call takes a single-device context (the point arithmetic, the work memory) and a domain handle (the twiddle tables, 1/n, the
// offset tables) of the same curve family on the same device.  Work memory: two vectors of n packed Affine images between the
// stages (104 B per G1 point, 200 B per G2 point), and per chunk of butterflies what a chunk of mul_points holds -- 2^(w-1) table
// entries per butterfly as XYZZ, as records, one prefix element and one flag byte each; the default chunk is mul_points' (2^19 table
// points for G1, 2^18 for G2 at w = 4: 2 GiB) and a wider test window shrinks it.  The two results of a butterfly land in the head
// of the staging buffer, which is free once the records are written.
#pragma once

#include "launch_gfft.hpp"

namespace {

constexpr size_t kGfftVecLimit = (size_t)64 << 30;   // the two work vectors: 2^28 G1 points, 2^27 G2 points

size_t gfft_chunk(const mi355_msm_ctx* ctx) {
  const size_t dflt = pmul_chunk_cap(ctx->curve, PM_DEFAULT_WINDOW), cap = pmul_chunk_cap(ctx->curve, pmul_window(ctx));
  const size_t want = ctx->opt_fft_points_chunk > 0 ? (size_t)ctx->opt_fft_points_chunk : dflt;
  return want < cap ? want : cap;
}

// everything a call can be refused for, decided before any device call; g: the offset as the offset tables need it
void gfft_check_call(mi355_msm_ctx* ctx, mi355_msm_domain* d, const void* out, size_t out_stride, const void* in, size_t in_len, size_t stride, unsigned kind,
                     unsigned flags, const void* offset, bool device_ptrs, Fr& g) {
  char buf[256];
  if (const char* m = gf_check_kind(kind, flags, offset != nullptr, buf, sizeof buf)) bad_arg("%s", m);
  if (!ctx) bad_arg("null context");
  if (!d) bad_arg("null domain handle");
  GfCall c{};
  c.ctx_curve = ctx->curve;
  c.ctx_sharded = !ctx->shards.empty();
  c.ctx_device = ctx->device;
  c.dom_curve = d->curve;
  c.dom_device = d->device;
  c.k = d->k;
  c.out = out;
  c.out_stride = out_stride;
  c.in = in;
  c.in_len = in_len;
  c.stride = stride;
  c.kind = kind;
  c.flags = flags;
  c.has_offset = offset != nullptr;
  c.work_limit = kGfftVecLimit;
  if (const char* m = gf_check_call(c, buf, sizeof buf)) bad_arg("%s", m);
  if (device_ptrs && (((uintptr_t)in | (uintptr_t)out) & 3)) bad_arg("device pointers must be 4-byte aligned");
  with_fr(d->curve, [&]<class FR>() { domain_offset<FR>(g, offset, kind, 0); });   // (refuses a zero offset)
}

// the whole transform, everything in device memory, enqueued on st; d_out == d_in with equal strides is allowed
template <class C>
void gfft_enqueue(mi355_msm_ctx* ctx, mi355_msm_domain* d, uint8_t* d_out, size_t out_stride, const uint8_t* d_in, size_t in_len, size_t stride, unsigned kind,
                  unsigned flags, const Fr& g, hipStream_t st) {
  using E = typename C::E;
  using El = typename E::T;
  using AD = AffineDevT<El>;
  using XD = XyzzDevT<El>;
  using FR = GfFr<E>;
  const uint32_t k = d->k, w = pmul_window(ctx), entries = pm_table_entries(w);
  const size_t n = (size_t)1 << k, half = n / 2, piece = gfft_chunk(ctx), cmax = std::min(piece, n);
  const size_t img0 = 2 * coord_bytes(ctx->curve) + 8, slots = std::max<size_t>(entries, 2) * cmax;
  const bool inverse = (kind & kNttKindInverse) != 0, coset = (kind & kNttKindCoset) != 0, projective = (flags & kGfProjective) != 0;
  const NttLayout at(k);
  Fr* t = d->tables.as<Fr>();
  if (coset && (!d->g_valid || !fr_same(g, d->g_have))) {
    d->g_valid = false;
    domain_two_level<FR>(d, g, at.glo, at.ghi, st);
    d->g_have = g;
    d->g_valid = true;
  }
  ctx->gf_stage.reserve(slots * sizeof(XD));
  ctx->gf_prefix.reserve(slots * sizeof(El));
  ctx->gf_rec.reserve((size_t)entries * cmax * sizeof(AD));
  ctx->gf_inf.reserve((size_t)entries * cmax);
  XD* stage = ctx->gf_stage.as<XD>();
  El* prefix = ctx->gf_prefix.as<El>();
  AD* rec = ctx->gf_rec.as<AD>();

  // the tables of cn points (B of the butterflies from b0 on of stage s, or the points from b0 on) as records
  auto tables = [&](const GfVec& v, bool stage_mode, uint32_t s, size_t b0, size_t cn, uint32_t ent) {
    HIP_OK(LaunchGfft<E>::table(v, k, s, stage_mode, (uint32_t)b0, (uint32_t)cn, ent, stage, st));
    if (ent == entries)
      HIP_OK(Launch<E>::pre_normalize(stage, (uint32_t)(ent * cn), FB_NORM_RUN, prefix, rec, ctx->gf_inf.as<uint8_t>(), st));
  };
  auto emit = [&](size_t from, size_t count, uint8_t* dst, size_t dstride, bool proj) {
    HIP_OK(LaunchFixed<E>::normalize(stage + from, (uint32_t)count, prefix, dst, dstride, proj, st));
  };
  // dst[j] = factor(j) * v[j] for j < count
  auto scale_pass = [&](const GfVec& v, size_t count, uint8_t* dst, size_t dstride, bool proj) {
    GfScale fs{};
    fs.g = NttTable{t + at.glo, t + at.ghi};
    fs.scale = d->size_inv;
    fs.has_g = coset ? 1u : 0u;
    fs.has_scale = inverse ? 1u : 0u;
    for (size_t j0 = 0; j0 < count; j0 += piece) {
      const size_t cn = std::min(piece, count - j0);
      tables(v, false, 0, j0, cn, entries);
      HIP_OK(LaunchGfft<E>::scale(rec, fs, k, (uint32_t)j0, (uint32_t)cn, w, stage, st));
      emit(0, cn, dst + j0 * dstride, dstride, proj);
    }
  };

  GfVec src{d_in, stride, (uint32_t)in_len};
  if (k == 0) {   // one point: every factor is 1
    tables(src, false, 0, 0, 1, 1);
    emit(0, 1, d_out, out_stride, projective);
    return;
  }
  ctx->gf_vec[0].reserve(n * img0);
  ctx->gf_vec[1].reserve(n * img0);
  int cur = -1;   // the work vector src is, -1: the caller's input
  if (coset && !inverse) {
    scale_pass(src, in_len, ctx->gf_vec[0].as<uint8_t>(), img0, false);
    cur = 0;
    src = GfVec{ctx->gf_vec[0].as<uint8_t>(), img0, (uint32_t)in_len};
  }
  const NttTable tw{t + (inverse ? at.ilo : at.wlo), t + (inverse ? at.ihi : at.whi)};
  for (uint32_t s = 0; s < k; s++) {
    const bool to_out = s + 1 == k && !inverse;
    const int nxt = cur == 0 ? 1 : 0;
    uint8_t* dst = to_out ? d_out : ctx->gf_vec[nxt].as<uint8_t>();
    const size_t dstride = to_out ? out_stride : img0;
    const bool proj = to_out && projective;
    for (size_t b0 = 0; b0 < half; b0 += piece) {
      const size_t cn = std::min(piece, half - b0);
      if (s > 0) tables(src, true, s, b0, cn, entries);
      HIP_OK(LaunchGfft<E>::stage(src, rec, tw, k, s, (uint32_t)b0, (uint32_t)cn, w, stage, st));
      if (cn == half) {
        emit(0, n, dst, dstride, proj);
      } else {
        emit(0, cn, dst + b0 * dstride, dstride, proj);
        emit(cn, cn, dst + (half + b0) * dstride, dstride, proj);
      }
    }
    if (!to_out) {
      cur = nxt;
      src = GfVec{ctx->gf_vec[cur].as<uint8_t>(), img0, (uint32_t)n};
    }
  }
  if (inverse) scale_pass(src, n, d_out, out_stride, projective);
}

void gfft_events(mi355_msm_ctx* ctx) {
  for (hipEvent_t& e : ctx->gf_ev)
    if (!e) HIP_OK(hipEventCreate(&e));
}

void gfft_finish(mi355_msm_ctx* ctx, std::chrono::steady_clock::time_point t0) {
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, ctx->gf_ev[0], ctx->gf_ev[1]));
  ctx->last_fft_points_device_us = (uint64_t)(ms * 1000.0f);
  ctx->last_fft_points_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

void gfft_device(mi355_msm_ctx* ctx, mi355_msm_domain* d, void* d_out, size_t out_stride, const void* d_in, size_t in_len, size_t stride, unsigned kind,
                 unsigned flags, const void* offset, hipStream_t st) {
  Fr g;
  gfft_check_call(ctx, d, d_out, out_stride, d_in, in_len, stride, kind, flags, offset, true, g);
  ensure_device(ctx);
  gfft_events(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(ctx->gf_ev[0], st));
    with_curve(ctx->curve, [&]<class C>() {
      gfft_enqueue<C>(ctx, d, (uint8_t*)d_out, out_stride, (const uint8_t*)d_in, in_len, stride, kind, flags, g, st);
    });
    HIP_OK(hipEventRecord(ctx->gf_ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  gfft_finish(ctx, t0);
}

// Host pointers: the in_len input images are staged in as they lie, the transform runs between the staged input and a packed output
// vector on the context's stream, and the copy out spreads the images to `out_stride`, so the caller's bytes between two images stay
// as they were.
void gfft_host(mi355_msm_ctx* ctx, mi355_msm_domain* d, void* out, size_t out_stride, const void* in, size_t in_len, size_t stride, unsigned kind, unsigned flags,
               const void* offset) {
  Fr g;
  gfft_check_call(ctx, d, out, out_stride, in, in_len, stride, kind, flags, offset, false, g);
  ensure_device(ctx);
  gfft_events(ctx);
  const hipStream_t st = ctx->own_stream;
  const size_t n = (size_t)1 << d->k, img = gf_image_bytes(ctx->curve, flags), cb = coord_bytes(ctx->curve);
  const auto t0 = std::chrono::steady_clock::now();
  try {
    ctx->gf_out.reserve(n * img);
    HIP_OK(hipEventRecord(ctx->gf_ev[0], st));
    if (in_len) {
      // (the last image of a strided array may end before its stride does: copy up to the end of its coordinates and flag)
      ctx->gf_points.reserve(in_len * stride);
      HIP_OK(hipMemcpyAsync(ctx->gf_points.p, in, (in_len - 1) * stride + 2 * cb + 1, hipMemcpyHostToDevice, st));
    }
    with_curve(ctx->curve, [&]<class C>() {
      gfft_enqueue<C>(ctx, d, ctx->gf_out.as<uint8_t>(), img, ctx->gf_points.as<uint8_t>(), in_len, stride, kind, flags, g, st);
    });
    if (out_stride == img)
      HIP_OK(hipMemcpyAsync(out, ctx->gf_out.p, n * img, hipMemcpyDeviceToHost, st));
    else
      HIP_OK(hipMemcpy2DAsync(out, out_stride, ctx->gf_out.p, img, img, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(ctx->gf_ev[1], st));
    HIP_OK(hipStreamSynchronize(st));   // (pageable host memory: the caller's buffers are free to go when the call returns)
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  gfft_finish(ctx, t0);
}

}  // namespace

extern "C" {

RustError mi355_msm_fft_points(mi355_msm_ctx* ctx, mi355_msm_domain* domain, void* out, size_t out_stride, const void* in, size_t in_len, size_t stride,
                               unsigned kind, unsigned flags, const void* offset) {
  return guarded_dev([&] { gfft_host(ctx, domain, out, out_stride, in, in_len, stride, kind, flags, offset); });
}

RustError mi355_msm_fft_points_device(mi355_msm_ctx* ctx, mi355_msm_domain* domain, void* d_out, size_t out_stride, const void* d_in, size_t in_len,
                                      size_t stride, unsigned kind, unsigned flags, const void* offset, void* stream) {
  return guarded_dev([&] { gfft_device(ctx, domain, d_out, out_stride, d_in, in_len, stride, kind, flags, offset, (hipStream_t)stream); });
}

}  // extern "C"

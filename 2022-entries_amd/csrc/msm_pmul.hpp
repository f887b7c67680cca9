// msm_pmul.hpp -- batch variable-base scalar multiplication over the MI355X engine (included by msm_engine.hip): the C ABI
// mi355_msm_mul_points[_device] of include/mi355_msm.h over the kernels of point_mul.hpp.
//
// Reference: ARK ec/src/lib.rs:188,294,305-319 (mul_bigint, mul_by_cofactor), ec/src/models/short_weierstrass.rs:413-422.
// Work memory does not grow with n: a call runs in chunks through DevBufs the context keeps.  Per point and table entry the pairwise
// path holds one XYZZ staging slot, one AffineDev record, one prefix element and one flag byte (G1: 224 + 128 + 56 + 1 B, G2 twice
// that but for the flag), 2^(w-1) entries per point; the default chunk is the largest power of two that keeps those buffers within
// 2 GiB at the default window (w = 4: 2^19 points for G1, 2^18 for G2), and a wider test window shrinks the chunk instead of growing the
// buffers.  The results of a chunk land in the head of the staging buffer, which is free once the records are written.  The
// one-scalar path needs the result slots and their prefix only.
#pragma once

#include "launch_fixed.hpp"   // the output normalisation
#include "launch_pmul.hpp"

namespace {

#include "cofactor_consts.inc"

constexpr unsigned kMulMont = 1u, kMulProjective = 2u, kMulUniform = 4u, kMulCofactor = 8u;
constexpr size_t kMulWorkLimit = (size_t)2 << 30;

// the largest power of two of points whose table buffers stay within kMulWorkLimit at window size w
size_t pmul_chunk_cap(int curve, uint32_t w) {
  const size_t el = is_g2(curve) ? 2 * sizeof(Fe) : sizeof(Fe);
  const size_t per_point = (size_t)pm_table_entries(w) * (4 * el + (is_g2(curve) ? sizeof(AffineDevT<Fe2>) : sizeof(AffineDev)) + el + 1);
  size_t c = 1;
  while (2 * c * per_point <= kMulWorkLimit) c *= 2;
  return c;
}

uint32_t pmul_window(const mi355_msm_ctx* ctx) { return ctx->opt_mul_window > 0 ? (uint32_t)ctx->opt_mul_window : PM_DEFAULT_WINDOW; }

size_t pmul_chunk(const mi355_msm_ctx* ctx) {
  const size_t dflt = pmul_chunk_cap(ctx->curve, PM_DEFAULT_WINDOW), cap = pmul_chunk_cap(ctx->curve, pmul_window(ctx));
  const size_t want = ctx->opt_mul_chunk > 0 ? (size_t)ctx->opt_mul_chunk : dflt;
  return want < cap ? want : cap;
}

size_t pmul_image_bytes(int curve, unsigned flags) { return (flags & kMulProjective) ? 3 * coord_bytes(curve) : 2 * coord_bytes(curve) + 8; }

// everything a call can be refused for, decided before any device call; fills the NAF of a one-scalar call
void pmul_check_call(mi355_msm_ctx* ctx, const void* points, size_t n, size_t stride, const void* scalars, size_t scalar_bytes, unsigned flags,
                     const void* out, size_t out_stride, PmNaf& naf) {
  if (!ctx) bad_arg("null context");
  if (!ctx->shards.empty()) bad_arg("mul_points is not available on a sharded context: use a single-device context");
  if (flags & ~(kMulMont | kMulProjective | kMulUniform | kMulCofactor))
    bad_arg("unknown mul_points flag bits 0x%x (bit 0: Fr Montgomery scalars, bit 1: Projective images, bit 2: one scalar for all points, bit 3: the cofactor)", flags);
  const bool uniform = (flags & (kMulUniform | kMulCofactor)) != 0;
  if (uniform && (flags & kMulMont)) bad_arg("flag bit 0 (Fr Montgomery scalars) contradicts a single integer scalar (bits 2, 3)");
  const size_t cb = coord_bytes(ctx->curve), img = pmul_image_bytes(ctx->curve, flags);
  if (stride % 4 || stride < 2 * cb + 1) bad_arg("stride %zu is not a 4-byte multiple >= %zu", stride, 2 * cb + 1);
  if (out_stride % 4) bad_arg("out_stride %zu is not a multiple of 4", out_stride);
  if (out_stride < img) bad_arg("out_stride %zu is smaller than the %zu-byte image", out_stride, img);
  if (flags & kMulCofactor) {
    if (scalars) bad_arg("the cofactor flag (bit 3) takes no scalars: pass NULL");
    if (scalar_bytes != 0) bad_arg("scalar_bytes %zu with the cofactor flag (bit 3): must be 0", scalar_bytes);
    pm_naf_recode(naf, kCofactorWords[ctx->curve], 16);
  } else if (uniform) {
    if (!scalars) bad_arg("null scalar pointer");
    if (scalar_bytes % 4 || scalar_bytes < 4 || scalar_bytes > 64) bad_arg("scalar_bytes %zu: one scalar for all points is a multiple of 4 from 4 to 64 bytes", scalar_bytes);
    uint32_t w[16] = {0};
    memcpy(w, scalars, scalar_bytes);
    pm_naf_recode(naf, w, 16);
  } else {
    if (scalar_bytes != 32) bad_arg("scalar_bytes %zu: pairwise scalars are 32-byte integers", scalar_bytes);
    if (n && !scalars) bad_arg("null scalars pointer");
  }
  if (n && (!points || !out)) bad_arg("null points or output pointer");
  if (n >= (1ull << 31)) bad_arg("npoints %zu exceeds 2^31-1", n);
}

// one chunk, everything in device memory, enqueued on st
template <class C>
void pmul_chunk_run(mi355_msm_ctx* ctx, const uint8_t* d_points, size_t stride, const uint32_t* d_scalars, const PmNaf& naf, size_t cn, unsigned flags,
                    uint8_t* d_out, size_t out_stride, hipStream_t st) {
  using E = typename C::E;
  using El = typename E::T;
  using AD = AffineDevT<El>;
  using XD = XyzzDevT<El>;
  if (flags & (kMulUniform | kMulCofactor)) {
    ctx->pm_stage.reserve(cn * sizeof(XD));
    ctx->pm_prefix.reserve(cn * sizeof(El));
    HIP_OK(LaunchPmul<E>::mul_uniform(d_points, stride, (uint32_t)cn, naf, ctx->pm_stage.as<XD>(), st));
  } else {
    const uint32_t w = pmul_window(ctx);
    const size_t entries = (size_t)pm_table_entries(w) * cn;
    ctx->pm_stage.reserve(entries * sizeof(XD));
    ctx->pm_rec.reserve(entries * sizeof(AD));
    ctx->pm_prefix.reserve(entries * sizeof(El));
    ctx->pm_inf.reserve(entries);
    HIP_OK(LaunchPmul<E>::table(d_points, stride, (uint32_t)cn, pm_table_entries(w), ctx->pm_stage.as<XD>(), st));
    HIP_OK(Launch<E>::pre_normalize(ctx->pm_stage.as<XD>(), (uint32_t)entries, FB_NORM_RUN, ctx->pm_prefix.as<El>(), ctx->pm_rec.as<AD>(),
                                    ctx->pm_inf.as<uint8_t>(), st));
    HIP_OK(LaunchPmul<E>::mul(ctx->pm_rec.as<AD>(), d_scalars, (uint32_t)cn, w, (flags & kMulMont) != 0, ctx->pm_stage.as<XD>(), st));
  }
  HIP_OK(LaunchFixed<E>::normalize(ctx->pm_stage.as<XD>(), (uint32_t)cn, ctx->pm_prefix.as<El>(), d_out, out_stride, (flags & kMulProjective) != 0, st));
}

void pmul_events(mi355_msm_ctx* ctx) {
  for (hipEvent_t& e : ctx->pm_ev)
    if (!e) HIP_OK(hipEventCreate(&e));
}

void pmul_finish(mi355_msm_ctx* ctx, std::chrono::steady_clock::time_point t0) {
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, ctx->pm_ev[0], ctx->pm_ev[1]));
  ctx->last_mul_device_us = (uint64_t)(ms * 1000.0f);
  ctx->last_mul_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

void pmul_device(mi355_msm_ctx* ctx, const void* d_points, size_t n, size_t stride, const void* scalars, size_t scalar_bytes, unsigned flags, void* d_out,
                 size_t out_stride, hipStream_t st) {
  PmNaf naf{};
  pmul_check_call(ctx, d_points, n, stride, scalars, scalar_bytes, flags, d_out, out_stride, naf);
  const bool uniform = (flags & (kMulUniform | kMulCofactor)) != 0;
  if (n == 0) return;
  if (((uintptr_t)d_points | (uintptr_t)d_out | (uniform ? 0 : (uintptr_t)scalars)) & 3) bad_arg("device pointers must be 4-byte aligned");
  ensure_device(ctx);
  pmul_events(ctx);
  const size_t piece = pmul_chunk(ctx);
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(ctx->pm_ev[0], st));
    for (size_t at = 0; at < n; at += piece) {
      const size_t cn = std::min(piece, n - at);
      with_curve(ctx->curve, [&]<class C>() {
        pmul_chunk_run<C>(ctx, (const uint8_t*)d_points + at * stride, stride, uniform ? nullptr : (const uint32_t*)scalars + 8 * at, naf, cn, flags,
                          (uint8_t*)d_out + at * out_stride, out_stride, st);
      });
    }
    HIP_OK(hipEventRecord(ctx->pm_ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  pmul_finish(ctx, t0);
}

// Host pointers: every chunk is staged in, computed and copied out on the context's stream, whose order keeps a chunk's buffers from
// being refilled before they were read.  The images are packed in device memory and spread to `out_stride` by the copy out, so the
// caller's bytes between two images stay as they were.
void pmul_host(mi355_msm_ctx* ctx, const void* points, size_t n, size_t stride, const void* scalars, size_t scalar_bytes, unsigned flags, void* out,
               size_t out_stride) {
  PmNaf naf{};
  pmul_check_call(ctx, points, n, stride, scalars, scalar_bytes, flags, out, out_stride, naf);
  const bool uniform = (flags & (kMulUniform | kMulCofactor)) != 0;
  if (n == 0) return;
  ensure_device(ctx);
  pmul_events(ctx);
  const hipStream_t st = ctx->own_stream;
  const size_t piece = pmul_chunk(ctx), img = pmul_image_bytes(ctx->curve, flags), cb = coord_bytes(ctx->curve);
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(ctx->pm_ev[0], st));
    for (size_t at = 0; at < n; at += piece) {
      const size_t cn = std::min(piece, n - at);
      ctx->pm_points.reserve(cn * stride);
      ctx->pm_out.reserve(cn * img);
      // (the last image of a strided array may end before its stride does: copy up to the end of its coordinates and flag)
      HIP_OK(hipMemcpyAsync(ctx->pm_points.p, (const uint8_t*)points + at * stride, (cn - 1) * stride + 2 * cb + 1, hipMemcpyHostToDevice, st));
      if (!uniform) {
        ctx->pm_scalars.reserve(cn * 32);
        HIP_OK(hipMemcpyAsync(ctx->pm_scalars.p, (const uint8_t*)scalars + 32 * at, cn * 32, hipMemcpyHostToDevice, st));
      }
      with_curve(ctx->curve, [&]<class C>() {
        pmul_chunk_run<C>(ctx, ctx->pm_points.as<uint8_t>(), stride, uniform ? nullptr : ctx->pm_scalars.as<uint32_t>(), naf, cn, flags,
                          ctx->pm_out.as<uint8_t>(), img, st);
      });
      uint8_t* dst = (uint8_t*)out + at * out_stride;
      if (out_stride == img)
        HIP_OK(hipMemcpyAsync(dst, ctx->pm_out.p, cn * img, hipMemcpyDeviceToHost, st));
      else
        HIP_OK(hipMemcpy2DAsync(dst, out_stride, ctx->pm_out.p, img, img, cn, hipMemcpyDeviceToHost, st));
      if (at + cn >= n) HIP_OK(hipEventRecord(ctx->pm_ev[1], st));
      HIP_OK(hipStreamSynchronize(st));   // (pageable host memory: the caller's buffers are free to go when the call returns)
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  pmul_finish(ctx, t0);
}

}  // namespace

extern "C" {

RustError mi355_msm_mul_points(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t scalar_bytes,
                               unsigned flags, void* out, size_t out_stride) {
  return guarded_dev([&] { pmul_host(ctx, points, npoints, stride, scalars, scalar_bytes, flags, out, out_stride); });
}

RustError mi355_msm_mul_points_device(mi355_msm_ctx* ctx, const void* d_points, size_t npoints, size_t stride, const void* scalars, size_t scalar_bytes,
                                      unsigned flags, void* d_out, size_t out_stride, void* stream) {
  return guarded_dev([&] { pmul_device(ctx, d_points, npoints, stride, scalars, scalar_bytes, flags, d_out, out_stride, (hipStream_t)stream); });
}

}  // extern "C"

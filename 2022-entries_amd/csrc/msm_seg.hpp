// msm_seg.hpp -- segmented MSM over the MI355X engine (included by msm_engine.hip): the C ABI mi355_msm_segments of
// include/mi355_msm.h over the kernels of seg_msm.hpp.  One entry point with a pointer-kind flag, the convention of mi355_msm_expr_run.
//
// Work memory grows with the number of segments, never with their lengths: per segment ceil(257 / c) window sums, one result slot,
// one prefix element and one id (sm_seg_work).  A call runs its segments in chunks that keep these within 2 GiB -- the budget of
// mul_points -- or within "seg_chunk" segments; the offsets (8 bytes a segment) are uploaded once.  Host-pointer calls stage the
// points, the scalars (through FrStage) and the packed output whole.
#pragma once

#include "launch_fixed.hpp"   // the output normalisation
#include "launch_seg.hpp"

namespace {

constexpr unsigned kSegMont = 1u, kSegDevice = 2u, kSegShared = 4u, kSegProjective = 8u;
constexpr size_t kSegWorkLimit = (size_t)2 << 30;

size_t seg_image_bytes(int curve, unsigned flags) { return (flags & kSegProjective) ? 3 * coord_bytes(curve) : 2 * coord_bytes(curve) + 8; }

bool seg_ranges_meet(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// everything a call can be refused for, decided before any device call
void seg_check_call(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t nscalars, const uint64_t* offsets,
                    size_t nseg, unsigned flags, const void* out, size_t out_stride, hipStream_t st) {
  if (!ctx) bad_arg("null context");
  if (!ctx->shards.empty()) bad_arg("msm_segments is not available on a sharded context: use a single-device context");
  if (flags & ~(kSegMont | kSegDevice | kSegShared | kSegProjective))
    bad_arg("unknown msm_segments flag bits 0x%x (bit 0: Fr Montgomery scalars, bit 1: device pointers, bit 2: shared bases, bit 3: Projective images)", flags);
  const bool device_ptrs = (flags & kSegDevice) != 0;
  if (!device_ptrs && st) bad_arg("a stream goes with device pointers (flag bit 1) only");
  const size_t cb = coord_bytes(ctx->curve), img = seg_image_bytes(ctx->curve, flags);
  if (stride % 4 || stride < 2 * cb + 1) bad_arg("stride %zu is not a 4-byte multiple >= %zu", stride, 2 * cb + 1);
  if (out_stride % 4) bad_arg("out_stride %zu is not a multiple of 4", out_stride);
  if (out_stride < img) bad_arg("out_stride %zu is smaller than the %zu-byte image", out_stride, img);
  if (npoints >= (1ull << 32)) bad_arg("npoints %zu exceeds 2^32-1", npoints);
  if (nseg >= (1ull << 32)) bad_arg("nsegments %zu exceeds 2^32-1", nseg);
  if (flags & kSegShared) {
    if (offsets) bad_arg("offsets must be NULL in the shared form (flag bit 2): every segment reads all %zu points", npoints);
    if (nscalars != nseg * npoints) bad_arg("nscalars %zu: the shared form takes nsegments * npoints = %zu scalars", nscalars, nseg * npoints);
  } else {
    if (!offsets) bad_arg("null offsets pointer (nsegments + 1 host values; the shared form, flag bit 2, takes none)");
    if (offsets[0] != 0) bad_arg("offsets[0] = %llu: the first offset must be 0", (unsigned long long)offsets[0]);
    for (size_t s = 0; s < nseg; s++)
      if (offsets[s + 1] < offsets[s])
        bad_arg("offsets[%zu] = %llu is smaller than offsets[%zu] = %llu: offsets must not decrease", s + 1, (unsigned long long)offsets[s + 1], s,
                (unsigned long long)offsets[s]);
    if (offsets[nseg] != npoints) bad_arg("offsets[%zu] = %llu: the last offset must equal npoints %zu", nseg, (unsigned long long)offsets[nseg], npoints);
    if (nscalars != npoints) bad_arg("nscalars %zu: the general form takes one scalar per point (npoints %zu)", nscalars, npoints);
  }
  if (npoints && !points) bad_arg("null points pointer");
  if (nscalars && !scalars) bad_arg("null scalars pointer");
  if (nseg && !out) bad_arg("null output pointer");
  if (device_ptrs && (((uintptr_t)points | (uintptr_t)scalars | (uintptr_t)out) & 3)) bad_arg("device pointers must be 4-byte aligned");
  const size_t out_bytes = nseg ? (nseg - 1) * out_stride + img : 0;
  if (seg_ranges_meet(out, out_bytes, points, npoints ? (npoints - 1) * stride + 2 * cb + 1 : 0)) bad_arg("out overlaps points");
  if (seg_ranges_meet(out, out_bytes, scalars, nscalars * 32)) bad_arg("out overlaps scalars");
}

uint32_t seg_tile(const mi355_msm_ctx* ctx) { return ctx->opt_seg_tile > 0 ? (uint32_t)ctx->opt_seg_tile : SM_DEFAULT_TILE; }

// the chunks of one call, everything in device memory, enqueued on st; d_out: images out_stride apart
template <class C>
void seg_enqueue(mi355_msm_ctx* ctx, const SmPlan& plan, const uint8_t* d_points, size_t npoints, size_t stride, const uint32_t* d_scalars,
                 const uint64_t* offsets, size_t nseg, unsigned flags, uint8_t* d_out, size_t out_stride, hipStream_t st) {
  using E = typename C::E;
  using El = typename E::T;
  using XD = XyzzDevT<El>;
  const bool shared = (flags & kSegShared) != 0;
  ctx->sg_wsum.reserve((plan.max_wsum_records ? plan.max_wsum_records : 1) * sizeof(XD));
  ctx->sg_stage.reserve(plan.max_segs * sizeof(XD));
  ctx->sg_prefix.reserve(plan.max_segs * sizeof(El));
  if (!shared) {
    ctx->sg_ids.reserve(plan.max_segs * 4);
    ctx->sg_offs.reserve((nseg + 1) * 8);
    HIP_OK(hipMemcpyAsync(ctx->sg_offs.p, offsets, (nseg + 1) * 8, hipMemcpyHostToDevice, st));
  }
  for (const SmChunk& ch : plan.chunks) {
    const size_t cn = ch.s1 - ch.s0;
    HIP_OK(hipMemsetAsync(ctx->sg_stage.p, 0, cn * sizeof(XD), st));   // (all zero is the point at infinity: what an empty segment gives)
    if (!shared && !ch.ids.empty()) {
      // (stream order keeps the previous chunk's kernels ahead of this copy)
      HIP_OK(hipMemcpyAsync(ctx->sg_ids.p, ch.ids.data(), ch.ids.size() * 4, hipMemcpyHostToDevice, st));
    }
    for (const SmClass& k : ch.classes) {
      SmLaunch a{};
      a.points = d_points;
      a.stride = stride;
      a.scalars = d_scalars;
      a.offs = shared ? nullptr : ctx->sg_offs.as<uint64_t>() + ch.s0;
      a.ids = shared ? nullptr : ctx->sg_ids.as<uint32_t>() + k.ids_at;   // (the shared form has one class, every segment in order)
      a.shared_len = shared ? npoints : 0;
      a.shared_seg0 = ch.s0;
      a.nseg = k.nseg;
      a.c = k.c;
      a.nwin = k.nwin;
      a.tile = k.tile;
      a.from_mont = (flags & kSegMont) ? 1u : 0u;
      XD* wsum = ctx->sg_wsum.as<XD>() + k.wsum_at;
      HIP_OK(LaunchSeg<E>::accumulate(a, wsum, st));
      HIP_OK(LaunchSeg<E>::tail(wsum, a.ids, k.nseg, k.nwin, k.c, ctx->sg_stage.as<XD>(), st));
    }
    HIP_OK(LaunchFixed<E>::normalize(ctx->sg_stage.as<XD>(), (uint32_t)cn, ctx->sg_prefix.as<El>(), d_out + ch.s0 * out_stride, out_stride,
                                     (flags & kSegProjective) != 0, st));
  }
}

void seg_run(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t nscalars, const uint64_t* offsets, size_t nseg,
             unsigned flags, void* out, size_t out_stride, hipStream_t st) {
  seg_check_call(ctx, points, npoints, stride, scalars, nscalars, offsets, nseg, flags, out, out_stride, st);
  if (nseg == 0) return;
  const bool device_ptrs = (flags & kSegDevice) != 0, shared = (flags & kSegShared) != 0;
  const size_t el = is_g2(ctx->curve) ? 2 * sizeof(Fe) : sizeof(Fe), img = seg_image_bytes(ctx->curve, flags), cb = coord_bytes(ctx->curve);
  SmPlan plan;
  sm_plan(plan, shared ? nullptr : offsets, nseg, shared ? npoints : 0, (uint32_t)ctx->opt_seg_window, seg_tile(ctx), (size_t)ctx->opt_seg_chunk, kSegWorkLimit,
          4 * el, el);
  if (!plan.fits) bad_arg("one segment's work memory exceeds the limit");
  ensure_device(ctx);
  for (hipEvent_t& e : ctx->sg_ev)
    if (!e) HIP_OK(hipEventCreate(&e));
  const hipStream_t on = device_ptrs ? st : ctx->own_stream;
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(ctx->sg_ev[0], on));
    const uint8_t* d_points = (const uint8_t*)points;
    const uint32_t* d_scalars = (const uint32_t*)scalars;
    uint8_t* d_out = (uint8_t*)out;
    size_t d_out_stride = out_stride;
    if (!device_ptrs) {
      FrStage g(ctx->sg_scalars, false, on, nscalars);
      d_scalars = g.in(scalars, nscalars);
      ctx->sg_points.reserve(npoints ? npoints * stride : 16);
      // (the last image of a strided array may end before its stride does: copy up to the end of its coordinates and flag)
      if (npoints) HIP_OK(hipMemcpyAsync(ctx->sg_points.p, points, (npoints - 1) * stride + 2 * cb + 1, hipMemcpyHostToDevice, on));
      ctx->sg_out.reserve(nseg * img);
      d_points = ctx->sg_points.as<uint8_t>();
      d_out = ctx->sg_out.as<uint8_t>();
      d_out_stride = img;
    }
    with_curve(ctx->curve, [&]<class C>() { seg_enqueue<C>(ctx, plan, d_points, npoints, stride, d_scalars, offsets, nseg, flags, d_out, d_out_stride, on); });
    if (!device_ptrs) {
      // the images are packed in device memory and spread to out_stride by the copy out: the caller's bytes between two images stay
      if (out_stride == img)
        HIP_OK(hipMemcpyAsync(out, d_out, nseg * img, hipMemcpyDeviceToHost, on));
      else
        HIP_OK(hipMemcpy2DAsync(out, out_stride, d_out, img, img, nseg, hipMemcpyDeviceToHost, on));
    }
    HIP_OK(hipEventRecord(ctx->sg_ev[1], on));
    HIP_OK(hipStreamSynchronize(on));   // (the plan's host arrays and pageable host memory are free to go when the call returns)
  } catch (...) {
    (void)hipStreamSynchronize(on);
    throw;
  }
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, ctx->sg_ev[0], ctx->sg_ev[1]));
  ctx->last_segments_device_us = (uint64_t)(ms * 1000.0f);
  ctx->last_segments_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

RustError mi355_msm_segments(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, const void* scalars, size_t nscalars,
                             const uint64_t* offsets, size_t nsegments, unsigned flags, void* out, size_t out_stride, void* stream) {
  return guarded_dev(
      [&] { seg_run(ctx, points, npoints, stride, scalars, nscalars, offsets, nsegments, flags, out, out_stride, (hipStream_t)stream); });
}

}  // extern "C"

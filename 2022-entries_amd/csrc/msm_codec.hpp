// msm_codec.hpp -- arkworks' compressed point records over the MI355X engine (included by msm_engine.hip): the C ABI
// mi355_msm_decompress_points / _compress_points / _set_bases_compressed / _point_to_compressed of include/mi355_msm.h over the
// kernels of point_codec.hpp.
//
// Work runs in chunks of "codec_chunk" records (default 2^22) through DevBufs the context keeps (codec_in, codec_out, codec_stat):
// host input is staged chunk by chunk, so device memory does not grow with n; device input is read and device output written in
// place, chunk by chunk, with only the status bytes staged.  Status bytes come back chunk by chunk and are counted here in index
// order, so the first invalid index is the smallest one.  A requested subgroup check is a second launch -- the existing
// k_check_points over the records just decoded (both output forms are forms it reads); a record that already failed to decode keeps
// its decode status (k_check_points calls its all-zero record off the curve, which is dropped here).
#pragma once

#include "launch_codec.hpp"
#include "sqrt.hpp"   // el_lex_largest of mi355_msm_point_to_compressed

namespace {

constexpr unsigned kCodecSerialized = 1u, kCodecValidate = 2u, kCodecExact = 4u;
constexpr size_t kCodecDefaultChunk = (size_t)1 << 22;

size_t codec_chunk(const mi355_msm_ctx* ctx, size_t n) {
  const size_t c = ctx->opt_codec_chunk > 0 ? (size_t)ctx->opt_codec_chunk : kCodecDefaultChunk;
  return n < c ? n : c;
}

void codec_check_ctx(mi355_msm_ctx* ctx, const char* what) {
  if (!ctx) bad_arg("null context");
  if (!ctx->shards.empty()) bad_arg("%s is not available on a sharded context: use a single-device context", what);
}

struct CodecEvents {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void create() {
    HIP_OK(hipEventCreate(&ev0));
    HIP_OK(hipEventCreate(&ev1));
  }
  ~CodecEvents() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

void codec_summary(uint64_t* out, const uint64_t (&cnt)[4], uint64_t flagged, uint64_t first, uint64_t method, float ms) {
  out[0] = cnt[0];
  out[1] = flagged;
  out[2] = cnt[1];
  out[3] = cnt[2];
  out[4] = cnt[3];
  out[5] = first;
  out[6] = method;
  out[7] = (uint64_t)(ms * 1000.0f);
}

// `records` -> `out`; in_dev / out_dev: the pointer is device memory of the context's device.  `status` (host, may be null).
// `first_status` (may be null): the status of the first failing record.
void decompress_impl(mi355_msm_ctx* ctx, const void* records, size_t n, void* out, size_t stride, unsigned flags, uint8_t* status, uint64_t* out8,
                     bool in_dev, bool out_dev, uint8_t* first_status = nullptr) {
  codec_check_ctx(ctx, "decompress_points");
  if (!out8) bad_arg("null result pointer");
  if (n && (!records || !out)) bad_arg("null records or output pointer");
  if (flags & ~7u) bad_arg("unknown decompress_points flags 0x%x", flags);
  const bool serialized = (flags & kCodecSerialized) != 0, validate = (flags & kCodecValidate) != 0, exact = (flags & kCodecExact) != 0;
  const size_t cb = coord_bytes(ctx->curve);
  if (serialized)
    stride = 2 * cb;
  else if (stride < 2 * cb + 1 || (stride & 3))
    bad_arg("affine stride %zu is not a 4-byte multiple >= %zu", stride, 2 * cb + 1);
  if (n >= (1ull << 31)) bad_arg("npoints %zu exceeds 2^31-1", n);
  if ((in_dev && ((uintptr_t)records & 3)) || (out_dev && ((uintptr_t)out & 3))) bad_arg("device pointers must be 4-byte aligned");
  uint64_t cnt[4] = {0, 0, 0, 0}, flagged = 0, first = n;
  uint8_t first_st = 0;
  float ms = 0;
  if (n) {
    ensure_device(ctx);
    hipStream_t st = ctx->own_stream;
    const size_t piece = codec_chunk(ctx, n);
    CodecEvents ev;
    std::vector<uint8_t> hstat(piece), hstat2(validate ? piece : 0);
    try {
      ev.create();
      ctx->codec_stat[0].reserve(piece);
      if (validate) ctx->codec_stat[1].reserve(piece);
      if (!in_dev) ctx->codec_in.reserve(piece * cb);
      if (!out_dev) ctx->codec_out.reserve(piece * stride);
      for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        const uint8_t* src = (const uint8_t*)records + at * cb;
        if (!in_dev) {
          HIP_OK(hipMemcpyAsync(ctx->codec_in.p, src, m * cb, hipMemcpyHostToDevice, st));
          src = ctx->codec_in.as<uint8_t>();
        }
        uint8_t* dst = out_dev ? (uint8_t*)out + at * stride : ctx->codec_out.as<uint8_t>();
        HIP_OK(hipEventRecord(ev.ev0, st));   // device microseconds = the codec kernels alone: no copies, no subgroup check
        with_curve(ctx->curve, [&]<class C>() {
          HIP_OK(LaunchCodec<typename C::E>::decompress(src, (uint32_t)m, dst, stride, serialized, ctx->codec_stat[0].as<uint8_t>(), st));
        });
        HIP_OK(hipEventRecord(ev.ev1, st));
        if (validate)
          with_curve(ctx->curve, [&]<class C>() {
            HIP_OK(Launch<typename C::E>::check_points(dst, stride, (uint32_t)m, serialized, exact, ctx->codec_stat[1].as<uint8_t>(), st));
          });
        HIP_OK(hipMemcpyAsync(hstat.data(), ctx->codec_stat[0].p, m, hipMemcpyDeviceToHost, st));
        if (validate) HIP_OK(hipMemcpyAsync(hstat2.data(), ctx->codec_stat[1].p, m, hipMemcpyDeviceToHost, st));
        if (!out_dev) HIP_OK(hipMemcpyAsync((uint8_t*)out + at * stride, dst, m * stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        float t = 0;
        HIP_OK(hipEventElapsedTime(&t, ev.ev0, ev.ev1));
        ms += t;
        for (size_t i = 0; i < m; i++) {
          uint8_t s = hstat[i] & 3;
          if (validate && s == 0 && (hstat2[i] & 3) == CHECK_OFF_SUBGROUP) s = CHECK_OFF_SUBGROUP;
          cnt[s]++;
          if (s == 0 && (hstat[i] & 0x80)) flagged++;
          if (s && first == n) {
            first = at + i;
            first_st = s;
          }
          if (status) status[at + i] = s;
        }
      }
    } catch (...) {
      (void)hipStreamSynchronize(st);
      throw;
    }
  }
  codec_summary(out8, cnt, flagged, first, validate ? (exact ? 0 : 1) : 0, ms);
  if (first_status) *first_status = first_st;
}

void compress_impl(mi355_msm_ctx* ctx, const void* points, size_t n, size_t stride, unsigned flags, void* out_records, uint8_t* status, uint64_t* out8,
                   bool in_dev, bool out_dev) {
  codec_check_ctx(ctx, "compress_points");
  if (!out8) bad_arg("null result pointer");
  if (n && (!points || !out_records)) bad_arg("null points or output pointer");
  if (flags & ~1u) bad_arg("unknown compress_points flags 0x%x", flags);
  const bool serialized = (flags & kCodecSerialized) != 0;
  const size_t cb = coord_bytes(ctx->curve);
  if (serialized)
    stride = 2 * cb;
  else if (stride < 2 * cb + 1 || (stride & 3))
    bad_arg("affine stride %zu is not a 4-byte multiple >= %zu", stride, 2 * cb + 1);
  if (n >= (1ull << 31)) bad_arg("npoints %zu exceeds 2^31-1", n);
  if ((in_dev && ((uintptr_t)points & 3)) || (out_dev && ((uintptr_t)out_records & 3))) bad_arg("device pointers must be 4-byte aligned");
  uint64_t cnt[4] = {0, 0, 0, 0}, flagged = 0, first = n;
  float ms = 0;
  if (n) {
    ensure_device(ctx);
    hipStream_t st = ctx->own_stream;
    const size_t piece = codec_chunk(ctx, n);
    CodecEvents ev;
    std::vector<uint8_t> hstat(piece);
    try {
      ev.create();
      ctx->codec_stat[0].reserve(piece);
      if (!in_dev) ctx->codec_out.reserve(piece * stride);   // (the image-sized buffer, whichever direction fills it)
      if (!out_dev) ctx->codec_in.reserve(piece * cb);
      for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        const uint8_t* src = (const uint8_t*)points + at * stride;
        if (!in_dev) {
          // (the last image of a strided array may end before its stride does: copy up to the end of its coordinates and flag)
          const size_t bytes = (m - 1) * stride + (serialized ? 2 * cb : 2 * cb + 1);
          HIP_OK(hipMemcpyAsync(ctx->codec_out.p, src, bytes, hipMemcpyHostToDevice, st));
          src = ctx->codec_out.as<uint8_t>();
        }
        uint8_t* dst = out_dev ? (uint8_t*)out_records + at * cb : ctx->codec_in.as<uint8_t>();
        HIP_OK(hipEventRecord(ev.ev0, st));
        with_curve(ctx->curve, [&]<class C>() {
          HIP_OK(LaunchCodec<typename C::E>::compress(src, stride, (uint32_t)m, serialized, dst, ctx->codec_stat[0].as<uint8_t>(), st));
        });
        HIP_OK(hipEventRecord(ev.ev1, st));
        HIP_OK(hipMemcpyAsync(hstat.data(), ctx->codec_stat[0].p, m, hipMemcpyDeviceToHost, st));
        if (!out_dev) HIP_OK(hipMemcpyAsync((uint8_t*)out_records + at * cb, dst, m * cb, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        float t = 0;
        HIP_OK(hipEventElapsedTime(&t, ev.ev0, ev.ev1));
        ms += t;
        for (size_t i = 0; i < m; i++) {
          const uint8_t s = hstat[i] & 3;
          cnt[s]++;
          if (s == 0 && (hstat[i] & 0x80)) flagged++;
          if (s && first == n) first = at + i;
          if (status) status[at + i] = s;
        }
      }
    } catch (...) {
      (void)hipStreamSynchronize(st);
      throw;
    }
  }
  codec_summary(out8, cnt, flagged, first, 0, ms);
}

// the producer of a device buffer (e.g. torch) may have written it on another stream: make it visible first
void codec_sync_producer(mi355_msm_ctx* ctx, size_t n) {
  if (ctx && ctx->shards.empty() && n) {
    ensure_device(ctx);
    HIP_OK(hipDeviceSynchronize());
  }
}

}  // namespace

extern "C" {

RustError mi355_msm_decompress_points(mi355_msm_ctx* ctx, const void* records, size_t npoints, void* out, size_t stride, unsigned flags, uint8_t* status,
                                      uint64_t* out8) {
  return guarded_dev([&] { decompress_impl(ctx, records, npoints, out, stride, flags, status, out8, false, false); });
}

RustError mi355_msm_decompress_points_device(mi355_msm_ctx* ctx, const void* d_records, size_t npoints, void* d_out, size_t stride, unsigned flags,
                                             uint8_t* status, uint64_t* out8) {
  return guarded_dev([&] {
    codec_sync_producer(ctx, npoints);
    decompress_impl(ctx, d_records, npoints, d_out, stride, flags, status, out8, true, true);
  });
}

RustError mi355_msm_compress_points(mi355_msm_ctx* ctx, const void* points, size_t npoints, size_t stride, unsigned flags, void* out_records,
                                    uint8_t* status, uint64_t* out8) {
  return guarded_dev([&] { compress_impl(ctx, points, npoints, stride, flags, out_records, status, out8, false, false); });
}

RustError mi355_msm_compress_points_device(mi355_msm_ctx* ctx, const void* d_points, size_t npoints, size_t stride, unsigned flags, void* d_out_records,
                                           uint8_t* status, uint64_t* out8) {
  return guarded_dev([&] {
    codec_sync_producer(ctx, npoints);
    compress_impl(ctx, d_points, npoints, stride, flags, d_out_records, status, out8, true, true);
  });
}

RustError mi355_msm_set_bases_compressed(mi355_msm_ctx* ctx, const void* records, size_t npoints) {
  return guarded_dev([&] {
    codec_check_ctx(ctx, "set_bases_compressed");
    if (npoints && !records) bad_arg("null records pointer");
    const size_t stride = 2 * coord_bytes(ctx->curve) + 8;
    ScratchBuf raw(ctx->own_stream);
    if (npoints) {
      ensure_device(ctx);
      raw.reserve(npoints * stride);
    }
    uint64_t o[8];
    uint8_t st1 = 0;
    // decode through the staged-input branch straight into `raw`: chunk by chunk, the images never visit the host
    decompress_impl(ctx, records, npoints, raw.p, stride, 0, nullptr, o, false, true, &st1);
    if (o[5] != npoints) {
      static const char* const kWhy[4] = {"valid", "malformed: x is not below p or both flag bits are set", "no point has this x", ""};
      bad_arg("set_bases_compressed: record %llu does not decode (status %u: %s); %llu of %zu records fail; the previous bases are kept",
              (unsigned long long)o[5], (unsigned)st1, kWhy[st1 & 3], (unsigned long long)(o[2] + o[3]), npoints);
    }
    validate_new_bases(ctx, raw.p, npoints, stride, false, true);
    ctx->bases_validated = false;
    set_bases_device(ctx, raw.p, npoints, stride);
    ctx->bases_validated = ctx->opt_validate_bases != 0;
  });
}

RustError mi355_msm_point_to_compressed(int curve, const void* projective, void* out_record) {
  return guarded([&] {
    if (!projective || !out_record) bad_arg("null pointer");
    with_curve(curve, [&]<class C>() {
      using E = typename C::E;
      typename E::Md md;
      constexpr int CB = 4 * E::WORDS;
      XyzzT<typename E::T> p;
      xyzz_from_projective_abi<E>(p, (const uint8_t*)projective, md);
      uint8_t* out = (uint8_t*)out_record;
      memset(out, 0, CB);
      if (xyzz_is_inf<E>(p)) {
        out[CB - 1] |= 0x40;   // x = 0 with SWFlags::Infinity (ARK ec/src/models/short_weierstrass.rs:1120-1126)
        return;
      }
      typename E::T t, ti, zzi, zzzi, x, y;
      E::mul(t, p.zz, p.zzz, md);
      el_inv(ti, t, md, (E*)nullptr);
      E::mul(zzi, ti, p.zzz, md);
      E::mul(zzzi, ti, p.zz, md);
      E::mul(x, p.x, zzi, md);
      E::mul(y, p.y, zzzi, md);
      uint32_t w[E::WORDS];
      E::to_plain(w, x, md);
      if (el_lex_largest<E>(y, md)) w[E::WORDS - 1] |= 0x80000000u;
      memcpy(out, w, CB);
    });
  });
}

}  // extern "C"

// msm_fixed.hpp -- batch fixed-base scalar multiplication over the MI355X engine (included by msm_engine.hip): the C ABI
// mi355_msm_fixed_* of include/mi355_msm.h over the kernels of fixed_base.hpp.
//
// Reference: ARK ec/src/msm/fixed_base.rs:8-97.  A handle is arkworks' window table made resident: one base g, one window size w,
// ceil(256 / w) levels of 2^w normalised points in device memory.  A call walks it once per scalar and writes normalised images.
// Work memory does not grow with the number of scalars: a call runs in chunks of at most `max_chunk` scalars (default 2^22: 224 + 56 B
// each for G1, twice that for G2) through buffers the handle keeps; the table and those buffers are its only device allocations, all
// DevBufs (so MI355_MSM_GUARD_TAIL=1 places each of them against an unmapped page).
#pragma once

#include "fixed_base.hpp"   // window constants, fb_levels
#include "launch_fixed.hpp"

struct mi355_msm_fixed {
  int curve = 0;
  int device = -1;
  uint32_t w = 0, levels = 0;
  size_t max_chunk = (size_t)1 << 22;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};   // around the kernels (and copies) of a call, on the stream it runs on
  DevBuf table, table_inf;               // levels << w AffineDev records, and the infinity flags k_pre_normalize writes with them
  DevBuf xyzz, prefix;                   // one chunk of results before normalisation, and its scratch
  DevBuf d_scalars, d_out;               // host-pointer calls: one chunk of staged input / packed output images
  uint64_t build_us = 0, last_mul_us = 0, last_device_us = 0;
};

namespace {

constexpr unsigned kFixedMont = 1u, kFixedProjective = 2u;

// FixedBase::get_mul_window_size (fixed_base.rs:11-17): 3 below 32 scalars, else ln_without_floats(n) = ceil(log2 n) * 69 / 100
size_t fixed_ark_window_size(size_t n) {
  if (n < 32) return 3;
  size_t lg = 0;
  while (((size_t)1 << lg) < n && lg < 8 * sizeof(size_t) - 1) lg++;
  return lg * 69 / 100;
}

// The window size of a handle.  Additions: 2 * levels(w) * 2^w to build the table (every entry is added once and normalised once) plus
// n * levels(w) to use it; the table must stay inside the Infinity Cache, which ends the search at 16 bits for G1 (16 levels, 134 MB)
// and at 15 for G2 (18 levels, 151 MB).  n = 0 (unknown) plans for a large batch.
uint32_t fixed_auto_window(int curve, size_t expected) {
  const uint32_t cap = is_g2(curve) ? 15 : 16;
  if (expected == 0) return cap;
  uint32_t best = 1;
  double best_cost = 1e300;
  for (uint32_t w = 1; w <= cap; w++) {
    const double levels = (double)fb_levels(w);
    const double cost = levels * (2.0 * (double)(1u << w) + (double)expected);
    if (cost < best_cost) { best_cost = cost; best = w; }
  }
  return best;
}

size_t fixed_image_bytes(int curve, unsigned flags) {
  return (flags & kFixedProjective) ? 3 * coord_bytes(curve) : 2 * coord_bytes(curve) + 8;
}

void fixed_release(mi355_msm_fixed* fb) {
  for (DevBuf* b : {&fb->table, &fb->table_inf, &fb->xyzz, &fb->prefix, &fb->d_scalars, &fb->d_out}) b->release();
  for (hipEvent_t& e : fb->ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  if (fb->own_stream) { (void)hipStreamDestroy(fb->own_stream); fb->own_stream = nullptr; }
}

void fixed_device_time(mi355_msm_fixed* fb) {
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, fb->ev[0], fb->ev[1]));
  fb->last_device_us = (uint64_t)(ms * 1000.0f);
}

template <class C>
void fixed_build_table(mi355_msm_fixed* fb, const uint8_t* base_affine) {
  using E = typename C::E;
  using El = typename E::T;
  using AD = AffineDevT<El>;
  using XD = XyzzDevT<El>;
  const hipStream_t st = fb->own_stream;
  const uint32_t w = fb->w, levels = fb->levels;
  const size_t entries = (size_t)levels << w, img_bytes = 2 * coord_bytes(fb->curve) + 8;
  ScratchBuf img(st), lb_x(st), lb_prefix(st), lb_a(st), lb_inf(st), t_x(st), t_prefix(st);
  img.reserve(img_bytes);
  lb_x.reserve(levels * sizeof(XD));
  lb_prefix.reserve(levels * sizeof(El));
  lb_a.reserve(levels * sizeof(AD));
  lb_inf.reserve(levels);
  t_x.reserve(entries * sizeof(XD));
  t_prefix.reserve(entries * sizeof(El));
  fb->table.reserve(entries * sizeof(AD));
  fb->table_inf.reserve(entries);
  uint8_t packed[208] = {0};
  memcpy(packed, base_affine, 2 * coord_bytes(fb->curve) + 1);   // (the caller's image may end at its flag byte)
  HIP_OK(hipMemcpyAsync(img.p, packed, img_bytes, hipMemcpyHostToDevice, st));
  HIP_OK(LaunchFixed<E>::level_bases(img.as<uint8_t>(), w, levels, lb_x.as<XD>(), st));
  HIP_OK(Launch<E>::pre_normalize(lb_x.as<XD>(), levels, 1, lb_prefix.as<El>(), lb_a.as<AD>(), lb_inf.as<uint8_t>(), st));
  HIP_OK(LaunchFixed<E>::table(lb_a.as<AD>(), lb_inf.as<uint8_t>(), w, levels, t_x.as<XD>(), st));
  HIP_OK(Launch<E>::pre_normalize(t_x.as<XD>(), (uint32_t)entries, FB_NORM_RUN, t_prefix.as<El>(), fb->table.as<AD>(), fb->table_inf.as<uint8_t>(), st));
  HIP_OK(hipStreamSynchronize(st));
}

// one chunk, everything in device memory, enqueued on st
template <class C>
void fixed_chunk(mi355_msm_fixed* fb, uint8_t* d_out, size_t out_stride, const uint32_t* d_scalars, size_t cn, unsigned flags, hipStream_t st) {
  using E = typename C::E;
  using El = typename E::T;
  using AD = AffineDevT<El>;
  using XD = XyzzDevT<El>;
  fb->xyzz.reserve(cn * sizeof(XD));
  fb->prefix.reserve(cn * sizeof(El));
  HIP_OK(LaunchFixed<E>::mul(fb->table.as<AD>(), d_scalars, (uint32_t)cn, fb->w, fb->levels, (flags & kFixedMont) != 0, fb->xyzz.as<XD>(), st));
  HIP_OK(LaunchFixed<E>::normalize(fb->xyzz.as<XD>(), (uint32_t)cn, fb->prefix.as<El>(), d_out, out_stride, (flags & kFixedProjective) != 0, st));
}

void fixed_check_call(mi355_msm_fixed* fb, const void* out, size_t out_stride, const void* scalars, size_t n, unsigned flags) {
  if (!fb) bad_arg("null fixed-base handle");
  if (flags & ~(kFixedMont | kFixedProjective)) bad_arg("unknown flag bits 0x%x (bit 0: Fr Montgomery scalars, bit 1: Projective images)", flags);
  const size_t img = fixed_image_bytes(fb->curve, flags);
  if (out_stride % 4) bad_arg("out_stride %zu is not a multiple of 4", out_stride);
  if (out_stride < img) bad_arg("out_stride %zu is smaller than the %zu-byte image", out_stride, img);
  if (n && (!out || !scalars)) bad_arg("null output or scalars pointer");
}

void fixed_mul_device(mi355_msm_fixed* fb, void* d_out, size_t out_stride, const void* d_scalars, size_t n, unsigned flags, hipStream_t st) {
  fixed_check_call(fb, d_out, out_stride, d_scalars, n, flags);
  if (n == 0) return;
  if (((uintptr_t)d_out | (uintptr_t)d_scalars) & 3) bad_arg("device pointers must be 4-byte aligned");
  HIP_OK(hipSetDevice(fb->device));
  const auto t0 = std::chrono::steady_clock::now();
  HIP_OK(hipEventRecord(fb->ev[0], st));
  for (size_t off = 0; off < n; off += fb->max_chunk) {
    const size_t cn = std::min(fb->max_chunk, n - off);
    with_curve(fb->curve, [&]<class C>() {
      fixed_chunk<C>(fb, (uint8_t*)d_out + off * out_stride, out_stride, (const uint32_t*)d_scalars + 8 * off, cn, flags, st);
    });
  }
  HIP_OK(hipEventRecord(fb->ev[1], st));
  HIP_OK(hipStreamSynchronize(st));
  fixed_device_time(fb);
  fb->last_mul_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

// Host pointers: every chunk is staged in, computed and copied out on the handle's stream, whose order keeps a chunk's buffers from
// being refilled before they were read.  The images are packed in device memory and spread to `out_stride` by the copy out, so the
// caller's bytes between two images stay as they were.
void fixed_mul_host(mi355_msm_fixed* fb, void* out, size_t out_stride, const void* scalars, size_t n, unsigned flags) {
  fixed_check_call(fb, out, out_stride, scalars, n, flags);
  if (n == 0) return;
  HIP_OK(hipSetDevice(fb->device));
  const hipStream_t st = fb->own_stream;
  const size_t img = fixed_image_bytes(fb->curve, flags);
  const auto t0 = std::chrono::steady_clock::now();
  HIP_OK(hipEventRecord(fb->ev[0], st));
  for (size_t off = 0; off < n; off += fb->max_chunk) {
    const size_t cn = std::min(fb->max_chunk, n - off);
    fb->d_scalars.reserve(cn * 32);
    fb->d_out.reserve(cn * img);
    HIP_OK(hipMemcpyAsync(fb->d_scalars.p, (const uint8_t*)scalars + 32 * off, cn * 32, hipMemcpyHostToDevice, st));
    with_curve(fb->curve, [&]<class C>() { fixed_chunk<C>(fb, fb->d_out.as<uint8_t>(), img, fb->d_scalars.as<uint32_t>(), cn, flags, st); });
    uint8_t* dst = (uint8_t*)out + off * out_stride;
    if (out_stride == img)
      HIP_OK(hipMemcpyAsync(dst, fb->d_out.p, cn * img, hipMemcpyDeviceToHost, st));
    else
      HIP_OK(hipMemcpy2DAsync(dst, out_stride, fb->d_out.p, img, img, cn, hipMemcpyDeviceToHost, st));
    if (off + cn >= n) HIP_OK(hipEventRecord(fb->ev[1], st));
    HIP_OK(hipStreamSynchronize(st));   // (pageable host memory: the caller's buffers are free to go when the call returns)
  }
  fixed_device_time(fb);
  fb->last_mul_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

size_t mi355_msm_fixed_window_size(size_t num_scalars) { return fixed_ark_window_size(num_scalars); }

RustError mi355_msm_fixed_create(mi355_msm_fixed** out, int curve, int device, const void* base_affine, int window_bits, size_t expected_scalars) {
  return guarded_dev([&] {
    if (!out) bad_arg("null handle out-pointer");
    *out = nullptr;
    if (!known_curve(curve)) bad_arg("unknown curve id %d", curve);
    if (!base_affine) bad_arg("null base pointer");
    if (window_bits < 0 || window_bits > (int)FB_MAX_WINDOW) bad_arg("window_bits %d out of range [1, %u] (0 = automatic)", window_bits, FB_MAX_WINDOW);
    const int count = require_device();
    if (device >= count) bad_arg("device %d out of range (%d visible)", device, count);
    if (device < 0) HIP_OK(hipGetDevice(&device));
    HIP_OK(hipSetDevice(device));
    mi355_msm_fixed* fb = new mi355_msm_fixed();
    fb->curve = curve;
    fb->device = device;
    fb->w = window_bits ? (uint32_t)window_bits : fixed_auto_window(curve, expected_scalars);
    fb->levels = fb_levels(fb->w);
    try {
      HIP_OK(hipStreamCreateWithFlags(&fb->own_stream, hipStreamNonBlocking));
      for (hipEvent_t& e : fb->ev) HIP_OK(hipEventCreate(&e));
      const auto t0 = std::chrono::steady_clock::now();
      with_curve(curve, [&]<class C>() { fixed_build_table<C>(fb, (const uint8_t*)base_affine); });
      fb->build_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
      fixed_release(fb);
      delete fb;
      throw;
    }
    *out = fb;
  });
}

RustError mi355_msm_fixed_mul(mi355_msm_fixed* fb, void* out, size_t out_stride, const void* scalars, size_t n, unsigned flags) {
  return guarded_dev([&] { fixed_mul_host(fb, out, out_stride, scalars, n, flags); });
}

RustError mi355_msm_fixed_mul_device(mi355_msm_fixed* fb, void* d_out, size_t out_stride, const void* d_scalars, size_t n, unsigned flags, void* stream) {
  return guarded_dev([&] { fixed_mul_device(fb, d_out, out_stride, d_scalars, n, flags, (hipStream_t)stream); });
}

RustError mi355_msm_fixed_set_option(mi355_msm_fixed* fb, const char* key, long value) {
  return guarded([&] {
    if (!fb || !key) bad_arg("null argument");
    const std::string k(key);
    if (k == "max_chunk") {   // scalars per chunk; 0 restores the default.  Results do not depend on it (a test hook, as for contexts)
      if (value < 0 || value > (1L << 27)) bad_arg("max_chunk %ld out of range [1, 2^27]", value);
      fb->max_chunk = value ? (size_t)value : (size_t)1 << 22;
    } else
      bad_arg("unknown fixed-base option '%s'", key);
  });
}

RustError mi355_msm_fixed_query(mi355_msm_fixed* fb, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!fb || !key || !value) bad_arg("null argument");
    const std::string k(key);
    if (k == "window_bits") *value = fb->w;
    else if (k == "levels") *value = fb->levels;
    else if (k == "table_bytes") *value = fb->table.bytes + fb->table_inf.bytes;
    else if (k == "signed_digits") *value = 0;
    else if (k == "build_us") *value = fb->build_us;
    else if (k == "device") *value = (uint64_t)fb->device;
    else if (k == "last_mul_us") *value = fb->last_mul_us;
    else if (k == "last_device_us") *value = fb->last_device_us;
    else if (k == "max_chunk") *value = fb->max_chunk;
    else if (k == "work_bytes") *value = fb->xyzz.bytes + fb->prefix.bytes + fb->d_scalars.bytes + fb->d_out.bytes;
    else bad_arg("unknown fixed-base query '%s'", key);
  });
}

RustError mi355_msm_fixed_destroy(mi355_msm_fixed* fb) {
  return guarded_dev([&] {
    if (!fb) return;
    (void)hipSetDevice(fb->device);
    fixed_release(fb);
    delete fb;
  });
}

}  // extern "C"

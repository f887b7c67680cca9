// msm_h2c.hpp -- batch hash-to-curve (included by msm_engine.hip after msm_pairing.hpp): the C ABI
// mi355_msm_h2c_{create, field, map, hash, query, destroy} of include/mi355_msm.h over the kernels of h2c.hpp.
//
// A hash-to-curve handle belongs to a device, one group of BLS12-381 and one domain separation tag.  It owns DST_prime in device
// memory and the state after the zero block, a stream for its host-pointer calls, the staged bytes of such a call, and the work
// buffers (field images, mapped points, the clearing kernel's slots, results, the normalisation's prefix), which are sized by the
// lanes in flight of one chunk (H2C_MAX_LANES) and grown on demand -- never by n.  The one exception is `stage`: a host-pointer call
// stages its whole input, the offsets and the packed output there, n images at most (device-pointer calls do not use it).
// Every call judges its arguments first, in the order of the header, and the handle last.
#pragma once

#include "launch_fixed.hpp"   // the output normalisation
#include "launch_h2c.hpp"

struct mi355_msm_h2c {
  int curve = 0, device = 0;
  hipStream_t own_stream = nullptr;
  DevBuf table, u, pts, res, ws, prefix, stage;
  H2cDst dst{};
  uint32_t dst_len = 0, oversize = 0;
  uint64_t last_launches = 0, last_lanes = 0;
};

namespace {

constexpr unsigned kH2cEncode = 1u, kH2cDevice = 2u, kH2cPairs = 4u, kH2cProjective = 8u;

void h2c_release(mi355_msm_h2c* h) {
  (void)hipSetDevice(h->device);
  for (DevBuf* b : {&h->table, &h->u, &h->pts, &h->res, &h->ws, &h->prefix, &h->stage}) b->release();
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  h->own_stream = nullptr;
}

void h2c_create(mi355_msm_h2c** out, int curve, const void* dst, size_t dst_len, int device) {
  if (!out) bad_arg("null handle out-pointer");
  *out = nullptr;
  if (!known_curve(curve)) bad_arg("unknown curve id %d", curve);
  if (!dst || dst_len == 0) bad_arg("a domain separation tag of at least one byte is required (RFC 9380 section 3.1)");
  if (dst_len >= ((size_t)1 << 28)) bad_arg("a domain separation tag of %zu bytes", dst_len);
  if (!is_381(curve)) bad_arg("no standard hash-to-curve suite exists for BLS12-377 (RFC 9380 defines none): bls12_381_g1 or bls12_381_g2");
  const int count = require_device();
  if (device >= count) bad_arg("device %d out of range (%d visible)", device, count);
  if (device < 0) HIP_OK(hipGetDevice(&device));
  HIP_OK(hipSetDevice(device));
  std::unique_ptr<mi355_msm_h2c> h(new mi355_msm_h2c());
  h->curve = curve;
  h->device = device;
  uint8_t prime[256];
  h2c_make_dst(prime, h->dst.prime_len, h->dst.z_pad, (const uint8_t*)dst, dst_len);
  h->dst_len = h->dst.prime_len - 1;
  h->oversize = dst_len > H2C_MAX_DST;
  try {
    HIP_OK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->table.reserve(256);
    HIP_OK(hipMemcpyAsync(h->table.p, prime, h->dst.prime_len, hipMemcpyHostToDevice, h->own_stream));
    HIP_OK(hipStreamSynchronize(h->own_stream));
  } catch (...) {
    h2c_release(h.get());
    throw;
  }
  h->dst.prime = h->table.as<uint8_t>();
  *out = h.release();
}

size_t h2c_image_bytes(int curve, unsigned flags) { return (flags & kH2cProjective) ? 3 * coord_bytes(curve) : 2 * coord_bytes(curve) + 8; }

// one chunk, everything in device memory, enqueued on st.  msgs > 0: expand first (elems images per message into h->u); then, with
// points, map `nu` images (from h->u or d_u), clear (pairs or singles) when asked, and write `nout` images.
template <class E>
void h2c_chunk(mi355_msm_h2c* h, const H2cRun* run, uint32_t msgs, uint32_t elems, uint32_t* d_field_out, const uint32_t* d_u, uint32_t nu, bool clear,
               bool pairs, unsigned flags, uint8_t* d_out, size_t out_stride, hipStream_t st) {
  using El = typename E::T;
  using XD = XyzzDevT<El>;
  if (msgs) {
    uint32_t* dst = d_field_out;
    if (!dst) {
      h->u.reserve((size_t)msgs * elems * 48);
      dst = h->u.as<uint32_t>();
      d_u = dst;
    }
    HIP_OK(LaunchH2c<E>::expand(*run, msgs, elems, dst, st));
    h->last_launches++;
    if (d_field_out) return;
  }
  const uint32_t nout = pairs ? nu / 2 : nu;
  h->pts.reserve((size_t)nu * sizeof(XD));
  h->prefix.reserve((size_t)nout * sizeof(El));
  h->ws.reserve(std::max((size_t)nu * h2c_map_ws_bytes<E>(), clear ? (size_t)nout * h2c_clear_ws_bytes<E>() : (size_t)0) + 16);
  HIP_OK(LaunchH2c<E>::map(d_u, nu, h->ws.as<uint8_t>(), h->pts.as<XD>(), st));
  h->last_launches++;
  const XD* fin = h->pts.as<XD>();
  if (clear) {
    h->res.reserve((size_t)nout * sizeof(XD));
    HIP_OK(LaunchH2c<E>::clear(h->pts.as<XD>(), nout, pairs, h->ws.as<uint8_t>(), h->res.as<XD>(), st));
    h->last_launches++;
    fin = h->res.as<XD>();
  }
  HIP_OK(LaunchFixed<E>::normalize(fin, nout, h->prefix.as<El>(), d_out, out_stride, (flags & kH2cProjective) != 0, st));
  h->last_launches++;
}

template <class Fn>
void with_h2c_group(int curve, Fn&& fn) {
  if (is_g2(curve)) fn.template operator()<Bls12_381_G2::E>();
  else fn.template operator()<Bls12_381_G1::E>();
}

enum H2cCall { kH2cField, kH2cMap, kH2cHash };

// field: out = n * count * m images; map: in = n images, out = n or n / 2 points; hash: out = n points
void h2c_call(H2cCall what, mi355_msm_h2c* h, void* out, size_t out_stride, const void* in, size_t in_bytes, const uint64_t* offsets, size_t n, unsigned count,
              unsigned flags, hipStream_t st) {
  const unsigned known = what == kH2cField ? kH2cDevice : what == kH2cMap ? (kH2cDevice | kH2cPairs | kH2cProjective) : (kH2cEncode | kH2cDevice | kH2cProjective);
  if (flags & ~known)
    bad_arg("unknown flag bits 0x%x (%sbit 1: device pointers%s)", flags & ~known, what == kH2cHash ? "bit 0: encode_to_curve, " : "",
            what == kH2cField ? "" : what == kH2cMap ? ", bit 2: pairs, bit 3: Projective images" : ", bit 3: Projective images");
  if (what == kH2cField && (count < 1 || count > 2)) bad_arg("count %u: hash_to_field writes 1 or 2 elements per message", count);
  if (what == kH2cMap && (flags & kH2cPairs) && (n & 1)) bad_arg("%zu field images are not whole pairs", n);
  if (n >= ((size_t)1 << 31)) bad_arg("n %zu exceeds 2^31-1", n);
  // the curve is the handle's; the smallest image of either group bounds the stride before the handle is looked at
  if (what != kH2cField) {
    const size_t least = (flags & kH2cProjective) ? 144 : 104;
    if (out_stride % 4 || out_stride < least) bad_arg("out_stride %zu is not a 4-byte multiple >= %zu", out_stride, least);
  }
  if (n && (!out || (what == kH2cMap && !in))) bad_arg("null output or input pointer");
  if (what != kH2cMap && n && !offsets) bad_arg("null offsets pointer");
  if (what != kH2cMap && in_bytes && !in) bad_arg("null message buffer of %zu bytes", in_bytes);
  const bool device_ptrs = (flags & kH2cDevice) != 0;
  if (device_ptrs && (((uintptr_t)out & 3) || (what == kH2cMap && ((uintptr_t)in & 3)) || ((uintptr_t)offsets & 7))) bad_arg("device pointers must be 4-byte aligned, offsets 8-byte aligned");
  poly_check_stream(device_ptrs, st);
  if (what != kH2cMap && !device_ptrs) {
    if (const char* m = h2c_check_offsets(offsets, n, in_bytes)) bad_arg("%s", m);
  }
  if (!h) bad_arg("null hash-to-curve handle");
  const size_t cb = coord_bytes(h->curve), m = cb / 48;
  const unsigned nflags = flags & kH2cProjective;
  const size_t img = what == kH2cField ? 0 : h2c_image_bytes(h->curve, flags);
  if (what != kH2cField && out_stride < img) bad_arg("out_stride %zu is smaller than the %zu-byte image", out_stride, img);
  const bool pairs = what == kH2cMap ? (flags & kH2cPairs) != 0 : !(flags & kH2cEncode);
  const size_t nout = what == kH2cField ? n * count * m : (what == kH2cMap && pairs) ? n / 2 : n;
  const size_t out_bytes = what == kH2cField ? nout * 48 : (nout ? (nout - 1) * out_stride + img : 0);
  const size_t in_total = what == kH2cMap ? n * cb : in_bytes;
  if (pr_overlap(out, out_bytes, in, in_total) || (what != kH2cMap && pr_overlap(out, out_bytes, offsets, (n + 1) * 8))) bad_arg("the output overlaps an input");
  h->last_launches = 0;
  h->last_lanes = 0;
  if (n == 0) return;
  HIP_OK(hipSetDevice(h->device));
  const hipStream_t on = device_ptrs ? st : h->own_stream;
  try {
    const uint8_t* d_in = (const uint8_t*)in;
    const uint64_t* d_off = offsets;
    uint8_t* d_out = (uint8_t*)out;
    size_t d_stride = what == kH2cField ? 0 : out_stride;
    if (!device_ptrs) {
      const size_t ib = (in_total + 7) & ~(size_t)7, ob = what == kH2cMap ? 0 : (n + 1) * 8;
      const size_t packed = what == kH2cField ? nout * 48 : nout * img;
      h->stage.reserve(ib + ob + packed + 8);
      uint8_t* s = h->stage.as<uint8_t>();
      if (in_total) HIP_OK(hipMemcpyAsync(s, in, in_total, hipMemcpyHostToDevice, on));
      if (ob) HIP_OK(hipMemcpyAsync(s + ib, offsets, ob, hipMemcpyHostToDevice, on));
      d_in = s;
      d_off = (const uint64_t*)(s + ib);
      d_out = s + ib + ob;
      d_stride = img;
    }
    const size_t elems = (what == kH2cField ? count : pairs ? 2 : 1) * m;   // images per message
    const size_t per = what == kH2cMap ? (pairs ? 2 : 1) : 1;                // inputs per lane of the widest kernel
    const size_t piece = H2C_MAX_LANES / (what == kH2cMap ? 1 : (what == kH2cHash && pairs ? 2 : 1));
    with_h2c_group(h->curve, [&]<class E>() {
      if (what == kH2cMap) {
        const size_t step = pairs ? (size_t)H2C_MAX_LANES & ~(size_t)1 : H2C_MAX_LANES;
        for (size_t at = 0; at < n; at += step) {
          const size_t cn = std::min(step, n - at);
          h2c_chunk<E>(h, nullptr, 0, 0, nullptr, (const uint32_t*)(d_in + at * cb), (uint32_t)cn, pairs, pairs, nflags,
                       d_out + (at / per) * d_stride, d_stride, on);
          h->last_lanes = std::max<uint64_t>(h->last_lanes, cn);
        }
      } else {
        for (size_t at = 0; at < n; at += piece) {
          const size_t cn = std::min(piece, n - at);
          H2cRun run{h->dst, d_in, d_off + at, in_bytes};
          if (what == kH2cField)
            h2c_chunk<E>(h, &run, (uint32_t)cn, (uint32_t)elems, (uint32_t*)(d_out + at * elems * 48), nullptr, 0, false, false, 0, nullptr, 0, on);
          else
            h2c_chunk<E>(h, &run, (uint32_t)cn, (uint32_t)elems, nullptr, nullptr, (uint32_t)(cn * (pairs ? 2 : 1)), true, pairs, nflags,
                         d_out + at * d_stride, d_stride, on);
          h->last_lanes = std::max<uint64_t>(h->last_lanes, cn * (what == kH2cHash && pairs ? 2 : 1));
        }
      }
    });
    if (!device_ptrs) {
      if (what == kH2cField || out_stride == img)
        HIP_OK(hipMemcpyAsync(out, d_out, what == kH2cField ? nout * 48 : nout * img, hipMemcpyDeviceToHost, on));
      else
        HIP_OK(hipMemcpy2DAsync(out, out_stride, d_out, img, img, nout, hipMemcpyDeviceToHost, on));
    }
    HIP_OK(hipStreamSynchronize(on));   // the work buffers are the handle's: the next call may grow them
  } catch (...) {
    (void)hipStreamSynchronize(on);
    throw;
  }
}

}  // namespace

extern "C" {

RustError mi355_msm_h2c_create(mi355_msm_h2c** out, int curve, const void* dst, size_t dst_len, int device) {
  return guarded_dev([&] { h2c_create(out, curve, dst, dst_len, device); });
}

RustError mi355_msm_h2c_field(mi355_msm_h2c* h, void* out, const void* data, size_t data_bytes, const uint64_t* offsets, size_t n, unsigned count,
                              unsigned flags, void* stream) {
  return guarded_dev([&] { h2c_call(kH2cField, h, out, 0, data, data_bytes, offsets, n, count, flags, (hipStream_t)stream); });
}

RustError mi355_msm_h2c_map(mi355_msm_h2c* h, void* out, size_t out_stride, const void* u, size_t n, unsigned flags, void* stream) {
  return guarded_dev([&] { h2c_call(kH2cMap, h, out, out_stride, u, 0, nullptr, n, 0, flags, (hipStream_t)stream); });
}

RustError mi355_msm_h2c_hash(mi355_msm_h2c* h, void* out, size_t out_stride, const void* data, size_t data_bytes, const uint64_t* offsets, size_t n,
                             unsigned flags, void* stream) {
  return guarded_dev([&] { h2c_call(kH2cHash, h, out, out_stride, data, data_bytes, offsets, n, 0, flags, (hipStream_t)stream); });
}

RustError mi355_msm_h2c_query(mi355_msm_h2c* h, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    // constants of the kernels need no handle
    if (k == "block_lanes") { *value = H2C_LANES; return; }
    if (k == "max_lanes") { *value = H2C_MAX_LANES; return; }
    if (!h) bad_arg("null hash-to-curve handle");
    if (k == "work_bytes") *value = h->table.bytes + h->u.bytes + h->pts.bytes + h->res.bytes + h->ws.bytes + h->prefix.bytes + h->stage.bytes;
    else if (k == "lanes_in_flight") *value = h->last_lanes;
    else if (k == "last_launches") *value = h->last_launches;
    else if (k == "device") *value = (uint64_t)h->device;
    else if (k == "curve") *value = (uint64_t)h->curve;
    else if (k == "dst_bytes") *value = h->dst_len;
    else if (k == "dst_oversize") *value = h->oversize;
    else bad_arg("unknown hash-to-curve query '%s'", key);
  });
}

RustError mi355_msm_h2c_destroy(mi355_msm_h2c* h) {
  return guarded_dev([&] {
    if (!h) return;
    h2c_release(h);
    delete h;
  });
}

}  // extern "C"

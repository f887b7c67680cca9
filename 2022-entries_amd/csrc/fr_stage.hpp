// fr_stage.hpp -- the vectors of one Fr-vector call, wherever the caller keeps them (included by msm_ntt.hpp, before the glue of
// msm_poly.hpp .. msm_poseidon.hpp, which all stage through it).
//
// With device pointers every vector is the caller's pointer and nothing is enqueued.  With host pointers the vectors lie one behind
// the other in `buf` -- the staging buffer of the call's family on its handle -- which is reserved ONCE, for `total` elements of 32
// bytes, before the first pointer is handed out (growing later would move the vectors already handed out); the copies go to `on`,
// the stream of the call's launches.
#pragma once

namespace {

struct FrStage {
  DevBuf& buf;
  const bool device_ptrs;
  const hipStream_t on;
  size_t used = 0;
  FrStage(DevBuf& buf_, bool device_ptrs_, hipStream_t on_, size_t total) : buf(buf_), device_ptrs(device_ptrs_), on(on_) {
    if (!device_ptrs && total) buf.reserve(total * 32);
  }
  // an input of n elements: copied in unless it is empty
  const uint32_t* in(const void* v, size_t n) {
    if (device_ptrs) return (const uint32_t*)v;
    uint32_t* p = out(nullptr, n);
    if (n) HIP_OK(hipMemcpyAsync(p, v, n * 32, hipMemcpyHostToDevice, on));
    return p;
  }
  // an output of n elements; `back` brings it to the caller
  uint32_t* out(void* v, size_t n) {
    if (device_ptrs) return (uint32_t*)v;
    uint8_t* p = (uint8_t*)buf.p + used;
    used += n * 32;
    return (uint32_t*)p;
  }
  // an output that may be the input `staged`: the caller's, or the staged input itself -- the operation then runs in place
  uint32_t* out_over(void* v, const uint32_t* staged) { return device_ptrs ? (uint32_t*)v : (uint32_t*)staged; }
  // n elements of a staged output to the caller's host memory
  void back(void* host, const uint32_t* dev, size_t n) {
    if (!device_ptrs && n) HIP_OK(hipMemcpyAsync(host, dev, n * 32, hipMemcpyDeviceToHost, on));
  }
};

}  // namespace

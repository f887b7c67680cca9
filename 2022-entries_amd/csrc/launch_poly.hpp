// launch_poly.hpp -- host-callable launchers of the kernels of poly.hpp.  Declared here, defined and instantiated for the two scalar
// fields in kernels_poly.hip; the only other unit that includes it is the engine (msm_poly.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "poly.hpp"

namespace msm {

template <class FR>
struct LaunchPoly {
  // one block per tile of p.t.n elements
  static hipError_t eval(const PolyEval& p, hipStream_t st);
  static hipError_t div(const PolyDiv& p, hipStream_t st);
  static hipError_t inv_prod(const PolyInv& p, hipStream_t st);
  static hipError_t inv_apply(const PolyInv& p, hipStream_t st);
  // tiles[t] = coeff / tiles[t], one lane per tile
  static hipError_t inv_tiles(Fr* tiles, uint64_t count, const Fr& coeff, hipStream_t st);
  static hipError_t lagrange(const PolyLagrange& p, hipStream_t st);
  static hipError_t vec_op(const PolyVecOp& p, hipStream_t st);
};

extern template struct LaunchPoly<Bls12_377_Fr29>;
extern template struct LaunchPoly<Bls12_381_Fr29>;

}  // namespace msm

// launch_sparse.hpp -- host-callable launchers of the kernels of sparse.hpp.  Declared here, defined and instantiated for the two
// scalar fields in kernels_sparse.hip; the only other unit that includes it is the engine (msm_sparse.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "sparse.hpp"

namespace msm {

template <class FR>
struct LaunchSparse {
  // create: one lane per slot
  static hipError_t vals(const SparseVals& p, hipStream_t st);
  // one lane per column
  static hipError_t z(const SparseZ& p, hipStream_t st);
  // one lane per E entries
  static hipError_t totals(const SparseRun& p, hipStream_t st);
  static hipError_t rows(const SparseRun& p, hipStream_t st);
  // one lane per row
  static hipError_t cross(const SparseRun& p, hipStream_t st);
};

extern template struct LaunchSparse<Bls12_377_Fr29>;
extern template struct LaunchSparse<Bls12_381_Fr29>;

}  // namespace msm

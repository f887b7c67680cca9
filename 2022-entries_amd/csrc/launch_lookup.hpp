// launch_lookup.hpp -- host-callable launchers of the kernels of lookup.hpp.  Declared here, defined and instantiated for the two
// scalar fields in kernels_lookup.hip; the only other unit that includes it is the engine (msm_lookup.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "lookup.hpp"

namespace msm {

template <class FR>
struct LaunchLookup {
  // one lane per table entry
  static hipError_t canon(const LookupCanon& p, hipStream_t st);
  static hipError_t build(const LookupBuild& p, hipStream_t st);
  static hipError_t mult(const LookupMult& p, hipStream_t st);
  // one lane per p.batches values (p.batches >= 1)
  static hipError_t probe(const LookupProbe& p, hipStream_t st);
  // one block per tile of 1024 u32
  static hipError_t scan_up(const LookupScan& p, hipStream_t st);
  static hipError_t scan_down(const LookupScan& p, hipStream_t st);
  // one lane per output element
  static hipError_t expand(const LookupExpand& p, hipStream_t st);
  // one lane per row
  static hipError_t logup_den(const LogupRows& p, hipStream_t st);
  static hipError_t logup_term(const LogupRows& p, hipStream_t st);
};

extern template struct LaunchLookup<Bls12_377_Fr29>;
extern template struct LaunchLookup<Bls12_381_Fr29>;

}  // namespace msm

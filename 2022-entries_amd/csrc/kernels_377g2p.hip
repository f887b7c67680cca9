// kernels_377g2p.hip -- the throughput kernels of Bls12_377_G2 with two lanes per point (fp2pair.hpp); its own translation unit so
// that it compiles beside kernels_377g2.hip.
#include "launch_impl.hpp"

namespace msm {
template struct WalkLaunch<PairedForm<SwLaw<Bls12_377_G2::E>>::L>;   // (no sum_bases and no quad form: launch_impl.hpp)
}

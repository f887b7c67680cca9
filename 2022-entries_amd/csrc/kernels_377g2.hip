// kernels_377g2.hip -- the gfx950 kernels instantiated for Bls12_377_G2 (one translation unit per curve: see launch.hpp).
#include "launch_impl.hpp"

namespace msm {
MSM_INSTANTIATE_SW_LAUNCHERS(Bls12_377_G2::E)
}

// launch_pair_impl.hpp -- nothing lives here any more: the two-lanes-per-point launchers are WalkLaunch<SwPairLaw<F, NB>> of
// launch_impl.hpp, which kernels_<curve>p.hip include directly.  The name stays because bench.py's kernel_source_sha16 reads
// every file of its list by name, this one among them.
#pragma once
#include "launch_impl.hpp"

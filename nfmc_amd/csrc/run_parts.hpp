// A run split into parts (nfmc_jump_run_f32, sampler_kernels.hip): each part is a range of chains whose launches go to a
// stream of their own, so that kernels of different parts run side by side.  The entry points' internals take a
// LaunchPart to launch one part: everything else about the launch -- checks, layout, kernel -- is what the whole run gets.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nfmc_hip.h"

namespace nfmc {

struct LaunchPart {
    int slab0;         // first statistics slab of the part: its workgroups write slabs [slab0, slab0 + grid_cap), which no
                       // other part touches (block_stats_flush adds to a slab with a plain read-modify-write)
    int grid_cap;      // most workgroups a launch of the part may have: its share of kMaxGrid
    int64_t layout_n;  // chains of the whole run: where a layout choice depends on the chain count, it is made for this
                       // one, so that every chain goes through the kernel the unsplit run would use
};

// nfmc_flow_mh_steps_f32 behind its NULL check; `part` = NULL is the entry point itself.  A part can be launched on the
// register-layout kernels only (flow_b_kernels.hip): NFMC_EUNSUPPORTED elsewhere.
int flow_mh_steps(const NfmcFlowMhArgs& args, hipStream_t st, const LaunchPart* part);
// chains per workgroup tile of the register-layout kernel that takes `args`, or 0 when another kernel does
int64_t flow_mh_tile_chains(const NfmcFlowMhArgs& args);

}  // namespace nfmc

// vpt_fluid.h — a stable-fluids step over four volumes of a resident scene (include/vpt.h: vpt_scene_fluid_step): the call
// vpt_capi.hip forwards to.  Kernels and host logic: vpt_fluid.hip, the rule: vpt_fluid_rule.h.
#pragma once
#include "vpt_resident.h"

// Validates `step` (nothing a scene owns is written before it has passed) and launches, step.steps times, in order, on stream 0 of
// r.device: force + walls, the advection into r.d_fluid_scratch (grown to four fields), its move into place + walls, the divergence, the
// Jacobi sweeps between two of the scratch's fields (K sweeps a launch, K from VPT_FLUID_BLOCK) and project + walls.  Only the voxels of
// the four volumes change: no table, no mirror, no light.  r's counters (vpt_scene_update_stats) describe this call; the device has
// finished when the call returns.
// solver (include/vpt.h: vpt_scene_fluid_step_solver): null or VPT_FLUID_JACOBI, the above; VPT_FLUID_MULTIGRID, solver->cycles V-cycles in
// the Jacobi launches' place, the levels above the volume in r.d_fluid_mg (grown to three fields a level), VPT_FLUID_MG_BLOCK half-sweeps
// a smoothing launch.
// detail (include/vpt.h: vpt_scene_fluid_step_detail): null or off, the above.  vorticity > 0: the confinement launch takes the force
// launch's place and leaves the fields in the scratch, the advection goes from there back into the pool and the move runs in place.
// VPT_FLUID_MACCORMACK: one launch more after the advection, and the scratch grown to eight fields.
int fluid_apply(resident& r, const vpt_fluid_step& step, const vpt_fluid_solver* solver, const vpt_fluid_detail* detail, edit_outcome& out);

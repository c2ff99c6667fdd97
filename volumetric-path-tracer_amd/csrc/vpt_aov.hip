// vpt_aov.hip — the first-hit pass of vpt_render_aov_device (vpt_aov_kernel.hip.h) for scenes of faces.  The layout copies of its
// planes (vpt_resolve_ids_device, vpt_render_aov) are vpt_layout.hip's.
#include "vpt_aov_kernel.hip.h"
VPT_AOV_DEFINE(true, false)
VPT_AOV_DEFINE(false, false)

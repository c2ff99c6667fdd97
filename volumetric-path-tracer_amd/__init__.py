"""vpt-mi355x: ctypes bindings over the C-ABI of ``include/vpt.h`` (libvpt_hip.so, the HIP
path) and over the host library (libvpt_host.so: scene.json loader, BVH / light / state builders
that mirror ``libs/yocto_pathtrace/yocto_pathtrace.h:119-139`` of the reference).

Nothing in this package computes radiance on the CPU and nothing here touches ``oracle/``: if
the HIP library is missing or no GPU is present, rendering raises ``VptError``.

The directory name contains a dash, so import it with ``vpt_loader.load()`` (repo root) or
``importlib``; inside, everything is ordinary Python, split by role and re-exported here:
``_abi`` (libraries, structures, prototypes, call idioms), ``edits`` (the edit classes),
``host_scene`` (HostScene and the free host functions), ``device`` (DeviceScene, MultiDeviceScene,
device-resident state), ``session`` (RenderSession), ``images`` (denoise, tone map, resolve).
"""
from ._abi import *   # noqa: F401,F403 - every structure, record dtype and constant, hip, host, VptError
from ._abi import _check, _p   # noqa: F401 - the measuring tools under profiles/tools call the C-ABI directly
from .edits import (BvhRebuild, InstanceEdit, SceneEdit, SculptEdit, SculptEntry, ShapeEdit, Stamp, SubdivEdit, SubdivPlan, TextureEdit,   # noqa: F401
                    VolumeEdit, VolumeNew, VolumeSetEdit, VolumeSource, mesh)
from .device import (AdaptiveRun, DeviceScene, DisplayParams, MultiDeviceScene, PathtraceParams, PathtraceState, box3_device,   # noqa: F401
                     device_count, layout_pixel_index, layout_slots, make_state_jump, resolve_device, resolve_hits_device, resolve_ids_device,
                     resolve_sdf_ids_device, resolve_srgb8_device, selftest_reciprocal, state_download, state_init_device, state_upload)
from .host_scene import (BakedVolume, HostScene, bake_sdf, bake_sdf_grid, bake_triangles, build_bvh, catmullclark, density_from_sdf,   # noqa: F401
                         displace_vertices, fit_volume, mesh_sdf, save_mesh_ply, save_volume, vertex_normals)
from .session import RenderSession   # noqa: F401
from .images import (denoise_device, denoise_render, denoise_scratch_bytes, encode_jpeg_q75, get_render, get_render_hits, half_variance,   # noqa: F401
                     half_variance_device, linear_to_srgb8, pathtrace_guides, tonemap_device, tonemap_image, upscale_device, upscale_preview)

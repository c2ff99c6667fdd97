"""The C-ABI as ctypes sees it: the two libraries, every structure and record dtype of include/vpt.h, the constants, the prototypes,
and the few idioms every call into the libraries goes through (_check, _host_call, _filled, _counted, _edit_call)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SHADER_NAMES = ["volpathtrace", "pathtrace", "naive", "eyelight", "normal", "texcoord", "color",
                "implicit", "implicit_normal"]  # yocto_pathtrace.h:101-103
# the shaders the reference does not have, beside its list: name -> id (include/vpt.h: ids 9 .. 15 name nothing)
EXTENSION_SHADERS = {"volgrid": 16}


def shader_id(name: str) -> int:
    """the id of a shader name: the reference's by their place in SHADER_NAMES, the extensions' from EXTENSION_SHADERS"""
    if name in SHADER_NAMES:
        return SHADER_NAMES.index(name)
    if name in EXTENSION_SHADERS:
        return EXTENSION_SHADERS[name]
    raise VptError("sampler unknown")  # reference: get_shader throws (cpp:947-950)


def shader_name(ident: int) -> str:
    """the name of a shader id; ids that name nothing (9 .. 15 among them) raise VptError("sampler unknown")"""
    if 0 <= ident < len(SHADER_NAMES):
        return SHADER_NAMES[ident]
    for name, value in EXTENSION_SHADERS.items():
        if value == ident:
            return name
    raise VptError("sampler unknown")


class VptError(RuntimeError):
    pass


def _lib(name: str) -> C.CDLL:
    path = os.path.join(_HERE, name)
    if not os.path.exists(path):
        raise VptError(f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


hip = _lib("libvpt_hip.so")    # must load first: libvpt_host.so links against it
host = _lib("libvpt_host.so")


class VptParams(C.Structure):  # vpt_params
    _fields_ = [("camera", C.c_int32), ("resolution", C.c_int32), ("shader", C.c_int32),
                ("samples", C.c_int32), ("bounces", C.c_int32), ("noparallel", C.c_int32),
                ("noimplicit_mis", C.c_int32), ("spheretrace_maxiter", C.c_int32)]


class VptLayout(C.Structure):  # vpt_layout
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("tile_w", C.c_int32),
                ("tile_h", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32)]


class VptAdaptive(C.Structure):  # vpt_adaptive
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_int32), ("step", C.c_int32)]


class VptDenoise(C.Structure):  # vpt_denoise_params
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float)]


class VptDisplay(C.Structure):  # vpt_display_params
    _fields_ = [("exposure", C.c_float), ("filmic", C.c_int32), ("srgb", C.c_int32)]


class VptSessionParams(C.Structure):  # vpt_session_params
    _fields_ = [("render", VptParams), ("pratio", C.c_int32), ("display", VptDisplay), ("denoise", C.c_int32), ("filter", VptDenoise),
                ("guide_samples", C.c_int32)]


AOV_PLANES = ("normal", "albedo", "texcoord", "depth", "ids", "uvt")


class VptAovPlanes(C.Structure):  # vpt_aov_planes: any of them None
    _fields_ = [(name, C.c_void_p) for name in AOV_PLANES]


class VptPick(C.Structure):  # vpt_pick
    _fields_ = [("hit", C.c_int32), ("instance", C.c_int32), ("element", C.c_int32), ("shape", C.c_int32), ("material", C.c_int32),
                ("u", C.c_float), ("v", C.c_float), ("distance", C.c_float)]


SDF_AOV_PLANES = ("normal", "albedo", "depth", "ids", "hit")


class VptSdfAovPlanes(C.Structure):  # vpt_sdf_aov_planes: any of them None
    _fields_ = [(name, C.c_void_p) for name in SDF_AOV_PLANES]


class VptSdfPick(C.Structure):  # vpt_sdf_pick
    _fields_ = [("hit", C.c_int32), ("vol_instance", C.c_int32), ("sdf", C.c_int32), ("volume", C.c_int32), ("material", C.c_int32),
                ("distance", C.c_float), ("position", C.c_float * 3), ("normal", C.c_float * 3)]


class VptFrame(C.Structure):  # vpt_frame: x, y, z, o
    _fields_ = [("x", C.c_float * 3), ("y", C.c_float * 3), ("z", C.c_float * 3), ("o", C.c_float * 3)]


class VptCamera(C.Structure):  # vpt_camera
    _fields_ = [("frame", VptFrame), ("orthographic", C.c_int32), ("lens", C.c_float), ("film", C.c_float), ("aspect", C.c_float),
                ("focus", C.c_float), ("aperture", C.c_float)]


class VptMaterial(C.Structure):  # vpt_material
    _fields_ = [("type", C.c_int32), ("emission", C.c_float * 3), ("color", C.c_float * 3), ("roughness", C.c_float),
                ("metallic", C.c_float), ("ior", C.c_float), ("scattering", C.c_float * 3), ("scanisotropy", C.c_float),
                ("trdepth", C.c_float), ("opacity", C.c_float), ("emission_tex", C.c_int32), ("color_tex", C.c_int32),
                ("roughness_tex", C.c_int32), ("scattering_tex", C.c_int32), ("normal_tex", C.c_int32)]


class VptSceneEdit(C.Structure):  # vpt_scene_edit
    _fields_ = [("num_cameras", C.c_int32), ("camera_ids", C.c_void_p), ("cameras", C.c_void_p),
                ("num_instances", C.c_int32), ("instance_ids", C.c_void_p), ("instance_frames", C.c_void_p),
                ("num_environments", C.c_int32), ("environment_ids", C.c_void_p), ("environment_frames", C.c_void_p),
                ("num_materials", C.c_int32), ("material_ids", C.c_void_p), ("materials", C.c_void_p),
                ("num_shapes", C.c_int32), ("shape_ids", C.c_void_p), ("shape_positions", C.c_void_p), ("shape_normals", C.c_void_p)]


class VptEnvironment(C.Structure):  # vpt_environment
    _fields_ = [("frame", VptFrame), ("emission", C.c_float * 3), ("emission_tex", C.c_int32)]


class VptTexture(C.Structure):  # vpt_texture
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("linear", C.c_int32), ("is_float", C.c_int32), ("offset", C.c_int64)]


class VptTextureEdit(C.Structure):  # vpt_texture_edit
    _fields_ = [("num_environments", C.c_int32), ("environment_ids", C.c_void_p), ("environments", C.c_void_p),
                ("num_textures", C.c_int32), ("texture_ids", C.c_void_p), ("textures", C.c_void_p),
                ("num_texels_f", C.c_int64), ("texels_f", C.c_void_p), ("num_texels_b", C.c_int64), ("texels_b", C.c_void_p)]


class VptVolume(C.Structure):  # vpt_volume
    _fields_ = [("whd", C.c_int32 * 3), ("res", C.c_float), ("offset", C.c_int64)]


class VptVolumeInstance(C.Structure):  # vpt_volume_instance
    _fields_ = [("frame", VptFrame), ("volume", C.c_int32), ("material", C.c_int32), ("scalef", C.c_float)]


class VptSdf(C.Structure):  # vpt_sdf
    _fields_ = [("frame", VptFrame), ("type", C.c_int32), ("material", C.c_int32), ("whd", C.c_float * 3), ("p", C.c_float * 4)]


class VptVolumeSource(C.Structure):  # vpt_volume_source
    _fields_ = [("whd", C.c_int32 * 3), ("res", C.c_float), ("region_lo", C.c_int32 * 3), ("region_whd", C.c_int32 * 3), ("mode", C.c_int32),
                ("offset", C.c_int64), ("bake", C.c_void_p)]


class VptVolumeEdit(C.Structure):  # vpt_volume_edit
    _fields_ = [("num_vol_instances", C.c_int32), ("vol_instance_ids", C.c_void_p), ("vol_instances", C.c_void_p),
                ("num_sdfs", C.c_int32), ("sdf_ids", C.c_void_p), ("sdfs", C.c_void_p),
                ("num_volumes", C.c_int32), ("volume_ids", C.c_void_p), ("volumes", C.c_void_p),
                ("num_voxels", C.c_int64), ("voxels", C.c_void_p)]


class VptSculptStamp(C.Structure):  # vpt_sculpt_stamp
    _fields_ = [("brush", VptSdf), ("op", C.c_int32), ("blend", C.c_float)]


class VptSculptEntry(C.Structure):  # vpt_sculpt_entry
    _fields_ = [("volume", C.c_int32), ("region_lo", C.c_int32 * 3), ("region_whd", C.c_int32 * 3), ("origin", C.c_float * 3), ("step", C.c_float * 3),
                ("first_stamp", C.c_int32), ("num_stamps", C.c_int32)]


class VptSculptEdit(C.Structure):  # vpt_sculpt_edit
    _fields_ = [("num_entries", C.c_int32), ("entries", C.c_void_p), ("num_stamps", C.c_int32), ("stamps", C.c_void_p)]


assert C.sizeof(VptSculptStamp) == 92 and C.sizeof(VptSculptEntry) == 60 and C.sizeof(VptSculptEdit) == 32


class VptVolumeNew(C.Structure):  # vpt_volume_new
    _fields_ = [("whd", C.c_int32 * 3), ("res", C.c_float), ("source", C.c_int32), ("offset", C.c_int64), ("bake", C.c_void_p), ("fill", C.c_float),
                ("copy_of", C.c_int32)]


class VptVolumeSetEdit(C.Structure):  # vpt_volume_set_edit
    _fields_ = [("num_remove_vol_instances", C.c_int32), ("remove_vol_instance_ids", C.c_void_p), ("num_remove_sdfs", C.c_int32), ("remove_sdf_ids", C.c_void_p),
                ("num_remove_volumes", C.c_int32), ("remove_volume_ids", C.c_void_p), ("num_add_volumes", C.c_int32), ("add_volumes", C.c_void_p),
                ("num_add_vol_instances", C.c_int32), ("add_vol_instances", C.c_void_p), ("num_add_sdfs", C.c_int32), ("add_sdfs", C.c_void_p),
                ("num_voxels", C.c_int64), ("voxels", C.c_void_p)]


assert C.sizeof(VptVolumeNew) == 48 and C.sizeof(VptVolumeSetEdit) == 112

SDF_TYPES = ["bbox", "box", "capped_cone", "plane", "sphere", "torus"]
VOXELS_REPLACE, VOXELS_UNION = 0, 1
SCULPT_REPLACE, SCULPT_UNION, SCULPT_SUBTRACT, SCULPT_INTERSECT = 0, 1, 2, 3
VOLUME_FROM_HOST, VOLUME_FROM_BAKE, VOLUME_FILL, VOLUME_COPY = 0, 1, 2, 3   # vpt_volume_new::source
SCULPT_RECORD_BYTES = 80   # VPT_SCULPT_RECORD_BYTES: one stamp as the device reads it
MATERIAL_TYPES = ["matte", "glossy", "reflective", "transparent", "refractive", "subsurface", "volumetric", "gltfpbr"]


class VptBakeDesc(C.Structure):  # vpt_bake_desc
    _fields_ = [("num_vertices", C.c_int32), ("positions", C.c_void_p), ("num_triangles", C.c_int32), ("triangles", C.c_void_p),
                ("whd", C.c_int32 * 3), ("origin", C.c_float * 3), ("step", C.c_float * 3)]


class VptBakeStats(C.Structure):  # vpt_bake_stats
    _fields_ = [("dropped_triangles", C.c_int32), ("bvh_nodes", C.c_int32), ("bvh_depth", C.c_int32), ("launches", C.c_int32),
                ("device_ms", C.c_float)]


class VptSdfMeshDesc(C.Structure):  # vpt_sdf_mesh_desc
    _fields_ = [("whd", C.c_int32 * 3), ("origin", C.c_float * 3), ("step", C.c_float * 3), ("iso", C.c_float)]


class VptSdfMeshRegion(C.Structure):  # vpt_sdf_mesh_region
    _fields_ = [("lo", C.c_int32 * 3), ("whd", C.c_int32 * 3)]


class VptSdfMeshStats(C.Structure):  # vpt_sdf_mesh_stats
    _fields_ = [("num_vertices", C.c_int32), ("num_quads", C.c_int32), ("launches", C.c_int32), ("device_ms", C.c_float)]


assert C.sizeof(VptSdfMeshDesc) == 40 and C.sizeof(VptSdfMeshRegion) == 24 and C.sizeof(VptSdfMeshStats) == 16


class VptBvhRebuild(C.Structure):  # vpt_bvh_rebuild
    _fields_ = [("num_shapes", C.c_int32), ("shape_ids", C.POINTER(C.c_int32)), ("scene", C.c_int32)]


class VptInstance(C.Structure):  # vpt_instance
    _fields_ = [("frame", VptFrame), ("shape", C.c_int32), ("material", C.c_int32)]


class VptInstanceEdit(C.Structure):  # vpt_instance_edit
    _fields_ = [("num_remove", C.c_int32), ("remove_ids", C.c_void_p), ("num_set", C.c_int32), ("set_ids", C.c_void_p), ("set", C.c_void_p),
                ("num_add", C.c_int32), ("add", C.c_void_p)]


INSTANCE = np.dtype([("frame", np.float32, 12), ("shape", np.int32), ("material", np.int32)])   # vpt_instance
assert INSTANCE.itemsize == C.sizeof(VptInstance) == 56


class VptShapeData(C.Structure):  # vpt_shape_data
    _fields_ = [("num_vertices", C.c_int32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("colors", C.c_void_p),
                ("radius", C.c_void_p), ("num_triangles", C.c_int32), ("triangles", C.c_void_p), ("num_quads", C.c_int32), ("quads", C.c_void_p),
                ("num_points", C.c_int32), ("points", C.c_void_p), ("num_lines", C.c_int32), ("lines", C.c_void_p)]


class VptShapeEdit(C.Structure):  # vpt_shape_edit
    _fields_ = [("num_remove", C.c_int32), ("remove_ids", C.c_void_p), ("num_set", C.c_int32), ("set_ids", C.c_void_p), ("set", C.c_void_p),
                ("num_add", C.c_int32), ("add", C.c_void_p)]


assert C.sizeof(VptShapeData) == 112 and C.sizeof(VptShapeEdit) == 56


class VptSubdivLevel(C.Structure):  # vpt_subdiv_level
    _fields_ = [("dim", C.c_int32), ("num_vertices", C.c_int32), ("num_edges", C.c_int32), ("num_faces", C.c_int32), ("num_new_faces", C.c_int32),
                ("edges", C.c_void_p), ("faces", C.c_void_p), ("new_faces", C.c_void_p), ("valence", C.c_void_p), ("offsets", C.c_void_p),
                ("items", C.c_void_p), ("num_items", C.c_int64)]


class VptSubdivPlan(C.Structure):  # vpt_subdiv_plan
    _fields_ = [("shape", C.c_int32), ("subdivisions", C.c_int32), ("smooth", C.c_int32), ("displacement", C.c_float), ("displacement_tex", C.c_int32),
                ("num_cage_positions", C.c_int32), ("cage_positions", C.c_void_p), ("num_cage_normals", C.c_int32), ("cage_normals", C.c_void_p),
                ("num_levels", C.c_int32), ("levels", C.c_void_p), ("num_quads", C.c_int32), ("quads", C.c_void_p),
                ("num_vertices", C.c_int32), ("verts", C.c_void_p)]


class VptSubdivEdit(C.Structure):  # vpt_subdiv_edit
    _fields_ = [("num", C.c_int32), ("subdiv_ids", C.c_void_p), ("cage_positions", C.c_void_p), ("displacement", C.c_void_p)]


assert C.sizeof(VptSubdivLevel) == 80 and C.sizeof(VptSubdivPlan) == 96 and C.sizeof(VptSubdivEdit) == 32

MESH_FLOATS = {"positions": 3, "normals": 3, "texcoords": 2, "colors": 4, "radius": 0}     # floats per vertex (0: a plain array)
MESH_ELEMENTS = {"triangles": 3, "quads": 4, "points": 0, "lines": 2}                        # indices per element


# defaults of the denoising filter (include/vpt.h: VPT_DENOISE_DEFAULT_*)
DENOISE_ITERATIONS, DENOISE_SIGMA_LUMINANCE, DENOISE_SIGMA_NORMAL, DENOISE_SIGMA_ALBEDO = 5, 4.0, 0.35, 0.1


# ---- prototypes -----------------------------------------------------------------------------
_p = C.c_void_p
hip.vpt_last_error.restype = C.c_char_p
hip.vpt_version.restype = C.c_char_p
hip.vpt_device_count.restype = C.c_int
hip.vpt_scene_create.argtypes = [_p, C.c_int, C.POINTER(_p)]
hip.vpt_scene_create_curves.argtypes = [_p, _p, C.c_int, C.POINTER(_p)]
hip.vpt_scene_destroy.argtypes = [_p]
hip.vpt_scene_destroy.restype = None
hip.vpt_scene_update.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_multi_update.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_scene_update_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_multi_update_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_session_edit_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_scene_update_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_multi_update_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_session_edit_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_scene_update_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_multi_update_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_session_edit_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_scene_sculpt_volumes.argtypes = [_p, C.POINTER(VptSculptEdit)]
hip.vpt_multi_sculpt_volumes.argtypes = [_p, C.POINTER(VptSculptEdit)]
hip.vpt_session_sculpt_volumes.argtypes = [_p, C.POINTER(VptSculptEdit)]
hip.vpt_scene_update_volume_set.argtypes = [_p, C.POINTER(VptVolumeSetEdit)]
hip.vpt_multi_update_volume_set.argtypes = [_p, C.POINTER(VptVolumeSetEdit)]
hip.vpt_session_edit_volume_set.argtypes = [_p, C.POINTER(VptVolumeSetEdit)]
hip.vpt_scene_get_volumes.argtypes =[_p, _p, C.c_int, _p, C.c_int, _p, C.c_int]
hip.vpt_scene_count_implicit.argtypes = [_p, _p]
hip.vpt_scene_get_voxels.argtypes = [_p, C.c_int, _p, C.c_int64]
hip.vpt_scene_get_lights.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int), _p, C.c_int64, C.POINTER(C.c_int64)]
hip.vpt_scene_light_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_get_media.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_scene_get_bvh.argtypes = [_p, _p, C.c_int, _p, C.c_int64]
hip.vpt_scene_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_multi_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_session_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_scene_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_multi_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_session_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_scene_update_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_multi_update_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_session_edit_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_scene_get_instances.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int)]
hip.vpt_scene_instance_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_update_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_multi_update_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_session_edit_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_scene_attach_subdiv.argtypes = [_p, C.POINTER(VptSubdivPlan), C.POINTER(C.c_int)]
hip.vpt_multi_attach_subdiv.argtypes = [_p, C.POINTER(VptSubdivPlan), C.POINTER(C.c_int)]
hip.vpt_scene_detach_subdiv.argtypes = [_p, C.c_int]
hip.vpt_multi_detach_subdiv.argtypes = [_p, C.c_int]
hip.vpt_scene_subdiv_count.argtypes = [_p]
hip.vpt_scene_subdiv_shape.argtypes = [_p, C.c_int]
hip.vpt_multi_subdiv_shape.argtypes = [_p, C.c_int]
hip.vpt_scene_update_subdivs.argtypes = [_p, C.POINTER(VptSubdivEdit)]
hip.vpt_multi_update_subdivs.argtypes = [_p, C.POINTER(VptSubdivEdit)]
hip.vpt_session_edit_subdivs.argtypes = [_p, C.POINTER(VptSubdivEdit)]
hip.vpt_scene_shape_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_get_shape_counts.argtypes = [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.vpt_scene_get_bvh_counts.argtypes = [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _p]
hip.vpt_scene_get_bvh_prims.argtypes = [_p, _p, C.c_int, _p, C.c_int64]
hip.vpt_scene_update_stats.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
hip.vpt_render.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_layout_slots.argtypes = [C.POINTER(VptLayout)]
hip.vpt_layout_slots.restype = C.c_int64
hip.vpt_state_upload.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p, _p, _p]
hip.vpt_state_download.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p, _p, _p]
hip.vpt_render_device.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptLayout), C.c_int, _p, _p, _p, _p]
hip.vpt_resolve_device.argtypes = [C.POINTER(VptLayout), _p, C.c_int, _p, _p]
hip.vpt_render_adaptive.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int64)]
hip.vpt_render_device_adaptive.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.POINTER(VptLayout), _p, _p, _p, _p,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int64)]
hip.vpt_resolve_hits_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p]
hip.vpt_denoise_scratch_bytes.argtypes = [C.c_int, C.c_int]
hip.vpt_denoise_scratch_bytes.restype = C.c_int64
hip.vpt_denoise_device.argtypes = [C.POINTER(VptDenoise), C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, _p]
hip.vpt_half_variance_device.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, _p, _p]
hip.vpt_denoise.argtypes = [C.POINTER(VptDenoise), C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p]
hip.vpt_half_variance.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, _p]
hip.vpt_state_init_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p]
hip.vpt_tonemap_device.argtypes = [C.POINTER(VptDisplay), C.c_int, C.c_int, _p, _p, _p, _p]
hip.vpt_upscale_device.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, C.c_int, _p, _p]
hip.vpt_tonemap.argtypes = [C.POINTER(VptDisplay), C.c_int, C.c_int, C.c_int, _p, _p, _p]
hip.vpt_scene_get_camera.argtypes = [_p, C.c_int, C.POINTER(VptCamera)]
hip.vpt_scene_get_device.argtypes = [_p]
hip.vpt_session_create.argtypes = [_p, C.POINTER(VptSessionParams), C.POINTER(_p)]
hip.vpt_session_destroy.argtypes = [_p]
hip.vpt_session_destroy.restype = None
hip.vpt_session_reset.argtypes = [_p, C.POINTER(VptSessionParams)]
hip.vpt_session_advance.argtypes = [_p, C.c_int]
hip.vpt_session_set_display.argtypes = [_p, C.POINTER(VptDisplay)]
hip.vpt_session_edit.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_session_get_display.argtypes = [_p, _p, _p]
hip.vpt_session_get_image.argtypes = [_p, _p]
hip.vpt_session_get_denoised.argtypes = [_p, _p]
hip.vpt_session_get_state.argtypes = [_p, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_session_size.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_session_samples.argtypes = [_p]
hip.vpt_session_stats.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.vpt_adaptive_run_create.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.POINTER(VptLayout), _p, _p, _p, _p, C.POINTER(_p)]
hip.vpt_adaptive_run_rounds.argtypes = [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
hip.vpt_adaptive_run_progress.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_adaptive_run_noise_device.argtypes = [_p, _p, _p, _p]
hip.vpt_adaptive_run_stats_device.argtypes = [_p, _p, _p, _p]
hip.vpt_adaptive_run_destroy.argtypes = [_p]
hip.vpt_adaptive_run_destroy.restype = None
hip.vpt_box3_device.argtypes = [C.c_int, C.c_int, _p, _p, _p]
hip.vpt_session_set_adaptive.argtypes = [_p, C.POINTER(VptAdaptive)]
hip.vpt_session_progress.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
hip.vpt_session_get_hits.argtypes = [_p, _p]
hip.vpt_session_get_noise.argtypes = [_p, _p, _p]
hip.vpt_session_get_adaptive_stats.argtypes = [_p, _p, _p]
hip.vpt_render_aov_device.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptLayout), C.c_int, C.POINTER(VptAovPlanes), _p, _p, _p]
hip.vpt_resolve_ids_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p]
hip.vpt_render_aov.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, C.POINTER(VptAovPlanes), _p, _p, C.POINTER(C.c_int)]
hip.vpt_session_get_guides.argtypes = [_p, _p, _p]
hip.vpt_session_pick.argtypes = [_p, C.c_int, C.c_int, C.POINTER(VptPick)]
hip.vpt_session_get_ids.argtypes = [_p, _p, _p]
hip.vpt_render_sdf_aov_device.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptLayout), C.c_int, C.POINTER(VptSdfAovPlanes), _p, _p, _p]
hip.vpt_resolve_sdf_ids_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p]
hip.vpt_render_sdf_aov.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, C.POINTER(VptSdfAovPlanes), _p, _p, C.POINTER(C.c_int)]
hip.vpt_session_pick_sdf.argtypes = [_p, C.c_int, C.c_int, C.POINTER(VptSdfPick)]
hip.vpt_session_get_sdf_ids.argtypes = [_p, _p, _p]
hip.vpt_last_kernel_ms.argtypes = [_p, C.POINTER(C.c_float)]
hip.vpt_intersect.argtypes = [_p, C.c_int, _p, C.c_int, _p, _p]
hip.vpt_build_bvh.argtypes = [C.c_int, _p, C.c_int, _p, C.c_int, C.POINTER(C.c_int), _p]
hip.vpt_build_bvh_quality.argtypes = [C.c_int, _p, C.c_int, C.c_int, _p, C.c_int, C.POINTER(C.c_int), _p]
hip.vpt_bake_sdf.argtypes = [C.c_int, C.POINTER(VptBakeDesc), _p, C.POINTER(VptBakeStats)]
hip.vpt_bake_feature_normals.argtypes = [C.POINTER(VptBakeDesc), _p, _p]
hip.vpt_mesh_sdf.argtypes = [C.c_int, C.POINTER(VptSdfMeshDesc), _p, _p, _p, C.c_int32, _p, C.c_int32, C.POINTER(VptSdfMeshStats)]
hip.vpt_scene_mesh_volume.argtypes = [_p, C.c_int, C.POINTER(VptSdfMeshDesc), C.POINTER(VptSdfMeshRegion), _p, _p, C.c_int32, _p, C.c_int32,
                                      C.POINTER(VptSdfMeshStats)]
hip.vpt_last_wave_costs.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int)]
hip.vpt_scene_record_bytes.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_multi_create.argtypes = [_p, C.POINTER(C.c_int), C.c_int, C.POINTER(_p)]
hip.vpt_multi_create_curves.argtypes = [_p, _p, C.POINTER(C.c_int), C.c_int, C.POINTER(_p)]
hip.vpt_multi_destroy.argtypes = [_p]
hip.vpt_multi_destroy.restype = None
hip.vpt_multi_device_count.argtypes = [_p]
hip.vpt_multi_render.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_multi_get_render.argtypes = [_p, _p]
hip.vpt_multi_uploaded_parts.argtypes = [_p]
hip.vpt_multi_transport.argtypes = [_p]
hip.vpt_multi_transport.restype = C.c_char_p
hip.vpt_multi_set_state.argtypes = [_p, C.c_int, C.c_int, _p, _p, _p, C.c_int]
hip.vpt_multi_get_state.argtypes = [_p, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_check_watchdog.argtypes = [_p]
hip.vpt_resolve_srgb8_device.argtypes = [C.POINTER(VptLayout), _p, C.c_int, _p, _p]
hip.vpt_selftest_reciprocal.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
hip.vpt_selftest_light_cdf.argtypes = [_p, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
hip.vpt_kat_strides.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_kat.argtypes = [_p, C.c_int, C.c_int, C.c_int, _p, _p]
hip.vpt_spheretrace.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p]
hip.vpt_eval_lobes.argtypes = [_p, C.c_int, _p, _p]
hip.vpt_split_plan.argtypes = [C.c_int, _p, C.c_int, C.c_int, C.c_int, _p, C.POINTER(C.c_int)]
host.vpth_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
host.vpth_scene_load.restype = _p
host.vpth_scene_load_ex.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_load_ex.restype = _p
host.vpth_vertex_normals.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_displace_vertices.argtypes = [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_catmullclark.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.POINTER(C.c_int), _p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
host.vpth_scene_free.argtypes = [_p]
host.vpth_scene_count.argtypes = [_p, C.c_int]
host.vpth_scene_get_item.argtypes = [_p, C.c_int, C.c_int, _p, C.c_int64]
host.vpth_scene_get_item.restype = C.c_int64
host.vpth_scene_set_item.argtypes = [_p, C.c_int, C.c_int, _p, C.c_int64, C.c_char_p, C.c_int]
host.vpth_scene_update_bvh.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh.argtypes = [_p, _p, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh_quality.argtypes = [_p, _p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_edit_instances.argtypes = [_p, _p, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_edit_shapes.argtypes = [_p, _p, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_update_lights.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_subdiv_count.argtypes = [_p]
host.vpth_scene_get_subdiv.argtypes = [_p, C.c_int, _p, C.POINTER(C.c_float)]
host.vpth_scene_subdiv_plan_item.argtypes = [_p, C.c_int, C.c_int, _p, C.c_int64]
host.vpth_scene_subdiv_plan_item.restype = C.c_int64
host.vpth_scene_set_subdiv.argtypes = [_p, C.c_int, _p, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
host.vpth_scene_free.restype = None
host.vpth_scene_get_environment.argtypes = [_p, C.c_int, C.POINTER(VptEnvironment)]
host.vpth_scene_set_environment.argtypes = [_p, C.c_int, C.POINTER(VptEnvironment), C.c_char_p, C.c_int]
host.vpth_scene_get_texture.argtypes = [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _p, C.c_int64]
host.vpth_scene_set_texture.argtypes = [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_scene_update_textures.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_count_implicit.argtypes = [_p, C.c_int]
host.vpth_scene_get_vol_instance.argtypes = [_p, C.c_int, C.POINTER(VptVolumeInstance)]
host.vpth_scene_set_vol_instance.argtypes = [_p, C.c_int, C.POINTER(VptVolumeInstance), C.c_char_p, C.c_int]
host.vpth_scene_get_sdf.argtypes = [_p, C.c_int, C.POINTER(VptSdf)]
host.vpth_scene_set_sdf.argtypes = [_p, C.c_int, C.POINTER(VptSdf), C.c_char_p, C.c_int]
host.vpth_scene_set_volume.argtypes = [_p, C.c_int, _p, C.c_float, _p, _p, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_scene_update_volumes.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_edit_volume_set.argtypes = [_p, C.POINTER(VptVolumeSetEdit), C.c_char_p, C.c_int]
host.vpth_scene_sculpt_volume.argtypes = [_p, C.POINTER(VptSculptEntry), _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_sculpt_eval.argtypes = [C.POINTER(VptSdf), _p, C.c_int, _p]
host.vpth_sculpt_combine.argtypes = [C.c_int, C.c_float, _p, _p, C.c_int, _p]
host.vpth_scene_desc.argtypes = [_p]
host.vpth_scene_desc.restype = _p
host.vpth_scene_curves.argtypes = [_p]
host.vpth_scene_curves.restype = _p
host.vpth_state_size.argtypes = [_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
host.vpth_make_state.argtypes = [_p, C.c_int, C.c_int, _p, _p, _p]
host.vpth_scene_stats.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh_device.argtypes = [_p, C.c_int, C.c_char_p, C.c_int]
host.vpth_build_bvh_host.argtypes = [_p, C.c_int, _p, C.POINTER(C.c_int), _p]
host.vpth_scene_rebuild_bvh_device_quality.argtypes = [_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_build_bvh_host_quality.argtypes = [_p, C.c_int, C.c_int, _p, C.POINTER(C.c_int), _p]
host.vpth_denoise.argtypes = [C.c_int, C.c_int, _p, _p, _p, _p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_half_variance.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_bake_triangles.argtypes = [_p, C.c_int, C.c_int, _p, C.POINTER(C.c_int)]
host.vpth_bake_grid.argtypes = [_p, C.c_int, _p, C.c_int, _p, _p, _p, C.c_int, _p, C.POINTER(VptBakeStats), C.c_char_p, C.c_int]
host.vpth_fit_volume.argtypes = [_p, _p, _p, C.c_int, C.POINTER(C.c_float), _p, _p, _p, C.c_char_p, C.c_int]
host.vpth_bake_volume.argtypes = [_p, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, _p, C.POINTER(C.c_float), _p, C.POINTER(VptBakeStats),
                                  C.c_char_p, C.c_int]
host.vpth_scene_get_volume.argtypes = [_p, C.c_int, _p, C.POINTER(C.c_float), _p, C.c_int64]
host.vpth_scene_get_volume.restype = C.c_int64
host.vpth_save_volume.argtypes = [C.c_char_p, _p, C.c_float, _p, C.c_char_p, C.c_int]
host.vpth_volgrid_majorants.argtypes = [_p, C.c_int, _p, C.c_int64, _p, C.c_char_p, C.c_int]
host.vpth_volgrid_density.argtypes = [_p, C.c_int, _p, _p, _p, C.c_char_p, C.c_int]
hip.vpt_scene_get_volgrid_majorants.argtypes = [_p, C.c_int, _p, C.c_int64, _p]
hip.vpt_scene_volgrid_density.argtypes = [_p, C.c_int, _p, _p, _p]
hip.vpt_scene_volgrid_track.argtypes = [_p, C.c_int, _p, _p, _p, _p, _p, _p, _p]
hip.vpt_scene_volgrid_stats.argtypes = [_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
host.vpth_mesh_sdf.argtypes = [C.POINTER(VptSdfMeshDesc), _p, C.POINTER(VptSdfMeshRegion), _p, _p, C.c_int32, _p, C.c_int32, C.POINTER(VptSdfMeshStats),
                               C.c_char_p, C.c_int]
host.vpth_save_mesh_ply.argtypes = [C.c_char_p, _p, _p, C.c_int, _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_tonemap.argtypes = [C.c_int64, _p, C.c_float, C.c_int, C.c_int, _p, _p]
host.vpth_upscale_preview.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, C.c_int, _p]
host.vpth_make_state_jump.argtypes = [C.c_int, C.c_int, _p]
host.vpth_linear_to_srgb8.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p]
host.vpth_linear_to_srgb8.restype = None
host.vpth_encode_jpeg_q75.argtypes = [C.c_int, C.c_int, _p, _p, C.c_int64]
host.vpth_encode_jpeg_q75.restype = C.c_int64


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise VptError(f"{what} failed ({rc}): {hip.vpt_last_error().decode()}")


class _Handle:
    """an object that owns one handle of a library: close() releases it, once, through the class's _free; so does __del__.  _free is
    the library's function itself, held by the class: at interpreter shutdown the module globals may be gone, a class's attributes are not"""
    _free = None

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._free(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


def _host_call(fn, *args, size: int = 512, handle: bool = False):
    """a vpth_* function whose last two arguments are an error buffer and its length, called with `args` before them: VptError with the
    buffer's text when it returns non-zero (handle: when it returns a null handle); else what it returned"""
    err = C.create_string_buffer(size)
    rc = fn(*args, err, len(err))
    if (not rc) if handle else rc != 0:
        raise VptError(err.value.decode())
    return rc


def _address(a) -> int:
    return a.ctypes.data if isinstance(a, np.ndarray) else C.addressof(a)


def _filled(call, make, refused: str):
    """the host library's "ask the size, then fill" getters: call(None, 0) returns the size n (negative: VptError(refused)), make(n) the
    numpy array or ctypes object of that size, call(its address, n) fills it"""
    n = call(None, 0)
    if n < 0:
        raise VptError(refused)
    out = make(n)
    call(_address(out), n)
    return out


def _counted(fn, handle, dtype, what: str, *tail) -> np.ndarray:
    """the C-ABI's "ask the count, then fill" getters fn(handle, out, capacity, &count, *tail): the array of `dtype` they fill"""
    n = C.c_int(0)
    _check(fn(handle, None, 0, C.byref(n), *tail), what)
    out = np.zeros(n.value, dtype)
    _check(fn(handle, out.ctypes.data if len(out) else None, len(out), C.byref(n), *tail), what)
    return out


def _mesh_desc(whd, origin, step, iso: float) -> VptSdfMeshDesc:
    """vpt_sdf_mesh_desc of whd = (w, h, d); origin and step: three floats each, or one for every axis"""
    f3 = lambda v: (C.c_float * 3)(*np.broadcast_to(np.asarray(v, np.float32), (3,)))
    return VptSdfMeshDesc((C.c_int32 * 3)(*(int(v) for v in whd)), f3(origin), f3(step), float(iso))


def _mesh_region(region):
    """vpt_sdf_mesh_region of (lo, whd), each (x, y, z); None stays None"""
    if region is None:
        return None
    lo, size = region
    return VptSdfMeshRegion((C.c_int32 * 3)(*(int(v) for v in lo)), (C.c_int32 * 3)(*(int(v) for v in size)))


def _meshed(call, stats=None) -> dict:
    """the "ask the counts, then fill" outputs of vpt_mesh_sdf, vpt_scene_mesh_volume and vpth_mesh_sdf: call(positions, normals,
    vertex_capacity, quads, quad_capacity, byref(stats)) raises what it refuses; the first call makes the counts, the second fills arrays of
    those sizes.  Returns {"positions", "normals": (n, 3) float32, "quads": (m, 4) int32}, empty arrays for an empty mesh; `stats`: a dict
    that receives the fields of vpt_sdf_mesh_stats as the last call left them."""
    st = VptSdfMeshStats()
    call(None, None, 0, None, 0, C.byref(st))
    nv, nq = st.num_vertices, st.num_quads
    out = {"positions": np.zeros((nv, 3), np.float32), "normals": np.zeros((nv, 3), np.float32), "quads": np.zeros((nq, 4), np.int32)}
    if nv:
        call(out["positions"].ctypes.data, out["normals"].ctypes.data, nv, out["quads"].ctypes.data if nq else None, nq, C.byref(st))
    if stats is not None:
        stats.update({name: getattr(st, name) for name, _ in VptSdfMeshStats._fields_})
    return out


def _edit_call(handle, name: str, edit, *extra) -> None:
    """the C-ABI's edit entry point `name` on a scene, multi-device scene or session handle, the arrays `edit` points into kept alive
    across the call"""
    abi, keep = edit.to_abi()
    _check(getattr(hip, name)(handle, C.byref(abi), *extra), name)
    del keep


BVH_NODE = np.dtype([("bbox_min", np.float32, 3), ("bbox_max", np.float32, 3), ("start", np.int32), ("num", np.int16), ("axis", np.int8),
                     ("internal", np.uint8)])
assert BVH_NODE.itemsize == 32


class VptSceneDescBvh(C.Structure):
    """the last four tables of vpt_scene_desc (the two-level BVH); OFFSET: where they start (10 int32 + pointer tables, then 10
    int64 + pointer pools: every pair takes 16 bytes)"""
    _fields_ = [("num_scene_bvh_nodes", C.c_int32), ("scene_bvh_nodes", C.c_void_p), ("num_scene_bvh_prims", C.c_int32),
                ("scene_bvh_prims", C.c_void_p), ("num_shape_bvh_nodes", C.c_int64), ("shape_bvh_nodes", C.c_void_p),
                ("num_shape_bvh_prims", C.c_int64), ("shape_bvh_prims", C.c_void_p)]
    OFFSET = 20 * 16


LIGHT = np.dtype([("instance", np.int32), ("environment", np.int32), ("sdf", np.int32), ("cdf_len", np.int32), ("cdf_offset", np.int64)])   # vpt_light
assert LIGHT.itemsize == 24


class VptSceneDescImplicit(C.Structure):
    """the three tables of vpt_scene_desc behind the implicit shaders: its seventh to ninth {int32 count, pointer} pairs"""
    _fields_ = [("num_volumes", C.c_int32), ("volumes", C.c_void_p), ("num_vol_instances", C.c_int32), ("vol_instances", C.c_void_p),
                ("num_sdfs", C.c_int32), ("sdfs", C.c_void_p)]
    OFFSET = 6 * 16


class VptSceneDescVoxels(C.Structure):
    """the voxel pool of vpt_scene_desc: its ninth {int64 count, pointer} pool"""
    _fields_ = [("num_voxels", C.c_int64), ("voxels", C.c_void_p)]
    OFFSET = 10 * 16 + 8 * 16


class VptSceneDescLights(C.Structure):
    """vpt_scene_desc up to its CDF pool, for the two tables of the lights: the tenth {int32 count, pointer} pair and the tenth
    {int64 count, pointer} pool"""
    _fields_ = [("tables", C.c_byte * (9 * 16)), ("num_lights", C.c_int32), ("lights", C.c_void_p), ("pools", C.c_byte * (9 * 16)),
                ("num_light_cdf", C.c_int64), ("light_cdf", C.c_void_p)]


BVH_MIDDLE, BVH_SAH = 0, 1   # VPT_BVH_MIDDLE, VPT_BVH_SAH

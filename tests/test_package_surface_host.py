"""The surface of the Python package: every public name it has exported stays an attribute of the package, a class is one object
however it is reached (so `except vpt.VptError` catches what any module of the package raises), and the structs the edit classes hand to
the C-ABI are, byte for byte, the ones recorded in tests/golden/edit_abi.npz - pointers compared as null / not null, the arrays they
point into by their bytes.  `python tests/test_package_surface_host.py` records that file from the tree it runs in."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

RECORD = os.path.join(GOLDEN, "edit_abi.npz")
F = np.float32

# every name of dir(vpt) without a leading underscore, but for what the package itself imports from the standard library and numpy
# (C, np, os, Optional, annotations, dataclass, field)
PUBLIC = """AOV_PLANES AdaptiveRun BVH_MIDDLE BVH_NODE BVH_SAH BakedVolume BvhRebuild DENOISE_ITERATIONS DENOISE_SIGMA_ALBEDO
DENOISE_SIGMA_LUMINANCE DENOISE_SIGMA_NORMAL DeviceScene DisplayParams HostScene INSTANCE InstanceEdit LIGHT MATERIAL_TYPES MESH_ELEMENTS
MESH_FLOATS MultiDeviceScene PathtraceParams PathtraceState RenderSession SDF_TYPES SHADER_NAMES SceneEdit ShapeEdit TextureEdit
VOXELS_REPLACE VOXELS_UNION VolumeEdit VolumeSource VptAdaptive VptAovPlanes VptBakeDesc VptBakeStats VptBvhRebuild VptCamera VptDenoise
VptDisplay VptEnvironment VptError VptFrame VptInstance VptInstanceEdit VptLayout VptMaterial VptParams VptPick VptSceneDescBvh
VptSceneDescImplicit VptSceneDescLights VptSceneDescVoxels VptSceneEdit VptSdf VptSessionParams VptShapeData VptShapeEdit VptTexture
VptTextureEdit VptVolume VptVolumeEdit VptVolumeInstance VptVolumeSource bake_sdf bake_sdf_grid bake_triangles box3_device build_bvh
catmullclark denoise_device denoise_render denoise_scratch_bytes device_count displace_vertices encode_jpeg_q75 fit_volume get_render
get_render_hits half_variance half_variance_device hip host layout_pixel_index layout_slots linear_to_srgb8 make_state_jump mesh
pathtrace_guides resolve_device resolve_hits_device resolve_ids_device resolve_srgb8_device save_volume selftest_reciprocal state_download
state_init_device state_upload tonemap_device tonemap_image upscale_device upscale_preview vertex_normals""".split()


def test_every_public_name_is_still_exported(vpt):
    assert PUBLIC == sorted(PUBLIC) and len(PUBLIC) == 104
    missing = [name for name in PUBLIC if not hasattr(vpt, name)]
    assert not missing, f"no longer exported: {missing}"


@pytest.mark.parametrize("name", ["HostScene", "DeviceScene", "RenderSession", "SceneEdit", "VptError"])
def test_a_class_is_one_object_however_it_is_reached(vpt, name):
    cls = getattr(vpt, name)
    assert getattr(sys.modules[cls.__module__], name) is cls
    assert cls.__module__ == vpt.__name__ or cls.__module__.startswith(vpt.__name__ + ".")
    for modname, mod in list(sys.modules.items()):
        if modname.startswith(vpt.__name__ + ".") and hasattr(mod, name):
            assert getattr(mod, name) is cls, f"{modname}.{name} is another object than vpt.{name}"


def test_an_error_of_the_host_library_is_caught_as_vpt_error(vpt):
    with pytest.raises(vpt.VptError):
        vpt.HostScene(os.path.join(GOLDEN, "no_such_scene.json"))
    with pytest.raises(vpt.VptError):
        vpt.save_volume(os.path.join(GOLDEN, "unused.sdf"), np.zeros((2, 2), F), 1.0)


# ---- the edits, from literals -------------------------------------------------------------------------------------------------------
FRAME = np.array([1, 0, 0, 0, 0.5, 0, 0, 0, 2, 0.25, -0.75, 3], F)
TRIANGLE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
UP = np.array([[0, 0, 1]] * 3, F)


def _frame(vpt, values=FRAME):
    f = vpt.VptFrame()
    C.memmove(C.byref(f), np.ascontiguousarray(values, F).ctypes.data, 48)
    return f


def _camera(vpt):
    return vpt.VptCamera(_frame(vpt), 1, 0.05, 0.036, 1.5, 10.0, 0.125)


def _material(vpt):
    m = vpt.VptMaterial(type=5, roughness=0.25, metallic=0.5, ior=1.5, scanisotropy=-0.25, trdepth=0.01, opacity=0.75, emission_tex=-1,
                        color_tex=2, roughness_tex=-1, scattering_tex=3, normal_tex=-1)
    m.emission[:], m.color[:], m.scattering[:] = (1, 2, 3), (0.5, 0.25, 0.125), (0.75, 0.5, 0.25)
    return m


def _environment(vpt):
    e = vpt.VptEnvironment(_frame(vpt), emission_tex=1)
    e.emission[:] = (0.5, 1, 2)
    return e


def _sdf(vpt):
    f = vpt.VptSdf(_frame(vpt), 4, 2)
    f.whd[:], f.p[:] = (1, 2, 3), (0.5, 0.25, 0, 0)
    return f


def _volumes(vpt):
    voxels = np.arange(8, dtype=F).reshape(2, 2, 2)
    return {0: vpt.VolumeSource((2, 2, 2), 0.5, (0, 0, 0), (2, 2, 2), vpt.VOXELS_REPLACE, voxels),
            1: vpt.VolumeSource((4, 3, 2), 0.25, (1, 0, 0), (2, 3, 2), vpt.VOXELS_UNION, None, (TRIANGLE, [[0, 1, 2]], (0.5, 0, -0.5), 0.125))}


EDITS = {
    "scene": lambda vpt: vpt.SceneEdit(cameras={1: _camera(vpt)}, instances={2: FRAME}, environments={0: FRAME[::-1]}, materials={3: _material(vpt)},
                                       shapes={4: (TRIANGLE, UP), 5: (TRIANGLE * F(2), None)}),
    "scene_empty": lambda vpt: vpt.SceneEdit(),
    "texture": lambda vpt: vpt.TextureEdit(environments={0: _environment(vpt)},
                                           textures={1: (np.array([[[1, 2, 3, 4], [5, 6, 7, 8]]], np.uint8), False),
                                                     2: (np.array([[[0.5, 0.25, 2, 1]]], F), True)}),
    "texture_empty": lambda vpt: vpt.TextureEdit(),
    "volume": lambda vpt: vpt.VolumeEdit(vol_instances={1: vpt.VptVolumeInstance(_frame(vpt), 1, 2, 0.5)}, sdfs={0: _sdf(vpt)}, volumes=_volumes(vpt)),
    "volume_empty": lambda vpt: vpt.VolumeEdit(),
    "instance": lambda vpt: vpt.InstanceEdit(remove=(2,), set={0: (FRAME, 1, 2)}, add=[(FRAME[::-1], 0, 1)]),
    "instance_empty": lambda vpt: vpt.InstanceEdit(),
    "shape": lambda vpt: vpt.ShapeEdit(remove=(1,), set={0: dict(positions=TRIANGLE, triangles=[[0, 1, 2]], normals=UP)},
                                       add=[dict(positions=TRIANGLE[:2], lines=[[0, 1]], radius=[0.125, 0.25])]),
    "shape_empty": lambda vpt: vpt.ShapeEdit(),
    "rebuild": lambda vpt: vpt.BvhRebuild((1, 2), True, quality=1),
    "rebuild_empty": lambda vpt: vpt.BvhRebuild((), False),
}


def _is_pointer(t):
    return t is C.c_void_p or t is C.c_char_p or issubclass(t, C._Pointer)


def struct_bytes(s) -> bytes:
    """the bytes of a ctypes structure, every pointer in it (nested structures included) written as 1 (not null) or 0"""
    out = bytearray(bytes(s))

    def walk(cls, base):
        for name, t in cls._fields_:
            d = getattr(cls, name)
            if _is_pointer(t):
                null = all(b == 0 for b in out[base + d.offset:base + d.offset + d.size])
                out[base + d.offset:base + d.offset + d.size] = (0 if null else 1).to_bytes(d.size, "little")
            elif issubclass(t, C.Structure):
                walk(t, base + d.offset)
    walk(type(s), 0)
    return bytes(out)


def blobs(obj) -> list:
    """the bytes of everything an edit keeps alive for its struct, one entry per array"""
    if obj is None:
        return []
    if isinstance(obj, np.ndarray):
        return [str(obj.dtype).encode() + b":" + obj.tobytes()]
    if isinstance(obj, C.Structure):
        return [type(obj).__name__.encode() + b":" + struct_bytes(obj)]
    if isinstance(obj, C.Array):
        if issubclass(obj._type_, C.Structure):
            return [type(obj[0]).__name__.encode() + b"[]:" + b"".join(struct_bytes(x) for x in obj)]
        return [b"pointers:" + bytes(1 if x else 0 for x in obj)] if _is_pointer(obj._type_) else [b"array:" + bytes(obj)]
    if isinstance(obj, dict):
        return [b for k in obj for b in blobs(obj[k])]
    if isinstance(obj, (list, tuple)):
        return [b for x in obj for b in blobs(x)]
    raise TypeError(f"an edit keeps a {type(obj).__name__} alive")


def abi_record(vpt, name):
    """(struct bytes, what it keeps alive as a sorted list of byte strings: the order things are kept in is nobody's business)"""
    abi, keep = EDITS[name](vpt).to_abi()
    return struct_bytes(abi), sorted(blobs(keep))


@pytest.mark.parametrize("name", list(EDITS))
def test_to_abi_gives_the_recorded_bytes(vpt, name):
    abi, keep = abi_record(vpt, name)
    with np.load(RECORD) as rec:
        assert abi == rec[name + ".abi"].tobytes(), f"{name}: the struct differs"
        want = [rec[f"{name}.keep{i}"].tobytes() for i in range(int(rec[name + ".count"]))]
    assert len(keep) == len(want), f"{name}: keeps {len(keep)} arrays alive, not {len(want)}"
    for i, (a, b) in enumerate(zip(keep, want)):
        assert a == b, f"{name}: kept array {i} differs: {a[:24]!r}..."
    assert EDITS[name](vpt).empty() == name.endswith("_empty")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vpt_loader
    package = vpt_loader.load()
    record = {}
    for case in EDITS:
        struct, kept = abi_record(package, case)
        record[case + ".abi"] = np.frombuffer(struct, np.uint8)
        record[case + ".count"] = np.int64(len(kept))
        for n, blob in enumerate(kept):
            record[f"{case}.keep{n}"] = np.frombuffer(blob, np.uint8)
    np.savez_compressed(RECORD, **record)
    print(f"{RECORD}: {len(record)} arrays, {os.path.getsize(RECORD)} bytes")

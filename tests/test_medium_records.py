"""A volumetric path's medium as a material id (vpt_device.h: medium records; vpt_mesh_kernel.hip.h: `med`).  K1 carries one word
per path and reads density, scattering, emission and anisotropy of the medium from a record per material after the BVH query;
the general instance (a scene whose media vary over the surface, or VPT_MEDIUM_REGS=1) carries the ten values themselves, copied
at the hit where the path entered.  Everything here is equality of bits, except the one case against the reference, which is held
the way tests/test_gpu_parity.py holds its cases."""
import json
import os

import numpy as np
import pytest

import light_edits as L
from conftest import GOLDEN
from kat_lib import OPS
from test_gpu_parity import _check_against_reference
from test_scene_update_gpu import same_state

pytestmark = pytest.mark.gpu

VOLUMETRIC_TYPES = {"refractive", "subsurface", "volumetric"}   # is_volumetric_type (vpt_scene.hip.h)


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


@pytest.mark.parametrize("scene_file", [L.S03, L.LOBES, L.HEAD])
def test_records_hold_what_a_hit_on_the_material_evaluates(vpt, scene_file):
    """the ten floats of every volumetric-type material's record against the device's own material evaluation at hits on an
    instance of that material (the KAT surface op: eval_surface_point, what K1 calls), bit for bit"""
    host = vpt.HostScene(path(scene_file))
    dev = vpt.DeviceScene(host, 0)
    assert not dev.media_vary()
    records = dev.get_media()
    assert records.shape == (host.count("materials"), 12)
    instance_of = {}
    for i in range(host.count("instances")):
        instance_of.setdefault(host.instance_ids(i)[1], i)
    checked = 0
    for material in range(host.count("materials")):
        if vpt.MATERIAL_TYPES[host.material(material).type] not in VOLUMETRIC_TYPES or material not in instance_of:
            continue
        rows = np.float32([[instance_of[material], element, u, v, 0.0, 0.0, 1.0] for element in (0, 1, 5) for u, v in ((0.25, 0.5), (0.0, 0.0), (0.7, 0.1))])
        out = dev.kat(OPS["surface"][0], rows)
        for o in out:   # density, scattering, emission, scanisotropy of the material point (include/vpt_kat.h)
            entry = np.concatenate([o[17:20], o[20:23], o[7:10], o[23:24]]).astype(np.float32)
            assert np.array_equal(records[material, :10].view(np.uint32), entry.view(np.uint32)), (scene_file, material, records[material], entry)
        assert not records[material, 10:].any()
        checked += 1
    assert checked >= 1
    if scene_file == L.S03:
        assert checked == 5 and records[:, :3].any()   # glass, jade, smoke, cloud, skin: densities from a logarithm


@pytest.mark.parametrize("scene_file", [L.S03, L.LOBES])   # the second runs the trip-spanning instance: pending and current medium in one word
def test_table_form_equals_register_form(vpt, monkeypatch, scene_file):
    """128 wide, 8 spp, 64 bounces: waves with lanes in different media, in none and entering one.  VPT_MEDIUM_REGS is read per launch."""
    host = vpt.HostScene(path(scene_file))
    dev = vpt.DeviceScene(host, 0)
    # which instance a scene runs is decided by its lights (vpt_render.hip: launch_mesh_instance): an emissive mesh of more than one
    # BVH leaf (more than four elements) makes sample_lights_pdf span trips - 03_volume_lobes has one, 03_volume has quads only.
    # No entry point names the instance; this is the rule of build_lights, restated, so that a change of the scenes shows here
    lights, _ = dev.get_lights()
    assert bool(((lights["instance"] >= 0) & (lights["cdf_len"] > 4)).any()) == (scene_file == L.LOBES)
    assert not dev.media_vary()   # else both renders below would take the general instance
    p = vpt.PathtraceParams(resolution=128, samples=8, shader="volpathtrace", bounces=64)
    a, b = host.make_state(p), host.make_state(p)
    dev.pathtrace_samples(a, p, 8)
    monkeypatch.setenv("VPT_MEDIUM_REGS", "1")
    dev.pathtrace_samples(b, p, 8)
    monkeypatch.delenv("VPT_MEDIUM_REGS")
    assert a.samples == b.samples == 8 and a.image.any()
    assert same_state(a, b)


def _varying_scene(tmp_path):
    """the 03_volume sphere with a volumetric material whose colour (hence density) and scattering follow the uv grid, over the
    floor, one area light and the sky"""
    src = os.path.join(GOLDEN, "scenes")
    os.symlink(os.path.join(src, "03_volume", "shapes"), tmp_path / "shapes")
    os.symlink(os.path.join(src, "03_volume", "textures"), tmp_path / "textures")
    os.symlink(os.path.join(src, "shared_textures"), tmp_path / "shared_textures")
    d = json.load(open(path(L.S03)))
    d["textures"].append({"name": "uvgrid", "uri": "shared_textures/uvgrid.png"})
    grid = len(d["textures"]) - 1
    keep = ("floor", "arealight1")
    d["materials"] = [m for m in d["materials"] if m["name"] in keep]
    d["materials"].append({"name": "patchy", "type": "volumetric", "color": [0.6, 0.6, 0.6], "color_tex": grid, "scattering": [0.7, 0.7, 0.7],
                           "scattering_tex": grid, "trdepth": 0.05})
    names = [m["name"] for m in d["materials"]]
    old = json.load(open(path(L.S03)))["instances"]
    d["instances"] = [dict(i, material=names.index(i["name"])) for i in old if i["name"] in keep]
    d["instances"].append({"name": "patchy", "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], "shape": 1, "material": names.index("patchy")})
    out = tmp_path / "varying.json"
    json.dump(d, open(out, "w"))
    return str(out)


# Floors on the shares of (identical streams, pixels matching the reference, stable pixels), set as tests/test_gpu_parity.py sets
# its own: just under what MI355X measures on this case - 0.9951, 0.9948 and 0.9742 (the test prints them).  The strict part of the
# check is what holds the device to the reference: no pixel that is stable under 1-ulp nudges of the reference's libm may differ.
# Why the identical share is below the 1.0000 of the 03_volume cases: a density is -logf(colour) / trdepth, and the device's logf is
# not the host's.  On 03_volume that is five constants, one of which differs in the last bits; here it is a texel, 1 342 distinct
# operands among 20 000 hits, and the density differs from the oracle's (by at most 3 ulp) at 0.969 of the hits (the KAT surface op,
# device against oracle: profiles/r05_varying_medium_density_device_vs_oracle.txt).  A density a few ulp off moves the free-flight
# distance, and a path that runs near a decision takes the other branch: such pixels are the ones the nudged oracle marks
# unstable (stream 0.0221, radiance 0.0042 of the frame), and the 19 pixels that differ are all among them.
VARYING_FLOORS = (0.992, 0.992, 0.965)


def test_a_varying_medium_replays_the_reference(vpt, oracle, monkeypatch, tmp_path):
    host = vpt.HostScene(_varying_scene(tmp_path))
    dev = vpt.DeviceScene(host, 0)
    assert dev.media_vary()   # the flag launch_mesh_instance routes on: the general instance, the medium in registers, copied at the entry hit
    p = vpt.PathtraceParams(resolution=96, samples=8, shader="volpathtrace", bounces=16)
    g, ref = host.make_state(p), host.make_state(p)
    dev.pathtrace_samples(g, p, 8)
    oracle.oracle_render(host, p, ref, 8, nthreads=0)
    _check_against_reference(oracle, host, p, 8, g, ref.image, ref.rngs, "varying_vol_96_8", *VARYING_FLOORS)
    # entry values do vary here: the records (one value per material) are not what the paths carried
    rows = np.float32([[2, e, 0.3, 0.3, 0.0, 0.0, 1.0] for e in range(0, 6144, 97)])
    assert len(np.unique(dev.kat(OPS["surface"][0], rows)[:, 17], axis=0)) > 1


def test_edits_reach_the_records(vpt):
    """smoke's emission through vpt_scene_update_lights (the sphere becomes a light with a BVH: the table is made anew), then the
    glass's colour through vpt_scene_update (the table stays, a density changes): each time the records and the state after 8 spp
    at 96 wide equal those of a scene created from the edited description"""
    host = vpt.HostScene(path(L.S03))
    dev = vpt.DeviceScene(vpt.HostScene(path(L.S03)), 0)
    before = dev.get_media()
    p = vpt.PathtraceParams(resolution=96, samples=8, shader="volpathtrace", bounces=64)
    smoke, glass = L.index_of(L.S03, "materials", "smoke"), L.index_of(L.S03, "materials", "glass")

    def check(what):
        fresh = vpt.DeviceScene(host, 0)
        assert dev.get_media().tobytes() == fresh.get_media().tobytes(), what
        a, b = host.make_state(p), host.make_state(p)
        dev.pathtrace_samples(a, p, 8)
        fresh.pathtrace_samples(b, p, 8)
        assert same_state(a, b), what
        return a

    L.emit(host, smoke, (0.5, 0.25, 0.125))
    dev.update_lights(host.update_lights())
    assert np.array_equal(dev.get_media()[smoke, 6:9], np.float32([0.5, 0.25, 0.125])) and not before[smoke, 6:9].any()
    lit = check("emission")
    m = host.material(glass)
    m.color[0], m.color[1], m.color[2] = 0.5, 1.0, 0.5
    host.set_material(glass, m)
    dev.update(host.update_bvh())
    assert not np.array_equal(dev.get_media()[glass, :3], before[glass, :3])
    assert not same_state(check("colour"), lit)

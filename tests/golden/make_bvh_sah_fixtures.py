"""Fixtures that pin the host mirror's SAH build (build_bvh / make_bvh at quality VPT_BVH_SAH, and through it vpt_build_bvh_quality and
vpt_scene_rebuild_bvh_quality) to the reference itself.  Run by hand where `make -C oracle ref` has left oracle/_ref/obj/: the driver
below - a few lines over the reference's public make_bvh(..., highquality = true) - is compiled in a temporary directory against those
objects and the reference's headers with the flags of oracle/Makefile, and run on the golden scenes (make_bvh(scene, true, false, true)
after load_scene and tesselate_surfaces) and on binary files of points and radii (make_bvh(shape, true, false)) written from
tests/bvh_sah_shapes.py.  It prints node counts and the FNV hashes that ref_driver --stats prints; only
tests/golden/bvh_sah_stats.json is kept.  The tie case is searched for here: the first seed of bvh_sah_shapes.tie whose root has
two candidates of equal least cost and different left sets."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bvh_sah_shapes as S  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
OBJS = ["yocto_bvh", "yocto_scene", "yocto_image", "yocto_shape", "yocto_modelio", "yocto_sceneio", "yocto_cli", "stb_image", "tinyexr", "yocto_sdfs", "yocto_pathtrace"]
CXXFLAGS = ["-O2", "-DNDEBUG", "-std=c++17", "-w", "-fPIC"]   # oracle/Makefile
SCENES = {
    "05_head1ss_sub": "05_head1ss_sub/head1ss_sub.json", "03_volume": "03_volume/volume.json", "09_curves_synth/curves": "09_curves_synth/curves.json",
    "09_curves_synth/dense": "09_curves_synth/dense.json", "01_surface_min": "01_surface_min/surface_min.json",
}

DRIVER = r"""
#include <yocto/yocto_bvh.h>
#include <yocto/yocto_sceneio.h>
#include <yocto_pathtrace/yocto_pathtrace.h>
#include <cstdio>
#include <cstring>
using namespace yocto;
static unsigned long long fnv(const void* data, size_t n) {
  auto p = (const unsigned char*)data;
  auto h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}
template <typename T> static unsigned long long fnv(const std::vector<T>& v) { return fnv(v.data(), v.size() * sizeof(T)); }
static void tree(const bvh_data& b) { printf("{\"nodes\": %zu, \"nodes_fnv\": \"%016llx\", \"prims_fnv\": \"%016llx\"}", b.nodes.size(), fnv(b.nodes), fnv(b.primitives)); }
int main(int argc, const char** argv) {
  static_assert(sizeof(bvh_node) == 32, "node layout");
  if (argc == 3 && !strcmp(argv[1], "scene")) {
    auto scene = scene_data{};
    auto error = std::string{};
    if (!load_scene(argv[2], scene, error)) return fprintf(stderr, "%s\n", error.c_str()), 1;
    tesselate_surfaces(scene);
    auto bvh = make_bvh(scene, true, false, true);
    printf("{\"scene_bvh\": "), tree(bvh), printf(", \"shapes\": [");
    for (size_t i = 0; i < bvh.shapes.size(); i++) printf(i ? ", " : ""), tree(bvh.shapes[i]);
    return printf("]}\n"), 0;
  }
  if (argc == 3 && !strcmp(argv[1], "points")) {
    auto f = fopen(argv[2], "rb");
    auto n = 0;
    if (!f || fread(&n, 4, 1, f) != 1) return 1;
    auto shape = shape_data{};
    shape.positions.resize(n), shape.radius.resize(n), shape.points.resize(n);
    if (fread(shape.positions.data(), 12, n, f) != (size_t)n || fread(shape.radius.data(), 4, n, f) != (size_t)n) return 1;
    for (auto i = 0; i < n; i++) shape.points[i] = i;
    return tree(make_bvh(shape, true, false)), printf("\n"), 0;
  }
  return 1;
}
"""


def find_tie():
    for seed in range(10000):
        costs = S.root_costs(S.boxes(*S.tie(seed)))
        finite = [c for c in costs if c[2] < np.finfo(np.float32).max]
        if not finite:
            continue
        least = min(c[2] for c in finite)
        if len({c[3] for c in finite if c[2] == least}) > 1:
            return seed
    raise SystemExit("no tie found")


def main():
    assert os.path.isdir(OBJ), "build the reference's objects first (make -C oracle ref)"
    out = {"scenes": {}, "points": {}}
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", *CXXFLAGS, f"-I{REF}/libs", f"-I{REF}/libs/yocto", f"-I{REF}/libs/yocto/ext", os.path.join(tmp, "driver.cpp"),
                               *[os.path.join(OBJ, o + ".o") for o in OBJS], "-o", exe, "-lpthread"])
        for name, rel in SCENES.items():
            out["scenes"][name] = json.loads(subprocess.check_output([exe, "scene", os.path.join(HERE, "scenes", rel)]))
            print(name, out["scenes"][name]["scene_bvh"], flush=True)
        out["tie_seed"] = find_tie()
        shapes = dict(S.SHAPES)
        shapes["tie"] = lambda: S.tie(out["tie_seed"])
        for name, make in shapes.items():
            p, r = make()
            with open(os.path.join(tmp, "points.bin"), "wb") as f:
                f.write(np.int32(len(p)).tobytes() + np.ascontiguousarray(p, np.float32).tobytes() + np.ascontiguousarray(r, np.float32).tobytes())
            out["points"][name] = json.loads(subprocess.check_output([exe, "points", os.path.join(tmp, "points.bin")]))
            print(name, out["points"][name], flush=True)
    json.dump(out, open(os.path.join(HERE, "bvh_sah_stats.json"), "w"), indent=1)


if __name__ == "__main__":
    main()

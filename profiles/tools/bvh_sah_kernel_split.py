"""Six rebuilds of every shape of a golden scene at one quality, for a per-kernel trace of the BVH build (the record is
profiles/bvh_sah_kernel_split.txt):

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/tools/bvh_sah_kernel_split.py 05_head1ss_sub/head1ss_sub.json 1"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader
vpt = vpt_loader.load()
path = os.path.join(ROOT, "tests/golden/scenes", sys.argv[1])
q = int(sys.argv[2])
h = vpt.HostScene(path)
A = vpt.DeviceScene(h, 0)
abi, keep = vpt.BvhRebuild(range(h.count("shapes")), True).to_abi()
for r in range(6):
    vpt._check(vpt.hip.vpt_scene_rebuild_bvh_quality(A.handle, C.byref(abi), q), "rebuild")
print("done", A.update_stats())

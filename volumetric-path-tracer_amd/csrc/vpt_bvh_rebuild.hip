// vpt_bvh_rebuild.hip — the BVHs of a resident scene built anew on the device (include/vpt.h: vpt_scene_rebuild_bvh).
// The reference's make_bvh for a scene that lives on a GPU: the element boxes of a named shape come from its leaf records, in
// element order; K6's core (vpt_bvh_build.h) builds the tree from them; the instance boxes come from the new roots and the resident
// frames, and the core builds the scene BVH over them.  No vertex, leaf record or box crosses PCIe.  What depends on topology alone -
// quad order and references, axes, stack needs - is derived on the host from ONE read-back of the new node arrays and primitive
// orders, by the function vpt_scene_create calls (vpt_scene_prep.h: prep_quad_nodes_and_stacks), so the layout keeps one description
// and the traversal limits one decision.
// Everything is built into buffers of its own; the scene's tables are first written (the leaf records, into their new order) after
// the last check has passed, and pointers, counts and mirrors are swapped at the end.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vpt_bvh_build.h"
#include "vpt_bvh_rebuild.h"
#include "vpt_error.h"
#include "vpt_scene_update.h"
#include "vpt_update_helpers.h"

namespace {

// source[k] = the old slot of the element the new slot k holds (both local to the shape)
__global__ void rb_source_slots_kernel(int n, const int* __restrict__ prims, const int* __restrict__ old_slot, int* __restrict__ source) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int e = prims[k];
  source[k] = (e >= 0 && e < n) ? old_slot[e] : k;
}
// The records of a shape from old slot to new slot, every form the scene keeps of them, into a temporary (never in place): `tmp` holds
// 4 n float4 of leaf_prims, then 6 n of leaf_attrs, then - a scene of triangles - 3 n of tri_prims and 4 n of tri_attrs.
__global__ void rb_gather_records_kernel(int n, const int* __restrict__ source, long long leaf_offset, const float4* __restrict__ leaf_prims,
    const float4* __restrict__ leaf_attrs, const float4* __restrict__ tri_prims, const float4* __restrict__ tri_attrs, float4* __restrict__ tmp) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int s = source[k];
  if (s < 0 || s >= n) return;
  const long long from = leaf_offset + s;
  float4* out = tmp;
  for (int c = 0; c < 4; c++) out[4 * (long long)k + c] = leaf_prims[4 * from + c];
  out += 4 * (long long)n;
  for (int c = 0; c < 6; c++) out[6 * (long long)k + c] = leaf_attrs[6 * from + c];
  if (!tri_prims) return;
  out += 6 * (long long)n;
  for (int c = 0; c < 3; c++) out[3 * (long long)k + c] = tri_prims[3 * from + c];
  out += 3 * (long long)n;
  for (int c = 0; c < 4; c++) out[4 * (long long)k + c] = tri_attrs[4 * from + c];
}

struct built_shape {   // one named shape's new tree, on the device until the swap
  int              id = 0, count = 0;
  device_buffer    nodes, source;   // vpt_bvh_node[count]; int[num_elems]: old slot per new slot
  std::vector<int> prims;           // the new primitive order, read back
};

}  // namespace

int scene_level_build(resident& r, bvh_build_scratch& core, const DInstance* instances, int ninst, const DShape* shapes, scene_level& lv, int quality) {
  lv.num_instances = ninst;
  if (int rc = lv.inst_box.allocate((size_t)ninst * 2 * sizeof(float4))) return rc;
  if (int rc = upd_instance_boxes(r, instances, ninst, shapes, lv.inst_box.get<float4>())) return rc;
  if (int rc = bvh_build_core(core, lv.inst_box.get<float>(), 8, ninst, &lv.count, &r.last_launches, quality)) return rc;
  if (int rc = lv.nodes.allocate((size_t)lv.count * sizeof(vpt_bvh_node))) return rc;
  if (int rc = lv.prims.allocate((size_t)ninst * sizeof(int))) return rc;
  if (int rc = copy_on_device(lv.nodes.get(), core.nodes(), (size_t)lv.count * sizeof(vpt_bvh_node))) return rc;
  if (int rc = copy_on_device(lv.prims.get(), core.primitives(), (size_t)ninst * sizeof(int))) return rc;
  if (int rc = fetch(r, lv.h_nodes, lv.nodes.get(), (size_t)lv.count)) return rc;
  if (int rc = fetch(r, lv.h_prims, lv.prims.get(), (size_t)ninst)) return rc;
  for (int k = 0; k < ninst; k++)
    if (lv.h_prims[(size_t)k] < 0 || lv.h_prims[(size_t)k] >= ninst) return vpt_set_error(VPT_ERR_HIP, "bvh rebuild: the scene's primitive order is not a permutation");
  return VPT_OK;
}

int scene_level_enter(resident& r, scene_level& lv, const scene_tables& t, const int* inst_shape, const DInstance* instances, const DShape* shapes) {
  const int ninst = lv.num_instances, scene_quads = (int)(t.scene_wnodes / 8);
  std::vector<float4> enter((size_t)ninst * 6, make_float4(0, 0, 0, 0));
  lv.slot_of.assign((size_t)ninst, -1);
  for (int k = 0; k < ninst; k++) {
    const int id = lv.h_prims[(size_t)k];
    prep_enter_tail(&enter[6 * (size_t)k], t.shapes[(size_t)inst_shape[(size_t)id]], scene_quads, id, 0);
    lv.slot_of[(size_t)id] = k;
  }
  if (int rc = send(r, lv.enter, enter)) return rc;
  if (int rc = send(r, lv.d_slot_of, lv.slot_of)) return rc;
  return upd_enter_records(r, lv.enter.get<float4>(), ninst, instances, shapes);
}

void scene_level_swap(resident& r, scene_level& lv, const scene_tables& t) {
  DScene& d = r.d;
  const struct { const void* old; device_buffer* fresh; } swaps[5] = {{d.scene_nodes, &lv.nodes}, {d.scene_prims, &lv.prims}, {d.scene_wnodes, &lv.wnodes},
      {d.scene_enter, &lv.enter}, {d.slot_of_instance, &lv.d_slot_of}};
  d.scene_nodes = lv.nodes.get<const float4>(), d.scene_prims = lv.prims.get<const int>();
  d.scene_wnodes = lv.wnodes.get<const float4>(), d.shape_wnodes = d.scene_wnodes + t.scene_wnodes;
  d.scene_enter = lv.enter.get<const float4>(), d.slot_of_instance = lv.d_slot_of.get<const int>();
  for (const auto& s : swaps) adopt(r.tables, s.old, std::move(*s.fresh));
  d.num_scene_nodes = lv.count, d.num_scene_prims = lv.num_instances, d.scene_root_ref = t.d.scene_root_ref;
  d.scene_root_lo_x = t.d.scene_root_lo_x, d.scene_root_lo_y = t.d.scene_root_lo_y, d.scene_root_lo_z = t.d.scene_root_lo_z;
  d.scene_root_hi_x = t.d.scene_root_hi_x, d.scene_root_hi_y = t.d.scene_root_hi_y, d.scene_root_hi_z = t.d.scene_root_hi_z;
  r.h.slot_of = lv.slot_of;
  r.scene_depth = t.scene_depth, r.scene_need4 = t.scene_need4;
  r.refit.ready = false;   // levels and quad slots belong to the old trees: the next refit makes them anew
}

int bvh_rebuild_apply(resident& r, const vpt_bvh_rebuild& w, edit_outcome& out, int quality) {
  if (quality != VPT_BVH_MIDDLE && quality != VPT_BVH_SAH) return vpt_set_error(VPT_ERR_INVALID_ARG, "unknown bvh quality %d", quality);
  DScene&       d = r.d;
  host_mirrors& h = r.h;
  edit_mirrors& m = r.m;
  // every refusal about the request happens here: nothing has been written
  if (int rc = check_ids("shape", w.num_shapes, w.shape_ids, d.num_shapes)) return rc;
  if (w.num_shapes == 0 && !w.scene) return VPT_OK;
  if (int rc = begin_update(r)) return rc;
  const int ninst = d.num_instances, nshapes = d.num_shapes;

  // scratch sized once, for the largest BVH of the call
  int most = ninst, most_elems = 0;
  for (int i = 0; i < w.num_shapes; i++) most_elems = std::max(most_elems, m.shapes[(size_t)w.shape_ids[i]].num_elems);
  most = std::max(most, most_elems);
  bvh_build_scratch core;
  device_buffer     d_boxes, d_old_slot;
  if (int rc = core.reserve(most, quality)) return rc;
  if (int rc = d_boxes.allocate(6 * (size_t)most_elems * sizeof(float))) return rc;
  if (int rc = d_old_slot.allocate((size_t)most_elems * sizeof(int))) return rc;
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));

  // 1. the named shapes: element boxes from the leaf records, the tree, the slot each new slot takes its records from
  std::vector<built_shape> built((size_t)w.num_shapes);
  std::vector<int>         built_of((size_t)nshapes, -1);
  for (int i = 0; i < w.num_shapes; i++) {
    built_shape&  b  = built[(size_t)i];
    const DShape& sh = m.shapes[(size_t)w.shape_ids[i]];
    const int     n  = sh.num_elems;
    b.id = w.shape_ids[i], built_of[(size_t)b.id] = i;
    if (int rc = upd_element_boxes(r, sh, d_boxes.get<float>(), d_old_slot.get<int>())) return rc;
    if (int rc = bvh_build_core(core, d_boxes.get<float>(), 6, n, &b.count, &r.last_launches, quality)) return rc;
    if (int rc = b.nodes.allocate((size_t)b.count * sizeof(vpt_bvh_node))) return rc;
    if (int rc = b.source.allocate((size_t)n * sizeof(int))) return rc;
    if (int rc = copy_on_device(b.nodes.get(), core.nodes(), (size_t)b.count * sizeof(vpt_bvh_node))) return rc;
    LAUNCH(r, rb_source_slots_kernel, n, n, core.primitives(), d_old_slot.get<int>(), b.source.get<int>());
    if (int rc = fetch(r, b.prims, core.primitives(), (size_t)n)) return rc;   // (after the launch above in stream order)
  }

  // 2. the shape node pool at its new size, contiguous in shape order: new trees and, device to device, the untouched ones
  std::vector<DShape> shapes = m.shapes;
  long long total = 0;
  for (int i = 0; i < nshapes; i++) {
    DShape& sh = shapes[(size_t)i];
    if (built_of[(size_t)i] >= 0) sh.num_nodes = built[(size_t)built_of[(size_t)i]].count;
    if (total + sh.num_nodes > 0x7fffffffLL) return vpt_set_error(VPT_ERR_UNSUPPORTED, "more than 2^31 shape bvh nodes");
    sh.node_offset = (int)total, total += sh.num_nodes;
  }
  device_buffer n_shape_nodes, n_shapes;
  if (int rc = n_shape_nodes.allocate((size_t)total * sizeof(vpt_bvh_node))) return rc;
  for (int i = 0; i < nshapes; i++) {
    const DShape& sh   = shapes[(size_t)i];
    const void*   from = built_of[(size_t)i] >= 0 ? built[(size_t)built_of[(size_t)i]].nodes.get() : (const void*)(d.shape_nodes + 2 * (long long)m.shapes[(size_t)i].node_offset);
    if (int rc = copy_on_device(n_shape_nodes.get<vpt_bvh_node>() + sh.node_offset, from, (size_t)sh.num_nodes * sizeof(vpt_bvh_node))) return rc;
  }
  // the shape records with the new offsets and counts, their root boxes from the new pool: what the instance boxes are made from
  if (int rc = send(r, n_shapes, shapes)) return rc;
  if (int rc = upd_shape_roots(r, n_shapes.get<DShape>(), n_shape_nodes.get<float4>())) return rc;

  // 3. the scene BVH over ALL instances (make_bvh's scene level holds every instance)
  // 4. the one read-back: node arrays (32 B per node) and the scene's primitive order; the topology-only tables from them, by
  // creation's own function - which also decides the traversal limits.  A tree past them is refused here, the scene untouched.
  scene_level lv;
  if (int rc = scene_level_build(r, core, d.instances, ninst, n_shapes.get<DShape>(), lv, quality)) return rc;
  std::vector<vpt_bvh_node> h_shape_nodes;
  if (int rc = fetch(r, h_shape_nodes, n_shape_nodes.get(), (size_t)total)) return rc;
  for (const built_shape& b : built)
    for (int e : b.prims)
      if (e < 0 || e >= (int)b.prims.size()) return vpt_set_error(VPT_ERR_HIP, "bvh rebuild: shape %d: the primitive order is not a permutation", b.id);
  std::vector<vpt_shape> desc_shapes((size_t)nshapes);
  for (int i = 0; i < nshapes; i++) desc_shapes[(size_t)i] = {}, desc_shapes[(size_t)i].bvh_node_offset = shapes[(size_t)i].node_offset, desc_shapes[(size_t)i].num_bvh_nodes = shapes[(size_t)i].num_nodes;
  vpt_scene_desc desc = {};
  desc.num_shapes = nshapes, desc.shapes = desc_shapes.data();
  desc.num_shape_bvh_nodes = total, desc.shape_bvh_nodes = h_shape_nodes.data();
  desc.num_scene_bvh_nodes = lv.count, desc.scene_bvh_nodes = lv.h_nodes.data();
  scene_tables t;
  t.d = d, t.shapes = shapes;
  if (int rc = prep_quad_nodes_and_stacks(desc, t)) return rc;
  // enter records: the integer words on the host, frames and root boxes by the refit's kernel; the slot of every instance
  if (int rc = send(r, lv.wnodes, t.wnodes)) return rc;
  if (int rc = send(r, n_shapes.get<const DShape>(), t.shapes.data(), t.shapes.size())) return rc;   // + wnode_offset, root_ref, stack_need
  if (int rc = scene_level_enter(r, lv, t, h.inst_shape.data(), d.instances, n_shapes.get<DShape>())) return rc;

  // ---- the last check has passed: from here on the scene's own tables are written ------------------------------------------
  // 5. leaf records of the rebuilt shapes into their new order: gathered into a temporary, moved back device to device
  const bool tris = d.tri_prims != nullptr;
  device_buffer d_tmp;
  if (int rc = d_tmp.allocate((size_t)most_elems * (tris ? 17 : 10) * sizeof(float4))) return rc;
  for (const built_shape& b : built) {
    const DShape&   sh = m.shapes[(size_t)b.id];
    const long long n = sh.num_elems, at = sh.leaf_offset;
    float4*         tmp = d_tmp.get<float4>();
    LAUNCH(r, rb_gather_records_kernel, n, (int)n, b.source.get<int>(), at, d.leaf_prims, d.leaf_attrs, d.tri_prims, d.tri_attrs, tmp);
    if (int rc = copy_on_device(mut(d.leaf_prims) + 4 * at, tmp, (size_t)(4 * n) * sizeof(float4))) return rc;
    if (int rc = copy_on_device(mut(d.leaf_attrs) + 6 * at, tmp + 4 * n, (size_t)(6 * n) * sizeof(float4))) return rc;
    if (tris) {
      if (int rc = copy_on_device(mut(d.tri_prims) + 3 * at, tmp + 10 * n, (size_t)(3 * n) * sizeof(float4))) return rc;
      if (int rc = copy_on_device(mut(d.tri_attrs) + 4 * at, tmp + 13 * n, (size_t)(4 * n) * sizeof(float4))) return rc;
    }
    for (int k = 0; k < (int)n; k++) h.prim_slot[(size_t)sh.elem_offset + (size_t)b.prims[(size_t)k]] = sh.leaf_offset + k;
  }

  // 6. the swap: tables, counts, mirrors
  const void* old_shape_nodes = d.shape_nodes, *old_shapes = d.shapes;
  d.shape_nodes = n_shape_nodes.get<const float4>(), d.shapes = n_shapes.get<const DShape>();
  adopt(r.tables, old_shape_nodes, std::move(n_shape_nodes)), adopt(r.tables, old_shapes, std::move(n_shapes));
  scene_level_swap(r, lv, t);
  r.num_shape_nodes = total, m.shapes = t.shapes;
  r.num_shape_wnodes = (long long)t.shape_wnodes, r.shape_depth = t.shape_depths, r.shape_need4 = t.shape_need4s, r.shape_quads = t.shape_quads;
  out.changed = out.topology = true, out.stack_cap = t.stack_cap, out.stack_lds4 = t.stack_lds4, out.stack_spill4 = t.stack_spill4;

  // 7. what hangs on the shapes' root boxes outside the BVHs: the mesh lights' records
  if (int rc = upd_light_records(r, d.shapes)) return rc;
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}

// vpt_subdiv_update.hip — the subdivision surfaces of a resident scene (include/vpt.h: vpt_scene_attach_subdiv, vpt_scene_update_subdivs;
// DESIGN.md §25).  tesselate_surface (yocto_pathtrace.cpp:1230-1273) split as host/vpt_tesselate.cpp splits it: the integer half - the
// levels' topology, split_facevarying's table, the per-vertex face lists - comes once, as a plan, and stays on the device; the float half
// runs here per edit, through the launchers of vpt_subdiv.h, from the cage's floats into staging buffers the refit of vpt_scene_update
// reads as its second source (vpt_scene_update.h: staged_vertices).  Only the cage's floats cross PCIe.
// The one kernel of its own is the gather of split_facevarying; everything else is vpt_subdiv.hip's and vpt_scene_update.hip's.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "vpt_error.h"
#include "vpt_light_update.h"
#include "vpt_scene_update.h"
#include "vpt_subdiv.h"
#include "vpt_subdiv_update.h"
#include "vpt_update_helpers.h"

namespace {

// split_facevarying's copy loops (yocto_shape.cpp:2636-2648): shape vertex v takes position verts[v].x and normal verts[v].y
__global__ void __launch_bounds__(256) subdiv_gather_kernel(int nv, const int* __restrict__ verts, const float* __restrict__ pos, const float* __restrict__ nrm,
    float* __restrict__ out_pos, float* __restrict__ out_nrm) {
  int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int p = verts[3 * v], n = verts[3 * v + 1];
  out_pos[3 * v] = pos[3 * p], out_pos[3 * v + 1] = pos[3 * p + 1], out_pos[3 * v + 2] = pos[3 * p + 2];
  if (nrm) out_nrm[3 * v] = nrm[3 * n], out_nrm[3 * v + 1] = nrm[3 * n + 1], out_nrm[3 * v + 2] = nrm[3 * n + 2];
}

// tesselate_surface's condition for the displacement step, and which pools the shape has afterwards (include/vpt.h)
bool displaced(const subdiv_plan_dev& p, float displacement, int num_elems) { return displacement != 0 && p.displacement_tex >= 0 && num_elems > 0; }
bool has_normals(const subdiv_plan_dev& p, bool is_displaced) { return p.subdivisions > 0 ? p.smooth != 0 : is_displaced ? p.smooth != 0 : p.num_cage_normals > 0; }

size_t aligned(size_t at) { return (at + 15) & ~(size_t)15; }

// the float half of tesselate_surface for one plan; *positions / *normals: where the shape's new vertices are (normals null: it has none)
int tesselate(resident& r, subdiv_plan_dev& p, const float** positions, const float** normals) {
  const DShape& sh = r.m.shapes[(size_t)p.shape];
  const bool fuse = !getenv("VPT_UPDATE_NO_FUSE");   // A/B switch of the tests and measurements, read per call - same bits
  const float* cur = p.cage;
  for (size_t l = 0; l < p.levels.size();) {
    float* a = cur == p.buf0 ? p.buf1 : p.buf0;
    float* b = a == p.buf0 ? p.buf1 : p.buf0;
    subdiv_fused_levels group = {};
    while (fuse && l + (size_t)group.count < p.levels.size() && group.count < SUBDIV_FUSE_LEVELS && refined_vertices(p.levels[l + (size_t)group.count]) <= SUBDIV_FUSE_WIDTH)
      group.L[group.count] = p.levels[l + (size_t)group.count], group.count++;
    if (group.count > 0) {
      r.last_launches += subdiv_launch_levels_fused(group, cur, p.tverts, a, b, 0);
      cur = (group.count & 1) ? a : b, l += (size_t)group.count;
    } else {
      r.last_launches += subdiv_launch_level(3, p.levels[l], cur, p.tverts, a, 0);
      cur = a, l++;
    }
    HIP_TRY(hipGetLastError());
  }
  const float* nrm = p.cage_normals;   // subdivisions == 0: the cage's own, or none
  if (p.subdivisions > 0) {
    nrm = nullptr;
    if (p.smooth) {
      r.last_launches += subdiv_launch_normals(p.num_refined, 4, 4, cur, (const int*)p.quads, p.quad_offsets, p.quad_items, p.refined_normals, 0);
      nrm = p.refined_normals;
    }
  }
  LAUNCH(r, subdiv_gather_kernel, p.num_vertices, p.num_vertices, p.verts, cur, nrm, p.stage_pos, p.stage_nrm);
  *positions = p.stage_pos, *normals = nrm ? p.stage_nrm : nullptr;
  if (!displaced(p, p.displacement, sh.num_elems)) return VPT_OK;
  const int* triangles = (const int*)(r.d.elems + sh.elem_offset);   // int4 per element: a triangle repeats z in w
  if (!nrm) r.last_launches += subdiv_launch_normals(p.num_vertices, 3, 4, p.stage_pos, triangles, p.tri_offsets, p.tri_items, p.stage_nrm, 0);
  const vpt_texture& t = r.m.textures[(size_t)p.displacement_tex];
  const int byte_texture = !t.is_float && (long long)t.width * t.height > 0;   // `!pixelsb.empty()` of the reference
  r.last_launches += subdiv_launch_displace(r.d, p.displacement_tex, byte_texture, p.displacement, p.num_vertices, p.stage_pos, p.stage_nrm,
      (const float*)(r.d.texcoords + sh.texcoord_offset), p.stage_tmp, 0);
  *positions = p.stage_tmp, *normals = nullptr;
  if (p.smooth) {
    r.last_launches += subdiv_launch_normals(p.num_vertices, 3, 4, p.stage_tmp, triangles, p.tri_offsets, p.tri_items, p.stage_nrm, 0);
    *normals = p.stage_nrm;
  }
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

}  // namespace

int subdiv_attach(resident& r, const vpt_subdiv_plan& P, int* id_out) {
  const DScene& d = r.d;
  REQUIRE(id_out, "subdiv plan: null id_out");
  REQUIRE(P.shape >= 0 && P.shape < d.num_shapes, "subdiv plan: shape %d out of range (%d)", P.shape, d.num_shapes);
  REQUIRE(P.subdivisions >= 0 && P.subdivisions <= 10 && P.num_levels == P.subdivisions, "subdiv plan: %d levels for %d subdivisions (0 .. 10)", P.num_levels, P.subdivisions);
  REQUIRE(P.smooth == 0 || P.smooth == 1, "subdiv plan: smooth is 0 or 1");
  REQUIRE(std::isfinite(P.displacement), "subdiv plan: the displacement is not finite");
  REQUIRE(P.displacement_tex >= -1 && P.displacement_tex < d.num_textures, "subdiv plan: displacement_tex %d is neither -1 nor a texture (%d)", P.displacement_tex, d.num_textures);
  REQUIRE(P.num_cage_positions >= 0 && P.num_cage_normals >= 0 && P.num_quads >= 0 && P.num_vertices >= 0, "subdiv plan: negative count");
  REQUIRE((!P.num_cage_positions || P.cage_positions) && (!P.num_cage_normals || P.cage_normals) && (!P.num_levels || P.levels) && (!P.num_quads || P.quads) &&
              (!P.num_vertices || P.verts),
      "subdiv plan: null array with a non-zero count");
  REQUIRE(finite_all(P.cage_positions, 3 * (size_t)P.num_cage_positions), "subdiv plan: a cage position is not finite");
  REQUIRE(finite_all(P.cage_normals, 3 * (size_t)P.num_cage_normals), "subdiv plan: a cage normal is not finite");
  int refined = P.num_cage_positions, widest = 0;
  for (int l = 0; l < P.num_levels; l++) {
    const vpt_subdiv_level& L = P.levels[l];
    REQUIRE(L.dim == 3 && L.num_vertices == refined && L.num_edges >= 0 && L.num_faces >= 0 && L.num_new_faces >= 0 && L.num_items >= 0 &&
                (long long)L.num_vertices + L.num_edges + L.num_faces <= (1ll << 28),
        "subdiv plan: level %d: bad sizes (it takes the %d vertices of the level before)", l, refined);
    REQUIRE(L.valence && L.offsets && (!L.num_edges || L.edges) && (!L.num_faces || L.faces) && (!L.num_new_faces || L.new_faces) && (!L.num_items || L.items),
        "subdiv plan: level %d: null table", l);
    if (int rc = subdiv_check_level_indices(L)) return rc;
    refined = L.num_vertices + L.num_edges + L.num_faces;
    widest  = refined > widest ? refined : widest;
  }
  long long triangles = 0;
  for (int i = 0; i < P.num_quads; i++) {
    for (int c = 0; c < 4; c++) REQUIRE(P.quads[4 * i + c] >= 0 && P.quads[4 * i + c] < refined, "subdiv plan: quad %d refers to vertex %d", i, P.quads[4 * i + c]);
    triangles += P.quads[4 * i + 2] != P.quads[4 * i + 3] ? 2 : 1;
  }
  subdiv_plan_dev p;
  p.shape = P.shape, p.subdivisions = P.subdivisions, p.smooth = P.smooth, p.displacement = P.displacement, p.displacement_tex = P.displacement_tex;
  p.num_cage = P.num_cage_positions, p.num_cage_normals = P.num_cage_normals, p.num_refined = refined, p.num_quads = P.num_quads, p.num_vertices = P.num_vertices;
  const bool normal_index = P.subdivisions > 0 ? P.smooth != 0 : P.num_cage_normals > 0;
  const int  num_normals  = P.subdivisions > 0 ? refined : P.num_cage_normals;
  const bool texcoords    = P.num_vertices > 0 && P.verts[2] >= 0;
  for (int v = 0; v < P.num_vertices; v++) {
    const int32_t* t = P.verts + 3 * (size_t)v;
    REQUIRE(t[0] >= 0 && t[0] < refined, "subdiv plan: vertex %d refers to position %d", v, t[0]);
    REQUIRE(normal_index ? t[1] >= 0 && t[1] < num_normals : t[1] == -1, "subdiv plan: vertex %d refers to normal %d", v, t[1]);
    REQUIRE(texcoords ? t[2] >= 0 : t[2] == -1, "subdiv plan: vertex %d: texcoord index %d where the others %s one", v, t[2], texcoords ? "have" : "have not");
  }
  // against the resident shape
  const DShape& sh = r.m.shapes[(size_t)P.shape];
  REQUIRE(sh.is_triangles || sh.num_elems == 0, "subdiv plan: shape %d does not hold triangles", P.shape);
  REQUIRE(r.h.shape_vertices[(size_t)P.shape] == P.num_vertices, "subdiv plan: %d vertices, shape %d has %d", P.num_vertices, P.shape, r.h.shape_vertices[(size_t)P.shape]);
  REQUIRE(triangles == sh.num_elems, "subdiv plan: its quads make %lld triangles, shape %d has %d", triangles, P.shape, sh.num_elems);
  const bool is_displaced = displaced(p, p.displacement, sh.num_elems);
  REQUIRE(has_normals(p, is_displaced) == (sh.normal_offset >= 0), "subdiv plan: its settings %s normals, shape %d has %s", has_normals(p, is_displaced) ? "make" : "make no",
      P.shape, sh.normal_offset >= 0 ? "some" : "none");
  REQUIRE(texcoords == (sh.texcoord_offset >= 0), "subdiv plan: its vertices %s texcoords, shape %d has %s", texcoords ? "have" : "have no", P.shape,
      sh.texcoord_offset >= 0 ? "some" : "none");
  REQUIRE(!is_displaced || texcoords, "subdiv plan: a displaced subdiv without texture coordinates");
  for (const subdiv_plan_dev& other : r.subdivs) REQUIRE(other.shape != P.shape, "subdiv plan: shape %d has a plan already", P.shape);

  if (int rc = begin_update(r)) return rc;
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  // the lists of quads_normals and triangles_normals (integers, host); the shape's triangles are the resident elements
  std::vector<int> quad_offsets, quad_items, tri_offsets, tri_items;
  const bool quad_lists = P.subdivisions > 0 && P.smooth, tri_lists = P.displacement_tex >= 0;
  if (quad_lists)
    if (int rc = subdiv_face_lists(refined, P.num_quads, 4, 4, P.quads, quad_offsets, quad_items)) return rc;
  if (tri_lists) {
    std::vector<int> elems;
    if (int rc = fetch(r, elems, d.elems + sh.elem_offset, 4 * (size_t)sh.num_elems)) return rc;
    if (int rc = subdiv_face_lists(P.num_vertices, sh.num_elems, 3, 4, elems.data(), tri_offsets, tri_items)) return rc;
  }
  // one block: what is uploaded, then the scratch
  staged_block pay;
  struct level_at { size_t edges, faces, tquads, valence, offsets, items; };
  std::vector<level_at> at((size_t)P.num_levels);
  const size_t at_cage = pay.add(P.cage_positions, 12 * (size_t)P.num_cage_positions), at_cage_nrm = pay.add(P.cage_normals, 12 * (size_t)P.num_cage_normals);
  for (int l = 0; l < P.num_levels; l++) {
    const vpt_subdiv_level& L  = P.levels[l];
    const size_t            nt = (size_t)L.num_vertices + L.num_edges + L.num_faces;
    at[(size_t)l] = {pay.add(L.edges, 8 * (size_t)L.num_edges), pay.add(L.faces, 16 * (size_t)L.num_faces), pay.add(L.new_faces, 16 * (size_t)L.num_new_faces),
        pay.add(L.valence, 4 * nt), pay.add(L.offsets, 4 * (nt + 1)), pay.add(L.items, 4 * (size_t)L.num_items)};
  }
  const size_t at_quads = pay.add(P.quads, quad_lists ? 16 * (size_t)P.num_quads : 0);
  const size_t at_qoff = pay.add(quad_offsets.data(), 4 * quad_offsets.size()), at_qitems = pay.add(quad_items.data(), 4 * quad_items.size());
  const size_t at_verts = pay.add(P.verts, 12 * (size_t)P.num_vertices);
  const size_t at_toff = pay.add(tri_offsets.data(), 4 * tri_offsets.size()), at_titems = pay.add(tri_items.data(), 4 * tri_items.size());
  size_t total = pay.host.size();
  auto room = [&](size_t bytes) {
    const size_t here = aligned(total);
    total = here + bytes;
    return here;
  };
  const size_t at_buf0 = room(12 * (size_t)widest), at_buf1 = room(12 * (size_t)widest), at_tverts = room(12 * (size_t)widest);
  const size_t at_rnrm = room(quad_lists ? 12 * (size_t)refined : 0);
  const size_t at_spos = room(12 * (size_t)P.num_vertices), at_snrm = room(12 * (size_t)P.num_vertices), at_stmp = room(tri_lists ? 12 * (size_t)P.num_vertices : 0);
  if (int rc = p.block.allocate(total)) return rc;
  p.block_bytes = total;
  char* base = p.block.get<char>();
  if (int rc = send(r, (const char*)base, pay.host.data(), pay.host.size())) return rc;
  p.cage = (float*)(base + at_cage), p.cage_normals = P.num_cage_normals ? (const float*)(base + at_cage_nrm) : nullptr;
  p.levels.resize((size_t)P.num_levels);
  for (int l = 0; l < P.num_levels; l++) {
    const vpt_subdiv_level& L = P.levels[l];
    const level_at&         a = at[(size_t)l];
    p.levels[(size_t)l] = {L.num_vertices, L.num_edges, L.num_faces, (const int2*)(base + a.edges), (const int4*)(base + a.faces), (const int4*)(base + a.tquads),
        (const int*)(base + a.valence), (const int*)(base + a.offsets), (const int*)(base + a.items)};
  }
  p.quads = (const int4*)(base + at_quads), p.quad_offsets = (const int*)(base + at_qoff), p.quad_items = (const int*)(base + at_qitems);
  p.verts = (const int*)(base + at_verts), p.tri_offsets = (const int*)(base + at_toff), p.tri_items = (const int*)(base + at_titems);
  p.buf0 = (float*)(base + at_buf0), p.buf1 = (float*)(base + at_buf1), p.tverts = (float*)(base + at_tverts), p.refined_normals = (float*)(base + at_rnrm);
  p.stage_pos = (float*)(base + at_spos), p.stage_nrm = (float*)(base + at_snrm), p.stage_tmp = (float*)(base + at_stmp);
  if (int rc = mark_end(r)) return rc;
  if (int rc = finish_update(r)) return rc;
  size_t slot = 0;
  while (slot < r.subdivs.size() && r.subdivs[slot].shape >= 0) slot++;
  if (slot == r.subdivs.size()) r.subdivs.emplace_back();
  r.subdivs[slot] = std::move(p);
  *id_out = (int)slot;
  return VPT_OK;
}

int subdiv_detach(resident& r, int id) {
  REQUIRE(id >= 0 && id < (int)r.subdivs.size() && r.subdivs[(size_t)id].shape >= 0, "subdiv %d is not attached", id);
  r.subdivs[(size_t)id] = subdiv_plan_dev{};
  return VPT_OK;
}

void subdiv_plans_follow_shapes(resident& r, const std::vector<int>& new_of_old, const std::vector<char>& is_set) {
  for (subdiv_plan_dev& p : r.subdivs) {
    if (p.shape < 0) continue;
    if (is_set[(size_t)p.shape] || new_of_old[(size_t)p.shape] < 0) p = subdiv_plan_dev{};
    else p.shape = new_of_old[(size_t)p.shape];
  }
}

int subdiv_update_apply(resident& r, const vpt_subdiv_edit& e, edit_outcome& out) {
  // every refusal happens here: nothing has been written
  REQUIRE(e.num >= 0 && (e.num == 0 || e.subdiv_ids), "edit: subdiv list is null or has a negative count");
  std::vector<char>  seen(r.subdivs.size(), 0);
  std::vector<float> amount((size_t)e.num);
  for (int i = 0; i < e.num; i++) {
    const int id = e.subdiv_ids[i];
    REQUIRE(id >= 0 && id < (int)r.subdivs.size(), "edit: subdiv entry %d: id %d out of range (%d)", i, id, (int)r.subdivs.size());
    REQUIRE(!seen[(size_t)id], "edit: subdiv entry %d: id %d repeated", i, id);
    seen[(size_t)id] = 1;
    const subdiv_plan_dev& p = r.subdivs[(size_t)id];
    REQUIRE(p.shape >= 0, "edit: subdiv entry %d: subdiv %d is not attached", i, id);
    const float* cage = e.cage_positions ? e.cage_positions[i] : nullptr;
    REQUIRE(!cage || finite_all(cage, 3 * (size_t)p.num_cage), "edit: subdiv entry %d: a cage position is not finite", i);
    const float given = e.displacement ? e.displacement[i] : NAN;
    REQUIRE(std::isnan(given) || std::isfinite(given), "edit: subdiv entry %d: the displacement is not finite", i);
    amount[(size_t)i] = std::isnan(given) ? p.displacement : given;
  }
  bool lit = false;
  for (int i = 0; i < e.num; i++) {
    const subdiv_plan_dev& p  = r.subdivs[(size_t)e.subdiv_ids[i]];
    const DShape&          sh = r.m.shapes[(size_t)p.shape];
    const bool is_displaced = displaced(p, amount[(size_t)i], sh.num_elems);
    if (has_normals(p, is_displaced) != (sh.normal_offset >= 0))
      return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: subdiv entry %d: a displacement switched between zero and non-zero would %s the normals of shape %d (an edit of vpt_scene_update_shapes)",
          i, sh.normal_offset >= 0 ? "drop" : "add", p.shape);
    if (is_displaced && sh.texcoord_offset < 0) return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: subdiv entry %d: a displaced subdiv needs the texcoords shape %d has not", i, p.shape);
    lit = lit || r.m.shape_lit[(size_t)p.shape];
  }
  if (int rc = begin_update(r)) return rc;
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  staged_vertices  staged;
  std::vector<int> shape_ids((size_t)e.num);
  for (int i = 0; i < e.num; i++) {
    subdiv_plan_dev& p = r.subdivs[(size_t)e.subdiv_ids[i]];
    if (e.cage_positions && e.cage_positions[i])
      if (int rc = send(r, (const float*)p.cage, e.cage_positions[i], 3 * (size_t)p.num_cage)) return rc;
    p.displacement = amount[(size_t)i];
    const float *pos = nullptr, *nrm = nullptr;
    if (int rc = tesselate(r, p, &pos, &nrm)) return rc;
    staged.positions.push_back(pos), staged.normals.push_back(nrm);
    shape_ids[(size_t)i] = p.shape;
  }
  vpt_scene_edit refit = {};
  refit.num_shapes = e.num, refit.shape_ids = shape_ids.data();
  if (int rc = scene_update_apply(r, refit, out, lit, &staged)) return rc;
  if (lit) return light_update_apply(r, refit, &out.lights_rebuilt);
  return VPT_OK;
}

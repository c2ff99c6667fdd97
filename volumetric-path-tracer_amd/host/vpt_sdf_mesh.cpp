// vpt_sdf_mesh.cpp — a quad mesh out of a signed-distance voxel grid on the CPU: the rule of include/vpt.h (vpt_mesh_sdf) through the same
// header as the kernels (csrc/vpt_sdf_mesh_rule.h) in plain serial loops, one voxel after another in index order - the statement the
// kernels are held to bit for bit; the same on a GPU through the C-ABI; and a binary PLY writer for what comes out.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "vpt_host.h"
#include "vpt_sdf_mesh_rule.h"

namespace vpt {

sdf_mesh mesh_sdf(const float* voxels, const vpt_sdf_mesh_desc& desc, const vpt_sdf_mesh_region* region) {
  if (!voxels) throw std::invalid_argument{"mesh_sdf: null voxels"};
  if (auto fault = vpt_sdf_mesh_desc_fault(desc)) throw std::invalid_argument{string{"mesh_sdf: "} + fault};
  if (region)
    if (auto fault = vpt_sdf_mesh_region_fault(*region, desc.whd)) throw std::invalid_argument{string{"mesh_sdf: "} + fault};
  const int lo[3]  = {region ? region->lo[0] : 0, region ? region->lo[1] : 0, region ? region->lo[2] : 0};
  const int dim[3] = {region ? region->whd[0] : desc.whd[0], region ? region->whd[1] : desc.whd[1], region ? region->whd[2] : desc.whd[2]};
  auto mesh = sdf_mesh{};
  if (dim[0] < 2 || dim[1] < 2 || dim[2] < 2) return mesh;
  const auto W = (size_t)desc.whd[0], H = (size_t)desc.whd[1];
  auto       at = [&](int x, int y, int z) { return voxels[(size_t)(lo[0] + x) + (size_t)(lo[1] + y) * W + (size_t)(lo[2] + z) * W * H]; };
  const long long stride[3] = {1, dim[0], (long long)dim[0] * dim[1]};
  auto flags = vector<unsigned char>((size_t)stride[2] * (size_t)dim[2], 0);
  auto ids   = vector<int>(flags.size(), -1);
  // the cells and the edges, voxel by voxel: flags, and the vertex of every active cell under the next id
  for (auto z = 0; z < dim[2]; z++)
    for (auto y = 0; y < dim[1]; y++)
      for (auto x = 0; x < dim[0]; x++) {
        const int  p[3]   = {x, y, z};
        const bool has[3] = {x + 1 < dim[0], y + 1 < dim[1], z + 1 < dim[2]};
        const auto idx    = (size_t)(x + y * stride[1] + z * stride[2]);
        auto       bits   = 0u;
        const auto v0     = at(x, y, z);
        if (has[0]) bits |= vpt_sdf_mesh_edge_bits(0, p, dim, v0, at(x + 1, y, z), desc.iso);
        if (has[1]) bits |= vpt_sdf_mesh_edge_bits(1, p, dim, v0, at(x, y + 1, z), desc.iso);
        if (has[2]) bits |= vpt_sdf_mesh_edge_bits(2, p, dim, v0, at(x, y, z + 1), desc.iso);
        if (has[0] && has[1] && has[2]) {
          float c[8];
          for (auto k = 0; k < 8; k++) c[k] = at(x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2));
          if (vpt_sdf_mesh_active(vpt_sdf_mesh_mask(c, desc.iso))) {
            bits |= VPT_SDF_MESH_ACTIVE;
            ids[idx]     = (int)mesh.positions.size();
            const auto u = vpt_sdf_mesh_cell_vertex(c, desc.iso);
            mesh.positions.push_back({vpt_sdf_mesh_position(desc.origin[0], desc.step[0], lo[0] + x, u.x),
                vpt_sdf_mesh_position(desc.origin[1], desc.step[1], lo[1] + y, u.y), vpt_sdf_mesh_position(desc.origin[2], desc.step[2], lo[2] + z, u.z)});
            const auto n = vpt_sdf_mesh_normal(c, u, desc.step);
            mesh.normals.push_back({n.x, n.y, n.z});
          }
        }
        flags[idx] = (unsigned char)bits;
      }
  // the quads, by owner voxel, then by axis
  for (size_t idx = 0; idx < flags.size(); idx++)
    for (auto a = 0; a < 3; a++) {
      if (!(flags[idx] & (VPT_SDF_MESH_QUAD << a))) continue;
      long long cell[4];
      vpt_sdf_mesh_quad_cells(a, (flags[idx] & (VPT_SDF_MESH_FLIP << a)) != 0, stride, cell);
      if (mesh.quads.size() == (size_t)2147483647) throw std::runtime_error{"mesh_sdf: more than 2^31 - 1 quads"};
      auto id = [&](int k) { return ids[(size_t)((long long)idx + cell[k])]; };
      mesh.quads.push_back({id(0), id(1), id(2), id(3)});
    }
  return mesh;
}

sdf_mesh mesh_sdf_device(const float* voxels, const vpt_sdf_mesh_desc& desc, int device) {
  auto mesh  = sdf_mesh{};
  auto stats = vpt_sdf_mesh_stats{};
  if (vpt_mesh_sdf(device, &desc, voxels, nullptr, nullptr, 0, nullptr, 0, &stats) != VPT_OK) throw std::runtime_error{vpt_last_error()};
  mesh.positions.resize((size_t)stats.num_vertices), mesh.normals.resize((size_t)stats.num_vertices), mesh.quads.resize((size_t)stats.num_quads);
  if (stats.num_vertices == 0) return mesh;
  if (vpt_mesh_sdf(device, &desc, voxels, &mesh.positions[0].x, &mesh.normals[0].x, stats.num_vertices, mesh.quads.empty() ? nullptr : &mesh.quads[0].x, stats.num_quads,
          &stats) != VPT_OK)
    throw std::runtime_error{vpt_last_error()};
  return mesh;
}

// binary little-endian PLY: x y z [nx ny nz] per vertex, a list of four int32 per face (the host is little-endian, as everywhere here)
bool save_mesh_ply(const string& filename, const sdf_mesh& mesh, string& error) {
  if (!mesh.normals.empty() && mesh.normals.size() != mesh.positions.size()) return error = filename + ": normals do not match positions", false;
  auto file = fopen(filename.c_str(), "wb");
  if (!file) return error = filename + ": file not found", false;
  const auto with_normals = !mesh.normals.empty();
  auto       ok = fprintf(file, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n%selement face %zu\n"
                                "property list uchar int vertex_indices\nend_header\n",
                      mesh.positions.size(), with_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "", mesh.quads.size()) > 0;
  for (size_t i = 0; ok && i < mesh.positions.size(); i++) {
    ok = fwrite(&mesh.positions[i], 12, 1, file) == 1;
    if (ok && with_normals) ok = fwrite(&mesh.normals[i], 12, 1, file) == 1;
  }
  for (size_t i = 0; ok && i < mesh.quads.size(); i++) {
    const unsigned char four = 4;
    ok = fwrite(&four, 1, 1, file) == 1 && fwrite(&mesh.quads[i], 16, 1, file) == 1;
  }
  ok = (fclose(file) == 0) && ok;
  if (!ok) error = filename + ": write error";
  return ok;
}

}  // namespace vpt

extern "C" {

static void mesh_error(char* err, int errlen, const char* msg) {
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", msg);
}

// the host mirror of vpt_mesh_sdf, with its outputs' convention (counts in *stats first; a null array is not written; a capacity below the
// count of an array that is given is refused with nothing written) and a region as vpt_scene_mesh_volume takes one; -1 and `err` for what
// it refuses, the outputs and *stats untouched by a refused descriptor
int vpth_mesh_sdf(const vpt_sdf_mesh_desc* desc, const float* voxels, const vpt_sdf_mesh_region* region, float* positions, float* normals, int32_t vertex_capacity,
    int32_t* quads, int32_t quad_capacity, vpt_sdf_mesh_stats* stats, char* err, int errlen) {
  try {
    if (!desc || !stats) throw std::invalid_argument{"mesh_sdf: null argument"};
    if (vertex_capacity < 0 || quad_capacity < 0) throw std::invalid_argument{"mesh_sdf: a capacity is negative"};
    const auto mesh = vpt::mesh_sdf(voxels, *desc, region);
    *stats = vpt_sdf_mesh_stats{(int32_t)mesh.positions.size(), (int32_t)mesh.quads.size(), 0, 0.0f};
    if ((positions || normals) && vertex_capacity < stats->num_vertices)
      throw std::invalid_argument{"vertex_capacity " + std::to_string(vertex_capacity) + " < " + std::to_string(stats->num_vertices) + " vertices"};
    if (quads && quad_capacity < stats->num_quads)
      throw std::invalid_argument{"quad_capacity " + std::to_string(quad_capacity) + " < " + std::to_string(stats->num_quads) + " quads"};
    if (positions && !mesh.positions.empty()) memcpy(positions, mesh.positions.data(), mesh.positions.size() * 12);
    if (normals && !mesh.normals.empty()) memcpy(normals, mesh.normals.data(), mesh.normals.size() * 12);
    if (quads && !mesh.quads.empty()) memcpy(quads, mesh.quads.data(), mesh.quads.size() * 16);
    return 0;
  } catch (const std::exception& e) {
    return mesh_error(err, errlen, e.what()), -1;
  }
}
// positions (and normals, unless null) of nv vertices and nq quads as a binary PLY file load_shape reads back with the same bits
int vpth_save_mesh_ply(const char* filename, const float* positions, const float* normals, int nv, const int32_t* quads, int nq, char* err, int errlen) {
  try {
    if (!filename || nv < 0 || nq < 0 || (nv > 0 && !positions) || (nq > 0 && !quads)) throw std::invalid_argument{"save_mesh_ply: null pointer or negative count"};
    auto mesh = vpt::sdf_mesh{};
    mesh.positions.assign((const vpt::vec3f*)positions, (const vpt::vec3f*)positions + nv);
    if (normals) mesh.normals.assign((const vpt::vec3f*)normals, (const vpt::vec3f*)normals + nv);
    mesh.quads.assign((const vpt::vec4i*)quads, (const vpt::vec4i*)quads + nq);
    auto error = std::string{};
    if (!vpt::save_mesh_ply(filename, mesh, error)) throw std::runtime_error{error};
    return 0;
  } catch (const std::exception& e) {
    return mesh_error(err, errlen, e.what()), -1;
  }
}

}  // extern "C"

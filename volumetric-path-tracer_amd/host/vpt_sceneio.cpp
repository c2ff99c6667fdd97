// vpt_sceneio.cpp — the subset of the reference's scene/asset IO that the hot path's callers
// need: JSON scene format 4.2 (yocto_sceneio.cpp:3544-3865), PLY meshes
// (yocto_modelio.cpp:1117-1231 semantics: quads-vs-triangles rule, texcoord v-flip), PNG -> RGBA8,
// Radiance HDR -> float4 (stb_image.h:7046-7071 conversion), `.sdf` voxel grids
// (yocto_sceneio.cpp:885-967).  Written from the file formats, not from the reference's parsers.
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <tuple>

#include "vpt_host.h"

namespace vpt {

// ---------------------------------------------------------------------------------------------
// files
// ---------------------------------------------------------------------------------------------
static bool read_file(const string& filename, vector<uint8_t>& data, string& error) {
  auto f = fopen(filename.c_str(), "rb");
  if (!f) {
    error = filename + ": file not found";
    return false;
  }
  fseek(f, 0, SEEK_END);
  auto n = ftell(f);
  fseek(f, 0, SEEK_SET);
  data.resize((size_t)n);
  auto ok = n == 0 || fread(data.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  if (!ok) error = filename + ": read error";
  return ok;
}
static string path_dirname(const string& filename) {
  auto pos = filename.find_last_of("/\\");
  return pos == string::npos ? string{"."} : filename.substr(0, pos);
}
static string path_extension(const string& filename) {
  auto pos = filename.rfind('.');
  if (pos == string::npos) return "";
  auto ext = filename.substr(pos);
  for (auto& c : ext) c = (char)tolower(c);
  return ext;
}
// std::filesystem's operator/ as the reference uses it (yocto_sceneio.cpp:105-107): an absolute second path replaces the first
static string path_join(const string& a, const string& b) { return (!b.empty() && b[0] == '/') ? b : a + "/" + b; }

// ---------------------------------------------------------------------------------------------
// minimal JSON (RFC 8259) — numbers kept as double (strtod), converted on access like the
// reference's json.value<float>()
// ---------------------------------------------------------------------------------------------
namespace {
struct json_value {
  enum kind_t { null_k, bool_k, number_k, string_k, array_k, object_k } kind = null_k;
  bool                                       boolean = false;
  double                                     number  = 0;
  string                                     text;
  vector<json_value>                         items;
  vector<std::pair<string, json_value>>      members;
  const json_value* find(const string& key) const {
    for (auto& [k, v] : members)
      if (k == key) return &v;
    return nullptr;
  }
};
struct json_parser {
  const char* p;
  const char* end;
  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
  }
  [[noreturn]] void fail() { throw std::runtime_error{"json"}; }
  json_value parse() {
    ws();
    if (p >= end) fail();
    auto v = json_value{};
    if (*p == '{') {
      v.kind = json_value::object_k;
      p++, ws();
      if (p < end && *p == '}') return p++, v;
      while (true) {
        ws();
        auto key = parse_string();
        ws();
        if (p >= end || *p++ != ':') fail();
        v.members.emplace_back(key, parse());
        ws();
        if (p >= end) fail();
        if (*p == ',') { p++; continue; }
        if (*p == '}') return p++, v;
        fail();
      }
    } else if (*p == '[') {
      v.kind = json_value::array_k;
      p++, ws();
      if (p < end && *p == ']') return p++, v;
      while (true) {
        v.items.push_back(parse());
        ws();
        if (p >= end) fail();
        if (*p == ',') { p++; continue; }
        if (*p == ']') return p++, v;
        fail();
      }
    } else if (*p == '"') {
      v.kind = json_value::string_k, v.text = parse_string();
    } else if (!strncmp(p, "true", 4) && end - p >= 4) {
      v.kind = json_value::bool_k, v.boolean = true, p += 4;
    } else if (!strncmp(p, "false", 5) && end - p >= 5) {
      v.kind = json_value::bool_k, v.boolean = false, p += 5;
    } else if (!strncmp(p, "null", 4) && end - p >= 4) {
      p += 4;
    } else {
      auto next = (char*)nullptr;
      v.kind = json_value::number_k, v.number = strtod(p, &next);
      if (next == p) fail();
      p = next;
    }
    return v;
  }
  string parse_string() {
    if (p >= end || *p != '"') fail();
    p++;
    auto s = string{};
    while (p < end && *p != '"') {
      if (*p == '\\') {
        p++;
        if (p >= end) fail();
        switch (*p) {
          case 'n': s += '\n'; break;
          case 't': s += '\t'; break;
          case 'r': s += '\r'; break;
          case 'b': s += '\b'; break;
          case 'f': s += '\f'; break;
          case 'u': {  // BMP code point -> UTF-8
            if (end - p < 5) fail();
            auto cp = (unsigned)strtoul(string(p + 1, p + 5).c_str(), nullptr, 16);
            p += 4;
            if (cp < 0x80) s += (char)cp;
            else if (cp < 0x800) s += (char)(0xc0 | (cp >> 6)), s += (char)(0x80 | (cp & 0x3f));
            else s += (char)(0xe0 | (cp >> 12)), s += (char)(0x80 | ((cp >> 6) & 0x3f)), s += (char)(0x80 | (cp & 0x3f));
          } break;
          default: s += *p;
        }
        p++;
      } else {
        s += *p++;
      }
    }
    if (p >= end) fail();
    p++;
    return s;
  }
};

// get_opt family: leave `value` untouched when the key is absent (json.value(key, default))
void get_opt(const json_value& js, const char* key, float& value) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::number_k) throw std::runtime_error{"json"};
    value = (float)v->number;
  }
}
void get_opt(const json_value& js, const char* key, int& value) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::number_k) throw std::runtime_error{"json"};
    value = (int)v->number;
  }
}
void get_opt(const json_value& js, const char* key, bool& value) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::bool_k) throw std::runtime_error{"json"};
    value = v->boolean;
  }
}
void get_opt(const json_value& js, const char* key, string& value) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::string_k) throw std::runtime_error{"json"};
    value = v->text;
  }
}
void get_floats(const json_value& js, const char* key, float* out, size_t n) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::array_k || v->items.size() != n) throw std::runtime_error{"json"};
    for (size_t i = 0; i < n; i++) {
      if (v->items[i].kind != json_value::number_k) throw std::runtime_error{"json"};
      out[i] = (float)v->items[i].number;
    }
  }
}
void get_opt(const json_value& js, const char* key, vec3f& value) { get_floats(js, key, &value.x, 3); }
void get_opt(const json_value& js, const char* key, frame3f& value) { get_floats(js, key, &value.x.x, 12); }
template <typename E>
void get_enum(const json_value& js, const char* key, E& value, const vector<string>& names) {
  if (auto v = js.find(key)) {
    if (v->kind != json_value::string_k) throw std::runtime_error{"json"};
    // nlohmann's enum mapping falls back to the FIRST entry for unknown names
    value = (E)0;
    for (size_t i = 0; i < names.size(); i++)
      if (names[i] == v->text) value = (E)i;
  }
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// PLY
// ---------------------------------------------------------------------------------------------
namespace {
enum ply_type { t_i8, t_u8, t_i16, t_u16, t_i32, t_u32, t_f32, t_f64, t_bad };
ply_type parse_ply_type(const string& s) {
  if (s == "char" || s == "int8") return t_i8;
  if (s == "uchar" || s == "uint8") return t_u8;
  if (s == "short" || s == "int16") return t_i16;
  if (s == "ushort" || s == "uint16") return t_u16;
  if (s == "int" || s == "int32") return t_i32;
  if (s == "uint" || s == "uint32") return t_u32;
  if (s == "float" || s == "float32") return t_f32;
  if (s == "double" || s == "float64") return t_f64;
  return t_bad;
}
int ply_size(ply_type t) {
  static const int sizes[] = {1, 1, 2, 2, 4, 4, 4, 8, 0};
  return sizes[t];
}
struct ply_property {
  string         name;
  bool           is_list = false;
  ply_type       type = t_bad, ltype = t_bad;
  vector<double> values;        // scalar: one per element; list: concatenated
  vector<int>    list_sizes;    // list only
};
struct ply_element {
  string               name;
  size_t               count = 0;
  vector<ply_property> props;
  const ply_property* find(const string& n) const {
    for (auto& p : props)
      if (p.name == n) return &p;
    return nullptr;
  }
};
double read_binary(const uint8_t*& p, const uint8_t* end, ply_type t, bool big_endian) {
  auto n = ply_size(t);
  if (end - p < n) throw std::runtime_error{"ply"};
  uint8_t b[8];
  for (auto i = 0; i < n; i++) b[i] = big_endian ? p[n - 1 - i] : p[i];
  p += n;
  switch (t) {
    case t_i8: { int8_t v; memcpy(&v, b, 1); return v; }
    case t_u8: { uint8_t v; memcpy(&v, b, 1); return v; }
    case t_i16: { int16_t v; memcpy(&v, b, 2); return v; }
    case t_u16: { uint16_t v; memcpy(&v, b, 2); return v; }
    case t_i32: { int32_t v; memcpy(&v, b, 4); return v; }
    case t_u32: { uint32_t v; memcpy(&v, b, 4); return v; }
    case t_f32: { float v; memcpy(&v, b, 4); return v; }
    case t_f64: { double v; memcpy(&v, b, 8); return v; }
    default: throw std::runtime_error{"ply"};
  }
}
}  // namespace

static bool load_ply_shape(const string& filename, shape_data& shape, string& error, bool flip_texcoord) {
  auto data = vector<uint8_t>{};
  if (!read_file(filename, data, error)) return false;
  auto read_error = [&]() {
    error = filename + ": read error";
    return false;
  };
  auto elements = vector<ply_element>{};
  try {
    // header
    const uint8_t* p   = data.data();
    const uint8_t* end = data.data() + data.size();
    auto next_line = [&]() {
      auto s = string{};
      while (p < end && *p != '\n') s += (char)*p++;
      if (p < end) p++;
      if (!s.empty() && s.back() == '\r') s.pop_back();
      return s;
    };
    if (next_line() != "ply") return read_error();
    auto format = string{};
    while (true) {
      if (p >= end) return read_error();
      auto line = next_line();
      auto ss   = std::istringstream{line};
      auto cmd  = string{};
      ss >> cmd;
      if (cmd == "format") ss >> format;
      else if (cmd == "element") {
        auto& e = elements.emplace_back();
        ss >> e.name >> e.count;
      } else if (cmd == "property") {
        if (elements.empty()) return read_error();
        auto& prop = elements.back().props.emplace_back();
        auto  t    = string{};
        ss >> t;
        if (t == "list") {
          auto lt = string{}, vt = string{};
          ss >> lt >> vt >> prop.name;
          prop.is_list = true, prop.ltype = parse_ply_type(lt), prop.type = parse_ply_type(vt);
          if (prop.ltype == t_bad) return read_error();
        } else {
          prop.type = parse_ply_type(t);
          ss >> prop.name;
        }
        if (prop.type == t_bad) return read_error();
      } else if (cmd == "end_header") break;
    }
    auto ascii = format == "ascii", big = format == "binary_big_endian";
    if (!ascii && !big && format != "binary_little_endian") return read_error();
    // body
    auto text = std::istringstream{};
    if (ascii) text.str(string((const char*)p, (size_t)(end - p)));
    auto next = [&](ply_type t) -> double {
      if (!ascii) return read_binary(p, end, t, big);
      auto v = 0.0;
      if (!(text >> v)) throw std::runtime_error{"ply"};
      return v;
    };
    for (auto& e : elements) {
      for (auto& prop : e.props) {
        if (prop.is_list) prop.list_sizes.reserve(e.count);
        prop.values.reserve(e.count * (prop.is_list ? 4 : 1));
      }
      for (size_t i = 0; i < e.count; i++)
        for (auto& prop : e.props) {
          if (prop.is_list) {
            auto n = (int)next(prop.ltype);
            prop.list_sizes.push_back(n);
            for (auto k = 0; k < n; k++) prop.values.push_back(next(prop.type));
          } else {
            prop.values.push_back(next(prop.type));
          }
        }
    }
  } catch (...) {
    return read_error();
  }
  // vertex attributes -> float32 (get_positions/normals/texcoords/colors, yocto_modelio.cpp:1124-1160)
  for (auto& e : elements) {
    if (e.name == "vertex") {
      auto get = [&](std::initializer_list<const char*> names, size_t n, float* out, size_t stride) {
        auto k = (size_t)0;
        for (auto name : names) {
          auto prop = e.find(name);
          if (!prop || prop->is_list) return false;
          for (size_t i = 0; i < n; i++) out[i * stride + k] = (float)prop->values[i];
          k++;
        }
        return true;
      };
      auto n = e.count;
      if (e.find("x") && e.find("y") && e.find("z")) {
        shape.positions.resize(n);
        get({"x", "y", "z"}, n, &shape.positions[0].x, 3);
      }
      if (e.find("nx") && e.find("ny") && e.find("nz")) {
        shape.normals.resize(n);
        get({"nx", "ny", "nz"}, n, &shape.normals[0].x, 3);
      }
      if ((e.find("u") && e.find("v")) || (e.find("s") && e.find("t"))) {
        shape.texcoords.resize(n);
        if (e.find("u")) get({"u", "v"}, n, &shape.texcoords[0].x, 2);
        else get({"s", "t"}, n, &shape.texcoords[0].x, 2);
        if (flip_texcoord)
          for (auto& uv : shape.texcoords) uv.y = 1 - uv.y;
      }
      if (e.find("radius") && !e.find("radius")->is_list) {   // get_radius, yocto_modelio.cpp:1157-1159
        shape.radius.resize(n);
        get({"radius"}, n, shape.radius.data(), 1);
      }
      if (e.find("red") && e.find("green") && e.find("blue")) {
        shape.colors.resize(n);
        get({"red", "green", "blue"}, n, &shape.colors[0].x, 4);
        if (e.find("alpha")) get({"alpha"}, n, &shape.colors[0].w, 4);
        else for (auto& c : shape.colors) c.w = 1;
        // 8-bit colours are normalised
        auto scale = e.find("red")->type == t_u8 ? 1 / 255.0f : 1.0f;
        if (scale != 1.0f)
          for (auto& c : shape.colors) c = {c.x * scale, c.y * scale, c.z * scale, e.find("alpha") ? c.w * scale : 1.0f};
      }
    } else if (e.name == "face") {
      auto prop = e.find("vertex_indices");
      if (!prop) prop = e.find("vertex_index");
      if (!prop || !prop->is_list) continue;
      // has_quads (yocto_modelio.cpp:1226-1232): ANY 4-sided face turns the whole mesh into quads,
      // triangles becoming degenerate quads (z == w); otherwise polygons are fanned into triangles.
      auto any_quad = false;
      for (auto n : prop->list_sizes) any_quad |= n == 4;
      auto cur = (size_t)0;
      for (auto n : prop->list_sizes) {
        auto idx = [&](int k) { return (int)prop->values[cur + (size_t)k]; };
        if (any_quad) {
          if (n == 4) shape.quads.push_back({idx(0), idx(1), idx(2), idx(3)});
          else for (auto c = 2; c < n; c++) shape.quads.push_back({idx(0), idx(c - 1), idx(c), idx(c)});
        } else {
          for (auto c = 2; c < n; c++) shape.triangles.push_back({idx(0), idx(c - 1), idx(c)});
        }
        cur += (size_t)n;
      }
    } else if (e.name == "line") {   // get_lines, yocto_modelio.cpp:1212-1227: a polyline of n vertices is n - 1 segments
      auto prop = e.find("vertex_indices");
      if (!prop || !prop->is_list) continue;
      auto cur = (size_t)0;
      for (auto n : prop->list_sizes) {
        for (auto c = 1; c < n; c++) shape.lines.push_back({(int)prop->values[cur + (size_t)c - 1], (int)prop->values[cur + (size_t)c]});
        cur += (size_t)n;
      }
    } else if (e.name == "point") {
      if (auto prop = e.find("vertex_indices"))
        for (auto v : prop->values) shape.points.push_back((int)v);
    }
  }
  // reject out-of-range indices here rather than on the device
  auto nv = (int)shape.positions.size();
  for (auto& t : shape.triangles)
    if (t.x < 0 || t.y < 0 || t.z < 0 || t.x >= nv || t.y >= nv || t.z >= nv) return read_error();
  for (auto& q : shape.quads)
    if (q.x < 0 || q.y < 0 || q.z < 0 || q.w < 0 || q.x >= nv || q.y >= nv || q.z >= nv || q.w >= nv)
      return read_error();
  for (auto p : shape.points)
    if (p < 0 || p >= nv) return read_error();
  for (auto& l : shape.lines)
    if (l.x < 0 || l.y < 0 || l.x >= nv || l.y >= nv) return read_error();
  if (!shape.radius.empty() && shape.radius.size() != shape.positions.size()) return read_error();
  if (shape.points.empty() && shape.lines.empty() && shape.triangles.empty() && shape.quads.empty()) {
    error = filename + ": empty shape";
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// OBJ geometry (yocto_modelio.cpp:1952-2072 load_obj(obj_shape), :2336-2488 accessors): v / vn / vt / f / l / p,
// negative indices, polygons fanned; everything else (materials, groups, objects) is skipped as the reference skips it.
// Two forms, as in the reference: vertices unified per distinct (position, texcoord, normal) triple in order of first
// appearance (load_shape), or face-varying index triples kept apart (load_fvshape -> load_subdiv).
// ---------------------------------------------------------------------------------------------
namespace {
struct obj_vertex { int position = 0, texcoord = 0, normal = 0; };
struct obj_element { int size = 0; char etype = 'f'; };
struct obj_raw {
  vector<vec3f>       positions, normals;
  vector<vec2f>       texcoords;
  vector<obj_vertex>  vertices;
  vector<obj_element> elements;
  int                 materials = 0;   // usemtl statements (only counted: a shape of lines or points may hold one)
};
void skip_ws(const char*& p, const char* end) {
  while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) p++;
}
bool parse_float(const char*& p, const char* end, float& v) {   // correctly rounded like the reference's fast_float
  skip_ws(p, end);
  if (p >= end) return false;
  auto q = p;   // the whole token, however long: a capped copy would split one long literal into two numbers
  while (q < end && !isspace((unsigned char)*q)) q++;
  auto tmp = string(p, (size_t)(q - p));
  auto stop = (char*)nullptr;
  v = std::strtof(tmp.c_str(), &stop);
  if (stop == tmp.c_str()) return false;
  p += stop - tmp.c_str();
  return true;
}
bool parse_int(const char*& p, const char* end, int& v) {
  skip_ws(p, end);
  if (p >= end) return false;
  auto tmp = string(p, (size_t)std::min<ptrdiff_t>(end - p, 31));
  auto stop = (char*)nullptr;
  v = (int)std::strtol(tmp.c_str(), &stop, 10);
  if (stop == tmp.c_str()) return false;
  if (stop == tmp.c_str() + 31) return false;   // an index that fills the whole 31-character window: not an OBJ index, and its tail would be read as the next one
  p += stop - tmp.c_str();
  return true;
}
bool parse_obj_vertex(const char*& p, const char* end, obj_vertex& v) {   // "p", "p/t", "p//n", "p/t/n" (yocto_modelio.cpp:1480-1497)
  v = {};
  if (!parse_int(p, end, v.position)) return false;
  if (p < end && *p == '/') {
    p++;
    if (p < end && *p == '/') {
      p++;
      if (!parse_int(p, end, v.normal)) return false;
    } else {
      if (!parse_int(p, end, v.texcoord)) return false;
      if (p < end && *p == '/') {
        p++;
        if (!parse_int(p, end, v.normal)) return false;
      }
    }
  }
  return true;
}
bool load_obj_raw(const string& filename, obj_raw& obj, string& error) {
  auto data = vector<uint8_t>{};
  if (!read_file(filename, data, error)) return false;
  auto parse_error = [&]() {
    error = filename + ": parse error";
    return false;
  };
  auto cur = (const char*)data.data(), file_end = cur + data.size();
  while (cur < file_end) {
    auto line_end = cur;
    while (line_end < file_end && *line_end != '\n') line_end++;
    auto p = cur, end = line_end;
    cur = line_end < file_end ? line_end + 1 : file_end;
    for (auto c = p; c < end; c++)   // remove_comment
      if (*c == '#') {
        end = c;
        break;
      }
    skip_ws(p, end);
    if (p >= end) continue;
    auto cmd = string{};
    while (p < end && *p != ' ' && *p != '\t' && *p != '\r') cmd += *p++;
    if (cmd == "v" || cmd == "vn") {
      auto v = vec3f{};
      if (!parse_float(p, end, v.x) || !parse_float(p, end, v.y) || !parse_float(p, end, v.z)) return parse_error();
      (cmd == "v" ? obj.positions : obj.normals).push_back(v);
    } else if (cmd == "vt") {
      auto v = vec2f{};
      if (!parse_float(p, end, v.x) || !parse_float(p, end, v.y)) return parse_error();
      obj.texcoords.push_back(v);
    } else if (cmd == "usemtl") {
      obj.materials++;
    } else if (cmd == "f" || cmd == "l" || cmd == "p") {
      auto& element = obj.elements.emplace_back();
      element.etype = cmd[0];
      skip_ws(p, end);
      while (p < end) {
        auto vert = obj_vertex{};
        if (!parse_obj_vertex(p, end, vert)) return parse_error();
        if (vert.position == 0) break;
        if (vert.position < 0) vert.position = (int)obj.positions.size() + vert.position + 1;
        if (vert.texcoord < 0) vert.texcoord = (int)obj.texcoords.size() + vert.texcoord + 1;
        if (vert.normal < 0) vert.normal = (int)obj.normals.size() + vert.normal + 1;
        // the reference trusts the file; the device path must not
        if (vert.position < 1 || vert.position > (int)obj.positions.size() || vert.texcoord < 0 || vert.texcoord > (int)obj.texcoords.size() ||
            vert.normal < 0 || vert.normal > (int)obj.normals.size())
          return parse_error();
        obj.vertices.push_back(vert);
        element.size += 1;
        skip_ws(p, end);
      }
    }
  }
  return true;
}
// faces of an obj as quads (a polygon with n != 4 corners is fanned into degenerate quads z == w), one index kind at a time
template <typename Get>
void obj_fan_quads(const obj_raw& obj, vector<vec4i>& quads, Get get) {
  auto cur = 0;
  for (auto& element : obj.elements) {
    if (element.etype == 'f') {
      auto at = [&](int k) { return get(obj.vertices[(size_t)(cur + k)]) - 1; };
      if (element.size == 4) quads.push_back({at(0), at(1), at(2), at(3)});
      else
        for (auto c = 2; c < element.size; c++) quads.push_back({at(0), at(c - 1), at(c), at(c)});
    }
    cur += element.size;
  }
}
bool load_obj_shape(const string& filename, shape_data& shape, string& error, bool flip_texcoord) {
  auto obj = obj_raw{};
  if (!load_obj_raw(filename, obj, error)) return false;
  // one vertex per distinct index triple, numbered by first appearance (yocto_modelio.cpp:2036-2068)
  auto seen = std::map<std::tuple<int, int, int>, int>{};
  for (auto& v : obj.vertices) {
    auto triple = std::make_tuple(v.position, v.texcoord, v.normal);
    auto it     = seen.find(triple);
    if (it == seen.end()) {
      auto index = (int)seen.size();
      shape.positions.push_back(obj.positions[(size_t)v.position - 1]);
      if (v.normal > 0) shape.normals.push_back(obj.normals[(size_t)v.normal - 1]);
      if (v.texcoord > 0) shape.texcoords.push_back(obj.texcoords[(size_t)v.texcoord - 1]);
      seen.emplace(triple, index);
      v.position = index + 1;
    } else {
      v.position = it->second + 1;
    }
  }
  // a file that gives normals / texcoords to some vertices only leaves the reference with arrays of different lengths
  if ((!shape.normals.empty() && shape.normals.size() != shape.positions.size()) ||
      (!shape.texcoords.empty() && shape.texcoords.size() != shape.positions.size())) {
    error = filename + ": parse error";
    return false;
  }
  if (flip_texcoord)
    for (auto& uv : shape.texcoords) uv.y = 1 - uv.y;
  // get_faces (yocto_modelio.cpp:2349-2356): any 4-corner face makes the whole mesh quads, else fanned triangles
  auto any_quad = false;
  for (auto& e : obj.elements) any_quad |= e.etype == 'f' && e.size == 4;
  if (any_quad) obj_fan_quads(obj, shape.quads, [](const obj_vertex& v) { return v.position; });
  else {
    auto cur = 0;
    for (auto& element : obj.elements) {
      if (element.etype == 'f')
        for (auto c = 2; c < element.size; c++)
          shape.triangles.push_back({obj.vertices[(size_t)cur].position - 1, obj.vertices[(size_t)(cur + c - 1)].position - 1, obj.vertices[(size_t)(cur + c)].position - 1});
      cur += element.size;
    }
  }
  // get_lines / get_points (yocto_modelio.cpp:2402-2434): `l` elements are polylines split into segments, every corner of a
  // `p` element reads the element's FIRST vertex.  Like get_fvquads they skip an element of another kind without advancing
  // their vertex cursor, so they only read the right vertices when every element is of their kind: a shape with `l` or `p`
  // elements is accepted only when all its elements are of that one kind under at most one usemtl, and refused otherwise
  // (no fixture pins the reference's shifted reads).  A face shape with `l` / `p` elements keeps them, and flatten refuses it.
  auto curves = false, faces = false, lines = true, points = true;
  for (auto& e : obj.elements) curves |= e.etype != 'f', faces |= e.etype == 'f', lines &= e.etype == 'l', points &= e.etype == 'p';
  if (curves && !faces && !((lines || points) && obj.materials <= 1)) {
    error = filename + ": a shape of lines or points must hold one element kind under one material";
    return false;
  }
  auto cur = 0;
  for (auto& element : obj.elements) {
    if (element.etype == 'l')
      for (auto c = 1; c < element.size; c++)
        shape.lines.push_back({obj.vertices[(size_t)(cur + c - 1)].position - 1, obj.vertices[(size_t)(cur + c)].position - 1});
    else if (element.etype == 'p')
      for (auto c = 0; c < element.size; c++) shape.points.push_back(obj.vertices[(size_t)cur].position - 1);
    cur += element.size;
  }
  if (shape.points.empty() && shape.lines.empty() && shape.triangles.empty() && shape.quads.empty()) {
    error = filename + ": empty shape";
    return false;
  }
  return true;
}
}  // namespace

bool load_shape(const string& filename, shape_data& shape, string& error, bool flip_texcoord) {
  shape    = {};
  auto ext = path_extension(filename);
  if (ext == ".ply") return load_ply_shape(filename, shape, error, flip_texcoord);
  if (ext == ".obj") return load_obj_shape(filename, shape, error, flip_texcoord);
  error = filename + ": unknown format";  // STL / ypreset are outside the hot-path scope
  return false;
}

// load_subdiv -> load_fvshape(filename, ., ., flip_texcoord = true) (yocto_sceneio.cpp:2829-2840, 1135-1186)
bool load_subdiv(const string& filename, subdiv_data& subdiv, string& error) {
  auto ext = path_extension(filename);
  auto empty_shape = [&]() {
    error = filename + ": empty shape";
    return false;
  };
  if (ext == ".ply") {   // one index set for all three attributes
    auto shape = shape_data{};
    if (!load_ply_shape(filename, shape, error, true)) return false;
    subdiv.positions = shape.positions, subdiv.normals = shape.normals, subdiv.texcoords = shape.texcoords;
    subdiv.quadspos = shape.quads;
    for (auto& t : shape.triangles) subdiv.quadspos.push_back({t.x, t.y, t.z, t.z});
    subdiv.quadsnorm     = subdiv.normals.empty() ? vector<vec4i>{} : subdiv.quadspos;
    subdiv.quadstexcoord = subdiv.texcoords.empty() ? vector<vec4i>{} : subdiv.quadspos;
    if (subdiv.quadspos.empty()) return empty_shape();
    return true;
  }
  if (ext == ".obj") {
    auto obj = obj_raw{};
    if (!load_obj_raw(filename, obj, error)) return false;
    subdiv.positions = obj.positions, subdiv.normals = obj.normals, subdiv.texcoords = obj.texcoords;
    for (auto& uv : subdiv.texcoords) uv.y = 1 - uv.y;
    subdiv.quadspos.clear(), subdiv.quadsnorm.clear(), subdiv.quadstexcoord.clear();
    // A cage that mixes faces with line / point elements is REJECTED, a deliberate divergence: the reference's get_fvquads
    // (yocto_modelio.cpp:2446) skips such an element WITHOUT advancing its vertex cursor, so every later face reads the
    // wrong vertices (a defect no test scene of the reference exercises: none of its cages holds l / p statements); there is
    // no fixture to pin either behaviour to, so the file is refused rather than rendered differently from the reference.
    for (auto& e : obj.elements)
      if (e.etype != 'f') {
        error = filename + ": line / point elements in a subdivision cage are not supported";
        return false;
      }
    // get_fvquads (yocto_modelio.cpp:2435-2488): which index kinds exist is decided by the FIRST vertex of the file
    if (!obj.vertices.empty()) {
      obj_fan_quads(obj, subdiv.quadspos, [](const obj_vertex& v) { return v.position; });
      if (obj.vertices[0].normal != 0) obj_fan_quads(obj, subdiv.quadsnorm, [](const obj_vertex& v) { return v.normal; });
      if (obj.vertices[0].texcoord != 0) obj_fan_quads(obj, subdiv.quadstexcoord, [](const obj_vertex& v) { return v.texcoord; });
    }
    if (subdiv.quadspos.empty()) return empty_shape();
    for (auto& q : subdiv.quadsnorm)   // a later vertex without the index kind the first one had: -1 in the reference, rejected here
      if (q.x < 0 || q.y < 0 || q.z < 0 || q.w < 0) return empty_shape();
    for (auto& q : subdiv.quadstexcoord)
      if (q.x < 0 || q.y < 0 || q.z < 0 || q.w < 0) return empty_shape();
    return true;
  }
  error = filename + ": unknown format";
  return false;
}

// ---------------------------------------------------------------------------------------------
// PNG (8/16-bit, all colour types, non-interlaced) -> RGBA8 ; Radiance HDR -> float4
// ---------------------------------------------------------------------------------------------
static bool zlib_inflate(const vector<uint8_t>& in, vector<uint8_t>& out, size_t expected) {
  out.resize(expected);
  auto n = (uLongf)expected;
  return uncompress(out.data(), &n, in.data(), (uLong)in.size()) == Z_OK && n == expected;
}

static bool decode_png(const vector<uint8_t>& data, texture_data& texture) {
  static const uint8_t magic[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  if (data.size() < 8 || memcmp(data.data(), magic, 8)) return false;
  auto be32 = [&](size_t o) { return (uint32_t)data[o] << 24 | (uint32_t)data[o + 1] << 16 | (uint32_t)data[o + 2] << 8 | data[o + 3]; };
  auto width = 0u, height = 0u;
  auto depth = 0, ctype = 0, interlace = 0;
  auto idat    = vector<uint8_t>{};
  auto palette = vector<uint8_t>{}, trns = vector<uint8_t>{};
  auto pos     = (size_t)8;
  while (pos + 8 <= data.size()) {
    auto len  = be32(pos);
    auto type = string((const char*)&data[pos + 4], 4);
    auto body = pos + 8;
    if (body + len + 4 > data.size()) return false;
    if (type == "IHDR") {
      if (len < 13) return false;
      width = be32(body), height = be32(body + 4);
      depth = data[body + 8], ctype = data[body + 9], interlace = data[body + 12];
    } else if (type == "PLTE") palette.assign(&data[body], &data[body] + len);
    else if (type == "tRNS") trns.assign(&data[body], &data[body] + len);
    else if (type == "IDAT") idat.insert(idat.end(), &data[body], &data[body] + len);
    else if (type == "IEND") break;
    pos = body + len + 4;
  }
  if (!width || !height || interlace || (depth != 8 && depth != 16)) return false;
  auto channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
  if (!channels || (ctype == 3 && depth != 8)) return false;
  auto bpp    = (size_t)channels * (depth / 8);
  auto stride = (size_t)width * bpp;
  auto raw    = vector<uint8_t>{};
  if (!zlib_inflate(idat, raw, (stride + 1) * height)) return false;
  auto pix  = vector<uint8_t>(stride * height);
  auto prev = vector<uint8_t>(stride, 0);
  for (size_t y = 0; y < height; y++) {
    auto filter = raw[y * (stride + 1)];
    auto src    = &raw[y * (stride + 1) + 1];
    auto dst    = &pix[y * stride];
    for (size_t x = 0; x < stride; x++) {
      int a = x >= bpp ? dst[x - bpp] : 0, b = prev[x], c = x >= bpp ? prev[x - bpp] : 0;
      auto v = 0;
      switch (filter) {
        case 0: v = 0; break;
        case 1: v = a; break;
        case 2: v = b; break;
        case 3: v = (a + b) / 2; break;
        case 4: {
          auto pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
          v = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        } break;
        default: return false;
      }
      dst[x] = (uint8_t)(src[x] + v);
    }
    memcpy(prev.data(), dst, stride);
  }
  texture.width = (int)width, texture.height = (int)height, texture.linear = false;
  texture.pixelsf.clear();
  texture.pixelsb.resize((size_t)width * height);
  auto step = depth / 8;  // 16-bit: keep the high byte
  for (size_t i = 0; i < (size_t)width * height; i++) {
    auto s  = &pix[i * bpp];
    auto& o = texture.pixelsb[i];
    switch (ctype) {
      case 0: o = {s[0], s[0], s[0], 255}; break;
      case 2: o = {s[0], s[step], s[2 * step], 255}; break;
      case 3: {
        auto k = (size_t)s[0];
        if (3 * k + 2 >= palette.size()) return false;
        o = {palette[3 * k], palette[3 * k + 1], palette[3 * k + 2], k < trns.size() ? trns[k] : (uint8_t)255};
      } break;
      case 4: o = {s[0], s[0], s[0], s[step]}; break;
      case 6: o = {s[0], s[step], s[2 * step], s[3 * step]}; break;
    }
  }
  return true;
}

static bool decode_hdr(const vector<uint8_t>& data, texture_data& texture) {
  auto p = data.data(), end = data.data() + data.size();
  auto next_line = [&]() {
    auto s = string{};
    while (p < end && *p != '\n') s += (char)*p++;
    if (p < end) p++;
    return s;
  };
  auto first = next_line();
  if (first != "#?RADIANCE" && first != "#?RGBE") return false;
  auto valid = false;
  while (p < end) {
    auto line = next_line();
    if (line.empty()) break;
    if (line == "FORMAT=32-bit_rle_rgbe") valid = true;
  }
  if (!valid) return false;
  auto dims  = next_line();
  auto width = 0, height = 0;
  if (sscanf(dims.c_str(), "-Y %d +X %d", &height, &width) != 2 || width <= 0 || height <= 0) return false;
  auto rgbe = vector<uint8_t>((size_t)width * height * 4);
  auto flat = [&](size_t from_pixel) {
    auto need = ((size_t)width * height - from_pixel) * 4;
    if ((size_t)(end - p) < need) return false;
    memcpy(&rgbe[from_pixel * 4], p, need);
    return true;
  };
  if (width < 8 || width >= 32768) {
    if (!flat(0)) return false;
  } else {
    for (auto j = 0; j < height; j++) {
      if (end - p < 4) return false;
      if (p[0] != 2 || p[1] != 2 || (p[2] & 0x80)) {
        if (j != 0) return false;  // stb only accepts a flat file decided on the first scanline
        if (!flat(0)) return false;
        break;
      }
      if (((int)p[2] << 8 | p[3]) != width) return false;
      p += 4;
      auto row = &rgbe[(size_t)j * width * 4];
      for (auto k = 0; k < 4; k++) {
        auto i = 0;
        while (i < width) {
          if (p >= end) return false;
          auto count = (int)*p++;
          if (count > 128) {
            count -= 128;
            if (p >= end || count == 0 || i + count > width) return false;
            auto value = *p++;
            for (auto z = 0; z < count; z++) row[(i++) * 4 + k] = value;
          } else {
            if (count == 0 || i + count > width || end - p < count) return false;
            for (auto z = 0; z < count; z++) row[(i++) * 4 + k] = *p++;
          }
        }
      }
    }
  }
  texture.width = width, texture.height = height, texture.linear = true;
  texture.pixelsb.clear();
  texture.pixelsf.resize((size_t)width * height);
  for (size_t i = 0; i < texture.pixelsf.size(); i++) {
    auto s = &rgbe[i * 4];
    if (s[3] != 0) {
      auto f = (float)ldexp(1.0f, (int)s[3] - (128 + 8));
      texture.pixelsf[i] = {s[0] * f, s[1] * f, s[2] * f, 1};
    } else {
      texture.pixelsf[i] = {0, 0, 0, 1};
    }
  }
  return true;
}

bool load_texture(const string& filename, texture_data& texture, string& error) {
  auto ext  = path_extension(filename);
  auto data = vector<uint8_t>{};
  if (ext != ".png" && ext != ".hdr") {
    error = filename + ": unknown format";
    return false;
  }
  if (!read_file(filename, data, error)) return false;
  auto ok = ext == ".png" ? decode_png(data, texture) : decode_hdr(data, texture);
  if (!ok) error = filename + ": rad error";  // (sic) the reference's message, yocto_sceneio.cpp:1740
  return ok;
}

// ---------------------------------------------------------------------------------------------
// .sdf voxel grids, yocto_sceneio.cpp:885-967
// ---------------------------------------------------------------------------------------------
bool load_volume(const string& filename, volume_data& vol, bool binary, string& error) {
  auto data = vector<uint8_t>{};
  if (!read_file(filename, data, error)) {
    error = filename + ": read error";
    return false;
  }
  vol = {};
  if (binary) {
    // int32 w,h,d ; float res ; 16 floats (ignored) ; w*h*d floats
    if (data.size() < 16 + 64) { error = filename + ": read error"; return false; }
    int32_t whd[3];
    memcpy(whd, data.data(), 12);
    memcpy(&vol.res, data.data() + 12, 4);
    auto n = (size_t)whd[0] * whd[1] * whd[2];
    if (whd[0] <= 0 || whd[1] <= 0 || whd[2] <= 0 || data.size() < 80 + n * 4) { error = filename + ": read error"; return false; }
    vol.vol.resize(n);
    memcpy(vol.vol.data(), data.data() + 80, n * 4);
    vol.whd = {whd[0], whd[1], whd[2]};
    return true;
  }
  // text (SDFGen): "W H D" / origin line (ignored) / cell size / values, x fastest
  auto text  = string((const char*)data.data(), data.size());
  auto lines = std::istringstream{text};
  auto line  = string{};
  auto count = 0;
  while (std::getline(lines, line)) {
    if (count == 0) {
      auto w = 0, h = 0, d = 0;
      if (sscanf(line.c_str(), "%d %d %d", &w, &h, &d) != 3) { error = filename + ": read error"; return false; }
      vol.whd = {w, h, d};
    } else if (count == 2) {
      vol.res = (float)atof(line.c_str());
    } else if (count > 2) {
      auto p = line.c_str();
      while (*p) {
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
        if (!*p) break;
        auto q = p;
        while (*q && *q != ' ' && *q != '\t' && *q != '\r' && *q != '\n') q++;
        vol.vol.push_back((float)atof(string(p, q).c_str()));
        p = q;
      }
    }
    count++;
  }
  if ((size_t)vol.whd.x * vol.whd.y * vol.whd.z > vol.vol.size() || vol.vol.empty()) {
    error = filename + ": read error";
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------
// JSON scene 4.2
// ---------------------------------------------------------------------------------------------
// one entry of a scene file's "cameras" (also the entries of a --cameras file, load_cameras)
static void read_camera(const json_value& e, camera_data& camera) {
  get_opt(e, "frame", camera.frame), get_opt(e, "orthographic", camera.orthographic);
  get_opt(e, "lens", camera.lens), get_opt(e, "aspect", camera.aspect), get_opt(e, "film", camera.film);
  get_opt(e, "focus", camera.focus), get_opt(e, "aperture", camera.aperture);
}

bool load_scene(const string& filename, scene_data& scene, string& error) {
  scene    = {};
  auto ext = path_extension(filename);
  if (ext != ".json") {
    error = filename + ": unknown format";
    return false;
  }
  auto data = vector<uint8_t>{};
  if (!read_file(filename, data, error)) return false;
  auto parse_error = [&]() {
    error = filename + ": parse error";
    return false;
  };
  auto shape_uris = vector<string>{}, texture_uris = vector<string>{}, volume_uris = vector<string>{}, subdiv_uris = vector<string>{};
  auto volume_binary = vector<bool>{};
  try {
    auto parser = json_parser{(const char*)data.data(), (const char*)data.data() + data.size()};
    auto js     = parser.parse();
    if (js.kind != json_value::object_k) return parse_error();
    auto version = string{};
    if (auto asset = js.find("asset")) {
      get_opt(*asset, "copyright", scene.copyright);
      get_opt(*asset, "version", version);
    }
    if (version != "4.2" && version != "5.0") return parse_error();  // 4.0/4.1 dialects: out of scope
    static const json_value empty{};
    auto group = [&](const char* name) -> const vector<json_value>& {
      auto g = js.find(name);
      if (!g) return empty.items;
      if (g->kind != json_value::array_k) throw std::runtime_error{"json"};
      return g->items;
    };
    for (auto& e : group("cameras")) read_camera(e, scene.cameras.emplace_back());
    for (auto& e : group("textures")) {
      scene.textures.emplace_back();
      get_opt(e, "uri", texture_uris.emplace_back());
    }
    for (auto& e : group("materials")) {
      auto& m = scene.materials.emplace_back();
      get_enum(e, "type", m.type, material_type_names);
      get_opt(e, "emission", m.emission), get_opt(e, "color", m.color), get_opt(e, "metallic", m.metallic);
      get_opt(e, "roughness", m.roughness), get_opt(e, "ior", m.ior), get_opt(e, "trdepth", m.trdepth);
      get_opt(e, "scattering", m.scattering), get_opt(e, "scanisotropy", m.scanisotropy);
      get_opt(e, "opacity", m.opacity), get_opt(e, "emission_tex", m.emission_tex);
      get_opt(e, "color_tex", m.color_tex), get_opt(e, "roughness_tex", m.roughness_tex);
      get_opt(e, "scattering_tex", m.scattering_tex), get_opt(e, "normal_tex", m.normal_tex);
    }
    for (auto& e : group("shapes")) {
      scene.shapes.emplace_back();
      get_opt(e, "uri", shape_uris.emplace_back());
    }
    for (auto& e : group("volumes")) {
      scene.volumes.emplace_back();
      auto binary = false;
      get_opt(e, "binary", binary);
      volume_binary.push_back(binary);
      get_opt(e, "uri", volume_uris.emplace_back());
    }
    for (auto& e : group("sdfunctions")) {
      auto& sdf = scene.sdfs.emplace_back();
      sdf.type  = sdf_type::bbox;  // enum fallback = first entry
      get_enum(e, "type", sdf.type, sdf_type_names);
      get_opt(e, "frame", sdf.frame), get_opt(e, "material", sdf.material);
      switch (sdf.type) {
        case sdf_type::bbox: {
          auto whd = vec3f{};
          get_opt(e, "thickness", sdf.p[0]), get_opt(e, "whd", whd);
          sdf.p[1] = whd.x, sdf.p[2] = whd.y, sdf.p[3] = whd.z;  // sdf.whd stays 0 (sceneio:3685-3692)
        } break;
        case sdf_type::box: get_opt(e, "whd", sdf.whd); break;
        case sdf_type::capped_cone:
          get_opt(e, "height", sdf.p[0]), get_opt(e, "r1", sdf.p[1]), get_opt(e, "r2", sdf.p[2]);
          break;
        case sdf_type::plane: break;
        case sdf_type::sphere: get_opt(e, "radius", sdf.p[0]); break;
        case sdf_type::torus: get_opt(e, "r1", sdf.p[0]), get_opt(e, "r2", sdf.p[1]); break;
      }
    }
    for (auto& e : group("subdivs")) {   // yocto_sceneio.cpp:3733-3751
      auto& subdiv = scene.subdivs.emplace_back();
      get_opt(e, "uri", subdiv_uris.emplace_back());
      get_opt(e, "shape", subdiv.shape), get_opt(e, "subdivisions", subdiv.subdivisions);
      get_opt(e, "catmullclark", subdiv.catmullclark), get_opt(e, "smooth", subdiv.smooth);
      get_opt(e, "displacement", subdiv.displacement), get_opt(e, "displacement_tex", subdiv.displacement_tex);
    }
    for (auto& e : group("instances")) {
      auto& instance = scene.instances.emplace_back();
      get_opt(e, "frame", instance.frame), get_opt(e, "shape", instance.shape);
      get_opt(e, "material", instance.material);
    }
    for (auto& e : group("vol_instances")) {
      auto& instance = scene.vol_instances.emplace_back();
      get_opt(e, "frame", instance.frame), get_opt(e, "volume", instance.volume);
      get_opt(e, "scale", instance.scalef), get_opt(e, "material", instance.material);
    }
    for (auto& e : group("environments")) {
      auto& environment = scene.environments.emplace_back();
      get_opt(e, "frame", environment.frame), get_opt(e, "emission", environment.emission);
      get_opt(e, "emission_tex", environment.emission_tex);
    }
  } catch (...) {
    return parse_error();
  }

  auto dirname = path_dirname(filename);
  auto dependent_error = [&]() {
    error = filename + ": error in " + error;
    return false;
  };
  for (size_t i = 0; i < scene.shapes.size(); i++)
    if (!load_shape(path_join(dirname, shape_uris[i]), scene.shapes[i], error, true)) return dependent_error();
  // add_missing_radius (yocto_sceneio.cpp:2071-2076, called at the end of load_json_scene)
  for (auto& shape : scene.shapes)
    if ((!shape.points.empty() || !shape.lines.empty()) && shape.radius.empty()) shape.radius.assign(shape.positions.size(), 0.001f);
  for (size_t i = 0; i < scene.volumes.size(); i++)
    if (!load_volume(path_join(dirname, volume_uris[i]), scene.volumes[i], volume_binary[i], error)) return dependent_error();
  for (size_t i = 0; i < scene.subdivs.size(); i++)
    if (!load_subdiv(path_join(dirname, subdiv_uris[i]), scene.subdivs[i], error)) return dependent_error();
  for (size_t i = 0; i < scene.textures.size(); i++)
    if (!load_texture(path_join(dirname, texture_uris[i]), scene.textures[i], error)) return dependent_error();

  // add_missing_camera is not restated: every BASELINE scene has cameras
  if (scene.cameras.empty()) {
    error = filename + ": no camera";
    return false;
  }
  // index validation (the reference trusts the file; the device path must not)
  auto bad = [&](int v, size_t n, bool optional) { return optional ? (v < -1 || v >= (int)n) : (v < 0 || v >= (int)n); };
  for (auto& i : scene.instances)
    if (bad(i.shape, scene.shapes.size(), false) || bad(i.material, scene.materials.size(), false)) return parse_error();
  for (auto& m : scene.materials)
    for (auto t : {m.emission_tex, m.color_tex, m.roughness_tex, m.scattering_tex, m.normal_tex}) (void)t;
  for (auto& e : scene.environments)
    if (bad(e.emission_tex, scene.textures.size(), true)) return parse_error();
  for (auto& i : scene.vol_instances)
    if (bad(i.volume, scene.volumes.size(), false) || bad(i.material, scene.materials.size(), false)) return parse_error();
  for (auto& s : scene.sdfs)
    if (bad(s.material, scene.materials.size(), false)) return parse_error();
  for (auto& s : scene.subdivs)
    if (bad(s.shape, scene.shapes.size(), false) || bad(s.displacement_tex, scene.textures.size(), true) || s.subdivisions < 0 || s.subdivisions > 10)
      return parse_error();
  return true;
}

// ---------------------------------------------------------------------------------------------
// output: linear float -> sRGB bytes (yocto_color.h:207-231), PNG writer
// ---------------------------------------------------------------------------------------------
vector<vec4b> linear_to_srgb8(const color_image& image) {
  auto out   = vector<vec4b>(image.pixels.size());
  auto curve = [](float rgb) { return (rgb <= 0.0031308f) ? 12.92f * rgb : (1 + 0.055f) * std::pow(rgb, 1 / 2.4f) - 0.055f; };
  auto quant = [](float a) {
    auto v = (int)(a * 256);
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  };
  for (size_t i = 0; i < out.size(); i++) {
    auto& p = image.pixels[i];
    out[i]  = {quant(curve(p.x)), quant(curve(p.y)), quant(curve(p.z)), quant(p.w)};
  }
  return out;
}

vector<uint8_t> encode_png(int width, int height, const vector<vec4b>& rgba) {
  auto raw = vector<uint8_t>(((size_t)width * 4 + 1) * height);
  for (auto y = 0; y < height; y++) {
    raw[(size_t)y * (width * 4 + 1)] = 0;
    memcpy(&raw[(size_t)y * (width * 4 + 1) + 1], &rgba[(size_t)y * width], (size_t)width * 4);
  }
  auto bound = compressBound((uLong)raw.size());
  auto comp  = vector<uint8_t>(bound);
  compress2(comp.data(), &bound, raw.data(), (uLong)raw.size(), 6);
  comp.resize(bound);
  auto out   = vector<uint8_t>{0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  auto chunk = [&](const char* type, const vector<uint8_t>& body) {
    auto len = (uint32_t)body.size();
    for (auto s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(len >> s));
    auto start = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), body.begin(), body.end());
    auto crc = (uint32_t)crc32(0, &out[start], (uInt)(out.size() - start));
    for (auto s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(crc >> s));
  };
  auto ihdr = vector<uint8_t>(13);
  for (auto k = 0; k < 4; k++) ihdr[k] = (uint8_t)(width >> (24 - 8 * k)), ihdr[4 + k] = (uint8_t)(height >> (24 - 8 * k));
  ihdr[8] = 8, ihdr[9] = 6;
  chunk("IHDR", ihdr), chunk("IDAT", comp), chunk("IEND", {});
  return out;
}

bool save_image(const string& filename, const color_image& image, string& error) {
  auto ext   = path_extension(filename);
  auto bytes = vector<uint8_t>{};
  // save_image on a linear image converts to sRGB bytes first (yocto_sceneio.cpp:523-531, 565-571)
  auto ldr = image.linear ? linear_to_srgb8(image) : vector<vec4b>{};
  if (!image.linear) {
    ldr.resize(image.pixels.size());
    for (size_t i = 0; i < ldr.size(); i++) {
      auto q = [](float a) { auto v = (int)(a * 256); return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
      ldr[i] = {q(image.pixels[i].x), q(image.pixels[i].y), q(image.pixels[i].z), q(image.pixels[i].w)};
    }
  }
  if (ext == ".png") bytes = encode_png(image.width, image.height, ldr);
  else if (ext == ".jpg" || ext == ".jpeg") bytes = encode_jpeg_q75(image.width, image.height, ldr);
  else if (ext == ".raw") {  // float32 RGBA dump, for tools
    bytes.resize(image.pixels.size() * 16);
    memcpy(bytes.data(), image.pixels.data(), bytes.size());
  } else {
    error = filename + ": unknown format";
    return false;
  }
  auto f = fopen(filename.c_str(), "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    if (f) fclose(f);
    error = filename + ": write error";
    return false;
  }
  fclose(f);
  return true;
}

// A JSON array of camera objects with the keys of a scene file's "cameras" entries (ypathtrace --cameras)
bool load_cameras(const string& filename, vector<camera_data>& cameras, string& error) {
  cameras.clear();
  auto data = vector<uint8_t>{};
  if (!read_file(filename, data, error)) return false;
  try {
    auto parser = json_parser{(const char*)data.data(), (const char*)data.data() + data.size()};
    auto js     = parser.parse();
    if (js.kind != json_value::array_k || js.items.empty()) throw std::runtime_error{"json"};
    for (auto& e : js.items) {
      if (e.kind != json_value::object_k) throw std::runtime_error{"json"};
      read_camera(e, cameras.emplace_back());
    }
  } catch (const std::exception&) {
    error = filename + ": parse error";
    return false;
  }
  return true;
}

// A --config file of the reference's command line (yocto_cli.cpp:912-945): one JSON object whose members are option
// values.  Returned as (name, text) pairs - strings as they are, numbers printed, booleans "true" / "false" - for the
// application's own option table to validate.
bool load_cli_config(const string& filename, vector<std::pair<string, string>>& options, string& error) {
  auto data = vector<uint8_t>{};
  auto ioerror = string{};
  if (!read_file(filename, data, ioerror)) {
    error = "missing configuration file " + filename;
    return false;
  }
  auto js = json_value{};
  try {
    auto parser = json_parser{(const char*)data.data(), (const char*)data.data() + data.size()};
    js          = parser.parse();
  } catch (const std::exception&) {
    error = "error converting configuration " + filename;
    return false;
  }
  if (js.kind != json_value::object_k) {
    error = "error converting configuration " + filename;
    return false;
  }
  for (auto& [key, v] : js.members) {
    char buf[64];
    switch (v.kind) {
      case json_value::string_k: options.emplace_back(key, v.text); break;
      case json_value::bool_k: options.emplace_back(key, v.boolean ? "true" : "false"); break;
      case json_value::number_k:
        if (v.number == (double)(long long)v.number) snprintf(buf, sizeof(buf), "%lld", (long long)v.number);
        else snprintf(buf, sizeof(buf), "%.17g", v.number);
        options.emplace_back(key, buf);
        break;
      default: error = "bad value for " + key; return false;
    }
  }
  return true;
}

}  // namespace vpt

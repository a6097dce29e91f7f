// yk_loaders_internal.h — what the scene loaders share: the loaded-scene container behind yk_loaded_scene_get, the PLY reader
// (scene/ply.rs), Mesh::new, the transform helpers and the thread pool that reads a scene's PLY files.  Defined in yk_loaders.cpp,
// used by yk_mitsuba.cpp.  Host only.
#pragma once
#include <string>
#include <vector>

#include "../../include/yuki_hip.h"
#include "yk_host.h"
#include "yk_math.h"

struct yk_loaded_scene {
    std::vector<float> points, normals, uvs;
    std::vector<uint32_t> indices, tri_mesh;
    std::vector<uint32_t> shape_order, shape_order_flat;  // file order of shapes: triangle id | 0x80000000+sphere id
    std::vector<int32_t> tri_material, tri_area_light;
    std::vector<yk_mesh_desc> meshes;
    std::vector<yk_sphere_desc> spheres;
    std::vector<yk_material_desc> materials;
    std::vector<yk_light_desc> lights;
    std::vector<std::vector<float>> texture_data;
    std::vector<yk_texture_desc> textures;
    float background[3] = {0, 0, 0};
    yk_camera_params camera;
    uint16_t tile_dim = 16;
    uint32_t split_method = YK_SPLIT_SAH, max_shapes_in_node = 1;
    bool any_normals = false, any_uvs = false;
};

// sets the calling thread's yk_loader_last_error() and returns st
yk_status lfail(yk_status st, const std::string& msg);
yk_material_desc make_mat(uint32_t kind, const float a[3], const float b[3], float c, bool remap);
// CameraParameters::default (camera.rs:32-41) + FilmSettings::default (film.rs:28-38)
void default_camera(yk_loaded_scene& s);

// The payload of one PLY file as ply::load reads it (scene/ply.rs:19-130), before any transform.
struct PlyMesh {
    std::vector<float> pts, nrm, uv;
    std::vector<uint32_t> indices;
};
yk_status read_ply_mesh(const std::string& path, PlyMesh& out);
// Mesh::new for a PLY payload.  No transform given (Scene::ply): scale / translate into the unit cube (ply.rs:99-108).
void add_ply_mesh(yk_loaded_scene& s, const PlyMesh& m, const yk::Xf* transform, int material);

// One PLY file of a scene file, read after the parse.  read_ply_jobs reads them with a few threads (YK_LOADER_THREADS overrides
// the count), each into its own job; status / error hold what read_ply_mesh returned for that file.
struct PlyJob {
    std::string ply_path;
    PlyMesh ply;
    yk_status status = YK_OK;
    std::string error;
    bool all_referenced = false;  // every vertex of the file belongs to a triangle (so vertex bounds are shape bounds)
};
void read_ply_jobs(const std::vector<PlyJob*>& jobs, bool find_stray_vertices = false);  // true: fill all_referenced

// transforms::rotation, math/transforms.rs:98-127 (sin/cos through yk_libm.h: glibc's sinf / cosf)
yk::Xf loader_rotation(float theta, yk::V3 axis);
// str::parse::<f32/f64> grammar (core::num::dec2flt): [+-]? (inf | infinity | nan | digits[.digits][e[+-]digits])
bool rust_float_grammar(const std::string& s);

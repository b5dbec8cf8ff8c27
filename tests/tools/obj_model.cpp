// CPU model of row f9 (DESIGN.md section 4 "Model output"): the .obj and .mtl text of build_model + ObjModel::save +
// MaterialLib::save_to_files, in upstream's order of loops, with the C++ library doing the formatting:
// std::ostringstream << std::fixed << std::setprecision(6), exactly the stream state upstream's std::ofstream is in.  Test infrastructure
// only; driven by obj_model.py.
#include <stdint.h>
#include <string.h>
#include <iomanip>
#include <sstream>
#include <string>

namespace {
struct Result { std::string obj, mtl; };

std::string filled(uint32_t n, int width) {   // util::string::get_filled: decimal, zero-filled to at least `width` characters
    std::string s = std::to_string(n);
    return s.size() < (size_t)width ? std::string((size_t)width - s.size(), '0') + s : s;
}
}  // namespace

extern "C" {

// verts [3 NV], mesh_faces [3 F], normals [3 NV] or null (no vn lines, faces V/T), face_ptr / tc_ptr [A + 1], faces [face_ptr[A]],
// merged [2 tc_ptr[A]], ids [3 face_ptr[A]]
void* obj_model_run(uint32_t NV, const float* verts, const uint32_t* mesh_faces, const float* normals, uint32_t A, const uint32_t* face_ptr,
                    const uint32_t* faces, const uint32_t* tc_ptr, const float* merged, const uint32_t* ids, const char* name) {
    Result* r = new Result();
    std::ostringstream out;
    out << "mtllib " << name << ".mtl" << '\n';
    out << std::fixed << std::setprecision(6);
    for (uint32_t i = 0; i < NV; ++i) out << "v " << verts[3 * (size_t)i] << " " << verts[3 * (size_t)i + 1] << " " << verts[3 * (size_t)i + 2] << '\n';
    const uint32_t NM = A ? tc_ptr[A] : 0u;
    for (uint32_t i = 0; i < NM; ++i) out << "vt " << merged[2 * (size_t)i] << " " << 1.0f - merged[2 * (size_t)i + 1] << '\n';
    if (normals)
        for (uint32_t i = 0; i < NV; ++i) out << "vn " << normals[3 * (size_t)i] << " " << normals[3 * (size_t)i + 1] << " " << normals[3 * (size_t)i + 2] << '\n';
    std::ostringstream mtl;
    for (uint32_t a = 0; a < A; ++a) {
        const std::string material = "material" + filled(a, 4);
        out << "usemtl " << material << '\n';
        for (uint32_t e = face_ptr[a]; e < face_ptr[a + 1]; ++e) {
            out << "f";
            for (int k = 0; k < 3; ++k) {
                const size_t v = (size_t)mesh_faces[3 * (size_t)faces[e] + k] + 1, t = (size_t)tc_ptr[a] + ids[3 * (size_t)e + k] + 1;
                out << " " << v << "/" << t;
                if (normals) out << "/" << v;
            }
            out << '\n';
        }
        mtl << "newmtl " << material << '\n'
            << "Ka 1.000000 1.000000 1.000000" << '\n'
            << "Kd 1.000000 1.000000 1.000000" << '\n'
            << "Ks 0.000000 0.000000 0.000000" << '\n'
            << "Tr 0.000000" << '\n'
            << "illum 1" << '\n'
            << "Ns 1.000000" << '\n'
            << "map_Kd " << name << "_" << material << "_map_Kd.png" << '\n';
    }
    r->obj = out.str(); r->mtl = mtl.str();
    return r;
}

// n floats, one per line, as the stream prints them
void* obj_model_floats(uint64_t n, const float* x) {
    Result* r = new Result();
    std::ostringstream out;
    out << std::fixed << std::setprecision(6);
    for (uint64_t i = 0; i < n; ++i) out << x[i] << '\n';
    r->obj = out.str();
    return r;
}

const char* obj_model_text(void* h, int which, uint64_t* n) {
    const std::string& s = which ? ((Result*)h)->mtl : ((Result*)h)->obj;
    *n = s.size();
    return s.data();
}

void obj_model_free(void* h) { delete (Result*)h; }

}  // extern "C"

// model_corner.h -- one corner of an atlas set's face list as the model writers read it (rows f9 and f11; DESIGN.md section 4 "Model output"
// items 1, 6 and 8): its mesh vertex, its global texture coordinate, and the two id rules of item 6, written once for k_model.hip and
// k_glb.hip.  Device code, header-only; nothing is read out of bounds for a bad id.
#pragma once
#include <stdint.h>

namespace mvs {

struct ModelCorner {
    uint32_t v, g;         // mesh vertex mesh_faces[3 faces[e] + k] (0 when the face id is bad); tc0 + texcoord_ids[3 e + k] (0 when the id is bad)
    bool face_ok, id_ok;   // faces[e] < F; texcoord_ids[3 e + k] < tcn
};

// corner k of list entry e, which lies in an atlas whose coordinates are [tc0, tc0 + tcn)
__device__ inline ModelCorner model_corner(const uint32_t* __restrict__ mesh_faces, uint32_t F, const uint32_t* __restrict__ faces, const uint32_t* __restrict__ ids,
                                           uint32_t tc0, uint32_t tcn, uint32_t e, uint32_t k) {
    const uint32_t f = faces[e], id = ids[3 * (size_t)e + k];
    ModelCorner c;
    c.face_ok = f < F; c.id_ok = id < tcn;
    c.v = c.face_ok ? mesh_faces[3 * (size_t)f + k] : 0u;
    c.g = c.id_ok ? tc0 + id : 0u;
    return c;
}

// the atlas of list entry e (or of anything else counted by an ascending ptr [A + 1] that starts at 0): the last a < A with ptr[a] <= e
__device__ inline uint32_t model_range_of(const uint32_t* __restrict__ ptr, uint32_t A, uint32_t e) {
    uint32_t lo = 0, hi = A;
    while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (ptr[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

}  // namespace mvs

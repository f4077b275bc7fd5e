// nr_mesh.h — what the mesh front end (nr_mesh.hip), the skin pass
// (nr_skin.hip) and the morph pass (nr_morph.hip) share: the Mesh handle, the
// pinned hand-off buffers of a host call's small per-draw arrays, the timed
// launch of a pass, the error latch of an entry point, and the MeshSkin handle
// with its bone loads (the skin kernel and the fused morph-and-skin kernel).
#pragma once
#include "nr_tri.h"

#include <string>

// Latches "<what>: <why>" and returns false.
inline bool fail(const char* what, const char* why) {
    nr_set_error_msg((std::string(what) + ": " + why).c_str());
    return false;
}

inline unsigned blocks_for(i64 threads) { return (unsigned)((threads + 255) / 256); }

// One pass of a mesh call: `kernel` over `threads` threads in blocks of 256 on the context's stream, reported
// under the timing id `kid`.
template <class K, class... A>
void mesh_launch(RenderContext* ctx, int kid, K kernel, i64 threads, A... args) {
    hipEvent_t a, b;
    nr_timing_begin(ctx, kid, &a, &b);
    hipLaunchKernelGGL(kernel, dim3(blocks_for(threads)), dim3(256), 0, ctx->stream, args...);
    NR_CHECK(hipGetLastError());
    nr_timing_end(ctx, kid, a, b);
}

struct Mesh {
    i64 nv = 0, n = 0;
    int mode = nrtri::ATTR_FLAT;   // AttrMode of the expanded attributes
    bool opaque = false;           // colour mesh: every vertex alpha == 1 (textured: decided per draw by the texture;
                                   // textured colour: by both)
    int device = 0;
    f64* pos = nullptr;            // nv*3
    u32* idx = nullptr;            // n*3, every entry < nv (checked on the host at creation)
    f64* attr = nullptr;           // expanded: n*12 Gouraud, n*4 flat (the colour of i0), n*6 textured, n*18 textured colour
    // a lit mesh (CreateLitMesh) also keeps what the light pass reads: the per-vertex colours and normals
    bool lit = false;
    f64* rgba = nullptr;           // nv*4 (with n > 0)
    f64* normal = nullptr;         // nv*3
    f64* uv = nullptr;             // nv*2: a textured colour mesh (ATTR_TEXC) also keeps its uv, and its rgba above whether lit or not
};
// pos and normal are read only by the vertex, clip-vertex and light kernels that a draw or Assemble* call
// launches on the device's main stream (nr_stream_for), and rgba only by the light kernels: a pending batch, or
// its overflow re-run, reads the context's staging and the expanded attr.  So a kernel on that stream that
// rewrites pos or normal (PoseMesh, nr_skin.hip; MorphMesh, nr_morph.hip) is ordered between the draws around it with no host wait.

// One of the context's two pinned buffers (TriScratch::h_minst), in turn, grown to `need` doubles, for the next
// asynchronous host-to-device copy of a call's matrices: the host waits only for the copy of the call before
// last, long done.  The caller fills it, enqueues its copy on the context's stream and records
// sc.evMinst[*slot] behind it.  Null: hipHostMalloc failed (nothing latched).
inline f64* nr_mesh_pinned(TriScratch& sc, size_t need, int* slot) {
    const int k = sc.minstNext;
    sc.minstNext ^= 1;
    if (sc.evMinst[k]) NR_CHECK(hipEventSynchronize(sc.evMinst[k]));
    else NR_CHECK(hipEventCreateWithFlags(&sc.evMinst[k], hipEventDisableTiming));
    if (sc.h_minst_cap[k] < need) {
        if (sc.h_minst[k]) NR_CHECK(hipHostFree(sc.h_minst[k]));
        sc.h_minst[k] = nullptr;
        sc.h_minst_cap[k] = 0;
        if (hipHostMalloc((void**)&sc.h_minst[k], need * sizeof(f64)) != hipSuccess) {
            (void)hipGetLastError();
            sc.h_minst[k] = nullptr;
            return nullptr;
        }
        sc.h_minst_cap[k] = need;
    }
    *slot = k;
    return sc.h_minst[k];
}

// ---- skinning: the handle and the loads of a bone (DESIGN.md §3 "Skinned meshes") ----
struct MeshSkin {
    i64 nv = 0, nb = 0;
    int device = 0;
    f64* pos = nullptr;        // bind positions nv*3
    f64* normal = nullptr;     // bind normals nv*3, or null
    u32* joints = nullptr;     // nv*4, every entry < nb
    f64* weights = nullptr;    // nv*4
    f64* palette = nullptr;    // nb*12: where a host palette lands (PoseMesh)
    int variant = 0;           // kernel: 0 automatic, 1 palette from global memory, 2 staged in LDS (SetMeshSkinVariant)
};

struct Bone { f64 m[12]; };   // only ever indexed by constants: registers

// Entries of bone j as six 16-byte loads; lanes of a wave that share a bone hit the same lines (cache-resident:
// the palette is nb*96 bytes).
__device__ __forceinline__ Bone load_bone(const double2* __restrict__ palette, u32 j) {
    const double2* p = palette + (size_t)j * 6;
    Bone B;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        const double2 q = p[e];
        B.m[2 * e] = q.x;
        B.m[2 * e + 1] = q.y;
    }
    return B;
}

// The LDS variant: the block first copies the whole palette (nb <= SKIN_LDS_MAX_BONES) into LDS, a bone every
// SKIN_LDS_STRIDE doubles -- 13, odd, so that lanes reading the same entry of different bones with 8-byte reads
// spread over the banks -- and every lane then reads its four bones from there.
constexpr int SKIN_LDS_MAX_BONES = 128;
constexpr int SKIN_LDS_STRIDE = 13;

__device__ __forceinline__ Bone load_bone_lds(const f64* sh, u32 j) {
    const f64* p = sh + j * (u32)SKIN_LDS_STRIDE;
    Bone B;
#pragma unroll
    for (int e = 0; e < 12; ++e) B.m[e] = p[e];
    return B;
}


// nr_skin.hip — skinned meshes: linear-blend skinning on the device (DESIGN.md
// §3 "Skinned meshes").
//
// A MeshSkin keeps a bind pose in HBM: nv positions, optionally nv normals, four
// joints (u32) and four weights (f64) per vertex, for nb bones.  PoseMesh hands
// over a palette of nb row-major 3x4 matrices [R | t] and ONE kernel rewrites
// the mesh's positions (and, for a lit mesh posed with a skin that has normals,
// its normals) from the bind pose; every draw issued afterwards reads the posed
// arrays through the vertex, clip-vertex and light kernels it has always run.
//
// Per vertex, f64, every product and sum rounded in the order written (the build
// has no FMA contraction); no division, no sqrt, no renormalisation; with
// B_k = palette[j_k], k = 0 .. 3, all four always evaluated:
//   x_k = ((B_k[0]*px + B_k[1]*py) + B_k[2]*pz) + B_k[3]     y_k: entries 4..7, z_k: entries 8..11
//   X   = ((w0*x_0 + w1*x_1) + w2*x_2) + w3*x_3              Y, Z likewise
//   a_k = (B_k[0]*nx + B_k[1]*ny) + B_k[2]*nz                b_k: entries 4..6, c_k: entries 8..10
//   NX  = ((w0*a_0 + w1*a_1) + w2*a_2) + w3*a_3              NY, NZ likewise
// Joints are checked against nb on the host at creation, zero-weight ones
// included, so no kernel sees an index outside the palette.
//
// Ordering without a host wait: the mesh's positions and normals are read only by
// kernels that draws launch on the device's main stream (nr_mesh.h), and the
// skin kernel runs on that stream, so it falls between the draws issued before
// and after the call.  A host palette travels through the context's two pinned
// buffers in turn (DrawMeshInstanced's hand-off) into the skin's own device copy
// by one asynchronous copy on the same stream.
#include "nr_mesh.h"

#include <cstdint>
#include <cstring>

namespace {

// One thread per vertex: 24 B of bind position, one 16-byte load of joints, two of weights, four bones of 96 B
// through the per-lane joints, 24 B out; NRM: the same for the normal under each bone's 3x3.
template <bool NRM, bool LDS>
__global__ __launch_bounds__(256) void k_mesh_skin(const f64* __restrict__ bpos, const f64* __restrict__ bnrm,
                                                   const uint4* __restrict__ joints,
                                                   const double2* __restrict__ weights,
                                                   const double2* __restrict__ palette, u32 nb, i64 nv,
                                                   f64* __restrict__ pos, f64* __restrict__ nrm) {
    __shared__ f64 sh[LDS ? SKIN_LDS_MAX_BONES * SKIN_LDS_STRIDE : 1];
    if constexpr (LDS) {
        for (u32 i = threadIdx.x; i < nb * 6u; i += 256u) {   // (nb <= SKIN_LDS_MAX_BONES: checked by the launch)
            const double2 q = palette[i];
            const u32 b = i / 6u, e = i - b * 6u;
            sh[b * (u32)SKIN_LDS_STRIDE + 2u * e] = q.x;
            sh[b * (u32)SKIN_LDS_STRIDE + 2u * e + 1u] = q.y;
        }
        __syncthreads();
    }
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const uint4 j4 = joints[v];
    const double2 wa = weights[v * 2], wb = weights[v * 2 + 1];
    const u32 j[4] = {j4.x, j4.y, j4.z, j4.w};
    const f64 w[4] = {wa.x, wa.y, wb.x, wb.y};
    const f64 px = bpos[v * 3], py = bpos[v * 3 + 1], pz = bpos[v * 3 + 2];
    f64 nx = 0, ny = 0, nz = 0;
    if constexpr (NRM) {
        nx = bnrm[v * 3];
        ny = bnrm[v * 3 + 1];
        nz = bnrm[v * 3 + 2];
    }
    f64 X = 0, Y = 0, Z = 0, NX = 0, NY = 0, NZ = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Bone B = LDS ? load_bone_lds(sh, j[k]) : load_bone(palette, j[k]);
        const f64 xk = ((B.m[0] * px + B.m[1] * py) + B.m[2] * pz) + B.m[3];
        const f64 yk = ((B.m[4] * px + B.m[5] * py) + B.m[6] * pz) + B.m[7];
        const f64 zk = ((B.m[8] * px + B.m[9] * py) + B.m[10] * pz) + B.m[11];
        // ((w0*x_0 + w1*x_1) + w2*x_2) + w3*x_3, left to right (the first term starts the sum: no 0 + ...)
        X = k == 0 ? w[k] * xk : X + w[k] * xk;
        Y = k == 0 ? w[k] * yk : Y + w[k] * yk;
        Z = k == 0 ? w[k] * zk : Z + w[k] * zk;
        if constexpr (NRM) {
            const f64 ak = (B.m[0] * nx + B.m[1] * ny) + B.m[2] * nz;
            const f64 bk = (B.m[4] * nx + B.m[5] * ny) + B.m[6] * nz;
            const f64 ck = (B.m[8] * nx + B.m[9] * ny) + B.m[10] * nz;
            NX = k == 0 ? w[k] * ak : NX + w[k] * ak;
            NY = k == 0 ? w[k] * bk : NY + w[k] * bk;
            NZ = k == 0 ? w[k] * ck : NZ + w[k] * ck;
        }
    }
    pos[v * 3] = X;
    pos[v * 3 + 1] = Y;
    pos[v * 3 + 2] = Z;
    if constexpr (NRM) {
        nrm[v * 3] = NX;
        nrm[v * 3 + 1] = NY;
        nrm[v * 3 + 2] = NZ;
    }
}

void free_skin(MeshSkin* s) {
    for (void* p : {(void*)s->pos, (void*)s->normal, (void*)s->joints, (void*)s->weights, (void*)s->palette})
        if (p) NR_CHECK(hipFree(p));
    delete s;
}

// PoseMesh and PoseMeshDevice under the caller's name: every check, then (a host palette) its hand-off, then the
// one kernel, on the context's stream.  Nothing here waits for the device but the pinned buffer's turn.
bool pose(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, bool onDevice, const char* what) {
    if (!ctx) return fail(what, "NULL context");
    if (!m) return fail(what, "NULL mesh");
    if (!s) return fail(what, "NULL skin");
    if (!palette) return fail(what, "NULL palette");
    if (m->nv != s->nv) return fail(what, "the mesh and the skin differ in their vertex count");
    if (m->device != ctx->device || s->device != ctx->device)
        return fail(what, "mesh, skin and context are not on one device");
    if (onDevice && (reinterpret_cast<uintptr_t>(palette) & 15u) != 0)
        return fail(what, "a device palette must be 16-byte aligned");
    if (s->nv == 0) return true;
    NR_CHECK(hipSetDevice(ctx->device));
    const f64* dpal = palette;
    if (!onDevice) {
        const size_t need = (size_t)s->nb * 12;
        int slot = 0;
        f64* h = nr_mesh_pinned(ctx->tri, need, &slot);
        if (!h) return fail(what, "hipHostMalloc failed");
        std::memcpy(h, palette, need * sizeof(f64));
        // (behind the skin kernel of an earlier call on this stream, which read the previous palette)
        NR_CHECK(hipMemcpyAsync(s->palette, h, need * sizeof(f64), hipMemcpyHostToDevice, ctx->stream));
        NR_CHECK(hipEventRecord(ctx->tri.evMinst[slot], ctx->stream));
        dpal = s->palette;
    }
    const bool nrm = m->lit && s->normal != nullptr;
    const bool lds = s->variant != 1 && s->nb <= (i64)SKIN_LDS_MAX_BONES;
    const auto kernel = lds ? (nrm ? k_mesh_skin<true, true> : k_mesh_skin<false, true>)
                            : (nrm ? k_mesh_skin<true, false> : k_mesh_skin<false, false>);
    mesh_launch(ctx, NRK_MESH_SKIN, kernel, s->nv, s->pos, s->normal, reinterpret_cast<const uint4*>(s->joints),
                reinterpret_cast<const double2*>(s->weights), reinterpret_cast<const double2*>(dpal), (u32)s->nb, s->nv,
                m->pos, m->normal);
    return true;
}

// nv*3 doubles of a mesh array to the host, behind everything enqueued on the device's main stream.
bool read_back(const Mesh* m, const f64* src, f64* out) {
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    NR_CHECK(hipSetDevice(m->device));
    hipStream_t st = nr_stream_for(m->device);
    NR_CHECK(hipMemcpyAsync(out, src, (size_t)m->nv * 3 * sizeof(f64), hipMemcpyDeviceToHost, st));
    NR_CHECK(hipStreamSynchronize(st));
    NR_CHECK(hipSetDevice(prev));
    return true;
}

}  // namespace

extern "C" {

// New: the bind pose of nv vertices for nb bones, uploaded once to the current device.  bindNormal NULL: a skin
// that poses positions only.  NULL + error (nothing allocated) for a negative or > 32-bit nv, nb <= 0 or beyond
// 32 bits, a NULL array with nv > 0, or any joint >= nb -- zero-weight joints included.  Weights are not validated.
MeshSkin* CreateMeshSkin(i64 nv, const f64* bindPos, const f64* bindNormal, const uint32_t* joints, const f64* weights,
                         i64 nb) {
    const char* what = "CreateMeshSkin";
    const char* why = nullptr;
    if (nv < 0) why = "negative vertex count";
    else if (nv > (i64)0xFFFFFFFFll) why = "vertex count beyond 32 bits";
    else if (nb <= 0) why = "the bone count must be positive";
    else if (nb > (i64)0xFFFFFFFFll) why = "bone count beyond 32 bits";
    else if (nv > 0 && !bindPos) why = "NULL bind positions";
    else if (nv > 0 && !joints) why = "NULL joints";
    else if (nv > 0 && !weights) why = "NULL weights";
    if (!why)
        for (i64 k = 0; k < nv * 4; ++k)
            if ((i64)joints[k] >= nb) { why = "joint out of range (>= bone count)"; break; }
    if (why) {
        fail(what, why);
        return nullptr;
    }
    MeshSkin* s = new MeshSkin();
    s->nv = nv;
    s->nb = nb;
    NR_CHECK(hipGetDevice(&s->device));
    if (nv == 0) return s;
    const size_t n = (size_t)nv;
    bool ok = hipMalloc(&s->pos, n * 3 * sizeof(f64)) == hipSuccess &&
              hipMalloc(&s->joints, n * 4 * sizeof(u32)) == hipSuccess &&
              hipMalloc(&s->weights, n * 4 * sizeof(f64)) == hipSuccess &&
              hipMalloc(&s->palette, (size_t)nb * 12 * sizeof(f64)) == hipSuccess;
    if (ok && bindNormal) ok = hipMalloc(&s->normal, n * 3 * sizeof(f64)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fail(what, "hipMalloc failed");
        free_skin(s);
        return nullptr;
    }
    hipStream_t st = nr_stream_for(s->device);
    NR_CHECK(hipMemcpyAsync(s->pos, bindPos, n * 3 * sizeof(f64), hipMemcpyHostToDevice, st));
    if (bindNormal) NR_CHECK(hipMemcpyAsync(s->normal, bindNormal, n * 3 * sizeof(f64), hipMemcpyHostToDevice, st));
    NR_CHECK(hipMemcpyAsync(s->joints, joints, n * 4 * sizeof(u32), hipMemcpyHostToDevice, st));
    NR_CHECK(hipMemcpyAsync(s->weights, weights, n * 4 * sizeof(f64), hipMemcpyHostToDevice, st));
    NR_CHECK(hipStreamSynchronize(st));   // caller may reuse its arrays on return
    return s;
}

// Waits for the device's main stream (a skin kernel may still read the arrays), as DestroyMesh does.
void DestroyMeshSkin(MeshSkin* s) {
    if (!s) return;
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    NR_CHECK(hipSetDevice(s->device));
    NR_CHECK(hipStreamSynchronize(nr_stream_for(s->device)));
    free_skin(s);
    NR_CHECK(hipSetDevice(prev));
}

i64 GetMeshSkinBoneCount(MeshSkin* s) { return s->nb; }

// New (A/B and tests): the skin kernel of this skin's poses: 0 automatic, 1 the palette read from global memory,
// 2 staged in LDS (at most 128 bones; above that the global path whatever the mode).  The results are the same bits.
void SetMeshSkinVariant(MeshSkin* s, i64 mode) { s->variant = mode == 1 || mode == 2 ? (int)mode : 0; }

// New: poses `m` from the skin's bind pose under `palette` (nb*12, host; the caller's again on return): its
// positions, and its normals when the mesh is lit and the skin has bind normals.  Draws issued before the call
// keep the old pose, draws issued after it see the new one; the host waits for nothing.
bool PoseMesh(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette) {
    return pose(ctx, m, s, palette, false, "PoseMesh");
}

// New: the same from a device-resident palette (16-byte aligned; as DrawTrianglesDevice: valid and unchanged until
// the call's kernel has executed).  Only the kernel launched inside the call reads it.
bool PoseMeshDevice(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette) {
    return pose(ctx, m, s, palette, true, "PoseMeshDevice");
}

// New: the mesh's current positions (nv*3) on the host: a sync point.
bool GetMeshPositions(Mesh* m, f64* out) {
    if (!m) return fail("GetMeshPositions", "NULL mesh");
    if (m->nv == 0) return true;
    if (!out) return fail("GetMeshPositions", "NULL output");
    return read_back(m, m->pos, out);
}

// New: the current normals (nv*3) of a lit mesh.
bool GetMeshNormals(Mesh* m, f64* out) {
    if (!m) return fail("GetMeshNormals", "NULL mesh");
    if (!m->lit) return fail("GetMeshNormals", "a mesh without normals (create it with CreateLitMesh)");
    if (m->nv == 0) return true;
    if (!out) return fail("GetMeshNormals", "NULL output");
    return read_back(m, m->normal, out);
}

}  // extern "C"

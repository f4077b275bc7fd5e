// nr_mesh.hip — indexed 3D meshes: a front end of the triangle path.
//
// A Mesh is nv positions (px, py, pz), n index triples and one per-vertex
// attribute (RGBA, or texel-unit UVs), uploaded once.  DrawMesh transforms the
// vertices by a row-major 4x4 matrix on the device (the vertex stage, DESIGN.md
// §3), gathers them through the indices into the soup layout of
// DrawTrianglesDevice (assembly) and hands the soup to nrtri::draw: binning,
// coverage, depth, interpolation and blending are those of any soup batch, and
// a triangle with a vertex at cw <= 0 (NaN position) is dropped by the rasters'
// own finiteness test.
//
// Vertex stage, f64, every product and sum rounded, left to right (the build
// has no FMA contraction):
//   cx = ((M[0]*px + M[1]*py) + M[2]*pz) + M[3]      cy, cz, cw: rows 1, 2, 3
//   !(cw > 0): x = y = z = NaN;  else x = cx / cw, y = cy / cw, z = cz / cw
// With the last row (0, 0, 0, 1) cw is exactly 1 and x == cx.
//
// The per-draw output lives in the context (TriScratch::mstage), not in the
// mesh: one mesh may be drawn on several contexts.  A pending batch, or its
// overflow re-run, reads it after DrawMesh returns, so every overwrite comes
// after nrtri::settle, the rule DrawTriangles follows for its staging buffer.
// The attributes do not depend on the matrix: they are expanded through the
// indices once, at creation.
#include "nr_tri.h"

#include <string>

struct Mesh {
    i64 nv = 0, n = 0;
    int mode = nrtri::ATTR_FLAT;   // AttrMode of the expanded attributes
    bool opaque = false;           // colour mesh: every vertex alpha == 1 (textured: decided per draw by the texture)
    int device = 0;
    f64* pos = nullptr;            // nv*3
    u32* idx = nullptr;            // n*3, every entry < nv (checked on the host at creation)
    f64* attr = nullptr;           // expanded: n*12 Gouraud, n*4 flat (the colour of i0), n*6 textured
};

namespace nrtri {
namespace {

struct Mat4 { f64 m[16]; };

// Pass 1: one thread per vertex.  (x, y) as one 16-byte store, z beside it.
__global__ __launch_bounds__(256) void k_mesh_vertex(const f64* __restrict__ pos, i64 nv, Mat4 M,
                                                     double2* __restrict__ vxy, f64* __restrict__ vz) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const f64 px = pos[v * 3], py = pos[v * 3 + 1], pz = pos[v * 3 + 2];
    const f64 cx = ((M.m[0] * px + M.m[1] * py) + M.m[2] * pz) + M.m[3];
    const f64 cy = ((M.m[4] * px + M.m[5] * py) + M.m[6] * pz) + M.m[7];
    const f64 cz = ((M.m[8] * px + M.m[9] * py) + M.m[10] * pz) + M.m[11];
    const f64 cw = ((M.m[12] * px + M.m[13] * py) + M.m[14] * pz) + M.m[15];
    f64 x = NAN, y = NAN, z = NAN;
    if (cw > 0) {
        x = cx / cw;
        y = cy / cw;
        z = cz / cw;
    }
    vxy[v] = make_double2(x, y);
    vz[v] = z;
}

// Pass 2: one thread per triangle corner (3n): indices, xy and z are read or
// written contiguously across a wave; only the gather from the vertex table
// (cache-resident) is irregular.
__global__ __launch_bounds__(256) void k_mesh_assemble(const u32* __restrict__ idx, i64 ncorner,
                                                       const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                       double2* __restrict__ xy, f64* __restrict__ z) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner) return;
    const u32 i = idx[c];
    xy[c] = vxy[i];
    z[c] = vz[i];
}

// Creation: per-vertex attributes (w2 16-byte words each: 2 for RGBA, 1 for a
// UV) through the indices.  perTri = 3: one thread per corner (Gouraud n*12,
// textured n*6); perTri = 1: one per triangle, the provoking vertex i0 (flat n*4).
__global__ __launch_bounds__(256) void k_mesh_attr(const u32* __restrict__ idx, i64 nout, int perTri, int w2,
                                                   const double2* __restrict__ vattr, double2* __restrict__ out) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= nout) return;
    const u32 i = idx[perTri == 3 ? t : t * 3];
    for (int k = 0; k < w2; ++k) out[t * w2 + k] = vattr[(i64)i * w2 + k];
}

unsigned blocks_for(i64 threads) { return (unsigned)((threads + 255) / 256); }

bool fail(const char* what, const char* why) {
    nr_set_error_msg((std::string(what) + ": " + why).c_str());
    return false;
}

// uv: texel coordinates nv*2 (a textured mesh) or null (rgba nv*4, flat or Gouraud)
Mesh* create_mesh(const char* what, i64 nv, const f64* pos, i64 n, const u32* idx, const f64* rgba, bool gouraud,
                  const f64* uv) {
    const f64* vattr = uv ? uv : rgba;
    const char* why = nullptr;
    if (nv < 0 || n < 0) why = "negative count";
    else if (nv > (i64)0xFFFFFFFFll) why = "vertex count does not fit 32-bit indices";
    else if (n > (i64)0xFFFFFFFFll / 3) why = "too many triangles";
    else if (nv > 0 && !pos) why = "NULL positions";
    else if (n > 0 && !idx) why = "NULL indices";
    else if (n > 0 && !vattr) why = "NULL rgba";   // (CreateTexturedMesh checks its uv itself)
    if (!why)
        for (i64 k = 0; k < n * 3; ++k)
            if ((i64)idx[k] >= nv) { why = "index out of range (>= vertex count)"; break; }
    if (why) {
        fail(what, why);
        return nullptr;
    }
    Mesh* m = new Mesh();
    m->nv = nv;
    m->n = n;
    m->mode = uv ? nrtri::ATTR_TEX : (gouraud ? nrtri::ATTR_GOURAUD : nrtri::ATTR_FLAT);
    NR_CHECK(hipGetDevice(&m->device));
    if (!uv && n > 0) {
        m->opaque = true;
        for (i64 v = 0; v < nv; ++v)
            if (rgba[v * 4 + 3] != 1) { m->opaque = false; break; }
    }
    if (nv == 0) return m;   // (then n == 0: every index would be out of range)
    hipStream_t s = nr_stream_for(m->device);
    const int w2 = uv ? 1 : 2;   // 16-byte words per vertex attribute
    f64* dv = nullptr;           // the per-vertex attributes, on the device until expanded
    bool ok = hipMalloc(&m->pos, (size_t)nv * 3 * sizeof(f64)) == hipSuccess;
    if (ok && n > 0) {
        ok = hipMalloc(&m->idx, (size_t)n * 3 * sizeof(u32)) == hipSuccess &&
             hipMalloc(&m->attr, (size_t)n * nrtri::attr_stride(m->mode) * sizeof(f64)) == hipSuccess &&
             hipMalloc(&dv, (size_t)nv * w2 * 2 * sizeof(f64)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        fail(what, "hipMalloc failed");
        if (dv) NR_CHECK(hipFree(dv));
        if (m->pos) NR_CHECK(hipFree(m->pos));
        if (m->idx) NR_CHECK(hipFree(m->idx));
        if (m->attr) NR_CHECK(hipFree(m->attr));
        delete m;
        return nullptr;
    }
    NR_CHECK(hipMemcpyAsync(m->pos, pos, (size_t)nv * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
    if (n > 0) {
        NR_CHECK(hipMemcpyAsync(m->idx, idx, (size_t)n * 3 * sizeof(u32), hipMemcpyHostToDevice, s));
        NR_CHECK(hipMemcpyAsync(dv, vattr, (size_t)nv * w2 * 2 * sizeof(f64), hipMemcpyHostToDevice, s));
        const int perTri = m->mode == nrtri::ATTR_FLAT ? 1 : 3;
        const i64 nout = n * perTri;
        hipLaunchKernelGGL(k_mesh_attr, dim3(blocks_for(nout)), dim3(256), 0, s, m->idx, nout, perTri, w2,
                           reinterpret_cast<const double2*>(dv), reinterpret_cast<double2*>(m->attr));
        NR_CHECK(hipGetLastError());
    }
    NR_CHECK(hipStreamSynchronize(s));   // caller may reuse its arrays on return
    if (dv) NR_CHECK(hipFree(dv));
    return m;
}

struct Soup { const f64* xy; const f64* z; };

// The vertex stage and the assembly of `m` under `matrix` into ctx's mesh
// staging, on the context's stream (m->n > 0).  False: the staging could not
// be grown (error latched).
bool assemble(RenderContext* ctx, const Mesh* m, const f64* matrix, Soup* out) {
    nrtri::settle(ctx);   // a pending batch may still read the staging (its re-run comes first)
    TriScratch& sc = ctx->tri;
    const size_t nv = (size_t)m->nv, n = (size_t)m->n;
    const size_t vzn = (nv + 1) & ~(size_t)1;   // keeps the soup's xy 16-byte aligned
    if (!sc.mstage.ensure(nv * 2 + vzn + n * 9)) return false;
    f64* vxy = sc.mstage;
    f64* vz = vxy + nv * 2;
    f64* xy = vz + vzn;
    f64* z = xy + n * 6;
    Mat4 M = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    if (matrix)
        for (int k = 0; k < 16; ++k) M.m[k] = matrix[k];
    hipEvent_t a, b;
    nr_timing_begin(ctx, NRK_MESH_VERTEX, &a, &b);
    hipLaunchKernelGGL(k_mesh_vertex, dim3(blocks_for(m->nv)), dim3(256), 0, ctx->stream, m->pos, m->nv, M,
                       reinterpret_cast<double2*>(vxy), vz);
    NR_CHECK(hipGetLastError());
    nr_timing_end(ctx, NRK_MESH_VERTEX, a, b);
    nr_timing_begin(ctx, NRK_MESH_ASSEMBLE, &a, &b);
    hipLaunchKernelGGL(k_mesh_assemble, dim3(blocks_for(m->n * 3)), dim3(256), 0, ctx->stream, m->idx, m->n * 3,
                       reinterpret_cast<const double2*>(vxy), vz, reinterpret_cast<double2*>(xy), z);
    NR_CHECK(hipGetLastError());
    nr_timing_end(ctx, NRK_MESH_ASSEMBLE, a, b);
    out->xy = xy;
    out->z = z;
    return true;
}

// The checks every mesh draw shares (in the style of check_texture).
bool check_mesh(RenderContext* ctx, const Mesh* m, bool textured, const char* what) {
    if (!m) return fail(what, "NULL mesh");
    if ((m->mode == nrtri::ATTR_TEX) != textured)
        return fail(what, textured ? "a colour mesh (use DrawMesh)" : "a textured mesh (use DrawTexturedMesh)");
    if (m->device != ctx->device) return fail(what, "mesh on another device");
    return true;
}

// Every context that may have a pending batch reading the mesh's arrays is
// settled and the device's streams are drained (as DestroyTriangleBuffer).
void quiesce(const Mesh* m) {
    nr_settle_all();
    NR_CHECK(hipSetDevice(m->device));
    NR_CHECK(hipStreamSynchronize(nr_stream_for(m->device)));
    NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(m->device)));
}

}  // namespace
}  // namespace nrtri

using namespace nrtri;

extern "C" {

// New: an indexed mesh with per-vertex colours (nv*4), flat (the colour of each
// triangle's first index) or Gouraud.  One H2D upload; NULL + error on an index
// >= nv, NULL rgba with n > 0, or nv beyond 32 bits.  n == 0 is a valid mesh.
Mesh* CreateMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* rgba, bool gouraud) {
    return create_mesh("CreateMesh", nv, pos, n, idx, rgba, gouraud, nullptr);
}

// New: an indexed mesh with per-vertex texture coordinates (nv*2, texel units).
Mesh* CreateTexturedMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* uv) {
    if (!uv && n > 0) {
        fail("CreateTexturedMesh", "NULL uv");
        return nullptr;
    }
    static const f64 none[2] = {0, 0};
    return create_mesh("CreateTexturedMesh", nv, pos, n, idx, nullptr, false, uv ? uv : none);
}

void DestroyMesh(Mesh* m) {
    if (!m) return;
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    quiesce(m);
    if (m->pos) NR_CHECK(hipFree(m->pos));
    if (m->idx) NR_CHECK(hipFree(m->idx));
    if (m->attr) NR_CHECK(hipFree(m->attr));
    NR_CHECK(hipSetDevice(prev));
    delete m;
}

i64 GetMeshVertexCount(Mesh* m) { return m->nv; }
i64 GetMeshTriangleCount(Mesh* m) { return m->n; }

// New: replaces the positions (nv*3) of a deforming mesh: an H2D copy of the
// positions only.  Draws issued before the call keep the old positions.
bool UpdateMeshPositions(Mesh* m, const f64* pos) {
    if (!m) return fail("UpdateMeshPositions", "NULL mesh");
    if (m->nv == 0) return true;
    if (!pos) return fail("UpdateMeshPositions", "NULL positions");
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    quiesce(m);
    hipStream_t s = nr_stream_for(m->device);
    NR_CHECK(hipMemcpyAsync(m->pos, pos, (size_t)m->nv * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
    NR_CHECK(hipStreamSynchronize(s));   // caller may reuse its array on return
    NR_CHECK(hipSetDevice(prev));
    return true;
}

// New: draws a colour mesh under the row-major 4x4 `matrix16` (NULL: the
// identity), then the context's transform, depth state and colour transform as
// for DrawTriangles.
void DrawMesh(RenderContext* ctx, Mesh* m, const f64* matrix16) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_mesh(ctx, m, false, "DrawMesh")) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    Soup s;
    if (!assemble(ctx, m, matrix16, &s)) return;
    nrtri::draw(ctx, s.xy, s.z, m->attr, m->n, m->mode, m->opaque ? nrtri::OPQ_OPAQUE : nrtri::OPQ_BLENDED, nullptr,
                false);
}

// New: draws a textured mesh sampled from `tex` (chosen per draw).
void DrawTexturedMesh(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrix16) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_mesh(ctx, m, true, "DrawTexturedMesh")) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (!nrtri::check_texture(ctx, tex, "DrawTexturedMesh")) return;
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    Soup s;
    if (!assemble(ctx, m, matrix16, &s)) return;
    nrtri::draw_textured(ctx, tex, s.xy, s.z, m->attr, m->n, nullptr, false);
}

// New: the vertex stage and the assembly alone -- exactly the kernels DrawMesh
// runs -- with the soup (xy n*6, z n*3) copied to the host: a sync point.  The
// mesh may be of either kind.
bool AssembleMesh(RenderContext* ctx, Mesh* m, const f64* matrix16, f64* xy_out, f64* z_out) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!m) return fail("AssembleMesh", "NULL mesh");
    if (m->device != ctx->device) return fail("AssembleMesh", "mesh on another device");
    if (m->n <= 0) return true;
    if (!xy_out || !z_out) return fail("AssembleMesh", "NULL output");
    Soup s;
    if (!assemble(ctx, m, matrix16, &s)) return false;
    NR_CHECK(hipMemcpyAsync(xy_out, s.xy, (size_t)m->n * 6 * sizeof(f64), hipMemcpyDeviceToHost, ctx->stream));
    NR_CHECK(hipMemcpyAsync(z_out, s.z, (size_t)m->n * 3 * sizeof(f64), hipMemcpyDeviceToHost, ctx->stream));
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    return true;
}

}  // extern "C"

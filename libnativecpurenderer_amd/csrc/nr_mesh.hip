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
// With the context's perspective state on (SetMeshPerspective) a textured draw
// also keeps q = 1.0 / cw (NaN where !(cw > 0)) per vertex, gathers it like z
// and hands it to the rasters as the batch's 1/w (ATTR_TEX_PERSP).
//
// The per-draw output lives in the context (TriScratch::mstage), not in the
// mesh: one mesh may be drawn on several contexts.  A pending batch, or its
// overflow re-run, reads it after DrawMesh returns, so every overwrite comes
// after nrtri::settle, the rule DrawTriangles follows for its staging buffer.
// The attributes do not depend on the matrix: they are expanded through the
// indices once, at creation.
//
// Near-plane clipping and back-face culling (SetMeshNearPlane / SetMeshCull,
// DESIGN.md §3 "Clip stage"): with either on, a draw runs another four passes
// instead of the two above -- clip coordinates per vertex, a per-triangle count
// of its 0, 1 or 2 output triangles, an exclusive scan, and an emit pass that
// writes the clipped soup and its interpolated attributes at the scanned
// offsets (a stable compaction: submission order is kept).  The draw reads the
// total back before it bins, so such a draw -- and only such a draw -- waits
// for the device once.  With both off nothing here runs.
//
// Instanced draws (DrawMeshInstanced and its kin, DESIGN.md §3 "Instanced mesh
// draws"): one mesh under K matrices as ONE batch whose frame is, by definition,
// that of K DrawMesh calls in instance order.  The same passes run once over
// K*nv vertices and K*n triangles (k_minst_*), the assembly also copying -- or
// tinting -- the mesh's attributes to each instance's place in the batch; the
// single-draw kernels and host path are untouched.
//
// Lit draws (DrawMeshLit and its kin, DESIGN.md §3 "Vertex lighting"): a mesh
// created with normals is lit per vertex under the context's ambient colour and
// directional lights by one more pass over the vertices (k_mesh_light,
// k_minst_light), whose output -- a per-draw vertex-colour table in the staging,
// never in the mesh -- feeds the assembly, clip and instancing passes in place
// of the mesh's own colours.  Unlit draws run none of it.
//
// Textured colour meshes (CreateTexturedColorMesh, DrawTexturedMeshLit, DESIGN.md
// §3 "Modulated textured draws"): a uv and a colour per vertex, expanded to three
// 16-byte words per corner (u v | r g | b a) and drawn as a modulated batch --
// the texel times the interpolated colour.  A lit draw runs the same light pass
// on the colours and gathers the corner words from the mesh's uv and the colour
// table; the clip stage emits three words per corner; every draw has a q (1.0
// without the perspective state).
//
// The host half, at the end of the file: every entry point describes its draw once (MeshDraw: the mesh, one matrix
// by value or K instances, the light input, where q comes from) and build_soup turns the description into a soup
// through one of two builders, soup_unclipped and soup_clipped.  Single and instanced draws differ only in the
// kernels chosen and in their counts (K*nv, K*n).  Every staging layout is carved by nr_mesh_stage.h, every timed
// pass goes through mesh_launch (nr_mesh.h), and the entry points end in submit (draws) or copy_soup (Assemble*).
#include "nr_mesh.h"
#include "nr_mesh_stage.h"

#include <hipcub/hipcub.hpp>

#include <climits>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

namespace nrtri {
namespace {

struct Mat4 { f64 m[16]; };

// Pass 1: one thread per vertex.  (x, y) as one 16-byte store, z beside it.
// Q: also q = 1.0 / cw (vq).
template <bool Q>
__global__ __launch_bounds__(256) void k_mesh_vertex(const f64* __restrict__ pos, i64 nv, Mat4 M,
                                                     double2* __restrict__ vxy, f64* __restrict__ vz,
                                                     f64* __restrict__ vq) {
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
    if constexpr (Q) vq[v] = cw > 0 ? 1.0 / cw : NAN;
}

// Pass 2: one thread per triangle corner (3n): indices, xy and z are read or
// written contiguously across a wave; only the gather from the vertex table
// (cache-resident) is irregular.  Q: q is gathered as z is.
template <bool Q>
__global__ __launch_bounds__(256) void k_mesh_assemble(const u32* __restrict__ idx, i64 ncorner,
                                                       const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                       double2* __restrict__ xy, f64* __restrict__ z,
                                                       const f64* __restrict__ vq, f64* __restrict__ q) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner) return;
    const u32 i = idx[c];
    xy[c] = vxy[i];
    z[c] = vz[i];
    if constexpr (Q) q[c] = vq[i];
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

// ---- near-plane clipping and back-face culling --------------------------------
// Pass C1: one thread per vertex, the clip coordinates (cx, cy | cz, cw) as two
// 16-byte stores; the expressions of k_mesh_vertex.
__global__ __launch_bounds__(256) void k_mesh_clip_vertex(const f64* __restrict__ pos, i64 nv, Mat4 M,
                                                          double2* __restrict__ clip) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const f64 px = pos[v * 3], py = pos[v * 3 + 1], pz = pos[v * 3 + 2];
    const f64 cx = ((M.m[0] * px + M.m[1] * py) + M.m[2] * pz) + M.m[3];
    const f64 cy = ((M.m[4] * px + M.m[5] * py) + M.m[6] * pz) + M.m[7];
    const f64 cz = ((M.m[8] * px + M.m[9] * py) + M.m[10] * pz) + M.m[11];
    const f64 cw = ((M.m[12] * px + M.m[13] * py) + M.m[14] * pz) + M.m[15];
    clip[v * 2] = make_double2(cx, cy);
    clip[v * 2 + 1] = make_double2(cz, cw);
}

// A source triangle's clip coordinates.  The arrays are only ever indexed by
// constants (unrolled loops) or through sel3: they stay in registers.
struct ClipTri { f64 cx[3], cy[3], cz[3], cw[3]; };
struct ClipPos { f64 x, y, z, t; };   // a polygon vertex on the screen; t: its cut parameter (a cut only)

__device__ __forceinline__ f64 sel3(int k, const f64 (&v)[3]) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

__device__ __forceinline__ void load_clip_tri(const u32* __restrict__ idx, const double2* __restrict__ clip, i64 t,
                                              ClipTri& c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const i64 i = (i64)idx[t * 3 + k];
        const double2 a = clip[i * 2], b = clip[i * 2 + 1];
        c.cx[k] = a.x; c.cy[k] = a.y; c.cz[k] = b.x; c.cw[k] = b.y;
    }
}

// in0 | in1 << 1 | in2 << 2 with in_k = (cw_k >= wNear), false for a NaN;
// without a near plane every corner counts as inside.
__device__ __forceinline__ int inside_code(const ClipTri& c, f64 wNear) {
    if (!(wNear > 0)) return 7;
    return (c.cw[0] >= wNear ? 1 : 0) | (c.cw[1] >= wNear ? 2 : 0) | (c.cw[2] >= wNear ? 4 : 0);
}

// The Sutherland-Hodgman walk from corner 0 (emit corner k if inside, then the
// cut of edge (k, k + 1) if its ends differ), tabulated: vertex s of the polygon
// under inside-code c is (a, b) -- the inside corner a itself when b == a, else
// the cut of the edge from a (inside) towards b (outside).
//   c = 1: 0 0>1 0>2        c = 2: 1>0 1 1>2        c = 4: 2>1 2 2>0
//   c = 3: 0 1 1>2 0>2      c = 5: 0 0>1 2>1 2      c = 6: 1>0 1 2 2>0      c = 7: 0 1 2
// Two bits per code; the lookups are shifts of a constant (no indexed array).
__host__ __device__ constexpr u32 pack7(u32 c1, u32 c2, u32 c3, u32 c4, u32 c5, u32 c6, u32 c7) {
    return c1 << 2 | c2 << 4 | c3 << 6 | c4 << 8 | c5 << 10 | c6 << 12 | c7 << 14;
}
__host__ __device__ constexpr u32 slot_a_tab(int s) {
    return s == 0 ? pack7(0, 1, 0, 2, 0, 1, 0) : s == 1 ? pack7(0, 1, 1, 2, 0, 1, 1)
         : s == 2 ? pack7(0, 1, 1, 2, 2, 2, 2) : pack7(0, 0, 0, 0, 2, 2, 0);
}
__host__ __device__ constexpr u32 slot_b_tab(int s) {
    return s == 0 ? pack7(0, 0, 0, 1, 0, 0, 0) : s == 1 ? pack7(1, 1, 1, 2, 1, 1, 1)
         : s == 2 ? pack7(2, 2, 2, 0, 1, 2, 2) : pack7(0, 0, 2, 0, 2, 0, 0);
}
__device__ __forceinline__ int slot_a(int s, int code) { return (int)((slot_a_tab(s) >> (2 * code)) & 3u); }
__device__ __forceinline__ int slot_b(int s, int code) { return (int)((slot_b_tab(s) >> (2 * code)) & 3u); }
// output triangles before the cull, as a mask: bit 0 (q0, q1, q2), bit 1 (q0, q2, q3)
__device__ __forceinline__ u32 clip_outputs(int code) {
    return code == 0 ? 0u : ((code == 3 || code == 5 || code == 6) ? 3u : 1u);
}

// Polygon vertex (a, b).  A corner: c / cw, NaN where !(cw > 0) -- k_mesh_vertex's
// bits (behind a near plane an inside corner has cw >= wNear > 0).  A cut, always
// from the inside end a towards the outside end b, every operation rounded:
//   t = (cw_a - wNear) / (cw_a - cw_b);  q = c_a + (c_b - c_a) * t;  q / wNear
__device__ __forceinline__ ClipPos clip_slot_pos(const ClipTri& c, int a, int b, f64 wNear) {
    const f64 ax = sel3(a, c.cx), ay = sel3(a, c.cy), az = sel3(a, c.cz), aw = sel3(a, c.cw);
    ClipPos q;
    q.t = 0;
    if (a == b) {
        q.x = q.y = q.z = NAN;
        if (aw > 0) {
            q.x = ax / aw;
            q.y = ay / aw;
            q.z = az / aw;
        }
    } else {
        const f64 bx = sel3(b, c.cx), by = sel3(b, c.cy), bz = sel3(b, c.cz), bw = sel3(b, c.cw);
        q.t = (aw - wNear) / (aw - bw);
        const f64 qx = ax + (bx - ax) * q.t;
        const f64 qy = ay + (by - ay) * q.t;
        const f64 qz = az + (bz - az) * q.t;
        q.x = qx / wNear;
        q.y = qy / wNear;
        q.z = qz / wNear;
    }
    return q;
}

// 1/w of polygon vertex (a, b): a corner's 1.0 / cw (NaN where !(cw > 0), the
// vertex stage's q), a cut's 1.0 / wNear -- the same value from either triangle
// that shares the cut edge.
__device__ __forceinline__ f64 clip_slot_q(const ClipTri& c, int a, int b, f64 wNear) {
    if (a != b) return 1.0 / wNear;
    const f64 aw = sel3(a, c.cw);
    return aw > 0 ? 1.0 / aw : NAN;
}

// cull 1 drops area2 > 0, cull 2 drops area2 < 0; a zero or NaN area is never culled
__device__ __forceinline__ bool clip_culled(const ClipPos& p0, const ClipPos& p1, const ClipPos& p2, int cull) {
    const f64 area2 = (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
    return cull == 1 ? area2 > 0 : (cull == 2 ? area2 < 0 : false);
}

// Pass C2: one thread per source triangle: which of its output triangles survive
// the clip and the cull (keep: bit 0 the first, bit 1 the second half of a
// quad) and how many (cnt, the scan's input).  Without a cull no vertex is formed.
// (clip_keep: the same decision for one triangle, shared with the instanced count pass)
__device__ __forceinline__ u32 clip_keep(const u32* __restrict__ idx, const double2* __restrict__ clip, i64 t, f64 wNear,
                                         int cull) {
    ClipTri c;
    load_clip_tri(idx, clip, t, c);
    const int code = inside_code(c, wNear);
    u32 k = clip_outputs(code);
    if (cull != 0 && k != 0) {
        const ClipPos q0 = clip_slot_pos(c, slot_a(0, code), slot_b(0, code), wNear);
        const ClipPos q1 = clip_slot_pos(c, slot_a(1, code), slot_b(1, code), wNear);
        const ClipPos q2 = clip_slot_pos(c, slot_a(2, code), slot_b(2, code), wNear);
        if (clip_culled(q0, q1, q2, cull)) k &= ~1u;
        if (k & 2u) {
            const ClipPos q3 = clip_slot_pos(c, slot_a(3, code), slot_b(3, code), wNear);
            if (clip_culled(q0, q2, q3, cull)) k &= ~2u;
        }
    }
    return k;
}
__global__ __launch_bounds__(256) void k_mesh_clip_count(const u32* __restrict__ idx, i64 n,
                                                         const double2* __restrict__ clip, f64 wNear, int cull,
                                                         u32* __restrict__ keep, u32* __restrict__ cnt) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const u32 k = clip_keep(idx, clip, t, wNear, cull);
    keep[t] = k;
    cnt[t] = (k & 1u) + (k >> 1);
}

// One attribute component of polygon vertex (a, b) from the corners' v0, v1, v2:
// the corner's own, or at a cut A_a + (A_b - A_a) * t (linear in clip space;
// 1 + 0 * t stays 1).
__device__ __forceinline__ f64 clip_attr(int a, int b, f64 t, f64 v0, f64 v1, f64 v2) {
    const f64 va = a == 0 ? v0 : (a == 1 ? v1 : v2);
    const f64 vb = b == 0 ? v0 : (b == 1 ? v1 : v2);
    return a == b ? va : va + (vb - va) * t;
}

__device__ __forceinline__ void clip_store_pos(i64 o, const ClipPos& p0, const ClipPos& p1, const ClipPos& p2,
                                               double2* __restrict__ xy, f64* __restrict__ z) {
    xy[o * 3] = make_double2(p0.x, p0.y);
    xy[o * 3 + 1] = make_double2(p1.x, p1.y);
    xy[o * 3 + 2] = make_double2(p2.x, p2.y);
    z[o * 3] = p0.z;
    z[o * 3 + 1] = p1.z;
    z[o * 3 + 2] = p2.z;
}

// Pass C3: one thread per source triangle with an output: forms the polygon
// again (the count pass's expressions) and writes its kept triangles at the
// scanned offset.  H 16-byte attribute words per corner: 2 (Gouraud RGBA), 1
// (UV), or 0 for a flat mesh, whose one colour (two words per triangle) is
// copied to each output.  The attributes go word by word -- the three corners'
// word j in, the polygon's word j out -- so nothing is held in an array.
// Q (a perspective textured draw): also each output corner's 1/w (clip_slot_q)
// into oq, laid out like z.
// (clip_emit_tri: source triangle t with keep mask k != 0, its first kept triangle at o0; shared with the
// instanced emit pass, whose TINT instances multiply each colour word by the instance's tint (r, g | b, a) as
// it is loaded, before any interpolation.)
template <int H, bool Q, bool TINT>
__device__ __forceinline__ void clip_emit_tri(const u32* __restrict__ idx, const double2* __restrict__ clip,
                                              const double2* __restrict__ attr, const f64* __restrict__ tint, f64 wNear,
                                              i64 t, u32 k, i64 o0, double2* __restrict__ xy, f64* __restrict__ z,
                                              double2* __restrict__ oattr, f64* __restrict__ oq) {
    const i64 o1 = o0 + (i64)(k & 1u);  // the second half of a quad, when kept
    ClipTri c;
    load_clip_tri(idx, clip, t, c);
    const int code = inside_code(c, wNear);
    const int a0 = slot_a(0, code), b0 = slot_b(0, code), a1 = slot_a(1, code), b1 = slot_b(1, code);
    const int a2 = slot_a(2, code), b2 = slot_b(2, code), a3 = slot_a(3, code), b3 = slot_b(3, code);
    const ClipPos q0 = clip_slot_pos(c, a0, b0, wNear);
    const ClipPos q2 = clip_slot_pos(c, a2, b2, wNear);
    f64 t1 = 0, t3 = 0;
    if (k & 1u) {
        const ClipPos q1 = clip_slot_pos(c, a1, b1, wNear);
        t1 = q1.t;
        clip_store_pos(o0, q0, q1, q2, xy, z);
    }
    if (k & 2u) {
        const ClipPos q3 = clip_slot_pos(c, a3, b3, wNear);
        t3 = q3.t;
        clip_store_pos(o1, q0, q2, q3, xy, z);
    }
    if constexpr (Q) {
        const f64 w0 = clip_slot_q(c, a0, b0, wNear), w2 = clip_slot_q(c, a2, b2, wNear);
        if (k & 1u) {
            oq[o0 * 3] = w0;
            oq[o0 * 3 + 1] = clip_slot_q(c, a1, b1, wNear);
            oq[o0 * 3 + 2] = w2;
        }
        if (k & 2u) {
            oq[o1 * 3] = w0;
            oq[o1 * 3 + 1] = w2;
            oq[o1 * 3 + 2] = clip_slot_q(c, a3, b3, wNear);
        }
    }
    if constexpr (H == 0) {
        double2 c0 = attr[t * 2], c1 = attr[t * 2 + 1];
        if constexpr (TINT) {
            c0 = make_double2(c0.x * tint[0], c0.y * tint[1]);
            c1 = make_double2(c1.x * tint[2], c1.y * tint[3]);
        }
        if (k & 1u) { oattr[o0 * 2] = c0; oattr[o0 * 2 + 1] = c1; }
        if (k & 2u) { oattr[o1 * 2] = c0; oattr[o1 * 2 + 1] = c1; }
    } else {
#pragma unroll
        for (int j = 0; j < H; ++j) {
            double2 w0 = attr[t * (3 * H) + j], w1 = attr[t * (3 * H) + H + j], w2 = attr[t * (3 * H) + 2 * H + j];
            if constexpr (TINT) {   // (H == 2: word j of a corner is (r, g) or (b, a))
                const f64 ta = tint[2 * j], tb = tint[2 * j + 1];
                w0 = make_double2(w0.x * ta, w0.y * tb);
                w1 = make_double2(w1.x * ta, w1.y * tb);
                w2 = make_double2(w2.x * ta, w2.y * tb);
            }
            const double2 e0 = make_double2(clip_attr(a0, b0, q0.t, w0.x, w1.x, w2.x),
                                            clip_attr(a0, b0, q0.t, w0.y, w1.y, w2.y));
            const double2 e2 = make_double2(clip_attr(a2, b2, q2.t, w0.x, w1.x, w2.x),
                                            clip_attr(a2, b2, q2.t, w0.y, w1.y, w2.y));
            if (k & 1u) {
                double2* q = oattr + o0 * (3 * H);
                q[j] = e0;
                q[H + j] = make_double2(clip_attr(a1, b1, t1, w0.x, w1.x, w2.x), clip_attr(a1, b1, t1, w0.y, w1.y, w2.y));
                q[2 * H + j] = e2;
            }
            if (k & 2u) {
                double2* q = oattr + o1 * (3 * H);
                q[j] = e0;
                q[H + j] = e2;
                q[2 * H + j] = make_double2(clip_attr(a3, b3, t3, w0.x, w1.x, w2.x), clip_attr(a3, b3, t3, w0.y, w1.y, w2.y));
            }
        }
    }
}
template <int H, bool Q = false>
__global__ __launch_bounds__(256) void k_mesh_clip_emit(const u32* __restrict__ idx, i64 n,
                                                        const double2* __restrict__ clip,
                                                        const double2* __restrict__ attr, f64 wNear,
                                                        const u32* __restrict__ keep, const u32* __restrict__ off,
                                                        double2* __restrict__ xy, f64* __restrict__ z,
                                                        double2* __restrict__ oattr, f64* __restrict__ oq) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const u32 k = keep[t];
    if (k == 0) return;
    const i64 o0 = (i64)off[t];         // the first kept triangle
    clip_emit_tri<H, Q, false>(idx, clip, attr, nullptr, wNear, t, k, o0, xy, z, oattr, oq);
}

// ---- instanced draws (DESIGN.md §3 "Instanced mesh draws") ----------------------
// One mesh under K matrices as one soup: instance k's vertices are vertices k*nv ..
// of the batch's vertex table, its triangles k*n .. of the soup.  Every pass runs
// on a flat thread index over all instances (K*nv, 3*K*n or K*n threads, each
// below 2^31), so that waves stay full however small the mesh; the instance of a
// thread is one 32-bit division, and its matrix is loaded per lane from the
// device array (lanes of one instance read the same 128 bytes: a wave of a large
// mesh fetches one matrix, a wave of tiny meshes a few neighbouring ones).
struct InstOf { u32 k, r; };   // instance and the index inside it
__device__ __forceinline__ InstOf inst_of(u32 g, u32 per) {
    const u32 k = g / per;
    return InstOf{k, g - k * per};
}

__device__ __forceinline__ Mat4 inst_matrix(const f64* __restrict__ mats, u32 k) {
    Mat4 M;
    const f64* p = mats + (size_t)k * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) M.m[j] = p[j];
    return M;
}

// the clip coordinates of k_mesh_vertex / k_mesh_clip_vertex: the same expressions
__device__ __forceinline__ void clip_rows(const Mat4& M, f64 px, f64 py, f64 pz, f64& cx, f64& cy, f64& cz, f64& cw) {
    cx = ((M.m[0] * px + M.m[1] * py) + M.m[2] * pz) + M.m[3];
    cy = ((M.m[4] * px + M.m[5] * py) + M.m[6] * pz) + M.m[7];
    cz = ((M.m[8] * px + M.m[9] * py) + M.m[10] * pz) + M.m[11];
    cw = ((M.m[12] * px + M.m[13] * py) + M.m[14] * pz) + M.m[15];
}

// Pass 1 of an instanced draw: one thread per (instance, vertex), g = k * nv + v.
template <bool Q>
__global__ __launch_bounds__(256) void k_minst_vertex(const f64* __restrict__ pos, u32 nv, u32 total,
                                                      const f64* __restrict__ mats, double2* __restrict__ vxy,
                                                      f64* __restrict__ vz, f64* __restrict__ vq) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const InstOf in = inst_of(g, nv);
    const Mat4 M = inst_matrix(mats, in.k);
    const f64 px = pos[(size_t)in.r * 3], py = pos[(size_t)in.r * 3 + 1], pz = pos[(size_t)in.r * 3 + 2];
    f64 cx, cy, cz, cw;
    clip_rows(M, px, py, pz, cx, cy, cz, cw);
    f64 x = NAN, y = NAN, z = NAN;
    if (cw > 0) {
        x = cx / cw;
        y = cy / cw;
        z = cz / cw;
    }
    vxy[g] = make_double2(x, y);
    vz[g] = z;
    if constexpr (Q) vq[g] = cw > 0 ? 1.0 / cw : NAN;
}

// Pass 2: one thread per corner of the batch, c = k * 3n + (the mesh's corner):
// the gather of k_mesh_assemble from instance k's part of the vertex table, and
// the batch's attributes -- the rasters index them by batch triangle -- from the
// mesh's expanded ones: H 16-byte words per corner (2 Gouraud, 1 textured), or
// for a flat mesh (H == 0) the triangle's two words, written by its corners 0 and
// 1.  TINT: each colour word times the instance's tint, else a plain copy.
template <int H, bool Q, bool TINT>
__global__ __launch_bounds__(256) void k_minst_assemble(const u32* __restrict__ idx, u32 per, u32 total, u32 nv,
                                                        const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                        const f64* __restrict__ vq, const double2* __restrict__ attr,
                                                        const f64* __restrict__ tint, double2* __restrict__ xy,
                                                        f64* __restrict__ z, f64* __restrict__ q,
                                                        double2* __restrict__ oattr) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= total) return;
    const InstOf in = inst_of(c, per);
    const size_t i = (size_t)in.k * nv + idx[in.r];
    xy[c] = vxy[i];
    z[c] = vz[i];
    if constexpr (Q) q[c] = vq[i];
    const f64* tk = tint + (size_t)in.k * 4;   // (TINT only)
    if constexpr (H == 0) {
        const u32 t = in.r / 3u, w = in.r - t * 3u;   // (c / 3 is the batch triangle: 3n divides k * 3n)
        if (w < 2u) {
            double2 a = attr[(size_t)t * 2 + w];
            if constexpr (TINT) a = make_double2(a.x * tk[2 * w], a.y * tk[2 * w + 1]);
            oattr[(size_t)(c / 3u) * 2 + w] = a;
        }
    } else {
#pragma unroll
        for (int j = 0; j < H; ++j) {
            double2 a = attr[(size_t)in.r * H + j];
            if constexpr (TINT) a = make_double2(a.x * tk[2 * j], a.y * tk[2 * j + 1]);
            oattr[(size_t)c * H + j] = a;
        }
    }
}

// Pass C1 of an instanced draw: k_mesh_clip_vertex per (instance, vertex).
__global__ __launch_bounds__(256) void k_minst_clip_vertex(const f64* __restrict__ pos, u32 nv, u32 total,
                                                           const f64* __restrict__ mats, double2* __restrict__ clip) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const InstOf in = inst_of(g, nv);
    const Mat4 M = inst_matrix(mats, in.k);
    const f64 px = pos[(size_t)in.r * 3], py = pos[(size_t)in.r * 3 + 1], pz = pos[(size_t)in.r * 3 + 2];
    f64 cx, cy, cz, cw;
    clip_rows(M, px, py, pz, cx, cy, cz, cw);
    clip[(size_t)g * 2] = make_double2(cx, cy);
    clip[(size_t)g * 2 + 1] = make_double2(cz, cw);
}

// Pass C2: k_mesh_clip_count per (instance, triangle), g = k * n + t: the keep
// masks and counts of the whole batch, scanned at once.
__global__ __launch_bounds__(256) void k_minst_clip_count(const u32* __restrict__ idx, u32 n, u32 total, u32 nv,
                                                          const double2* __restrict__ clip, f64 wNear, int cull,
                                                          u32* __restrict__ keep, u32* __restrict__ cnt) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const InstOf in = inst_of(g, n);
    const u32 k = clip_keep(idx, clip + (size_t)in.k * nv * 2, (i64)in.r, wNear, cull);
    keep[g] = k;
    cnt[g] = (k & 1u) + (k >> 1);
}

// Pass C3: k_mesh_clip_emit per (instance, triangle) at the batch's scanned offsets.
template <int H, bool Q, bool TINT>
__global__ __launch_bounds__(256) void k_minst_clip_emit(const u32* __restrict__ idx, u32 n, u32 total, u32 nv,
                                                         const double2* __restrict__ clip,
                                                         const double2* __restrict__ attr, const f64* __restrict__ tint,
                                                         f64 wNear, const u32* __restrict__ keep,
                                                         const u32* __restrict__ off, double2* __restrict__ xy,
                                                         f64* __restrict__ z, double2* __restrict__ oattr,
                                                         f64* __restrict__ oq) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const u32 k = keep[g];
    if (k == 0) return;
    const InstOf in = inst_of(g, n);
    clip_emit_tri<H, Q, TINT>(idx, clip + (size_t)in.k * nv * 2, attr, tint + (size_t)in.k * 4, wNear, (i64)in.r, k,
                              (i64)off[g], xy, z, oattr, oq);
}

// ---- vertex lighting (DESIGN.md §3 "Vertex lighting") ---------------------------
// A lit draw's first pass: per vertex, the normal under the row-major 3x3 normal
// matrix, the ambient plus every light's clamped dot product times its colour,
// and the base colour times that sum, clamped to [0, 1]; alpha is copied.  f64,
// every product and sum rounded in the order written; no sqrt, no division:
//   wx = (N[0]*nx + N[1]*ny) + N[2]*nz                      wy: row 1, wz: row 2
//   acc_c = A_c;  per light in order:  dot = (wx*dx + wy*dy) + wz*dz
//                                      d = dot > 0 ? dot : 0.0    (a NaN dot: 0)
//                                      acc_c = acc_c + d * c_c
//   p_c = base_c * acc_c;  lit_c = p_c < 0 ? 0.0 : (p_c > 1 ? 1.0 : p_c)   (a NaN p stays NaN)
// The output is the draw's vertex-colour table (two 16-byte words per vertex) in
// the context's staging; the assembly and clip passes read it through the indices
// where an unlit draw reads the mesh's expanded attributes.
struct Mat3 { f64 m[9]; };

__device__ __forceinline__ f64 clamp01(f64 p) { return p < 0 ? 0.0 : (p > 1 ? 1.0 : p); }

// The lights are uniform kernel arguments: the loop is unrolled to its bound, so
// every light is read at a constant offset and a draw with nl lights leaves after nl.
__device__ __forceinline__ void light_vertex(const Mat3& N, const MeshLights& L, f64 nx, f64 ny, f64 nz, double2 rg,
                                             double2 ba, double2* __restrict__ out) {
    const f64 wx = (N.m[0] * nx + N.m[1] * ny) + N.m[2] * nz;
    const f64 wy = (N.m[3] * nx + N.m[4] * ny) + N.m[5] * nz;
    const f64 wz = (N.m[6] * nx + N.m[7] * ny) + N.m[8] * nz;
    f64 ar = L.ambient[0], ag = L.ambient[1], ab = L.ambient[2];
#pragma unroll
    for (int l = 0; l < MESH_MAX_LIGHTS; ++l) {
        if (l >= L.nl) break;
        const f64 dot = (wx * L.light[l][0] + wy * L.light[l][1]) + wz * L.light[l][2];
        const f64 d = dot > 0 ? dot : 0.0;
        ar = ar + d * L.light[l][3];
        ag = ag + d * L.light[l][4];
        ab = ab + d * L.light[l][5];
    }
    out[0] = make_double2(clamp01(rg.x * ar), clamp01(rg.y * ag));
    out[1] = make_double2(clamp01(ba.x * ab), ba.y);
}

// One thread per vertex: 24 B of normal and 32 B of colour in, 32 B out.
__global__ __launch_bounds__(256) void k_mesh_light(const f64* __restrict__ normal, const double2* __restrict__ rgba,
                                                    i64 nv, Mat3 N, MeshLights L, double2* __restrict__ lit) {
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    light_vertex(N, L, normal[v * 3], normal[v * 3 + 1], normal[v * 3 + 2], rgba[v * 2], rgba[v * 2 + 1], lit + v * 2);
}

// One thread per (instance, vertex), g = k * nv + v: instance k's normal matrix is
// loaded per lane like its 4x4 matrix (inst_matrix); nmats null: the identity for
// every instance, through the same arithmetic.
__global__ __launch_bounds__(256) void k_minst_light(const f64* __restrict__ normal, const double2* __restrict__ rgba,
                                                     u32 nv, u32 total, const f64* __restrict__ nmats, MeshLights L,
                                                     double2* __restrict__ lit) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const InstOf in = inst_of(g, nv);
    Mat3 N = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    if (nmats) {
        const f64* p = nmats + (size_t)in.k * 9;
#pragma unroll
        for (int j = 0; j < 9; ++j) N.m[j] = p[j];
    }
    const size_t v = in.r;
    light_vertex(N, L, normal[v * 3], normal[v * 3 + 1], normal[v * 3 + 2], rgba[v * 2], rgba[v * 2 + 1],
                 lit + (size_t)g * 2);
}

// Pass 2 of an unclipped lit draw: k_mesh_assemble's gather, and the soup's
// attributes from the colour table in k_minst_assemble's shape -- H = 2: a
// Gouraud corner's two words; H = 0: a flat triangle's two words, the lit colour
// of its first index, written by its corners 0 and 1.
template <int H>
__global__ __launch_bounds__(256) void k_mesh_lit_assemble(const u32* __restrict__ idx, i64 ncorner,
                                                           const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                           const double2* __restrict__ lit, double2* __restrict__ xy,
                                                           f64* __restrict__ z, double2* __restrict__ oattr) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner) return;
    const u32 i = idx[c];
    xy[c] = vxy[i];
    z[c] = vz[i];
    if constexpr (H == 0) {
        const i64 t = c / 3, w = c - t * 3;
        if (w < 2) oattr[t * 2 + w] = lit[(i64)idx[t * 3] * 2 + w];
    } else {
        oattr[c * 2] = lit[(i64)i * 2];
        oattr[c * 2 + 1] = lit[(i64)i * 2 + 1];
    }
}

// The same for an instanced lit draw: k_minst_assemble with instance k's part of
// the colour table in place of the mesh's expanded attributes.
template <int H, bool TINT>
__global__ __launch_bounds__(256) void k_minst_lit_assemble(const u32* __restrict__ idx, u32 per, u32 total, u32 nv,
                                                            const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                            const double2* __restrict__ lit, const f64* __restrict__ tint,
                                                            double2* __restrict__ xy, f64* __restrict__ z,
                                                            double2* __restrict__ oattr) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= total) return;
    const InstOf in = inst_of(c, per);
    const size_t base = (size_t)in.k * nv, i = base + idx[in.r];
    xy[c] = vxy[i];
    z[c] = vz[i];
    const f64* tk = tint + (size_t)in.k * 4;   // (TINT only)
    if constexpr (H == 0) {
        const u32 t = in.r / 3u, w = in.r - t * 3u;
        if (w < 2u) {
            double2 a = lit[(base + idx[t * 3u]) * 2 + w];
            if constexpr (TINT) a = make_double2(a.x * tk[2 * w], a.y * tk[2 * w + 1]);
            oattr[(size_t)(c / 3u) * 2 + w] = a;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double2 a = lit[i * 2 + j];
            if constexpr (TINT) a = make_double2(a.x * tk[2 * j], a.y * tk[2 * j + 1]);
            oattr[(size_t)c * 2 + j] = a;
        }
    }
}

// A clipped instanced lit draw: k_mesh_attr per instance -- the colour table
// through the indices into per-triangle attributes, instance k's at k * n
// triangles (perTri = 3: one thread per batch corner; 1: per batch triangle, i0).
__global__ __launch_bounds__(256) void k_minst_lit_attr(const u32* __restrict__ idx, u32 per, u32 total, u32 nv,
                                                        int perTri, const double2* __restrict__ lit,
                                                        double2* __restrict__ out) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const InstOf in = inst_of(g, per);
    const size_t i = (size_t)in.k * nv + idx[perTri == 3 ? in.r : in.r * 3u];
    out[(size_t)g * 2] = lit[i * 2];
    out[(size_t)g * 2 + 1] = lit[i * 2 + 1];
}

// ... and its emit pass: k_minst_clip_emit reading instance k's own attributes
// (W 16-byte words per triangle: 6 Gouraud, 2 flat).
template <int H, bool TINT>
__global__ __launch_bounds__(256) void k_minst_lit_clip_emit(const u32* __restrict__ idx, u32 n, u32 total, u32 nv,
                                                             const double2* __restrict__ clip,
                                                             const double2* __restrict__ attr,
                                                             const f64* __restrict__ tint, f64 wNear,
                                                             const u32* __restrict__ keep, const u32* __restrict__ off,
                                                             double2* __restrict__ xy, f64* __restrict__ z,
                                                             double2* __restrict__ oattr) {
    constexpr size_t W = H == 0 ? 2 : 3 * H;
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    const u32 k = keep[g];
    if (k == 0) return;
    const InstOf in = inst_of(g, n);
    clip_emit_tri<H, false, TINT>(idx, clip + (size_t)in.k * nv * 2, attr + (size_t)in.k * n * W,
                                  tint + (size_t)in.k * 4, wNear, (i64)in.r, k, (i64)off[g], xy, z, oattr, nullptr);
}

// ---- textured colour meshes (DESIGN.md §3 "Modulated textured draws") -------------
// The soup's attributes are three 16-byte words per corner, (u v | r g | b a).  An unlit draw reads the mesh's
// own expansion (k_mesh_attr, three words per vertex); a lit draw gathers them from the mesh's per-vertex uv and
// the light pass's two-word colour table.
// Pass 2 of an unclipped lit draw: k_mesh_assemble's gather and the corner's three words.
template <bool Q>
__global__ __launch_bounds__(256) void k_mesh_uvc_assemble(const u32* __restrict__ idx, i64 ncorner,
                                                           const double2* __restrict__ vxy, const f64* __restrict__ vz,
                                                           const f64* __restrict__ vq, const double2* __restrict__ uv,
                                                           const double2* __restrict__ lit, double2* __restrict__ xy,
                                                           f64* __restrict__ z, f64* __restrict__ q,
                                                           double2* __restrict__ oattr) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner) return;
    const i64 i = (i64)idx[c];
    xy[c] = vxy[i];
    z[c] = vz[i];
    if constexpr (Q) q[c] = vq[i];
    oattr[c * 3] = uv[i];
    oattr[c * 3 + 1] = lit[i * 2];
    oattr[c * 3 + 2] = lit[i * 2 + 1];
}

// A clipped lit draw: the expansion the emit pass reads, one thread per corner.
__global__ __launch_bounds__(256) void k_mesh_uvc_attr(const u32* __restrict__ idx, i64 ncorner,
                                                       const double2* __restrict__ uv, const double2* __restrict__ lit,
                                                       double2* __restrict__ out) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncorner) return;
    const i64 i = (i64)idx[c];
    out[c * 3] = uv[i];
    out[c * 3 + 1] = lit[i * 2];
    out[c * 3 + 2] = lit[i * 2 + 1];
}

// The 1/w of a draw with the perspective state off: every corner's q is 1.0.
__global__ __launch_bounds__(256) void k_mesh_unit_q(f64* __restrict__ q, i64 count) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c < count) q[c] = 1.0;
}

// ---- host side --------------------------------------------------------------------------------------------------
void unit_q(RenderContext* ctx, f64* q, i64 count) {   // (untimed)
    hipLaunchKernelGGL(k_mesh_unit_q, dim3(blocks_for(count)), dim3(256), 0, ctx->stream, q, count);
    NR_CHECK(hipGetLastError());
}

// The mesh's device arrays, then the mesh.
void free_mesh(Mesh* m) {
    for (void* p : {(void*)m->pos, (void*)m->idx, (void*)m->attr, (void*)m->rgba, (void*)m->uv, (void*)m->normal})
        if (p) NR_CHECK(hipFree(p));
    delete m;
}

// uv: texel coordinates nv*2 (a textured mesh) or null (rgba nv*4, flat or Gouraud); both uv and rgba: a textured
// colour mesh (ATTR_TEXC), which keeps its per-vertex uv and rgba on the device beside the expansion
// normal: nv*3, a lit colour mesh (the per-vertex colours stay on the device beside it), or null
Mesh* create_mesh(const char* what, i64 nv, const f64* pos, i64 n, const u32* idx, const f64* rgba, bool gouraud,
                  const f64* uv, const f64* normal) {
    const f64* vattr = uv ? uv : rgba;   // (both: the interleaved array below)
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
    const bool uvc = uv && rgba;
    m->mode = uvc ? nrtri::ATTR_TEXC : (uv ? nrtri::ATTR_TEX : (gouraud ? nrtri::ATTR_GOURAUD : nrtri::ATTR_FLAT));
    m->lit = normal != nullptr;
    NR_CHECK(hipGetDevice(&m->device));
    if (rgba && n > 0) {
        m->opaque = true;
        for (i64 v = 0; v < nv; ++v)
            if (rgba[v * 4 + 3] != 1) { m->opaque = false; break; }
    }
    if (nv == 0) return m;   // (then n == 0: every index would be out of range)
    hipStream_t s = nr_stream_for(m->device);
    const int w2 = uvc ? 3 : (uv ? 1 : 2);   // 16-byte words per vertex attribute
    std::vector<f64> inter;                  // (a textured colour mesh: u v | r g | b a per vertex)
    if (uvc && n > 0) {
        inter.resize((size_t)nv * 6);
        for (i64 v = 0; v < nv; ++v) {
            inter[v * 6] = uv[v * 2]; inter[v * 6 + 1] = uv[v * 2 + 1];
            for (int c = 0; c < 4; ++c) inter[v * 6 + 2 + c] = rgba[v * 4 + c];
        }
        vattr = inter.data();
    }
    f64* dv = nullptr;           // the per-vertex attributes, on the device until expanded
    bool ok = hipMalloc(&m->pos, (size_t)nv * 3 * sizeof(f64)) == hipSuccess;
    if (ok && normal) ok = hipMalloc(&m->normal, (size_t)nv * 3 * sizeof(f64)) == hipSuccess;
    if (ok && n > 0) {
        ok = hipMalloc(&m->idx, (size_t)n * 3 * sizeof(u32)) == hipSuccess &&
             hipMalloc(&m->attr, (size_t)n * nrtri::attr_stride(m->mode) * sizeof(f64)) == hipSuccess &&
             hipMalloc(&dv, (size_t)nv * w2 * 2 * sizeof(f64)) == hipSuccess;
        if (ok && uvc)
            ok = hipMalloc(&m->uv, (size_t)nv * 2 * sizeof(f64)) == hipSuccess &&
                 hipMalloc(&m->rgba, (size_t)nv * 4 * sizeof(f64)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        fail(what, "hipMalloc failed");
        if (dv) NR_CHECK(hipFree(dv));
        free_mesh(m);
        return nullptr;
    }
    NR_CHECK(hipMemcpyAsync(m->pos, pos, (size_t)nv * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
    if (normal) NR_CHECK(hipMemcpyAsync(m->normal, normal, (size_t)nv * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
    if (n > 0) {
        NR_CHECK(hipMemcpyAsync(m->idx, idx, (size_t)n * 3 * sizeof(u32), hipMemcpyHostToDevice, s));
        NR_CHECK(hipMemcpyAsync(dv, vattr, (size_t)nv * w2 * 2 * sizeof(f64), hipMemcpyHostToDevice, s));
        if (uvc) {
            NR_CHECK(hipMemcpyAsync(m->uv, uv, (size_t)nv * 2 * sizeof(f64), hipMemcpyHostToDevice, s));
            NR_CHECK(hipMemcpyAsync(m->rgba, rgba, (size_t)nv * 4 * sizeof(f64), hipMemcpyHostToDevice, s));
        }
        const int perTri = m->mode == nrtri::ATTR_FLAT ? 1 : 3;
        const i64 nout = n * perTri;
        // (on the device's stream, with no context: a plain launch)
        hipLaunchKernelGGL(k_mesh_attr, dim3(blocks_for(nout)), dim3(256), 0, s, m->idx, nout, perTri, w2,
                           reinterpret_cast<const double2*>(dv), reinterpret_cast<double2*>(m->attr));
        NR_CHECK(hipGetLastError());
    }
    NR_CHECK(hipStreamSynchronize(s));   // caller may reuse its arrays on return
    if (normal && !uvc) m->rgba = dv;    // (a lit mesh keeps them; a textured colour mesh has its own copy)
    else if (dv) NR_CHECK(hipFree(dv));
    return m;
}

// `matrix`, or the identity for null.
Mat4 mat4_of(const f64* matrix) {
    Mat4 M = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    if (matrix)
        for (int k = 0; k < 16; ++k) M.m[k] = matrix[k];
    return M;
}

// `normal9`, or the identity for null.
Mat3 mat3_of(const f64* normal9) {
    Mat3 N = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    if (normal9)
        for (int k = 0; k < 9; ++k) N.m[k] = normal9[k];
    return N;
}

inline bool clip_stage_on(const RenderContext* ctx) { return ctx->meshNear > 0 || ctx->meshCull != 0; }

// ---- one draw description, two soup builders --------------------------------------------------------------------
// The K matrices (K*16) and tints (K*4, or null) of an instanced draw, on the device; a lit draw's normal
// matrices (K*9, or null: the identity for every instance).
struct Instances { const f64* mats; const f64* tint; i64 K; const f64* normals; };

// Where the soup's 1/w comes from: no q at all; 1 / cw from the vertex stage (a textured or textured colour mesh
// under the context's perspective state -- colour meshes ignore the state); or 1.0 everywhere (a textured colour
// mesh without the state: a modulated batch always has a q).
enum QSource { Q_NONE, Q_INV_CW, Q_UNIT };

// What a draw is, for every pass that builds its soup (m->n > 0; instanced: K > 0, K*n and K*nv below 2^31).
struct MeshDraw {
    const Mesh* m;
    Mat4 M;                  // a single draw's matrix, handed to its kernels by value ...
    const Instances* inst;   // ... or the instances (null: a single draw)
    bool lit;                // a light pass comes first: under *N (a single draw), under inst->normals
    const Mat3* N;
    QSource q;
    bool persp() const { return q == Q_INV_CW; }
    bool tint() const { return inst && inst->tint; }
};

QSource q_source(const RenderContext* ctx, const Mesh* m) {
    if (ctx->meshPersp && (m->mode == ATTR_TEX || m->mode == ATTR_TEXC)) return Q_INV_CW;
    return m->mode == ATTR_TEXC ? Q_UNIT : Q_NONE;
}
// lit: the normal matrix of a lit draw, else null
MeshDraw single_draw(const RenderContext* ctx, const Mesh* m, const f64* matrix16, const Mat3* lit) {
    return MeshDraw{m, mat4_of(matrix16), nullptr, lit != nullptr, lit, q_source(ctx, m)};
}
MeshDraw instanced_draw(const RenderContext* ctx, const Mesh* m, const Instances* in, bool lit) {
    return MeshDraw{m, Mat4{}, in, lit, nullptr, q_source(ctx, m)};
}

// The draw as the staging layouts see it (nr_mesh_stage.h): a lit or an instanced soup has attributes of its own.
nrmesh::StageNeeds stage_needs(const MeshDraw& d) {
    const size_t K = d.inst ? (size_t)d.inst->K : 1;
    return nrmesh::StageNeeds{K * (size_t)d.m->nv, K * (size_t)d.m->n, d.persp(), d.lit, d.q == Q_UNIT,
                              d.lit || d.inst, (size_t)nrtri::attr_stride(d.m->mode)};
}

// A layout's regions in the staging, resolved once mstage.ensure() has returned.
struct StagePtrs {
    double2* vxy; f64* vz; f64* vq;
    double2* table;
    double2* xy; f64* z; double2* attr; f64* q;
    double2* expanded;
};
StagePtrs stage_ptrs(f64* base, const nrmesh::Stage& s) {
    const auto w = [&](nrmesh::Region k) { return reinterpret_cast<double2*>(s.at(base, k)); };
    return StagePtrs{w(nrmesh::R_VXY), s.at(base, nrmesh::R_VZ), s.at(base, nrmesh::R_VQ), w(nrmesh::R_TABLE),
                     w(nrmesh::R_XY), s.at(base, nrmesh::R_Z), w(nrmesh::R_ATTR), s.at(base, nrmesh::R_Q),
                     w(nrmesh::R_EXPANDED)};
}
// ... as the soup handed on: its own attributes, else the mesh's expanded ones.
Soup stage_soup(const StagePtrs& p, const Mesh* m, size_t count) {
    return Soup{reinterpret_cast<const f64*>(p.xy), p.z, p.attr ? reinterpret_cast<const f64*>(p.attr) : m->attr, p.q,
                (i64)count};
}

inline const double2* words(const f64* p) { return reinterpret_cast<const double2*>(p); }

// The kernel instance of each pass: one selection per pass and draw form.
auto vertex_kernel(const MeshDraw& d) { return d.persp() ? k_mesh_vertex<true> : k_mesh_vertex<false>; }
auto inst_vertex_kernel(const MeshDraw& d) { return d.persp() ? k_minst_vertex<true> : k_minst_vertex<false>; }
auto assemble_kernel(const MeshDraw& d) { return d.persp() ? k_mesh_assemble<true> : k_mesh_assemble<false>; }
auto uvc_assemble_kernel(const MeshDraw& d) { return d.persp() ? k_mesh_uvc_assemble<true> : k_mesh_uvc_assemble<false>; }
auto lit_assemble_kernel(const MeshDraw& d) {
    return d.m->mode == ATTR_GOURAUD ? k_mesh_lit_assemble<2> : k_mesh_lit_assemble<0>;
}
auto inst_assemble_kernel(const MeshDraw& d) {
    const bool tint = d.tint();
    return d.m->mode == ATTR_GOURAUD ? (tint ? k_minst_assemble<2, false, true> : k_minst_assemble<2, false, false>)
           : d.m->mode != ATTR_TEX   ? (tint ? k_minst_assemble<0, false, true> : k_minst_assemble<0, false, false>)
           : d.persp()               ? k_minst_assemble<1, true, false>
                                     : k_minst_assemble<1, false, false>;
}
auto inst_lit_assemble_kernel(const MeshDraw& d) {
    const bool tint = d.tint();
    return d.m->mode == ATTR_GOURAUD ? (tint ? k_minst_lit_assemble<2, true> : k_minst_lit_assemble<2, false>)
                                     : (tint ? k_minst_lit_assemble<0, true> : k_minst_lit_assemble<0, false>);
}
auto emit_kernel(const MeshDraw& d) {
    return d.m->mode == ATTR_TEXC      ? (d.persp() ? k_mesh_clip_emit<3, true> : k_mesh_clip_emit<3>)
           : d.m->mode == ATTR_GOURAUD ? k_mesh_clip_emit<2>
           : d.m->mode != ATTR_TEX     ? k_mesh_clip_emit<0>
           : d.persp()                 ? k_mesh_clip_emit<1, true>
                                       : k_mesh_clip_emit<1>;
}
auto inst_emit_kernel(const MeshDraw& d) {
    const bool tint = d.tint();
    return d.m->mode == ATTR_GOURAUD ? (tint ? k_minst_clip_emit<2, false, true> : k_minst_clip_emit<2, false, false>)
           : d.m->mode != ATTR_TEX   ? (tint ? k_minst_clip_emit<0, false, true> : k_minst_clip_emit<0, false, false>)
           : d.persp()               ? k_minst_clip_emit<1, true, false>
                                     : k_minst_clip_emit<1, false, false>;
}
auto inst_lit_emit_kernel(const MeshDraw& d) {
    const bool tint = d.tint();
    return d.m->mode == ATTR_GOURAUD ? (tint ? k_minst_lit_clip_emit<2, true> : k_minst_lit_clip_emit<2, false>)
                                     : (tint ? k_minst_lit_clip_emit<0, true> : k_minst_lit_clip_emit<0, false>);
}

// The light pass of a lit draw under the context's lights, as they are now, into `table` (NV*4).
void light_pass(RenderContext* ctx, const MeshDraw& d, i64 NV, double2* table) {
    const Mesh* m = d.m;
    if (d.inst)
        mesh_launch(ctx, NRK_MESH_INST_LIGHT, k_minst_light, NV, m->normal, words(m->rgba), (u32)m->nv, (u32)NV,
                    d.inst->normals, ctx->meshLights, table);
    else
        mesh_launch(ctx, NRK_MESH_LIGHT, k_mesh_light, NV, m->normal, words(m->rgba), m->nv, *d.N, ctx->meshLights, table);
}

// The soup of a draw with the clip state off, in ctx's mesh staging, on the context's stream: the vertex stage
// over all NV vertices, a lit draw's light pass beside it, the assembly of the N triangles -- which also gathers,
// copies or tints the attributes of a lit or an instanced soup -- and a unit q where the draw needs one.
// False: the staging could not be grown (error latched).
bool soup_unclipped(RenderContext* ctx, const MeshDraw& d, Soup* out) {
    nrtri::settle(ctx);   // a pending batch may still read the staging (its re-run comes first)
    const Mesh* m = d.m;
    const nrmesh::StageNeeds need = stage_needs(d);
    const nrmesh::Stage lay = nrmesh::stage_unclipped(need);
    if (!ctx->tri.mstage.ensure(lay.total)) return false;
    const StagePtrs p = stage_ptrs(ctx->tri.mstage, lay);
    const i64 NV = (i64)need.NV, C = (i64)need.N * 3;   // vertices and corners in all
    const u32 nv = (u32)m->nv, per = (u32)(m->n * 3);
    if (d.inst)
        mesh_launch(ctx, NRK_MESH_INST_VERTEX, inst_vertex_kernel(d), NV, m->pos, nv, (u32)NV, d.inst->mats, p.vxy, p.vz,
                    p.vq);
    else
        mesh_launch(ctx, NRK_MESH_VERTEX, vertex_kernel(d), NV, m->pos, NV, d.M, p.vxy, p.vz, p.vq);
    if (d.lit) light_pass(ctx, d, NV, p.table);
    if (d.inst && d.lit)
        mesh_launch(ctx, NRK_MESH_INST_ASSEMBLE, inst_lit_assemble_kernel(d), C, m->idx, per, (u32)C, nv, p.vxy, p.vz,
                    p.table, d.inst->tint, p.xy, p.z, p.attr);
    else if (d.inst)
        mesh_launch(ctx, NRK_MESH_INST_ASSEMBLE, inst_assemble_kernel(d), C, m->idx, per, (u32)C, nv, p.vxy, p.vz, p.vq,
                    words(m->attr), d.inst->tint, p.xy, p.z, p.q, p.attr);
    else if (d.lit && m->mode == ATTR_TEXC)
        mesh_launch(ctx, NRK_MESH_ASSEMBLE, uvc_assemble_kernel(d), C, m->idx, C, p.vxy, p.vz, p.vq, words(m->uv),
                    p.table, p.xy, p.z, p.q, p.attr);
    else if (d.lit)
        mesh_launch(ctx, NRK_MESH_ASSEMBLE, lit_assemble_kernel(d), C, m->idx, C, p.vxy, p.vz, p.table, p.xy, p.z, p.attr);
    else
        mesh_launch(ctx, NRK_MESH_ASSEMBLE, assemble_kernel(d), C, m->idx, C, p.vxy, p.vz, p.xy, p.z, p.vq, p.q);
    if (d.q == Q_UNIT) unit_q(ctx, p.q, C);
    *out = stage_soup(p, m, need.N);
    return true;
}

// The front half of a draw with the clip state on, under the context's near plane and cull mode: clip coordinates
// per vertex (TriScratch::mclip), a keep mask and a count per triangle, the exclusive scan of the counts (mscan),
// and the total nout read back -- the one host wait of such a draw.  An instanced draw runs each pass once over
// all K*nv vertices or K*n triangles, so the instances' outputs follow each other in instance order.
// False: scratch could not be grown, or the read-back failed (latched).
struct ClipFront { const double2* clip; const u32* keep; const u32* off; size_t nout; };
bool clip_front(RenderContext* ctx, const MeshDraw& d, const nrmesh::StageNeeds& need, ClipFront* f) {
    const Mesh* m = d.m;
    const size_t NV = need.NV, N = need.N;
    if (N > (size_t)INT_MAX) return fail("mesh clip stage", "more than 2^31 - 1 triangles");
    nrtri::settle(ctx);   // a pending batch may still read the staging (its re-run comes first)
    TriScratch& sc = ctx->tri;
    if (!sc.mclip.ensure(NV * 4) || !sc.mscan.ensure(N * 3)) return false;
    u32* keep = sc.mscan;
    u32* cnt = keep + N;
    u32* off = cnt + N;
    size_t temp = 0;
    NR_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, cnt, off, (int)N, ctx->stream));
    if (!grow_temp(sc, temp > 0 ? temp : 1)) return false;
    u32* h = reinterpret_cast<u32*>(sc.totals());
    if (!h) return fail("mesh clip stage", "hipHostMalloc failed");
    const f64 wNear = ctx->meshNear;
    double2* clip = reinterpret_cast<double2*>(sc.mclip.p);
    if (d.inst) {
        mesh_launch(ctx, NRK_MESH_INST_CLIP_VERTEX, k_minst_clip_vertex, (i64)NV, m->pos, (u32)m->nv, (u32)NV,
                    d.inst->mats, clip);
        mesh_launch(ctx, NRK_MESH_INST_CLIP_COUNT, k_minst_clip_count, (i64)N, m->idx, (u32)m->n, (u32)N, (u32)m->nv,
                    clip, wNear, ctx->meshCull, keep, cnt);
    } else {
        mesh_launch(ctx, NRK_MESH_CLIP_VERTEX, k_mesh_clip_vertex, m->nv, m->pos, m->nv, d.M, clip);
        mesh_launch(ctx, NRK_MESH_CLIP_COUNT, k_mesh_clip_count, m->n, m->idx, m->n, clip, wNear, ctx->meshCull, keep, cnt);
    }
    const int scan = d.inst ? NRK_MESH_INST_CLIP_SCAN : NRK_MESH_CLIP_SCAN;
    hipEvent_t a, b;
    nr_timing_begin(ctx, scan, &a, &b);
    NR_CHECK(hipcub::DeviceScan::ExclusiveSum(sc.temp, temp, cnt, off, (int)N, ctx->stream));
    nr_timing_end(ctx, scan, a, b);
    // nout = the last offset + the last count (at most 2N < 2^32): the sync point of a clipped or culled draw
    NR_CHECK(hipMemcpyAsync(&h[0], off + (N - 1), sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    NR_CHECK(hipMemcpyAsync(&h[1], cnt + (N - 1), sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("mesh clip stage", "the count could not be read back");
    *f = ClipFront{clip, keep, off, (size_t)h[0] + (size_t)h[1]};
    return true;
}

// The soup of a draw with the clip state on: the front half, then -- in ctx's mesh staging, carved for nout
// triangles -- the emit pass at the scanned offsets and a unit q where the draw needs one.  A lit draw's light
// pass and the expansion of its colour table through the indices (k_mesh_attr's, per instance) run before the
// emit pass, behind the soup in the staging, and the emit pass reads that expansion where it reads the mesh's
// own attributes otherwise.  out->n == 0: nothing is left to draw (no staging is touched).
bool soup_clipped(RenderContext* ctx, const MeshDraw& d, Soup* out) {
    const Mesh* m = d.m;
    const nrmesh::StageNeeds need = stage_needs(d);
    ClipFront f;
    if (!clip_front(ctx, d, need, &f)) return false;
    *out = Soup{nullptr, nullptr, nullptr, nullptr, (i64)f.nout};
    if (f.nout == 0) return true;
    if (f.nout > 2 * need.N) return fail("mesh clip stage", "inconsistent triangle count");   // (never: the counts are 0, 1 or 2)
    const nrmesh::Stage lay = nrmesh::stage_clipped(need, f.nout);
    if (!ctx->tri.mstage.ensure(lay.total)) return false;
    const StagePtrs p = stage_ptrs(ctx->tri.mstage, lay);
    const i64 NV = (i64)need.NV, N = (i64)need.N;
    const u32 nv = (u32)m->nv, n = (u32)m->n;
    const f64 wNear = ctx->meshNear;
    const double2* src = words(m->attr);
    if (d.lit) {
        light_pass(ctx, d, NV, p.table);
        const int perTri = m->mode == ATTR_FLAT ? 1 : 3;
        if (d.inst)
            mesh_launch(ctx, NRK_MESH_INST_LIT_ATTR, k_minst_lit_attr, N * perTri, m->idx, n * (u32)perTri,
                        (u32)(N * perTri), nv, perTri, p.table, p.expanded);
        else if (m->mode == ATTR_TEXC)
            mesh_launch(ctx, NRK_MESH_LIT_ATTR, k_mesh_uvc_attr, N * 3, m->idx, N * 3, words(m->uv), p.table, p.expanded);
        else
            mesh_launch(ctx, NRK_MESH_LIT_ATTR, k_mesh_attr, N * perTri, m->idx, N * perTri, perTri, 2, p.table, p.expanded);
        src = p.expanded;
    }
    if (d.inst && d.lit)   // (the emit pass that reads instance k's own attributes)
        mesh_launch(ctx, NRK_MESH_INST_CLIP_EMIT, inst_lit_emit_kernel(d), N, m->idx, n, (u32)N, nv, f.clip, src,
                    d.inst->tint, wNear, f.keep, f.off, p.xy, p.z, p.attr);
    else if (d.inst)
        mesh_launch(ctx, NRK_MESH_INST_CLIP_EMIT, inst_emit_kernel(d), N, m->idx, n, (u32)N, nv, f.clip, src,
                    d.inst->tint, wNear, f.keep, f.off, p.xy, p.z, p.attr, p.q);
    else
        mesh_launch(ctx, NRK_MESH_CLIP_EMIT, emit_kernel(d), N, m->idx, N, f.clip, src, wNear, f.keep, f.off, p.xy, p.z,
                    p.attr, p.q);
    if (d.q == Q_UNIT) unit_q(ctx, p.q, (i64)f.nout * 3);
    *out = stage_soup(p, m, f.nout);
    return true;
}

// The soup a draw rasterises under the context's clip state.
bool build_soup(RenderContext* ctx, const MeshDraw& d, Soup* out) {
    return clip_stage_on(ctx) ? soup_clipped(ctx, d, out) : soup_unclipped(ctx, d, out);
}

// ---- what the entry points share ----------------------------------------------------------------------------------
// The checks every mesh draw shares (in the style of check_texture).
// uvcOk: the call also draws a textured colour mesh (as a textured one); every other call rejects that kind.
bool check_mesh(RenderContext* ctx, const Mesh* m, bool textured, bool uvcOk, const char* what) {
    if (!m) return fail(what, "NULL mesh");
    if (m->mode == nrtri::ATTR_TEXC) {
        if (!uvcOk) return fail(what, "not supported for a textured colour mesh");
    } else if ((m->mode == nrtri::ATTR_TEX) != textured)
        return fail(what, textured ? "a colour mesh (use DrawMesh)" : "a textured mesh (use DrawTexturedMesh)");
    if (m->device != ctx->device) return fail(what, "mesh on another device");
    return true;
}

// What a *Lit call needs of its mesh, after check_mesh(textured = false).
bool check_lit(const Mesh* m, const char* what) {
    return m->lit ? true : fail(what, "a mesh without normals (create it with CreateLitMesh)");
}

// The argument checks every instanced entry point shares, after the mesh's own: false with an error latched under
// `what`, or *empty when there is nothing to draw (no error).  Nothing is allocated or read before them.
// frame: an empty context counts as nothing to draw (the draws; AssembleMeshInstanced needs no frame).
bool check_instances(const RenderContext* ctx, const Mesh* m, const f64* matrices, const f64* tint, i64 K, bool frame,
                     bool* empty, const char* what) {
    *empty = true;
    if (K < 0) return fail(what, "negative instance count");
    if (tint && m->mode == nrtri::ATTR_TEX) return fail(what, "a textured mesh takes no tint");
    if (K == 0 || m->n <= 0 || (frame && (ctx->width <= 0 || ctx->height <= 0))) return true;
    if (!matrices) return fail(what, "NULL matrices");
    if (K > (i64)INT_MAX / m->n) return fail(what, "more than 2^31 - 1 triangles");
    if (K > (i64)INT_MAX / m->nv) return fail(what, "more than 2^31 - 1 vertices");
    *empty = false;
    return true;
}

// The checks the Assemble* calls with a capacity share (textured: a textured mesh only), in their order; *n_out is
// zeroed once it is known to be there.  outputs: every output array is there.
bool check_assemble(RenderContext* ctx, const Mesh* m, bool textured, i64 cap, bool outputs, i64* n_out,
                    const char* what) {
    if (!m) return fail(what, "NULL mesh");
    if (m->mode == nrtri::ATTR_TEXC) return fail(what, "not supported for a textured colour mesh");
    if (textured && m->mode != nrtri::ATTR_TEX) return fail(what, "a colour mesh");
    if (m->device != ctx->device) return fail(what, "mesh on another device");
    if (!n_out) return fail(what, "NULL output");
    *n_out = 0;
    if (cap < 0) return fail(what, "negative capacity");
    if (cap > 0 && !outputs) return fail(what, "NULL output");
    return true;
}

// The mesh checks of the two lit Assemble calls, after check_assemble.
bool check_assemble_lit(const Mesh* m, const char* what) {
    if (m->mode == nrtri::ATTR_TEX) return fail(what, "a textured mesh");
    return check_lit(m, what);
}

// A host call's matrices and tints onto the device (TriScratch::minst), through the context's pinned buffer by
// one asynchronous copy: the caller's arrays are free when this returns and the host waits for nothing but an
// earlier such copy (of the draw before last), long done.  (The copy-and-wait of DrawTriangles' staging would add a host wait to every
// draw, which is what an instanced draw is there to avoid.)  Settles first: minst follows mstage's rule.
// normals (a lit draw's, or null) travel behind the tints in the same copy.
bool upload_instances(RenderContext* ctx, const f64* matrices, const f64* tint, i64 K, const f64* normals,
                      Instances* out) {
    nrtri::settle(ctx);
    TriScratch& sc = ctx->tri;
    const size_t k = (size_t)K, ntint = tint ? k * 4 : 0, need = k * 16 + ntint + (normals ? k * 9 : 0);
    if (!sc.minst.ensure(need)) return false;
    int slot = 0;   // two pinned buffers in turn: the wait is for the copy of the draw before last
    f64* h = nr_mesh_pinned(sc, need, &slot);
    if (!h) return fail("instanced mesh draw", "hipHostMalloc failed");
    std::memcpy(h, matrices, k * 16 * sizeof(f64));
    if (tint) std::memcpy(h + k * 16, tint, k * 4 * sizeof(f64));
    if (normals) std::memcpy(h + k * 16 + ntint, normals, k * 9 * sizeof(f64));
    NR_CHECK(hipMemcpyAsync(sc.minst.p, h, need * sizeof(f64), hipMemcpyHostToDevice, ctx->stream));
    NR_CHECK(hipEventRecord(sc.evMinst[slot], ctx->stream));
    *out = Instances{sc.minst.p, tint ? sc.minst.p + k * 16 : nullptr, K,
                     normals ? sc.minst.p + k * 16 + ntint : nullptr};
    return true;
}

inline nrtri::Opacity mesh_opacity(const Mesh* m) { return m->opaque ? nrtri::OPQ_OPAQUE : nrtri::OPQ_BLENDED; }

// The tail of every mesh draw: the soup's count is the context's last count, and what is left of it goes to the
// rasters as one batch -- of the mesh's own mode, or sampled from `tex` (modulated: a textured colour mesh's, the
// texel times the interpolated colour; s.q: the perspective state, or the unit q).
void submit(RenderContext* ctx, const Mesh* m, Texture* tex, const Soup& s, nrtri::Opacity opq, bool modulated) {
    ctx->meshLastCount = s.n;
    if (s.n <= 0) return;   // (clipped or culled away)
    Batch b = soup_batch(s, tex ? nrtri::ATTR_TEX : m->mode, opq, nullptr, false);
    b.modulated = modulated;
    if (tex) nrtri::draw_textured(ctx, tex, b);
    else nrtri::draw(ctx, b);
}

// The instanced draw entry points under the caller's name `what`.  onDevice: matrices, tint and normals are device
// arrays, read only by the vertex, light and assembly kernels launched here; the batch reads the context's staging.
// lit: a lit draw (a colour mesh with normals), `normals` its K*9 normal matrices or null.
void draw_instanced(RenderContext* ctx, Mesh* m, Texture* tex, bool textured, const f64* matrices, const f64* tint,
                    i64 K, bool onDevice, const char* what, bool lit, const f64* normals) {
    NR_CHECK(hipSetDevice(ctx->device));
    ctx->meshLastCount = 0;
    if (!check_mesh(ctx, m, textured, false, what) || (lit && !check_lit(m, what))) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (textured && !nrtri::check_texture(ctx, tex, what)) return;
    bool empty;
    if (!check_instances(ctx, m, matrices, tint, K, true, &empty, what) || empty) return;
    Instances in{matrices, tint, K, normals};
    if (!onDevice && !upload_instances(ctx, matrices, tint, K, normals, &in)) return;
    Soup s;
    if (!build_soup(ctx, instanced_draw(ctx, m, &in, lit), &s)) return;
    // opaque: an opaque mesh under no tint or tints of alpha 1 (a device tint: the batch's own device scan); a
    // textured batch: decided by the texture
    nrtri::Opacity opq = textured ? nrtri::OPQ_UNKNOWN : mesh_opacity(m);
    if (tint && m->opaque) {
        if (onDevice) opq = nrtri::OPQ_UNKNOWN;
        else
            for (i64 k = 0; k < K; ++k)
                if (tint[k * 4 + 3] != 1) { opq = nrtri::OPQ_BLENDED; break; }
    }
    submit(ctx, m, textured ? tex : nullptr, s, opq, false);
}

// The tail of the Assemble* entry points: *n_out (where the call has one) is the full count, and the first
// k = min(cap, count) triangles of each part that is there on both sides go to the host, then the wait.
size_t copy_soup(RenderContext* ctx, const Soup& s, i64 cap, i64* n_out, f64* xy, f64* z, f64* attr, int stride, f64* q) {
    struct Part { f64* dst; const f64* src; size_t per; };
    if (n_out) *n_out = s.n;
    const size_t k = (size_t)(s.n < cap ? s.n : cap);
    for (const Part& c : {Part{xy, s.xy, 6}, Part{z, s.z, 3}, Part{attr, s.attr, (size_t)stride}, Part{q, s.q, 3}})
        if (k > 0 && c.dst && c.src)
            NR_CHECK(hipMemcpyAsync(c.dst, c.src, k * c.per * sizeof(f64), hipMemcpyDeviceToHost, ctx->stream));
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    return k;
}

// Every context that may have a pending batch reading the mesh's arrays is
// settled and the device's streams are drained (as DestroyTriangleBuffer).
void quiesce(const Mesh* m) {
    nr_settle_all();
    NR_CHECK(hipSetDevice(m->device));
    NR_CHECK(hipStreamSynchronize(nr_stream_for(m->device)));
    NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(m->device)));
}

// UpdateMeshPositions and UpdateMeshNormals: nv*3 doubles from the host into `dst`, once nothing reads it any more.
bool update_array(const Mesh* m, f64* dst, const f64* src) {
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    quiesce(m);
    hipStream_t s = nr_stream_for(m->device);
    NR_CHECK(hipMemcpyAsync(dst, src, (size_t)m->nv * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
    NR_CHECK(hipStreamSynchronize(s));   // caller may reuse its array on return
    NR_CHECK(hipSetDevice(prev));
    return true;
}

}  // namespace
}  // namespace nrtri

using namespace nrtri;

extern "C" {

// New: an indexed mesh with per-vertex colours (nv*4), flat (the colour of each
// triangle's first index) or Gouraud.  One H2D upload; NULL + error on an index
// >= nv, NULL rgba with n > 0, or nv beyond 32 bits.  n == 0 is a valid mesh.
Mesh* CreateMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* rgba, bool gouraud) {
    return create_mesh("CreateMesh", nv, pos, n, idx, rgba, gouraud, nullptr, nullptr);
}

// New: an indexed mesh with per-vertex texture coordinates (nv*2, texel units).
Mesh* CreateTexturedMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* uv) {
    if (!uv && n > 0) {
        fail("CreateTexturedMesh", "NULL uv");
        return nullptr;
    }
    static const f64 none[2] = {0, 0};
    return create_mesh("CreateTexturedMesh", nv, pos, n, idx, nullptr, false, uv ? uv : none, nullptr);
}

void DestroyMesh(Mesh* m) {
    if (!m) return;
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    quiesce(m);
    free_mesh(m);
    NR_CHECK(hipSetDevice(prev));
}

i64 GetMeshVertexCount(Mesh* m) { return m->nv; }
i64 GetMeshTriangleCount(Mesh* m) { return m->n; }

// New: replaces the positions (nv*3) of a deforming mesh: an H2D copy of the
// positions only.  Draws issued before the call keep the old positions.
bool UpdateMeshPositions(Mesh* m, const f64* pos) {
    if (!m) return fail("UpdateMeshPositions", "NULL mesh");
    if (m->nv == 0) return true;
    if (!pos) return fail("UpdateMeshPositions", "NULL positions");
    return update_array(m, m->pos, pos);
}

// New: draws a colour mesh under the row-major 4x4 `matrix16` (NULL: the
// identity), then the context's transform, depth state and colour transform as
// for DrawTriangles.
void DrawMesh(RenderContext* ctx, Mesh* m, const f64* matrix16) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_mesh(ctx, m, false, false, "DrawMesh")) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    ctx->meshLastCount = 0;
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, nullptr), &s)) return;
    submit(ctx, m, nullptr, s, mesh_opacity(m), false);
}

// New: draws a textured mesh sampled from `tex` (chosen per draw); a textured colour mesh: modulated by its own
// vertex colours, unlit -- opaque when the texture has no alpha (draw_textured) and every vertex alpha is 1 (a cut
// vertex's is 1 + 0 * t).
void DrawTexturedMesh(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrix16) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_mesh(ctx, m, true, true, "DrawTexturedMesh")) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (!nrtri::check_texture(ctx, tex, "DrawTexturedMesh")) return;
    ctx->meshLastCount = 0;
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    const bool uvc = m->mode == nrtri::ATTR_TEXC;
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, nullptr), &s)) return;
    submit(ctx, m, tex, s, uvc ? mesh_opacity(m) : nrtri::OPQ_UNKNOWN, uvc);
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
    MeshDraw d = single_draw(ctx, m, matrix16, nullptr);
    d.q = Q_NONE;   // (the clip and perspective state are ignored)
    Soup s;
    if (!soup_unclipped(ctx, d, &s)) return false;
    copy_soup(ctx, s, s.n, nullptr, xy_out, z_out, nullptr, 0, nullptr);
    return true;
}

// New: the near plane of this context's mesh draws: 0 (the default) is off, w > 0
// clips every mesh triangle against cw = w (DESIGN.md §3 "Clip stage").  Per
// context; not part of the save / restore stack, not recorded.  A negative or
// non-finite w latches an error and leaves the state unchanged.
bool SetMeshNearPlane(RenderContext* ctx, f64 wNear) {
    if (!(wNear >= 0) || !std::isfinite(wNear)) return fail("SetMeshNearPlane", "the plane must be finite and >= 0");
    ctx->meshNear = wNear;
    return true;
}
f64 GetMeshNearPlane(RenderContext* ctx) { return ctx->meshNear; }

// New: back-face culling of this context's mesh draws by the sign of
// area2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0) of each output triangle,
// before the context's 2D transform: 0 none (the default), 1 drops area2 > 0,
// 2 drops area2 < 0.  Another mode latches an error, the state unchanged.
bool SetMeshCull(RenderContext* ctx, i64 mode) {
    if (mode < 0 || mode > 2) return fail("SetMeshCull", "mode must be 0 (none), 1 (drop area2 > 0) or 2 (drop area2 < 0)");
    ctx->meshCull = (int)mode;
    return true;
}
i64 GetMeshCull(RenderContext* ctx) { return ctx->meshCull; }

// New: perspective-correct texture mapping of this context's DrawTexturedMesh
// draws: the vertex stage keeps q = 1.0 / cw per vertex (a cut
// vertex: 1.0 / wNear) and the rasters sample at (U / Q, V / Q) instead of the
// screen-affine (u, v).  Off by default; per context; not part of the save /
// restore stack, not recorded (the clip state's rule).  DrawMesh of a colour
// mesh ignores it: colours stay affine in screen space.  Returns true.
bool SetMeshPerspective(RenderContext* ctx, bool on) {
    ctx->meshPersp = on;
    return true;
}
bool GetMeshPerspective(RenderContext* ctx) { return ctx->meshPersp; }

// New: the soup a DrawTexturedMesh of `m` rasterises under the context's near
// plane, cull mode and perspective state -- the draw's own kernels -- copied to
// the host: *n_out = the full count, the first min(cap, *n_out) triangles in
// xy_out (x6), z_out (x3), uv_out (x6) and q_out (x3; 1.0 everywhere with the
// perspective state off).  A sync point; a textured mesh only.
bool AssembleMeshPerspective(RenderContext* ctx, Mesh* m, const f64* matrix16, i64 cap, f64* xy_out, f64* z_out,
                             f64* uv_out, f64* q_out, i64* n_out) {
    NR_CHECK(hipSetDevice(ctx->device));
    const bool outputs = xy_out && z_out && uv_out && q_out;
    if (!check_assemble(ctx, m, true, cap, outputs, n_out, "AssembleMeshPerspective")) return false;
    if (m->n <= 0) return true;
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, nullptr), &s)) return false;
    const size_t k = copy_soup(ctx, s, cap, n_out, xy_out, z_out, uv_out, 6, q_out);
    if (!s.q)
        for (size_t i = 0; i < k * 3; ++i) q_out[i] = 1.0;
    return true;
}

// New: the triangles the context's last mesh draw handed to the rasters: n_out of
// the clip stage, or the mesh's n when the stage was off.
i64 GetMeshLastTriangleCount(RenderContext* ctx) { return ctx->meshLastCount; }

// New: the soup a mesh draw rasterises under the context's near plane and cull
// mode -- the draw's own kernels -- copied to the host: *n_out = the full count,
// the first min(cap, *n_out) triangles in xy_out (x6), z_out (x3) and attr_out
// (x12 Gouraud, x4 flat, x6 textured).  A sync point; either mesh kind.
bool AssembleMeshClipped(RenderContext* ctx, Mesh* m, const f64* matrix16, i64 cap, f64* xy_out, f64* z_out,
                         f64* attr_out, i64* n_out) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_assemble(ctx, m, false, cap, xy_out && z_out && attr_out, n_out, "AssembleMeshClipped")) return false;
    if (m->n <= 0) return true;
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, nullptr), &s)) return false;
    copy_soup(ctx, s, cap, n_out, xy_out, z_out, attr_out, nrtri::attr_stride(m->mode), nullptr);
    return true;
}

// New: an instanced draw (DESIGN.md §3 "Instanced mesh draws"): the colour mesh `m` under each of the K row-major
// 4x4 `matrices` (K*16) as one batch -- the frame of DrawMesh(ctx, m, matrices + 16 k) for k = 0 .. K-1 in that
// order, from one vertex and assembly pass and one binning.  tint (K*4: r, g, b, a) or NULL: every vertex colour
// of instance k times tint[k], as if the mesh had been created with those colours; NULL is no product at all.
// Host arrays, free again on return.  K == 0 draws nothing; K < 0, NULL matrices with K > 0, or more than
// 2^31 - 1 triangles or vertices in all latch an error and draw nothing.
void DrawMeshInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K) {
    draw_instanced(ctx, m, nullptr, false, matrices, tint, K, false, "DrawMeshInstanced", false, nullptr);
}

// New: the same for a textured mesh sampled from `tex` (no tint).
void DrawTexturedMeshInstanced(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrices, i64 K) {
    draw_instanced(ctx, m, tex, true, matrices, nullptr, K, false, "DrawTexturedMeshInstanced", false, nullptr);
}

// New: the same from device-resident matrices and tint (as DrawTrianglesDevice: valid and unchanged until the
// draw has executed).  Only the vertex and assembly kernels launched in the call read them.
void DrawMeshInstancedDevice(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K) {
    draw_instanced(ctx, m, nullptr, false, matrices, tint, K, true, "DrawMeshInstancedDevice", false, nullptr);
}
void DrawTexturedMeshInstancedDevice(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrices, i64 K) {
    draw_instanced(ctx, m, tex, true, matrices, nullptr, K, true, "DrawTexturedMeshInstancedDevice", false, nullptr);
}

// New: the soup an instanced draw of `m` rasterises under the context's near plane, cull mode and perspective
// state -- the draw's own kernels, host matrices and tint -- copied to the host: *n_out = the full count, the
// first min(cap, *n_out) triangles in xy_out (x6), z_out (x3), attr_out (x12 Gouraud, x4 flat, x6 textured) and,
// for a perspective textured draw only, q_out (x3; may be NULL otherwise).  A sync point; either mesh kind.
bool AssembleMeshInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K, i64 cap,
                           f64* xy_out, f64* z_out, f64* attr_out, f64* q_out, i64* n_out) {
    const char* what = "AssembleMeshInstanced";
    NR_CHECK(hipSetDevice(ctx->device));
    const bool persp = m && q_source(ctx, m) == Q_INV_CW;
    const bool outputs = xy_out && z_out && attr_out && (q_out || !persp);
    if (!check_assemble(ctx, m, false, cap, outputs, n_out, what)) return false;
    bool empty;
    if (!check_instances(ctx, m, matrices, tint, K, false, &empty, what)) return false;
    if (empty) return true;
    Instances in;
    Soup s;
    if (!upload_instances(ctx, matrices, tint, K, nullptr, &in) || !build_soup(ctx, instanced_draw(ctx, m, &in, false), &s))
        return false;
    copy_soup(ctx, s, cap, n_out, xy_out, z_out, attr_out, nrtri::attr_stride(m->mode), q_out);
    return true;
}

// ---- lit meshes (DESIGN.md §3 "Vertex lighting") ---------------------------------------------------------------
// New: CreateMesh with per-vertex normals (nv*3): the mesh keeps them and its per-vertex colours on the device for
// the light pass of the *Lit draws.  CreateMesh's checks, and NULL normals with nv > 0.  DrawMesh and
// DrawMeshInstanced draw such a mesh unlit, from its expanded colours.
Mesh* CreateLitMesh(i64 nv, const f64* pos, const f64* normal, i64 n, const uint32_t* idx, const f64* rgba,
                    bool gouraud) {
    if (!normal && nv > 0) {
        fail("CreateLitMesh", "NULL normals");
        return nullptr;
    }
    static const f64 none[3] = {0, 0, 0};
    return create_mesh("CreateLitMesh", nv, pos, n, idx, rgba, gouraud, nullptr, normal ? normal : none);
}

// ---- textured colour meshes (DESIGN.md §3 "Modulated textured draws") -----------------------------------------
// New: an indexed mesh with both a texel-unit uv (nv*2) and a colour (nv*4) per vertex, and normals (nv*3) or NULL.
// It keeps the per-vertex uv and rgba on the device (and the normals, when given: GetMeshLit); its expanded
// attributes are n*18, per corner (u v | r g | b a).  CreateMesh's checks, and NULL uv or rgba with n > 0.
Mesh* CreateTexturedColorMesh(i64 nv, const f64* pos, const f64* normal, i64 n, const uint32_t* idx, const f64* uv,
                              const f64* rgba) {
    if ((!uv || !rgba) && n > 0) {
        fail("CreateTexturedColorMesh", !uv ? "NULL uv" : "NULL rgba");
        return nullptr;
    }
    static const f64 none[4] = {0, 0, 0, 0};
    return create_mesh("CreateTexturedColorMesh", nv, pos, n, idx, rgba ? rgba : none, true, uv ? uv : none, normal);
}

// New: DrawTexturedMesh of a textured colour mesh with normals, lit: the light pass of DrawMeshLit runs on the
// vertex colours (the uv untouched; alpha is copied) before anything else reads them, and the rest is
// DrawTexturedMesh's -- every state of it applies.  A mesh of another kind, or one without normals, latches an
// error and draws nothing (the last count 0).  With the default lights and colours in [0, 1] the frame is
// DrawTexturedMesh's bit for bit.
void DrawTexturedMeshLit(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrix16, const f64* normal9) {
    const char* what = "DrawTexturedMeshLit";
    NR_CHECK(hipSetDevice(ctx->device));
    ctx->meshLastCount = 0;
    if (!m) { fail(what, "NULL mesh"); return; }
    if (m->mode != nrtri::ATTR_TEXC) { fail(what, "not a textured colour mesh (create it with CreateTexturedColorMesh)"); return; }
    if (!check_mesh(ctx, m, true, true, what)) return;
    if (!m->lit) { fail(what, "a mesh without normals"); return; }
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (!nrtri::check_texture(ctx, tex, what)) return;
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    const Mat3 N = mat3_of(normal9);
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, &N), &s)) return;
    submit(ctx, m, tex, s, mesh_opacity(m), true);
}

// New: the soup such a draw rasterises -- the draw's own kernels -- in AssembleMeshPerspective's conventions:
// uvc_out x18, q_out x3 (1.0 with the perspective state off).  lit == false: DrawTexturedMesh's soup, normal9
// ignored; lit: DrawTexturedMeshLit's (the mesh needs normals).  A sync point.
bool AssembleTexturedColorMesh(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9, bool lit, i64 cap,
                               f64* xy_out, f64* z_out, f64* uvc_out, f64* q_out, i64* n_out) {
    const char* what = "AssembleTexturedColorMesh";
    NR_CHECK(hipSetDevice(ctx->device));
    // (check_assemble's checks but for the kind of mesh, which it would reject)
    if (!m) return fail(what, "NULL mesh");
    if (m->mode != nrtri::ATTR_TEXC) return fail(what, "not a textured colour mesh (create it with CreateTexturedColorMesh)");
    if (m->device != ctx->device) return fail(what, "mesh on another device");
    if (!n_out) return fail(what, "NULL output");
    *n_out = 0;
    if (cap < 0) return fail(what, "negative capacity");
    if (cap > 0 && !(xy_out && z_out && uvc_out && q_out)) return fail(what, "NULL output");
    if (lit && !m->lit) return fail(what, "a mesh without normals");
    if (m->n <= 0) return true;
    const Mat3 N = mat3_of(normal9);
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, lit ? &N : nullptr), &s)) return false;
    copy_soup(ctx, s, cap, n_out, xy_out, z_out, uvc_out, 18, q_out);
    return true;
}

// New: replaces the normals (nv*3) of a lit mesh; UpdateMeshPositions' contract.
bool UpdateMeshNormals(Mesh* m, const f64* normal) {
    if (!m) return fail("UpdateMeshNormals", "NULL mesh");
    if (!m->lit) return fail("UpdateMeshNormals", "a mesh without normals (create it with CreateLitMesh)");
    if (m->nv == 0) return true;
    if (!normal) return fail("UpdateMeshNormals", "NULL normals");
    return update_array(m, m->normal, normal);
}

bool GetMeshLit(Mesh* m) { return m->lit; }

// New: the light state of this context's lit mesh draws: ambient3 (NULL: (1, 1, 1)) and nl directional lights
// (dx, dy, dz, cr, cg, cb), nl*6, d towards the light in the space the normal matrix maps into.  Copied here; per
// context, not part of the save / restore stack, not recorded; read when a draw is issued.  nl outside 0 .. 8 or
// NULL lights with nl > 0 latch an error and leave the state unchanged.  The values are not validated.
bool SetMeshLights(RenderContext* ctx, const f64* ambient3, const f64* lights, i64 nl) {
    if (nl < 0 || nl > MESH_MAX_LIGHTS) return fail("SetMeshLights", "the light count must be 0 .. 8");
    if (nl > 0 && !lights) return fail("SetMeshLights", "NULL lights");
    MeshLights L;
    if (ambient3)
        for (int c = 0; c < 3; ++c) L.ambient[c] = ambient3[c];
    for (i64 k = 0; k < nl * 6; ++k) L.light[k / 6][k % 6] = lights[k];
    L.nl = (int)nl;
    ctx->meshLights = L;
    return true;
}
i64 GetMeshLightCount(RenderContext* ctx) { return ctx->meshLights.nl; }

// New: DrawMesh of a lit mesh under the context's lights and the row-major 3x3 normal matrix `normal9` (NULL: the
// identity): the light pass computes every vertex colour on the device, the rest of the draw is DrawMesh's.
void DrawMeshLit(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9) {
    NR_CHECK(hipSetDevice(ctx->device));
    ctx->meshLastCount = 0;
    if (!check_mesh(ctx, m, false, false, "DrawMeshLit") || !check_lit(m, "DrawMeshLit")) return;
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (m->n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    const Mat3 N = mat3_of(normal9);
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, &N), &s)) return;
    submit(ctx, m, nullptr, s, mesh_opacity(m), false);
}

// New: DrawMeshInstanced of a lit mesh: instance k under matrices[k] and the normal matrix normals[k] (K*9; NULL:
// the identity for every instance); a tint multiplies the lit colours.  Host arrays, free again on return.
void DrawMeshLitInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals, const f64* tint,
                          i64 K) {
    draw_instanced(ctx, m, nullptr, false, matrices, tint, K, false, "DrawMeshLitInstanced", true, normals);
}

// New: the same from device-resident matrices, normal matrices and tint (as DrawMeshInstancedDevice).
void DrawMeshLitInstancedDevice(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals,
                                const f64* tint, i64 K) {
    draw_instanced(ctx, m, nullptr, false, matrices, tint, K, true, "DrawMeshLitInstancedDevice", true, normals);
}

// New: the soup a DrawMeshLit rasterises under the context's lights, near plane and cull mode -- the draw's own
// kernels -- in AssembleMeshClipped's conventions (attr x12 Gouraud, x4 flat).  A sync point.
bool AssembleMeshLit(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9, i64 cap, f64* xy_out,
                     f64* z_out, f64* attr_out, i64* n_out) {
    const char* what = "AssembleMeshLit";
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_assemble(ctx, m, false, cap, xy_out && z_out && attr_out, n_out, what)) return false;
    if (!check_assemble_lit(m, what)) return false;
    if (m->n <= 0) return true;
    const Mat3 N = mat3_of(normal9);
    Soup s;
    if (!build_soup(ctx, single_draw(ctx, m, matrix16, &N), &s)) return false;
    copy_soup(ctx, s, cap, n_out, xy_out, z_out, attr_out, nrtri::attr_stride(m->mode), nullptr);
    return true;
}

// New: the same for a DrawMeshLitInstanced (host arrays), in AssembleMeshInstanced's conventions without q.
bool AssembleMeshLitInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals, const f64* tint,
                              i64 K, i64 cap, f64* xy_out, f64* z_out, f64* attr_out, i64* n_out) {
    const char* what = "AssembleMeshLitInstanced";
    NR_CHECK(hipSetDevice(ctx->device));
    if (!check_assemble(ctx, m, false, cap, xy_out && z_out && attr_out, n_out, what)) return false;
    if (!check_assemble_lit(m, what)) return false;
    bool empty;
    if (!check_instances(ctx, m, matrices, tint, K, false, &empty, what)) return false;
    if (empty) return true;
    Instances in;
    Soup s;
    if (!upload_instances(ctx, matrices, tint, K, normals, &in) || !build_soup(ctx, instanced_draw(ctx, m, &in, true), &s))
        return false;
    copy_soup(ctx, s, cap, n_out, xy_out, z_out, attr_out, nrtri::attr_stride(m->mode), nullptr);
    return true;
}

}  // extern "C"

